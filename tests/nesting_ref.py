"""The nesting of a voxel bitmap's outlines (fhip_outlines_nesting, include/fidget_hip.h) restated over the loops of outlines_ref.py by the
header's second definition, which follows no chain of `left` links: a loop e != l encloses l iff e has an odd number of vertical unit
edges on the pixel row of l's leader to the left of the leader, and parent[l] is the enclosing loop of smallest |area2|.  Every loop
is walked along `next` and its vertical unit edges listed one by one; `left` is the owner of the nearest of all of them.

  layer(L)                       L: outlines_ref.layer's dict -> dict: left, parent, depth, n_children, region_area2 (int64 [loops], ids
                                 local to the layer, NONE = -1) and outer, top, max_depth of the layer
  stack(S)                       S: outlines_ref.stack's dict -> the same with global ids (NONE = 0xFFFFFFFF, as the library has it),
                                 outer, top, max_depth per layer
  children(parent)               -> (child_start, children) by a stable argsort
  component_sizes(P, diagonal)   the sizes of the connected parts of the set pixels of P, by a flood fill; diagonal: 8-connected
  region_sizes(P, connectivity)  -> (sorted sizes of the set parts under `connectivity`, sorted sizes of the clear parts of the padded
                                 image under the dual connectivity, the outside part excluded)"""
import numpy as np

NONE = 0xFFFFFFFF


def vertical_edges(L):
    """per loop the list of (pixel row b, column a) of its vertical unit edges"""
    xy, nxt = L["xy"], L["next"]
    out = []
    for leader, m in zip(L["leader"], L["n_vertices"]):
        edges, v = [], int(leader)
        for _ in range(int(m)):
            w = int(nxt[v])
            (a, b), (a2, b2) = xy[v], xy[w]
            if a == a2:
                edges += [(int(r), int(a)) for r in range(min(b, b2), max(b, b2))]
            v = w
        out.append(edges)
    return out


def layer(L):
    n = len(L["leader"])
    edges = vertical_edges(L)
    rows = {}          # pixel row -> [(column, loop)] of all vertical edges on it
    for e, es in enumerate(edges):
        for b, a in es:
            rows.setdefault(b, []).append((a, e))
    left, parent = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    for l in range(n):
        a0, b0 = (int(x) for x in L["xy"][L["leader"][l]])
        before = [(a, e) for a, e in rows.get(b0, []) if a < a0]
        left[l] = max(before)[1] if before else -1
        count = {}
        for _, e in before:
            count[e] = count.get(e, 0) + 1
        enclosing = [(abs(int(L["area2"][e])), e) for e, c in count.items() if e != l and c % 2 == 1]
        if enclosing:
            assert len({a for a, _ in enclosing}) == len(enclosing)          # nested loops: no two of one size
            parent[l] = min(enclosing)[1]
    depth = np.zeros(n, np.int64)
    for l in range(n):
        p = parent[l]
        while p >= 0:
            depth[l] += 1
            p = parent[p]
    n_children, region = np.zeros(n, np.int64), L["area2"].astype(np.int64).copy()
    for l in range(n):
        if parent[l] >= 0:
            n_children[parent[l]] += 1
            region[parent[l]] += int(L["area2"][l])
    return {"left": left, "parent": parent, "depth": depth, "n_children": n_children, "region_area2": region,
            "outer": int((L["area2"] > 0).sum()), "top": int((parent < 0).sum()), "max_depth": int(depth.max(initial=0))}


def _split(S):
    """outlines_ref.stack's dict -> per layer a dict as outlines_ref.layer's, ids local"""
    vs, ls = S["vertex_start"], S["loop_start"]
    for q in range(len(ls) - 1):
        v0, v1, l0, l1 = int(vs[q]), int(vs[q + 1]), int(ls[q]), int(ls[q + 1])
        yield {"xy": S["xy"][v0:v1], "next": S["next"][v0:v1] - v0, "leader": S["leader"][l0:l1] - v0, "n_vertices": S["n_vertices"][l0:l1], "area2": S["area2"][l0:l1]}


def stack(S):
    ls = S["loop_start"]
    layers = [layer(L) for L in _split(S)]
    out = {"outer": np.array([T["outer"] for T in layers], np.uint64), "top": np.array([T["top"] for T in layers], np.uint64),
           "max_depth": np.array([T["max_depth"] for T in layers], np.uint32)}
    for key in ("left", "parent"):
        out[key] = np.concatenate([np.where(T[key] < 0, NONE, T[key] + int(ls[q])) for q, T in enumerate(layers)] or [np.zeros(0, np.int64)]).astype(np.uint32)
    for key, dtype in (("depth", np.uint32), ("n_children", np.uint32), ("region_area2", np.int64)):
        out[key] = np.concatenate([T[key] for T in layers] or [np.zeros(0, np.int64)]).astype(dtype)
    return out


def children(parent):
    parent = np.asarray(parent, np.uint32)
    n = len(parent)
    has = parent != NONE
    order = np.argsort(parent[has], kind="stable")
    start = np.zeros(n + 1, np.uint64)
    start[1:] = np.cumsum(np.bincount(parent[has].astype(np.int64), minlength=n)[:n])
    return start, np.nonzero(has)[0][order].astype(np.uint32)


def component_sizes(P, diagonal):
    """the sizes of the connected parts of the set pixels, in the order of their first pixels: labels spread to the neighbours'
    minimum until nothing changes"""
    P = np.asarray(P, bool)
    W, H = P.shape
    big = W * H
    lab = np.where(P, np.arange(big).reshape(W, H), big)
    steps = [(1, 0), (-1, 0), (0, 1), (0, -1)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if diagonal else [])
    while True:
        pad = np.pad(lab, 1, constant_values=big)
        new = lab
        for dx, dy in steps:
            new = np.minimum(new, pad[1 + dx:1 + dx + W, 1 + dy:1 + dy + H])
        new = np.where(P, new, big)
        if np.array_equal(new, lab):
            break
        lab = new
    ids, counts = np.unique(lab[P], return_counts=True)
    return ids, counts


def region_sizes(P, connectivity):
    P = np.asarray(P, bool)
    _, fg = component_sizes(P, connectivity == 8)
    ids, bg = component_sizes(~np.pad(P, 1), connectivity == 4)
    return np.sort(fg), np.sort(bg[ids != 0])          # (the padded image's pixel (0, 0) is clear and outside: its part has label 0)
