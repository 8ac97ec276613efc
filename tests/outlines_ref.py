"""The outlines of a voxel bitmap's layers (fhip_voxels_outlines, include/fidget_hip.h) restated with numpy and dicts, the long way round:
the directed unit edges of a layer image are built pixel by pixel, walked edge after edge into closed loops - where a corner offers
two exits, the walk turns left (connectivity 4) or right (connectivity 8) - collinear points are dropped, and only then are the
remaining vertices numbered, by sorting (b, a, outgoing heading).  No table of corner masks.

  layer(P, connectivity)              P bool [N, N] indexed [i, j] -> dict: xy int [n, 2], next [n], loop_of [n], leader, n_vertices,
                                      area2, perimeter, lo, hi per loop (ids local to the layer)
  stack(inside, k0, k1, connectivity) inside bool [N, N, N] indexed [i, j, k] -> dict with global ids: vertex_start, loop_start,
                                      layer_area2, layer_perimeter and the arrays above
  boundary_edges(P)                   the unit boundary edges of the image, counted by != on the padded image

Headings: 0 = -x, 1 = +x, 2 = -y, 3 = +y."""
import numpy as np

STEP = {0: (-1, 0), 1: (1, 0), 2: (0, -1), 3: (0, 1)}
LEFT = {1: 3, 3: 0, 0: 2, 2: 1}          # +x turns left to +y, +y to -x, -x to -y, -y to +x
RIGHT = {v: k for k, v in LEFT.items()}


def directed_edges(P):
    """{(a, b): [headings that leave the corner]}: the sides of the set pixels that face a clear pixel, inside on the left"""
    P = np.asarray(P, bool)
    N = P.shape[0]
    leaving = {}
    if not P.any():
        return leaving
    Q = np.zeros((N + 2, N + 2), bool)
    Q[1:-1, 1:-1] = P
    for i, j in zip(*np.nonzero(P)):
        i, j = int(i), int(j)
        if not Q[i + 1, j]:          # the pixel below is clear: the bottom side runs +x
            leaving.setdefault((i, j), []).append(1)
        if not Q[i + 1, j + 2]:      # above: the top side runs -x
            leaving.setdefault((i + 1, j + 1), []).append(0)
        if not Q[i + 2, j + 1]:      # to the right: the right side runs +y
            leaving.setdefault((i + 1, j), []).append(3)
        if not Q[i, j + 1]:          # to the left: the left side runs -y
            leaving.setdefault((i, j + 1), []).append(2)
    return leaving


def walk(P, connectivity):
    """the closed loops as lists of (a, b, incoming heading, outgoing heading) at the corners where the two differ"""
    assert connectivity in (4, 8)
    turn = LEFT if connectivity == 4 else RIGHT
    leaving = directed_edges(P)
    used = set()
    loops = []
    for start in sorted(leaving):
        for h0 in sorted(leaving[start]):
            if (start, h0) in used:
                continue
            corners, at, h = [], start, h0
            while True:
                used.add((at, h))
                nxt = (at[0] + STEP[h][0], at[1] + STEP[h][1])
                exits = leaving[nxt]
                if len(exits) == 1:
                    g = exits[0]
                else:
                    assert sorted(exits) in ([0, 1], [2, 3]) and turn[h] in exits
                    g = turn[h]
                if g != h:
                    corners.append((nxt[0], nxt[1], h, g))
                at, h = nxt, g
                if (at, h) == (start, h0):
                    break
            loops.append(corners)
    assert len(used) == sum(len(v) for v in leaving.values())
    return loops


def layer(P, connectivity):
    loops = walk(P, connectivity)
    verts = sorted((b, a, g) for loop in loops for a, b, _, g in loop)
    ident = {v: n for n, v in enumerate(verts)}
    assert len(ident) == len(verts)
    n = len(verts)
    xy = np.array([(a, b) for b, a, _ in verts], np.int64).reshape(n, 2)
    nxt = np.zeros(n, np.int64)
    rows = []
    for loop in loops:
        ids = [ident[(b, a, g)] for a, b, _, g in loop]
        for v, w in zip(ids, ids[1:] + ids[:1]):
            nxt[v] = w
        rows.append((min(ids), ids))
    rows.sort()
    loop_of = np.zeros(n, np.int64)
    table = {key: [] for key in ("leader", "n_vertices", "area2", "perimeter", "lo", "hi")}
    for q, (leader, ids) in enumerate(rows):
        loop_of[ids] = q
        p, s = xy[ids], xy[nxt[ids]]
        table["leader"].append(leader)
        table["n_vertices"].append(len(ids))
        table["area2"].append(int((p[:, 0] * s[:, 1] - s[:, 0] * p[:, 1]).sum()))
        table["perimeter"].append(int(np.abs(s - p).sum()))
        table["lo"].append(p.min(axis=0))
        table["hi"].append(p.max(axis=0))
    out = {"xy": xy, "next": nxt, "loop_of": loop_of}
    for key, v in table.items():
        out[key] = np.array(v, np.int64).reshape((len(rows), 2) if key in ("lo", "hi") else (len(rows),))
    return out


def stack(inside, k0, k1, connectivity):
    inside = np.asarray(inside, bool)
    layers = [layer(inside[:, :, k], connectivity) for k in range(k0, k1)]
    K = len(layers)
    vertex_start = np.zeros(K + 1, np.int64)
    loop_start = np.zeros(K + 1, np.int64)
    for q, L in enumerate(layers):
        vertex_start[q + 1] = vertex_start[q] + len(L["next"])
        loop_start[q + 1] = loop_start[q] + len(L["leader"])
    cat = lambda key, add=None: np.concatenate([L[key] + (0 if add is None else add[q]) for q, L in enumerate(layers)] or [np.zeros(0, np.int64)])          # noqa: E731
    out = {"vertex_start": vertex_start, "loop_start": loop_start,
           "layer_area2": np.array([int(L["area2"].sum()) for L in layers], np.int64), "layer_perimeter": np.array([int(L["perimeter"].sum()) for L in layers], np.int64),
           "xy": np.concatenate([L["xy"] for L in layers] or [np.zeros((0, 2), np.int64)]), "next": cat("next", vertex_start), "loop_of": cat("loop_of", loop_start),
           "leader": cat("leader", vertex_start), "n_vertices": cat("n_vertices"), "area2": cat("area2"), "perimeter": cat("perimeter"),
           "lo": np.concatenate([L["lo"] for L in layers] or [np.zeros((0, 2), np.int64)]), "hi": np.concatenate([L["hi"] for L in layers] or [np.zeros((0, 2), np.int64)])}
    return out


def boundary_edges(P):
    P = np.asarray(P, bool)
    N = P.shape[0]
    Q = np.zeros((N + 2, N + 2), bool)
    Q[1:-1, 1:-1] = P
    return int((Q[1:] != Q[:-1]).sum() + (Q[:, 1:] != Q[:, :-1]).sum())
