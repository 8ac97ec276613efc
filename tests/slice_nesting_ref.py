"""The nesting of a mesh's slices (fhip_slices_nesting) restated from the definition in include/fidget_hip.h and not from the kernels: no
bands, no hit lists.  For each leader and each other regular loop of its plane the loop's polygon is walked and its hit segments are
counted with the same binary64 operations in numpy; depth, parent, improper, misoriented, children and regions follow by plain Python
over sets.  `hits_exact` evaluates the same test with fractions.Fraction: on coordinates that are dyadic with few bits the binary64
sequence is exact, and the two must agree (`check_exact`).

The input is a slices result - tests/mesh_slices_ref.py's dict, or `from_device` of a `MeshSlices` - of which xy, next and the loops'
leader, plane, crossings, irregular and area2 are read."""
from fractions import Fraction

import numpy as np

NONE = 0xFFFFFFFF
PLANE_COUNTS = ("regular", "outer", "top", "max_depth", "improper", "misoriented")


def from_device(ms):
    """a fidget_amd.MeshSlices as the dict this module reads"""
    return {"counts": {"planes": ms.counts["planes"], "loops": ms.counts["loops"]}, "xy": ms.xy, "next": ms.next, "loops": ms.loops}


def walk(res, l):
    """the crossing ids of regular loop l from its leader on"""
    L = res["loops"]
    ids, v = [], int(L["leader"][l])
    for _ in range(int(L["crossings"][l])):
        ids.append(v)
        v = int(res["next"][v])
    assert v == int(L["leader"][l]), "a regular loop closes"
    return np.array(ids, np.int64)


def hits(q, s, d):
    """q float32 [2]; s, d float32 [m, 2], the segments s -> d: which are hit, by the header's operations one by one"""
    q, s, d = np.asarray(q, np.float32), np.asarray(s, np.float32).reshape(-1, 2), np.asarray(d, np.float32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        up = s[:, 1] <= q[1]
        straddles = up != (d[:, 1] <= q[1])
        q64, s64, d64 = q.astype(np.float64), s.astype(np.float64), d.astype(np.float64)
        ax, ay = d64[:, 0] - s64[:, 0], q64[1] - s64[:, 1]
        bx, by = q64[0] - s64[:, 0], d64[:, 1] - s64[:, 1]
        a, b = ax * ay, bx * by
        c = a - b
    return straddles & np.where(up, c < 0, c > 0)


def hits_exact(q, s, d):
    """the same in exact rational arithmetic"""
    out = []
    qx, qy = Fraction(float(q[0])), Fraction(float(q[1]))
    for (sx, sy), (dx, dy) in zip(np.asarray(s, np.float32).reshape(-1, 2).tolist(), np.asarray(d, np.float32).reshape(-1, 2).tolist()):
        sx, sy, dx, dy = Fraction(sx), Fraction(sy), Fraction(dx), Fraction(dy)
        up = sy <= qy
        if up == (dy <= qy):
            out.append(False)
            continue
        c = (dx - sx) * (qy - sy) - (qx - sx) * (dy - sy)
        out.append(c < 0 if up else c > 0)
    return np.array(out, bool)


def hit_counts(res, count=hits):
    """{l: {m: the number of m's segments that l's leader hits}} over the regular loops of each plane, zero counts included"""
    L, xy = res["loops"], np.asarray(res["xy"], np.float32).reshape(-1, 2)
    regular = [l for l in range(len(L["leader"])) if L["irregular"][l] == 0]
    out = {}
    for p in sorted({int(L["plane"][l]) for l in regular}):
        loops = [l for l in regular if L["plane"][l] == p]
        polys = [walk(res, l) for l in loops]
        # the plane's polygons one after the other: the segments' ends, and for each the place of its loop among `loops`
        s = xy[np.concatenate(polys)]
        d = xy[np.concatenate([np.roll(ids, -1) for ids in polys])]
        owner = np.concatenate([np.full(len(ids), k, np.int64) for k, ids in enumerate(polys)])
        for k, l in enumerate(loops):
            hit = count(xy[int(L["leader"][l])], s, d) & (owner != k)
            per_loop = np.bincount(owner[hit], minlength=len(loops))
            out[l] = {m: int(per_loop[j]) for j, m in enumerate(loops) if m != l}
    return out


def nesting(res, counts=None):
    """-> dict: parent, depth, n_children uint32 [L]; region_area2 float64 [L]; contains: {l: set}; per_plane {regular, outer, top,
    max_depth, improper, misoriented} uint64 [P]; the totals n_regular ...; `hit_counts` as given or computed"""
    P, L = int(res["counts"]["planes"]), res["loops"]
    n = len(L["leader"])
    counts = hit_counts(res) if counts is None else counts
    contains = {l: {m for m, k in row.items() if k % 2 == 1} for l, row in counts.items()}
    depth = np.full(n, NONE, np.uint32)
    for l, c in contains.items():
        depth[l] = len(c)
    parent = np.full(n, NONE, np.uint32)
    for l, c in contains.items():
        if c:
            parent[l] = min(c, key=lambda m: (-int(depth[m]), m))
    per_plane = {k: np.zeros(P, np.uint64) for k in PLANE_COUNTS}
    n_children = np.zeros(n, np.uint32)
    children = {l: [] for l in range(n)}
    for l in sorted(contains):
        p, d = int(L["plane"][l]), int(depth[l])
        per_plane["regular"][p] += 1
        per_plane["outer"][p] += d % 2 == 0
        per_plane["top"][p] += parent[l] == NONE
        per_plane["max_depth"][p] = max(int(per_plane["max_depth"][p]), d)
        if parent[l] != NONE:
            n_children[parent[l]] += 1
            children[int(parent[l])].append(l)
            per_plane["improper"][p] += int(depth[parent[l]]) != d - 1
        per_plane["misoriented"][p] += (d % 2 == 0) != bool(L["area2"][l] > 0)
    region = np.zeros(n, np.float64)
    for l in contains:
        total = np.float64(L["area2"][l])
        for c in children[l]:          # (ascending)
            total = total + np.float64(L["area2"][c])
        region[l] = total
    out = {"parent": parent, "depth": depth, "n_children": n_children, "region_area2": region, "contains": contains, "children": children, "per_plane": per_plane,
           "hit_counts": counts, "n_loops": n}
    for k in PLANE_COUNTS:
        out["n_" + k if k != "max_depth" else k] = int(per_plane[k].max()) if k == "max_depth" and P else int(per_plane[k].sum())
    return out


def regions(res, nest, p):
    """plane p's [(outer id, [hole ids])]: the regular loops of even depth, ascending, with their children"""
    L = res["loops"]
    return [(l, list(nest["children"][l])) for l in sorted(nest["contains"]) if L["plane"][l] == p and nest["depth"][l] % 2 == 0]


def check_exact(res):
    """on dyadic coordinates of few bits: the binary64 hit counts are the exact ones -> them"""
    a, b = hit_counts(res), hit_counts(res, hits_exact)
    assert a == b, "the binary64 predicate disagrees with exact arithmetic"
    return a
