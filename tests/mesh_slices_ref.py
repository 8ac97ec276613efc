"""The slices of a triangle mesh (fhip_topology_slices) restated in plain numpy and dicts, from the definition in include/fidget_hip.h
and not from the kernels: the levels by np.searchsorted, the crossing edges in a dict ordered by their first corners, the positions
in float64 operation by operation, the segments triangle by triangle, the loops by a union-find, area2 by math.fsum.  The weld and the
triangle order are mesh_topology_ref.topology's.  No hash table, no atomics, no order of arrival."""
import math

import numpy as np

import mesh_topology_ref as MT

NONE = 0xFFFFFFFF
COUNTS = ("planes", "vertices", "segments", "loops", "irregular")


def planes_ok(zs):
    zs = np.asarray(zs, np.float32)
    return bool(np.isfinite(zs).all() and (zs[1:] > zs[:-1]).all())


def slices(vertices, triangles, zs):
    """the indexed mesh as a Topology holds it (vertices [V, 3] float32, triangles [T, 3]) under the planes zs -> dict: counts; per plane
    `per_plane` {crossings, segments, loops}; per crossing xy (float32), plane, edge, next, loop_of, degree, out, in; per segment
    `segments` [m, 2], `segment_triangle`, `terms` (float64); per loop `loops` {leader, plane, crossings, segments, irregular, area2,
    area2_abs, lo, hi}"""
    vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    zs = np.ascontiguousarray(zs, np.float32).reshape(-1)
    if not planes_ok(zs):
        raise ValueError("the planes must be finite and strictly ascending")
    P, T = len(zs), len(tri)
    a = np.searchsorted(zs, vertices[:, 2], side="right").astype(np.int64) if len(vertices) else np.zeros(0, np.int64)
    flat = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])
    # crossings: the crossing edges by their first corners, each edge's planes ascending
    first = {}
    for t in range(T):
        if flat[t]:
            continue
        for k in range(3):
            u, v = int(tri[t, k]), int(tri[t, (k + 1) % 3])
            if a[u] != a[v]:
                first.setdefault((min(u, v), max(u, v)), 3 * t + k)
    base, plane, edge = {}, [], []
    for (u, v), _ in sorted(first.items(), key=lambda item: item[1]):
        base[(u, v)] = len(plane)
        for p in range(min(a[u], a[v]), max(a[u], a[v])):
            plane.append(p)
            edge.append((u, v))
    n = len(plane)
    plane, edge = np.array(plane, np.uint32), np.array(edge, np.uint32).reshape(n, 2)
    pu, pv = vertices[edge[:, 0].astype(np.int64)].astype(np.float64), vertices[edge[:, 1].astype(np.int64)].astype(np.float64)
    zp = zs[plane.astype(np.int64)].astype(np.float64)
    with np.errstate(all="ignore"):
        tt = (zp - pu[:, 2]) / (pv[:, 2] - pu[:, 2])
        xy = np.stack([pu[:, 0] + tt * (pv[:, 0] - pu[:, 0]), pu[:, 1] + tt * (pv[:, 1] - pu[:, 1])], axis=1).astype(np.float32)
    # segments: triangle by triangle, plane by plane
    seg, seg_tri = [], []

    def crossing(t, k, p):
        u, v = int(tri[t, k]), int(tri[t, (k + 1) % 3])
        return base[(min(u, v), max(u, v))] + p - min(a[u], a[v])
    for t in range(T):
        if flat[t]:
            continue
        lv = a[tri[t]]
        for p in range(lv.min(), lv.max()):
            above = lv > p
            lone = [k for k in range(3) if above[k] != above[(k + 1) % 3] and above[k] != above[(k + 2) % 3]][0]
            ab, ca = crossing(t, lone, p), crossing(t, (lone + 2) % 3, p)
            seg.append((ab, ca) if above[lone] else (ca, ab))
            seg_tri.append(t)
    m = len(seg)
    seg = np.array(seg, np.uint32).reshape(m, 2)
    out_n, in_n, nxt = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, NONE, np.uint32)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for s, d in seg.tolist():          # (triangles ascend: the first segment to leave a crossing is the smallest triangle's)
        out_n[s] += 1
        in_n[d] += 1
        if nxt[s] == NONE:
            nxt[s] = d
        ra, rb = find(s), find(d)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(x) for x in range(n)], np.int64)
    leaders = np.unique(roots)
    loop_of = np.searchsorted(leaders, roots).astype(np.uint32)
    L = len(leaders)
    irregular = (out_n != 1) | (in_n != 1)
    src, dst = xy[seg[:, 0].astype(np.int64)].astype(np.float64), xy[seg[:, 1].astype(np.int64)].astype(np.float64)
    terms = src[:, 0] * dst[:, 1] - dst[:, 0] * src[:, 1]
    seg_loop = loop_of[seg[:, 0].astype(np.int64)]
    canon = xy + np.float32(0.0)
    members = [np.flatnonzero(loop_of == q) for q in range(L)]
    of_loop = [np.flatnonzero(seg_loop == q) for q in range(L)]
    loops = {
        "leader": leaders.astype(np.uint32), "plane": plane[leaders] if L else np.zeros(0, np.uint32),
        "crossings": np.array([len(x) for x in members], np.uint32), "segments": np.array([len(x) for x in of_loop], np.uint32),
        "irregular": np.array([int(irregular[x].sum()) for x in members], np.uint32),
        "area2": np.array([math.fsum(terms[x]) for x in of_loop], np.float64), "area2_abs": np.array([math.fsum(np.abs(terms[x])) for x in of_loop], np.float64),
        "lo": np.array([canon[x].min(axis=0) for x in members], np.float32).reshape(L, 2), "hi": np.array([canon[x].max(axis=0) for x in members], np.float32).reshape(L, 2)}
    per_plane = {"crossings": np.bincount(plane.astype(np.int64), minlength=P).astype(np.uint64),
                 "segments": np.bincount(plane[seg[:, 0].astype(np.int64)].astype(np.int64), minlength=P).astype(np.uint64),
                 "loops": np.bincount(loops["plane"].astype(np.int64), minlength=P).astype(np.uint64)}
    degree = (np.minimum(out_n, 15) | (np.minimum(in_n, 15) << 4)).astype(np.uint8)
    return {"counts": dict(zip(COUNTS, (P, n, m, L, int(irregular.sum())))), "zs": zs, "per_plane": per_plane, "xy": xy, "plane": plane, "edge": edge, "next": nxt,
            "loop_of": loop_of, "degree": degree, "out": out_n, "in": in_n, "segments": seg, "segment_triangle": np.array(seg_tri, np.uint32), "terms": terms, "loops": loops}


def mesh_slices(mesh_vertices, mesh_triangles, zs, weld=None):
    """as the library's mesh_slices: mesh_topology_ref.topology first, then the slices of its indexed mesh"""
    topo = MT.topology(mesh_vertices, mesh_triangles, weld)
    assert topo["counts"]["rejected"] == 0
    return slices(topo["vertices"], topo["triangles"], zs)


def plane_area2(res):
    """per plane the sum of all segments' terms (fsum): twice the area of the cross-section of a closed mesh"""
    P = res["counts"]["planes"]
    p_of = res["plane"][res["segments"][:, 0].astype(np.int64)]
    return np.array([math.fsum(res["terms"][p_of == p]) for p in range(P)], np.float64)


def polygons(res, p):
    """-> (the closed loops of plane p as float32 [n, 2] from their leaders on along `next`, the number of loops left out)"""
    out, skipped = [], 0
    L = res["loops"]
    for q in np.flatnonzero(L["plane"] == p):
        if L["irregular"][q]:
            skipped += 1
            continue
        ids, v = [], int(L["leader"][q])
        for _ in range(int(L["crossings"][q])):
            ids.append(v)
            v = int(res["next"][v])
        assert v == int(L["leader"][q])
        out.append(res["xy"][ids])
    return out, skipped
