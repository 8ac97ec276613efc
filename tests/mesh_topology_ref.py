"""The check of a triangle mesh (fhip_triangles_topology) restated in plain numpy and dicts, from the definitions in
include/fidget_hip.h and not from the kernels: vertices by np.unique on the canonical bits, ranked by first index; edges in a dict;
shells by a union-find over the first triangles; the float sums by math.fsum over terms computed in the stated order of operations.
No hash table, no atomics, no order of arrival."""
import math

import numpy as np

COUNTS = ("triangles", "rejected", "degenerate", "vertices", "edges", "boundary", "flipped", "nonmanifold", "unbalanced", "shells")
KINDS = ("boundary", "flipped", "nonmanifold", "unbalanced")
NO_SHELL = 0xFFFFFFFF


def canonical(v):
    """float32 -> the bits after x + 0.0f: -0 becomes +0"""
    return (np.asarray(v, np.float32) + np.float32(0.0)).view(np.uint32)


def edge_classes(f, r):
    return {"boundary": f + r == 1, "flipped": f + r == 2 and f != r, "nonmanifold": f + r >= 3, "unbalanced": f != r}


def terms(vertices, triangles):
    """per triangle (volume6 term, area2 term), float64, in the order of operations the header states"""
    a, b, c = (vertices[triangles[:, k].astype(np.int64)].astype(np.float64) for k in range(3))
    x, y, z = 0, 1, 2
    n = (b[:, y] * c[:, z] - b[:, z] * c[:, y], b[:, z] * c[:, x] - b[:, x] * c[:, z], b[:, x] * c[:, y] - b[:, y] * c[:, x])
    vol = (a[:, x] * n[0] + a[:, y] * n[1]) + a[:, z] * n[2]
    u, v = b - a, c - a
    m = (u[:, y] * v[:, z] - u[:, z] * v[:, y], u[:, z] * v[:, x] - u[:, x] * v[:, z], u[:, x] * v[:, y] - u[:, y] * v[:, x])
    area = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    return vol, area


def topology(vertices, triangles=None, weld=None):
    """-> dict: counts; and, unless a triangle was rejected, vertices, triangles, triangle_shell, shells (a dict of arrays; volume6
    and area2 by fsum, volume6_abs and area2_abs the sums of the terms' magnitudes), edges (kind -> [n, 2] uint32), volume6_terms,
    area2_terms (per triangle)"""
    vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    soup = triangles is None
    weld = soup if weld is None else bool(weld)
    assert weld or not soup
    if soup:
        T = len(vertices) // 3
        index = np.arange(3 * T, dtype=np.uint64).reshape(T, 3)
    else:
        index = np.asarray(triangles, np.uint64).reshape(-1, 3)
        T = len(index)
    counts = dict.fromkeys(COUNTS, 0)
    counts["triangles"] = T
    beyond = index >= len(vertices)
    safe = np.where(beyond, 0, index).astype(np.int64)
    finite = np.isfinite(vertices).all(axis=1)[safe] if len(vertices) else np.zeros(index.shape, bool)
    counts["rejected"] = int((beyond | ~finite).any(axis=1).sum())
    if counts["rejected"]:
        return {"counts": counts}
    # vertices
    if weld:
        corners = vertices[safe.reshape(-1)]
        _, first, inverse = np.unique(canonical(corners), axis=0, return_index=True, return_inverse=True)
        rank = np.empty(len(first), np.int64)
        rank[np.argsort(first)] = np.arange(len(first))          # the welded vertices in the order of their first corners
        vid = rank[inverse.reshape(-1)].reshape(T, 3)
        out_vertices = corners[np.sort(first)]
        counts["vertices"] = len(first)
    else:
        vid = safe
        out_vertices = vertices
        counts["vertices"] = len(np.unique(vid))
    out_triangles = vid.astype(np.uint64)
    # edges
    flat = (vid[:, 0] == vid[:, 1]) | (vid[:, 1] == vid[:, 2]) | (vid[:, 0] == vid[:, 2])
    counts["degenerate"] = int(flat.sum())
    edges = {}          # (a, b) -> [f, r, first corner]
    for t in range(T):
        if flat[t]:
            continue
        for k in range(3):
            p, q = int(vid[t, k]), int(vid[t, (k + 1) % 3])
            e = edges.setdefault((min(p, q), max(p, q)), [0, 0, 3 * t + k])
            e[0 if p < q else 1] += 1
    counts["edges"] = len(edges)
    lists = {kind: [] for kind in KINDS}
    for (a, b), (f, r, c) in sorted(edges.items(), key=lambda item: item[1][2]):
        for kind, is_one in edge_classes(f, r).items():
            if is_one:
                lists[kind].append((a, b))
    for kind in KINDS:
        counts[kind] = len(lists[kind])
    # shells: every triangle with the first triangle of each of its edges
    parent = list(range(T))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for t in range(T):
        if flat[t]:
            continue
        for k in range(3):
            p, q = int(vid[t, k]), int(vid[t, (k + 1) % 3])
            a, b = find(t), find(edges[(min(p, q), max(p, q))][2] // 3)
            if a != b:
                parent[max(a, b)] = min(a, b)
    number, shell = {}, np.full(T, NO_SHELL, np.uint32)
    for t in range(T):          # (the root is the smallest triangle: met first)
        if not flat[t]:
            shell[t] = number.setdefault(find(t), len(number))
    S = len(number)
    counts["shells"] = S
    vol, area = terms(out_vertices, out_triangles) if T else (np.zeros(0), np.zeros(0))
    members = [np.flatnonzero(shell == s) for s in range(S)]
    canon_vertices = out_vertices + np.float32(0.0)
    unbalanced = np.zeros(S, np.uint64)
    for (a, b), (f, r, c) in edges.items():
        if f != r:
            unbalanced[shell[c // 3]] += 1
    shells = {
        "triangles": np.array([len(m) for m in members], np.uint64), "first": np.array([m[0] for m in members], np.uint32), "unbalanced": unbalanced,
        "lo": np.array([canon_vertices[vid[m].reshape(-1)].min(axis=0) for m in members], np.float32).reshape(S, 3),
        "hi": np.array([canon_vertices[vid[m].reshape(-1)].max(axis=0) for m in members], np.float32).reshape(S, 3),
        "volume6": np.array([math.fsum(vol[m]) for m in members], np.float64), "area2": np.array([math.fsum(area[m]) for m in members], np.float64),
        "volume6_abs": np.array([math.fsum(np.abs(vol[m])) for m in members], np.float64), "area2_abs": np.array([math.fsum(np.abs(area[m])) for m in members], np.float64)}
    return {"counts": counts, "vertices": out_vertices, "triangles": out_triangles, "triangle_shell": shell, "shells": shells,
            "edges": {kind: np.array(lists[kind], np.uint32).reshape(-1, 2) for kind in KINDS}, "volume6_terms": vol, "area2_terms": area}


def closed(res):
    return res["counts"]["unbalanced"] == 0


def manifold(res):
    return res["counts"]["boundary"] == res["counts"]["flipped"] == res["counts"]["nonmanifold"] == 0


def euler(res):
    c = res["counts"]
    return c["vertices"] - c["edges"] + c["triangles"] - c["degenerate"]
