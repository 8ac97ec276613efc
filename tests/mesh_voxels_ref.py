"""The solid voxelization of a triangle mesh (fhip_triangles_voxels, fhip_mesh_voxels; include/fidget_hip.h) restated in numpy on the
unpacked grid inside[i, j, k]: per triangle vectorised over the columns of its box, in int64, with a scalar variant in Python's
unbounded integers for the extremes - none of the bricks' bit arithmetic, so that the two check each other.

  snap      w = ((m0 x + m1 y) + m2 z) + m3 in float64; q = rint(w 128 N + 128 N): voxel i has its centre at 256 i + 128
  rejected  a coordinate w not finite or outside [-1.5, 1.5], or an index at or beyond the vertices
  flat      D = (b.y - a.y)(c.z - a.z) - (b.z - a.z)(c.y - a.y) == 0; D < 0 swaps b and c
  cover     P = (256 j + 128, 256 k + 128); e = (r.y - p.y)(P.z - p.z) - (r.z - p.z)(P.y - p.y) for b -> c, c -> a, a -> b; every e > 0, or
            e == 0 and dy > 0, or e == 0 and dy == 0 and dz < 0
  crossing  i* = ceil((num - (128 - xmin) D) / (256 D)), num = the e-weighted sum of x - xmin; <= 0: voxel 0; >= N: the exit plane
  fill      inside = the running XOR of the toggles along i; open_rows = the columns where inside(N - 1) differs from the exit plane
"""
import numpy as np

INFO = ("triangles", "rejected", "flat", "crossings", "clipped", "open_rows", "set_voxels", "W")


def world(vertices, mesh_to_world=None):
    """float32 [..., 3] -> float64 [..., 3], the matrix's rows applied in the stated order"""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    if mesh_to_world is None:
        return v
    m = np.asarray(mesh_to_world, np.float64).reshape(-1)[:12].reshape(3, 4)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], axis=-1)


def snap(w, N):
    """float64 in [-1.5, 1.5] -> int64 lattice units (np.rint rounds to nearest-even)"""
    return np.rint(w * (128.0 * N) + 128.0 * N).astype(np.int64)


def corners(vertices, triangles, N, mesh_to_world=None):
    """-> (q int64 [T, 3, 3], rejected bool [T]); q is 0 where rejected.  `triangles` None: a soup."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    if triangles is None:
        T = len(vertices) // 3
        idx = np.arange(3 * T, dtype=np.uint64).reshape(T, 3)
    else:
        idx = np.asarray(triangles, np.uint64).reshape(-1, 3)
    bad_index = idx >= np.uint64(len(vertices))
    safe = np.where(bad_index, np.uint64(0), idx).astype(np.int64)          # (a bad index is not read: vertex 0 stands in, if there is one)
    if len(vertices) == 0:
        return np.zeros((len(idx), 3, 3), np.int64), np.ones(len(idx), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        w = world(vertices, mesh_to_world)[safe]          # [T, 3, 3]
        ok = np.isfinite(w) & (w >= -1.5) & (w <= 1.5)
    rejected = bad_index.any(axis=1) | ~ok.all(axis=(1, 2))
    q = snap(np.where(ok, w, 0.0), N)
    q[rejected] = 0
    return q, rejected


def oriented(a, b, c):
    """-> (a, b, c, D) with D >= 0; integers of any kind"""
    D = (b[1] - a[1]) * (c[2] - a[2]) - (b[2] - a[2]) * (c[1] - a[1])
    return (a, c, b, -D) if D < 0 else (a, b, c, D)


def column_box(a, b, c, N):
    """the columns whose centres lie within the triangle's yz box, clipped to the grid: (j0, j1, k0, k1), inclusive; j1 < j0: none"""
    out = []
    for axis in (1, 2):
        lo, hi = min(a[axis], b[axis], c[axis]), max(a[axis], b[axis], c[axis])
        out += [max(-((-(lo - 128)) // 256), 0), min((hi - 128) // 256, N - 1)]
    return out


def _owns(p, r):
    dy, dz = r[1] - p[1], r[2] - p[2]
    return dy > 0 or (dy == 0 and dz < 0)


def crossing_scalar(tri, N, j, k):
    """One column against one triangle in Python's integers: tri = three corners of three ints -> None where the column is not covered
    (or the triangle flat), else the voxel the crossing toggles, 0 .. N - 1, or N for the exit plane"""
    a, b, c = ([int(x) for x in p] for p in tri)
    a, b, c, D = oriented(a, b, c)
    if D == 0:
        return None
    py, pz = 256 * j + 128, 256 * k + 128
    ws = []
    for p, r in ((b, c), (c, a), (a, b)):
        e = (r[1] - p[1]) * (pz - p[2]) - (r[2] - p[2]) * (py - p[1])
        if not (e > 0 or (e == 0 and _owns(p, r))):
            return None
        ws.append(e)
    assert sum(ws) == D
    xmin = min(a[0], b[0], c[0])
    num = ws[0] * (a[0] - xmin) + ws[1] * (b[0] - xmin) + ws[2] * (c[0] - xmin)
    t, den = num - (128 - xmin) * D, 256 * D
    istar = -((-t) // den)          # the exact quotient, rounded up
    return 0 if istar <= 0 else (N if istar >= N else istar)


def voxelize(vertices, triangles, N, mesh_to_world=None):
    """-> (inside bool [N, N, N] indexed [i, j, k], info dict)"""
    q, rejected = corners(vertices, triangles, N, mesh_to_world)
    toggles = np.zeros((N, N, N), bool)
    exit_plane = np.zeros((N, N), bool)
    info = dict.fromkeys(INFO, 0)
    info["triangles"], info["rejected"] = len(q), int(rejected.sum())
    for t in np.flatnonzero(~rejected):
        a, b, c, D = oriented(*[[int(x) for x in p] for p in q[t]])
        if D == 0:
            info["flat"] += 1
            continue
        j0, j1, k0, k1 = column_box(a, b, c, N)
        if j1 < j0 or k1 < k0:
            continue
        info["W"] += (j1 - j0 + 1) * (k1 - k0 + 1)
        J, K = np.meshgrid(np.arange(j0, j1 + 1, dtype=np.int64), np.arange(k0, k1 + 1, dtype=np.int64), indexing="ij")
        py, pz = 256 * J + 128, 256 * K + 128
        covered = np.ones(J.shape, bool)
        ws = []
        for p, r in ((b, c), (c, a), (a, b)):
            e = (r[1] - p[1]) * (pz - p[2]) - (r[2] - p[2]) * (py - p[1])
            covered &= (e > 0) | ((e == 0) & _owns(p, r))
            ws.append(e)
        xmin = min(a[0], b[0], c[0])
        num = ws[0] * (a[0] - xmin) + ws[1] * (b[0] - xmin) + ws[2] * (c[0] - xmin)
        istar = -((-(num - (128 - xmin) * D)) // (256 * D))          # (numpy's // floors, as Python's does)
        jc, kc, ic = J[covered], K[covered], istar[covered]
        info["crossings"] += len(ic)
        out = ic >= N
        info["clipped"] += int(out.sum())
        np.logical_xor.at(exit_plane, (jc[out], kc[out]), True)
        np.logical_xor.at(toggles, (np.maximum(ic[~out], 0), jc[~out], kc[~out]), True)
    inside = np.logical_xor.accumulate(toggles, axis=0)
    info["open_rows"] = int((inside[N - 1] ^ exit_plane).sum())
    info["set_voxels"] = int(inside.sum())
    return inside, info


def soup(vertices, triangles):
    """indexed -> float32 [T, 3, 3]"""
    return np.asarray(vertices, np.float32).reshape(-1, 3)[np.asarray(triangles, np.int64).reshape(-1, 3)]
