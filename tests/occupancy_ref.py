"""Shape occupancy (fhip_shape_occupancy, include/fidget_hip.h) restated in numpy over the CPU oracle, three ways:

  brute_force   every one of the N^3 voxel centres through the oracle's f32 bulk evaluator;
  recursion     the octree the definition names: interval evaluation per cell (midpoint splitting in f32, cell.rs:184-194), a cell with
                hi < 0 all inside, one with lo > 0 all outside, the ambiguous cells of the last level sampled at their 4 x 4 x 4 voxels;
  box_sums      the closed forms of a Full cell, in Python integers.

Both of the first return the [N, N, N] bool array `inside[i, j, k]`; `sums` turns one into the integers of the result struct.  Voxel i is
sampled at c(i) = float32(2 i + 1 - N) * float32(1 / N); a matrix other than the identity is applied in f32, operation for operation as
dev_ops.hpp's xf_point / xf_interval do (the library is built without contraction, numpy rounds every operation to f32)."""
import numpy as np

F32 = np.float32


def centres(N):
    return (2 * np.arange(N, dtype=np.int64) + 1 - N).astype(F32) * (F32(1.0) / F32(N))


def _matrix(w2m):
    if w2m is None:
        return None
    m = np.ascontiguousarray(w2m, F32).reshape(4, 4)
    return None if (m == np.eye(4, dtype=F32)).all() else m       # (octree.rs:487-492: no transform at all for the identity)


def xf_points(m, x, y, z):
    """nalgebra transform_point in f32 (xf_point): rows of ((m0 x + m1 y) + m2 z) + m3, divided by the fourth where that is not 0"""
    r = [((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3] for i in range(4)]
    nz = r[3] != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        return tuple(np.where(nz, r[i] / r[3], r[i]).astype(F32) for i in range(3))


def _iv_mul_f(a, r):
    if np.isnan(a[0]) or np.isnan(a[1]) or np.isnan(r):
        return (F32(np.nan), F32(np.nan))
    return (a[1] * r, a[0] * r) if r < 0 else (a[0] * r, a[1] * r)


def _iv_div(a, b):
    if np.isnan(a[0]) or np.isnan(a[1]) or not (b[0] > 0 or b[1] < 0):
        return (F32(np.nan), F32(np.nan))
    q = [a[0] / b[0], a[0] / b[1], a[1] / b[0], a[1] / b[1]]
    return (min(q), max(q))


def xf_interval(m, X, Y, Z):
    """xf_interval: the same rows in interval arithmetic (types/interval.rs), every bound rounded to f32"""
    r = []
    for i in range(4):
        a, b, c = _iv_mul_f(X, m[i, 0]), _iv_mul_f(Y, m[i, 1]), _iv_mul_f(Z, m[i, 2])
        lo = ((a[0] + b[0]) + c[0]) + m[i, 3]
        hi = ((a[1] + b[1]) + c[1]) + m[i, 3]
        r.append((F32(lo), F32(hi)))
    return _iv_div(r[0], r[3]), _iv_div(r[1], r[3]), _iv_div(r[2], r[3])


def _values(shape, x, y, z, m, vars_):
    if m is not None:
        x, y, z = xf_points(m, x, y, z)
    return shape.eval_float_slice(x, y, z, vars_)


def brute_force(shape, depth, world_to_model=None, vars=None):
    """inside[i, j, k] over all N^3 centres (NaN: not inside)"""
    N = 4 << depth
    m, c = _matrix(world_to_model), centres(N)
    inside = np.zeros((N, N, N), bool)
    step = max(1, (1 << 21) // (N * N))
    for i0 in range(0, N, step):
        i1 = min(N, i0 + step)
        x, y, z = (np.ascontiguousarray(a).ravel() for a in np.broadcast_arrays(c[i0:i1, None, None], c[None, :, None], c[None, None, :]))
        inside[i0:i1] = (_values(shape, x, y, z, m, vars) < 0).reshape(i1 - i0, N, N)
    return inside


def recursion(shape, depth, world_to_model=None, vars=None):
    """(inside[i, j, k], {"cells", "full", "empty", "leaf_cells"}, Full cells per level) by the octree of the definition"""
    N = 4 << depth
    m, c = _matrix(world_to_model), centres(N)
    inside = np.zeros((N, N, N), bool)
    counts = {"cells": 0, "full": 0, "empty": 0, "leaf_cells": 0}
    full_per_level = []
    one = F32(1.0)
    level = [((-one, one, -one, one, -one, one), (0, 0, 0))]        # (bounds, origin in cells of the level)
    for d in range(depth + 1):
        w = N >> d
        batch = []
        for b, _ in level:
            X, Y, Z = (b[0], b[1]), (b[2], b[3]), (b[4], b[5])
            if m is not None:
                X, Y, Z = xf_interval(m, X, Y, Z)
            vs = shape._xyz_vars(X, Y, Z, vars)
            batch.append([None if v is None else ((v, v) if np.isscalar(v) else v) for v in vs])
        amb, n_full = [], 0
        for (b, o), ((lo, hi), _) in zip(level, shape.eval_interval_batch(batch)):
            counts["cells"] += 1
            if hi < 0:
                counts["full"] += 1
                n_full += 1
                inside[o[0] * w:(o[0] + 1) * w, o[1] * w:(o[1] + 1) * w, o[2] * w:(o[2] + 1) * w] = True
            elif lo > 0:
                counts["empty"] += 1
            else:
                amb.append((b, o))
        full_per_level.append(n_full)
        if d == depth or not amb:
            if d == depth:
                counts["leaf_cells"] = len(amb)
                if amb:
                    org = np.array([o for _, o in amb], np.int64) * 4          # [n, 3]
                    l = np.arange(64)
                    ii = org[:, None, 0] + (l & 3)[None, :]
                    jj = org[:, None, 1] + ((l >> 2) & 3)[None, :]
                    kk = org[:, None, 2] + (l >> 4)[None, :]
                    v = _values(shape, c[ii.ravel()], c[jj.ravel()], c[kk.ravel()], m, vars)
                    inside[ii.ravel(), jj.ravel(), kk.ravel()] = v < 0
            break
        nxt = []
        for b, o in amb:
            mid = [(b[2 * k] + b[2 * k + 1]) / F32(2.0) for k in range(3)]
            for corner in range(8):
                cb, co = [], []
                for k in range(3):
                    up = (corner >> k) & 1
                    cb += [mid[k], b[2 * k + 1]] if up else [b[2 * k], mid[k]]
                    co.append(2 * o[k] + up)
                nxt.append((tuple(cb), tuple(co)))
        level = nxt
    return inside, counts, full_per_level


def sums(inside):
    """the integer fields of fhip_occupancy from inside[i, j, k], as Python ints"""
    N = inside.shape[0]
    idx = np.arange(N, dtype=np.int64)
    n = int(inside.sum())
    marg = [inside.sum(axis=tuple(a for a in range(3) if a != k), dtype=np.int64) for k in range(3)]        # inside voxels per index along axis k
    s1 = tuple(int((idx * marg[k]).sum()) for k in range(3))
    s2 = [int((idx * idx * marg[k]).sum()) for k in range(3)]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        plane = inside.sum(axis=3 - a - b, dtype=np.int64)       # [index along a, index along b]
        s2.append(int((idx[:, None] * idx[None, :] * plane).sum()))
    lo = tuple(int(np.flatnonzero(marg[k])[0]) if n else N for k in range(3))
    hi = tuple(int(np.flatnonzero(marg[k])[-1]) if n else 0 for k in range(3))
    return {"n": n, "s1": s1, "s2": tuple(s2), "lo": lo, "hi": hi, "grid": N}


def box_sums(origin, w, N):
    """the same fields for the box of w^3 voxels at `origin`, by the closed forms k_occ_full uses: S1(X) = w X + w (w - 1) / 2,
    S2(X) = w X^2 + X w (w - 1) + (w - 1) w (2 w - 1) / 6;  n = w^3, sum i = w^2 S1(X), sum i^2 = w^2 S2(X), sum ij = w S1(X) S1(Y)"""
    S1 = [w * X + w * (w - 1) // 2 for X in origin]
    S2 = [w * X * X + X * w * (w - 1) + (w - 1) * w * (2 * w - 1) // 6 for X in origin]
    s2 = [w * w * v for v in S2] + [w * S1[0] * S1[1], w * S1[0] * S1[2], w * S1[1] * S1[2]]
    return {"n": w ** 3, "s1": tuple(w * w * v for v in S1), "s2": tuple(s2), "lo": tuple(origin), "hi": tuple(X + w - 1 for X in origin), "grid": N}


def fields(occ):
    """an `Occupancy` of fidget_amd as the dict `sums` gives"""
    return {"n": occ.n, "s1": occ.s1, "s2": occ.s2, "lo": occ.lo, "hi": occ.hi, "grid": occ.grid}
