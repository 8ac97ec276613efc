"""The local thickness of fhip_distance_thickness (include/fidget_hip.h) restated in numpy, on squared-distance fields `F[i, j, k]` as
distance_ref.py makes them (uint32, 0 on the foreground): T(p) = max { F(c) : F(c) > |p - c|^2 }, 0 where no centre reaches p.

  by_offsets(F)         the gather: for every offset d within the largest ball, T = max(T, F shifted by d where that exceeds |d|^2)
  by_centres(F)         the scatter: every centre with F > 0 paints its ball, clipped to the grid - value by value, a value's centres
                        one at a time or, where they outnumber the ball's voxels, all at once per voxel of the ball.  No centre is left out.
  slab(N, a, b)         the closed form in one dimension for a solid a <= x < b that spans the grid in the other two axes
  field(T)              the layout of the library's layers: [k, j, i]
  summary(T)            (max, its voxel of smallest index k N^2 + j N + i, smallest positive value, its voxel likewise, voxels with T > 0)
  thin(T, t), within(T, t), beyond(T, t)      bool [i, j, k]
  histogram(T, edges)   counts per [e_i, e_i+1)

No tables, no pruning, no rows: it shares neither code nor algorithm with the library."""
import functools
import math

import numpy as np

NONE = 0xFFFFFFFF


def _check(F):
    F = np.asarray(F)
    assert F.ndim == 3 and F.shape[0] == F.shape[1] == F.shape[2]
    if (F == NONE).any():
        raise ValueError("a field without foreground has no bounded ball")
    return F.astype(np.int64)


def _window(N, a):
    """target and source slices along one axis for `target[p + a] <- source[p]`, both inside 0 .. N - 1"""
    return slice(max(0, a), N + min(0, a)), slice(max(0, -a), N - max(0, a))


def by_offsets(F):
    F = _check(F)
    N = F.shape[0]
    T = np.zeros_like(F)
    top = int(F.max())
    if top == 0:
        return T.astype(np.uint32)
    R = min(math.isqrt(top - 1), N - 1)          # (an offset longer than the grid moves everything out of it)
    for a in range(-R, R + 1):
        for b in range(-R, R + 1):
            for c in range(-R, R + 1):
                d2 = a * a + b * b + c * c
                if d2 >= top:
                    continue
                (ta, sa), (tb, sb), (tc, sc) = _window(N, a), _window(N, b), _window(N, c)
                src = F[sa, sb, sc]
                np.maximum(T[ta, tb, tc], np.where(src > d2, src, 0), out=T[ta, tb, tc])
    return T.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def ball(f):
    """(bool [2 R + 1]^3 of the offsets with |d|^2 < f, R)"""
    R = math.isqrt(f - 1)
    a = np.arange(-R, R + 1, dtype=np.int64)
    m = (a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2) < f
    m.setflags(write=False)
    return m, R


def by_centres(F):
    F = _check(F)
    N = F.shape[0]
    T = np.zeros_like(F)
    for f in np.unique(F[F > 0]):
        f = int(f)
        m, R = ball(f)
        here = F == f
        pts = np.argwhere(here)
        offs = np.argwhere(m) - R
        if len(pts) <= len(offs):
            for i, j, k in pts:
                lo = (max(i - R, 0), max(j - R, 0), max(k - R, 0))
                hi = (min(i + R, N - 1), min(j + R, N - 1), min(k + R, N - 1))
                w = m[lo[0] - i + R:hi[0] - i + R + 1, lo[1] - j + R:hi[1] - j + R + 1, lo[2] - k + R:hi[2] - k + R + 1]
                t = T[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
                np.maximum(t, np.where(w, f, 0), out=t)
        else:
            for a, b, c in offs:
                if max(abs(a), abs(b), abs(c)) >= N:
                    continue
                (ta, sa), (tb, sb), (tc, sc) = _window(N, int(a)), _window(N, int(b)), _window(N, int(c))
                np.maximum(T[ta, tb, tc], np.where(here[sa, sb, sc], f, 0), out=T[ta, tb, tc])
    return T.astype(np.uint32)


def slab(N, a, b):
    """uint32 [N]: T along the axis across a solid a <= x < b (0 <= a < b <= N, not the whole grid) that spans the grid in the other two
    axes.  A centre's offsets across the slab only shorten its reach along it, so the best centre for p lies on p's own line."""
    assert 0 <= a < b <= N and (a > 0 or b < N)
    x = np.arange(N, dtype=np.int64)
    clear = (x < a) | (x >= b)
    F1 = np.where(clear, 0, np.min(np.where(clear[None, :], (x[:, None] - x[None, :]) ** 2, np.int64(1) << 40), axis=1))
    reach = F1[None, :] > (x[:, None] - x[None, :]) ** 2          # [p, c]
    return np.max(np.where(reach, F1[None, :], 0), axis=1).astype(np.uint32)


def field(T):
    return np.ascontiguousarray(T.transpose(2, 1, 0))


def _voxel(idx, N):
    return (idx % N, idx // N % N, idx // (N * N))


def summary(T):
    flat = field(T).reshape(-1).astype(np.int64)
    N = T.shape[0]
    pos = flat > 0
    n = int(pos.sum())
    if n == 0:
        return 0, _voxel(0, N), None, None, 0
    hi, lo = int(flat.max()), int(flat[pos].min())
    return hi, _voxel(int(np.flatnonzero(flat == hi)[0]), N), lo, _voxel(int(np.flatnonzero(flat == lo)[0]), N), n


def thin(T, t):
    return (T > 0) & (T.astype(np.int64) <= int(t))


def within(T, t):
    return T.astype(np.int64) <= int(t)


def beyond(T, t):
    return T.astype(np.int64) > int(t)


def histogram(T, edges):
    edges = [int(e) for e in edges]
    assert len(edges) >= 2 and all(x <= y for x, y in zip(edges, edges[1:]))
    v = np.asarray(T).reshape(-1).astype(np.int64)
    return np.array([int(((v >= lo) & (v < hi)).sum()) for lo, hi in zip(edges, edges[1:])], np.uint64)
