"""The exact Euclidean distance transform of fhip_voxels_distance (include/fidget_hip.h) restated in numpy, on `fg[i, j, k]` bool arrays
as occupancy_ref.py and voxels_ref.py make them:

  line(f)               one line: out[p] = min over q of f[q] + (p - q)^2 by the literal min-plus product, NONE carried as a sentinel
  edt(fg)               uint32 [N, N, N] indexed [i, j, k]: that pass along each axis in turn, O(N^4), in chunks
  direct(fg)            the definition itself over the list of foreground voxels, O(N^3 * voxels): for grids with a handful of them
  field(d2)             the layout of the library's layers: [k, j, i]
  summary(d2)           (the largest finite value, the (i, j, k) of smallest index k N^2 + j N + i that has it or None, foreground voxels)
  within(d2, t), beyond(d2, t)     bool [i, j, k]

No envelope, no stack, no bit masks: it shares neither code nor algorithm with the library."""
import numpy as np

NONE = 0xFFFFFFFF
_INF = np.int64(1) << np.int64(40)          # the sentinel while adding: above every finite sum, far below overflow


def line(f):
    """f: [..., n] uint32 with NONE for "nothing here" -> the same shape: min over q of f[..., q] + (p - q)^2"""
    f = np.asarray(f)
    n = f.shape[-1]
    g = np.where(f == NONE, _INF, f.astype(np.int64))
    q = np.arange(n, dtype=np.int64)
    cost = (q[:, None] - q[None, :]) ** 2          # [p, q]
    out = (g[..., None, :] + cost).min(axis=-1)
    return np.where(out >= _INF, NONE, out).astype(np.uint32)


def _along(d, axis, chunk=1 << 14):
    n = d.shape[axis]
    lines = np.moveaxis(d, axis, -1).reshape(-1, n)
    out = np.empty_like(lines)
    step = max(1, chunk // n)
    for a in range(0, len(lines), step):
        out[a:a + step] = line(lines[a:a + step])
    return np.moveaxis(out.reshape(np.moveaxis(d, axis, -1).shape), -1, axis)


def edt(fg):
    fg = np.asarray(fg, bool)
    d = np.where(fg, 0, NONE).astype(np.uint32)
    for axis in range(3):
        d = _along(d, axis)
    return d


def direct(fg):
    fg = np.asarray(fg, bool)
    N = fg.shape[0]
    pts = np.argwhere(fg).astype(np.int64)
    if len(pts) == 0:
        return np.full(fg.shape, NONE, np.uint32)
    i, j, k = np.indices(fg.shape, dtype=np.int64, sparse=True)
    best = np.full(fg.shape, _INF, np.int64)
    for a, b, c in pts:
        np.minimum(best, (i - a) ** 2 + (j - b) ** 2 + (k - c) ** 2, out=best)
    assert N and best.max() < _INF
    return best.astype(np.uint32)


def field(d2):
    return np.ascontiguousarray(d2.transpose(2, 1, 0))


def summary(d2):
    flat = field(d2).reshape(-1)
    finite = flat != NONE
    n = int((flat == 0).sum())
    if not finite.any():
        return 0, None, n
    m = int(flat[finite].max())
    idx = int(np.flatnonzero(flat == m)[0])
    N = d2.shape[0]
    return m, (idx % N, idx // N % N, idx // (N * N)), n


def within(d2, t):
    return (d2 != NONE) & (d2.astype(np.int64) <= int(t))


def beyond(d2, t):
    return (d2 == NONE) | (d2.astype(np.int64) > int(t))
