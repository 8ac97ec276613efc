"""A voxel bitmap along a direction (fhip_voxels_flow, fhip_voxels_overhangs, fhip_voxels_heights; include/fidget_hip.h) restated in
numpy on `inside[i, j, k]` arrays, the plain way:

  flow(seeds, blockers, d, with_seeds)    a loop over the N layers along the axis, r = (r | s_prev) & ~k_cur
  overhangs(solid, up, reach2, bed)       an OR over the explicit list of offsets with u^2 + v^2 <= reach2 of the shifted layers below
  supports(solid, up, reach2, bed)        flow(overhangs, solid, up ^ 1)
  heights(solid, axis)                    int32 [3, N, N] with argmax / sum

A direction d = 0 .. 5 is -x, +x, -y, +y, -z, +z.  Outside the grid every bitmap is clear."""
import numpy as np


def _along(a, d):
    """a view of `a` whose first index runs in the direction d: layer 0 is the one the flow leaves first"""
    v = np.moveaxis(a, d >> 1, 0)
    return v if d & 1 else v[::-1]


def flow(seeds, blockers, d, with_seeds=False):
    seeds = np.asarray(seeds, bool)
    blockers = np.zeros_like(seeds) if blockers is None else np.asarray(blockers, bool)
    s, k = np.ascontiguousarray(_along(seeds, d)), np.ascontiguousarray(_along(blockers, d))          # [layer, ., .]: a layer is one run of memory
    r = np.zeros_like(s)
    for layer in range(1, s.shape[0]):          # (layer 0 has nothing behind it)
        r[layer] = (r[layer - 1] | s[layer - 1]) & ~k[layer]
    out = np.zeros_like(seeds)
    _along(out, d)[...] = r          # (a view: writing it fills `out`)
    return out | seeds if with_seeds else out


def disc(reach2):
    """the offsets (u, v) with u^2 + v^2 <= reach2"""
    return [(u, v) for u in range(-4, 5) for v in range(-4, 5) if u * u + v * v <= reach2]


def overhangs(solid, up, reach2, bed):
    solid = np.asarray(solid, bool)
    a = np.ascontiguousarray(_along(solid, up))          # layers ascend towards `up`; the two other axes keep their order
    n = a.shape[0]
    below = np.zeros_like(a)          # [layer] = the layer below it, clear under the first
    below[1:] = a[:-1]
    supported = np.zeros_like(a)
    for u, v in disc(reach2):          # [layer, p, q] |= below[layer, p + u, q + v], clear outside
        p0, p1, q0, q1 = max(0, -u), min(n, n - u), max(0, -v), min(n, n - v)
        supported[:, p0:p1, q0:q1] |= below[:, p0 + u:p1 + u, q0 + v:q1 + v]
    supported[0] = bool(bed)          # under the first layer every voxel counts as set, or none
    out = np.zeros_like(solid)
    _along(out, up)[...] = a & ~supported
    return out


def supports(solid, up, reach2, bed):
    return flow(overhangs(solid, up, reach2, bed), solid, up ^ 1)


def heights(solid, axis):
    """[3, N, N]: the lower of the two remaining axes is the last index"""
    solid = np.asarray(solid, bool)
    n = solid.shape[0]
    cols = np.moveaxis(solid, axis, 0)          # [along, lower, higher]
    any_ = cols.any(axis=0)
    lo = np.where(any_, cols.argmax(axis=0), -1)
    hi = np.where(any_, n - 1 - cols[::-1].argmax(axis=0), -1)
    return np.stack([lo.T, hi.T, cols.sum(axis=0).T]).astype(np.int32)
