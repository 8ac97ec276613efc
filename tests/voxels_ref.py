"""The voxel bitmap of fhip_shape_voxels (include/fidget_hip.h) restated in numpy, from the `inside[i, j, k]` arrays of occupancy_ref.py:

  pack(inside)           uint64 [B, B, B], indexed [bz, by, bx]: bit lx + 4 ly + 16 lz of word (bz, by, bx) is voxel
                         (4 bx + lx, 4 by + ly, 4 bz + lz); N = 4 B
  unpack(bricks)         the other way
  slices(inside, k0, k1) uint8 [k1 - k0, N, N], [k - k0, j, i] = 255 inside, 0 outside
  layer_counts(inside)   [N] inside voxels per third index k

Written with one shift per local coordinate - not with the byte-order tricks fidget_amd.voxels_unpack uses - so that the two check each
other."""
import numpy as np


def pack(inside):
    inside = np.asarray(inside, bool)
    N = inside.shape[0]
    assert inside.shape == (N, N, N) and N % 4 == 0
    B = N // 4
    words = np.zeros((B, B, B), np.uint64)          # [bx, by, bz]
    for lz in range(4):
        for ly in range(4):
            for lx in range(4):
                words |= inside[lx::4, ly::4, lz::4].astype(np.uint64) << np.uint64(lx + 4 * ly + 16 * lz)
    return np.ascontiguousarray(words.transpose(2, 1, 0))


def unpack(bricks):
    bricks = np.asarray(bricks, np.uint64)
    B = bricks.shape[0]
    assert bricks.shape == (B, B, B)
    words = bricks.transpose(2, 1, 0)               # [bx, by, bz]
    inside = np.zeros((4 * B,) * 3, bool)
    for lz in range(4):
        for ly in range(4):
            for lx in range(4):
                inside[lx::4, ly::4, lz::4] = (words >> np.uint64(lx + 4 * ly + 16 * lz)) & np.uint64(1) != 0
    return inside


def slices(inside, k0, k1):
    return np.ascontiguousarray(np.asarray(inside, bool)[:, :, k0:k1].transpose(2, 1, 0)).astype(np.uint8) * np.uint8(255)


def layer_counts(inside):
    return np.asarray(inside, bool).sum(axis=(0, 1), dtype=np.int64)


def popcount(bricks):
    return int(np.unpackbits(np.ascontiguousarray(bricks, np.uint64).view(np.uint8)).sum(dtype=np.int64))
