// The index arithmetic of the voxel bitmap (fhip_shape_voxels, include/fidget_hip.h): where the cell with a given octree path lies in the
// array of bricks, and how the words of a Full cell are dealt out to the lanes of k_vox_full.  No HIP and no memory access: compiled for
// the device by mesh.hip and for the host by tests/host_build/mesh_vox_host.cpp - but for the device helper at the end (wave_sum), which the
// kernels of trivox.hip and topo.hip share and the host build does not see.
//
// The bitmap of depth `depth` is B^3 words, B = 1 << depth: word (bz * B + by) * B + bx is the brick of the voxels
// (4 bx + lx, 4 by + ly, 4 bz + lz), bit lx + 4 ly + 16 lz.  A cell of level l covers r^3 bricks, r = B >> l, from brick (ox r, oy r, oz r)
// on, (ox, oy, oz) being its origin in cells of its level.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FHV_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define FHV_HD __attribute__((always_inline)) inline
#endif

namespace fhvox {
constexpr uint32_t MAX_DEPTH = 10;       // B = 1024, N = 4096: 2^30 words, 8 GiB
FHV_HD uint64_t n_words(uint32_t depth) { return depth > MAX_DEPTH ? 0 : (uint64_t)1 << (3 * depth); }
FHV_HD uint32_t voxel_bit(uint32_t lx, uint32_t ly, uint32_t lz) { return lx + 4 * ly + 16 * lz; }

// the origin (in cells of its level) of the cell with this path: 3 bits per level below a leading 1, bit 0 x, 1 y, 2 z, the last level lowest
FHV_HD void cell_origin(uint64_t path, uint32_t level, uint32_t o[3]) {
    o[0] = o[1] = o[2] = 0;
    for (uint32_t l = 0; l < level; l++) {
        const uint32_t b = (uint32_t)(path >> (3 * l)) & 7u;
        o[0] |= (b & 1u) << l; o[1] |= ((b >> 1) & 1u) << l; o[2] |= ((b >> 2) & 1u) << l;
    }
}
FHV_HD uint64_t word_index(uint32_t depth, uint32_t bx, uint32_t by, uint32_t bz) { return (((((uint64_t)bz) << depth) + by) << depth) + bx; }
// the first word of the cell of level `level` with this path (its only one at level == depth)
FHV_HD uint64_t cell_word(uint64_t path, uint32_t level, uint32_t depth) {
    uint32_t o[3];
    cell_origin(path, level, o);
    const uint32_t s = depth - level;
    return word_index(depth, o[0] << s, o[1] << s, o[2] << s);
}

// A Full cell of level `level` is r^2 x-rows of r words, one for each (y, z) of its bricks.  The work is dealt out in slots, one lane one slot:
// `vec` consecutive words (2 = one 16-byte store; 1 for single-word rows or a bitmap that is not 16-byte aligned) at the same place of
// `rows` rows in turn, so that the cell's origin is worked out once per up to 8 stores.  Consecutive slots are consecutive pieces of a row,
// then the next group of rows, then the next cell: the lanes of a wave store next to each other.  Everything is a power of two.
struct FullSlots {
    uint32_t r, vec, rows;      // words per row; words per store; rows per slot
    uint32_t lg_r, lg_per_row, lg_rows, lg_per_cell;      // log2 of: r, slots side by side along a row, rows per slot, slots per cell
};
FHV_HD FullSlots full_slots(uint32_t depth, uint32_t level, bool aligned16) {
    FullSlots S;
    S.r = (1u << depth) >> level;
    S.vec = (S.r >= 2 && aligned16) ? 2 : 1;
    S.lg_r = depth - level;
    const uint32_t lg_rr = 2 * S.lg_r;
    S.lg_rows = lg_rr < 3 ? lg_rr : 3;
    S.rows = 1u << S.lg_rows;
    S.lg_per_row = S.lg_r - (S.vec - 1);
    S.lg_per_cell = S.lg_per_row + (lg_rr - S.lg_rows);
    return S;
}
// store q (< S.rows) of slot k (< 1 << S.lg_per_cell) of the cell at `cell` (cell_word): the first of its S.vec words
FHV_HD uint64_t slot_word(const FullSlots& S, uint32_t depth, uint64_t cell, uint32_t k, uint32_t q) {
    const uint32_t p = k & ((1u << S.lg_per_row) - 1), row = ((k >> S.lg_per_row) << S.lg_rows) + q;
    const uint32_t ry = row & (S.r - 1), rz = row >> S.lg_r;
    return cell + word_index(depth, p * S.vec, ry, rz);
}
#if defined(__HIPCC__)
// the sum of v over the 64 lanes of a wave, in every lane
template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (uint32_t step = 32; step > 0; step >>= 1) v += __shfl_xor(v, step, 64);
    return v;
}
#endif
}  // namespace fhvox
