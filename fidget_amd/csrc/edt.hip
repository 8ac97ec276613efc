// The exact Euclidean distance transform of a voxel bitmap (fhip_voxels_distance, include/fidget_hip.h; the host side is capi_edt.hpp):
// d2[k][j][i] = the squared distance, in voxels, from voxel (i, j, k) to the nearest foreground voxel, as a uint32.  Separable, three
// passes of O(N^3), each line by the integer arithmetic of mesh_edt.hpp:
//   k_edt_rows       along i, from the bitmap: a block takes the 16 rows of one row of bricks - their words into LDS, the rows' bit masks
//                    made of the bricks' nibbles, per mask word the nearest set bit beyond it - and then every lane writes runs of four
//                    voxels as one 16-byte store, the lanes of a wave next to each other along i
//   k_edt_cols       along j, then along k, in place: a lane takes a column and the lanes of a wave consecutive i, so every load and
//                    store of the field is a wave-wide run along i.  The lower envelope's stack - 8 bytes an entry, N entries a column -
//                    is laid out [entry][lane]: in LDS up to N = 64 (32 KiB a wave), in a device workspace above
//   k_edt_threshold  64 voxels of the field -> one word of a bitmap (d2 <= t, d2 > t, or 0 < d2 <= t)
//   k_edt_reduce, k_edt_reduce_sum   the largest finite d2, the smallest index that has it, the number of zeros: per-block partials, then one block
//   k_edt_copy       layers of the field into a buffer of the caller's
// No kernel waits for another workgroup; every word written has one writer; integers throughout, so the field is the same in any order.
// Included by mesh.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "mesh_edt.hpp"

namespace fhm {
constexpr uint32_t FH_EDT_LANES = 64;            // a wave: the columns one block of k_edt_cols runs side by side
constexpr uint32_t FH_EDT_LDS_MAX_N = 64;        // columns up to this length keep their stacks in LDS
constexpr uint32_t FH_EDT_COL_BLOCKS = 2048;     // blocks of k_edt_cols at most (each owns N * 64 entries of the workspace)
constexpr uint32_t FH_EDT_REDUCE_BLOCKS = 2048, FH_EDT_COPY_BLOCKS = 1u << 16;

// Along i.  Block (by + B * bz) takes the bricks (0 .. B - 1, by, bz): row r = ly + 4 lz of them is the voxels (0 .. N - 1, 4 by + ly,
// 4 bz + lz), its bits the nibbles at shift 4 r of the B words.  `flip`: all ones for the complement.
__global__ void __launch_bounds__(256) k_edt_rows(const uint64_t* __restrict__ bricks, uint32_t depth, uint64_t flip, uint32_t* __restrict__ field) {
    __shared__ uint64_t sh_bricks[1u << fhedt::MAX_DEPTH];
    __shared__ uint64_t sh_mask[16][fhedt::MAX_WORDS];
    __shared__ int32_t sh_below[16][fhedt::MAX_WORDS], sh_above[16][fhedt::MAX_WORDS];
    const uint32_t B = 1u << depth, N = 4u << depth, tid = threadIdx.x;
    const uint32_t n_words = B < 16 ? 1 : B >> 4, per_word = B < 16 ? B : 16;          // mask words of a row; bricks in one of them
    const uint32_t by = blockIdx.x & (B - 1), bz = blockIdx.x >> depth;
    if (tid < B) sh_bricks[tid] = bricks[fhvox::word_index(depth, tid, by, bz)] ^ flip;
    __syncthreads();
    const uint32_t mr = tid / n_words, mw = tid % n_words;          // this thread's mask word, if tid < 16 * n_words (<= 256)
    if (mr < 16) {
        uint64_t m = 0;
        for (uint32_t q = 0; q < per_word; q++) m |= ((sh_bricks[16 * mw + q] >> (4 * mr)) & 0xFull) << (4 * q);
        sh_mask[mr][mw] = m;
    }
    __syncthreads();
    if (mr < 16) {
        int32_t below, above;
        fhedt::row_links(sh_mask[mr], n_words, mw, below, above);
        sh_below[mr][mw] = below;
        sh_above[mr][mw] = above;
    }
    __syncthreads();
    for (uint32_t item = tid; item < 16 * B; item += 256) {          // B runs of four voxels a row
        const uint32_t r = item >> depth, g = item & (B - 1), w = g >> 4, b = 4 * (g & 15);
        const uint64_t m = sh_mask[r][w];
        const int32_t below = sh_below[r][w], above = sh_above[r][w];
        const uint4 v = make_uint4(fhedt::row_d2(m, w, b, below, above), fhedt::row_d2(m, w, b + 1, below, above), fhedt::row_d2(m, w, b + 2, below, above),
                                   fhedt::row_d2(m, w, b + 3, below, above));
        const uint32_t j = 4 * by + (r & 3), k = 4 * bz + (r >> 2);
        *(uint4*)(field + ((size_t)k * N + j) * N + 4 * g) = v;
    }
}

// a lane's stack: entry k at base[k * 64], the lanes of a wave side by side
struct EdtLaneStack {
    fhedt::Entry* base;
    __device__ __forceinline__ fhedt::Entry get(uint32_t k) const { return base[(size_t)k * FH_EDT_LANES]; }
    __device__ __forceinline__ void set(uint32_t k, const fhedt::Entry& v) { base[(size_t)k * FH_EDT_LANES] = v; }
};
// Along j (axis 1) or k (axis 2), in place.  A block is one wave; it strides over the groups of 64 columns, numbered so that
// consecutive columns are consecutive i: along j column c is (i, k) = (c mod N, c / N), along k it is (i, j) likewise - element q of it
// lies q * stride words after its first.  IN_LDS: the stacks in dynamic LDS, N * 64 * 8 bytes; otherwise block b owns
// work[b * N * 64 ...].  Values come in four at a time, so that four loads are in flight.
template <bool IN_LDS>
__global__ void __launch_bounds__(FH_EDT_LANES) k_edt_cols(uint32_t* __restrict__ field, uint32_t depth, uint32_t axis, fhedt::Entry* __restrict__ work) {
    extern __shared__ fhedt::Entry sh_edt_stack[];
    const uint32_t N = 4u << depth, lane = threadIdx.x;
    const uint32_t n_cols = N * N, n_groups = (n_cols + FH_EDT_LANES - 1) / FH_EDT_LANES;
    const size_t stride = axis == 1 ? (size_t)N : (size_t)N * N;
    EdtLaneStack stack{IN_LDS ? sh_edt_stack + lane : work + (size_t)blockIdx.x * N * FH_EDT_LANES + lane};
    for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const uint32_t c = g * FH_EDT_LANES + lane;
        if (c >= n_cols) continue;          // (N = 4: 16 columns)
        uint32_t* const col = field + (axis == 1 ? (size_t)(c >> (depth + 2)) * N * N + (c & (N - 1)) : (size_t)c);
        int32_t top = -1;
        fhedt::Entry t = fhedt::entry(0, 0, 0);
        for (uint32_t q0 = 0; q0 < N; q0 += 4) {
            uint32_t f[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; u++) f[u] = col[(q0 + u) * stride];
#pragma unroll
            for (uint32_t u = 0; u < 4; u++)
                if (f[u] != fhedt::NONE) fhedt::env_add(stack, top, t, N, q0 + u, f[u]);
        }
        if (top < 0) continue;          // no foreground in this column's plane so far: it stays NONE
        fhedt::env_scan(stack, top, N, [&](uint32_t p, uint32_t v) { col[p * stride] = v; });
    }
}

// One word of the bitmap per thread: bit lx + 4 ly + 16 lz = edt_passes at voxel (4 bx + lx, 4 by + ly, 4 bz + lz).  Per
// (ly, lz) one 16-byte load, a wave's loads a run of 1 KiB along i.  NONE is above every t <= 0xFFFFFFFE: never within, always beyond.
// mode 0: d2 <= t ("within"); 1: d2 > t ("beyond"); 2: 0 < d2 <= t (the thin parts of a thickness field, thick.hip)
__device__ __forceinline__ uint32_t edt_passes(uint32_t v, uint32_t t, uint32_t mode) {
    return mode == 2 ? (uint32_t)(v != 0 && v <= t) : (uint32_t)((v > t) == (mode != 0));
}
__global__ void __launch_bounds__(256) k_edt_threshold(const uint32_t* __restrict__ field, uint32_t depth, uint32_t t, uint32_t mode, uint64_t* __restrict__ out) {
    const uint64_t n_words = (uint64_t)1 << (3 * depth), w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= n_words) return;
    const uint32_t N = 4u << depth, Bm = (1u << depth) - 1;
    const uint32_t bx = (uint32_t)w & Bm, by = (uint32_t)(w >> depth) & Bm, bz = (uint32_t)(w >> (2 * depth));
    uint64_t word = 0;
    for (uint32_t r = 0; r < 16; r++) {
        const uint32_t j = 4 * by + (r & 3), k = 4 * bz + (r >> 2);
        const uint4 v = *(const uint4*)(field + ((size_t)k * N + j) * N + 4 * bx);
        const uint32_t nib = edt_passes(v.x, t, mode) | (edt_passes(v.y, t, mode) << 1) | (edt_passes(v.z, t, mode) << 2) | (edt_passes(v.w, t, mode) << 3);
        word |= (uint64_t)nib << (4 * r);
    }
    out[w] = word;
}

// The summary.  A voxel's key is d2 << 32 | (0xFFFFFFFF - index), index = (k N + j) N + i < 2^30: the largest key is the largest d2 at
// the smallest index; NONE takes no part, and key 0 - which no voxel has - says that nothing finite was seen.  parts: [gridDim.x][2] =
// {largest key, number of zeros}.
__device__ __forceinline__ void edt_block_reduce(uint64_t key, uint64_t zeros, uint64_t* __restrict__ out) {
    __shared__ uint64_t sh_key[256], sh_zeros[256];
    const uint32_t tid = threadIdx.x;
    sh_key[tid] = key;
    sh_zeros[tid] = zeros;
    __syncthreads();
    for (uint32_t d = 128; d > 0; d >>= 1) {
        if (tid < d) {
            if (sh_key[tid + d] > sh_key[tid]) sh_key[tid] = sh_key[tid + d];
            sh_zeros[tid] += sh_zeros[tid + d];
        }
        __syncthreads();
    }
    if (tid == 0) { out[0] = sh_key[0]; out[1] = sh_zeros[0]; }
}
__global__ void __launch_bounds__(256) k_edt_reduce(const uint32_t* __restrict__ field, uint32_t depth, uint64_t* __restrict__ parts) {
    const uint64_t n_runs = (uint64_t)16 << (3 * depth);          // runs of four voxels
    uint64_t key = 0;
    uint32_t zeros = 0;          // (a thread sees at most 2^30 voxels)
    for (uint64_t run = (uint64_t)blockIdx.x * 256 + threadIdx.x; run < n_runs; run += (uint64_t)gridDim.x * 256) {
        const uint4 v = ((const uint4*)field)[run];
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            zeros += d[u] == 0;
            const uint64_t k = ((uint64_t)d[u] << 32) | (0xFFFFFFFFu - (uint32_t)(4 * run + u));
            if (d[u] != fhedt::NONE && k > key) key = k;
        }
    }
    edt_block_reduce(key, zeros, parts + 2 * (size_t)blockIdx.x);
}
__global__ void __launch_bounds__(256) k_edt_reduce_sum(const uint64_t* __restrict__ parts, uint32_t n_parts, uint64_t* __restrict__ out) {
    uint64_t key = 0, zeros = 0;
    for (uint32_t p = threadIdx.x; p < n_parts; p += 256) {
        if (parts[2 * (size_t)p] > key) key = parts[2 * (size_t)p];
        zeros += parts[2 * (size_t)p + 1];
    }
    edt_block_reduce(key, zeros, out);
}

// n runs of four values from src to dst, both 16-byte aligned
__global__ void __launch_bounds__(256) k_edt_copy(const uint4* __restrict__ src, uint64_t n, uint4* __restrict__ dst) {
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (uint64_t)gridDim.x * 256) dst[t] = src[t];
}
}  // namespace fhm
