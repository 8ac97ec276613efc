// The solid voxelization of a triangle mesh (fhip_triangles_voxels, fhip_mesh_voxels, include/fidget_hip.h; the host side is
// capi_trivox.hpp): parity counting along +x.  The arithmetic is mesh_trivox.hpp's, which the tests also build for the host.
//   k_tv_setup      a lane per triangle: its three vertices - by uint64 indices or, as a soup, three in a row - through the transform
//                   and the snap; rejected, flat, or oriented with its box of columns; a record of 48 bytes and the number of columns.
//                   An index at or beyond n_vertices rejects the triangle before anything is read.
//   (the prefix sums of the column counts are k_scan_block / k_scan_add of mesh.hip, in 32 bits; a count is below 2^32, so the sum
//   wrapped at triangle t exactly where low[t + 1] < low[t] - k_tv_wraps - and the prefix sums of those flags are the high words)
//   k_tv_cross      the W (triangle, column) items in equal contiguous shares, one per wave, walked 64 at a time: neither the launch
//                   nor a lane's loop knows one triangle's size.  The wave looks its first item's triangle up by bisection once and
//                   from then on gallops forward from the last one - the items ascend; a lane whose item lies beyond the wave's
//                   triangle gallops on from there.  Three edge tests; a covered column makes the division and one 64-bit atomic XOR
//                   whose result is not used, into the bitmap's word or the exit plane.  XOR commutes: the result does not depend
//                   on the order of arrival.
//   k_tv_fill       the prefix XOR along x, in place.  Inside a word two shift-and-XOR steps over all 16 rows; across the bricks of a
//                   row the words' 16 parities are scanned over the lanes with XOR.  The layout is k_flow_x's: rows shorter than 64
//                   bricks share a wave, the scan restarting at each row's first brick; longer rows go in chunks of 64, lane 63's
//                   parity handed on.  The lane of a row's last brick compares the parity that leaves with the exit plane: the open
//                   rows.
// The tallies: a lane counts in a register, the wave sums, one lane adds - one atomic add per wave and counter, into one of
// FH_TV_SLOTS rows of counters chosen by the wave's number, which the host sums.  (With one row, the adds of some 10^5 .. 10^6 waves to
// one address took longer than everything else the kernels do: profiles/mesh_voxels/README.md.)
// No kernel waits for another workgroup, none uses scratch, and nothing is a float after the snap.  Included by mesh.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "mesh_trivox.hpp"

namespace fhm {
constexpr uint32_t FH_TV_CROSS_BLOCKS = 4096;          // k_tv_cross: at most so many blocks of 256 - 16 waves to each of 256 CUs, four shares to each
// the counters of a call, uint64 each: FH_TV_SLOTS rows of FH_TV_COUNTERS - a row is a line of 64 bytes
constexpr uint32_t FH_TV_REJECTED = 0, FH_TV_FLAT = 1, FH_TV_CROSSINGS = 2, FH_TV_CLIPPED = 3, FH_TV_OPEN = 4, FH_TV_SET = 5, FH_TV_COUNTERS = 8, FH_TV_SLOTS = 256;

struct FhTvTransform {
    double m[12];
    uint32_t present;
};

__device__ __forceinline__ void tv_count(uint64_t* counters, uint32_t which, uint32_t in_wave) {          // (called by one lane of the wave)
    const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (in_wave) atomicAdd((unsigned long long*)counters + (wave & (FH_TV_SLOTS - 1)) * FH_TV_COUNTERS + which, (unsigned long long)in_wave);
}

__global__ void __launch_bounds__(256) k_tv_setup(const float* __restrict__ vertices, uint64_t n_vertices, const uint64_t* __restrict__ triangles, uint32_t n_triangles,
                                                  FhTvTransform M, uint32_t depth, fhtv::Tri* __restrict__ records, uint32_t* __restrict__ columns,
                                                  uint64_t* __restrict__ counters) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;          // (64 bits: n_triangles rounded up to 256 may pass 2^32)
    const bool live = t < n_triangles;
    uint32_t kind = fhtv::TV_OK;
    if (live) {
        int32_t q[3][3];
        bool ok = true;
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) {
            const uint64_t at = triangles ? triangles[(uint64_t)3 * t + c] : (uint64_t)3 * t + c;
            q[c][0] = q[c][1] = q[c][2] = 0;
            if (at >= n_vertices) { ok = false; continue; }
            const float v[3] = {vertices[3 * at], vertices[3 * at + 1], vertices[3 * at + 2]};
            ok = fhtv::snap_vertex(v, M.present ? M.m : nullptr, depth, q[c]) && ok;
        }
        fhtv::Tri T;
        if (ok) kind = fhtv::setup(q[0], q[1], q[2], depth, T);
        else {
            kind = fhtv::TV_REJECTED;
            const int32_t zero[3] = {0, 0, 0};
            (void)fhtv::setup(zero, zero, zero, depth, T);          // a record without columns
        }
        records[t] = T;
        columns[t] = fhtv::n_columns(T);
    }
    const uint32_t rejected = (uint32_t)__popcll(__ballot(live && kind == fhtv::TV_REJECTED)), flat = (uint32_t)__popcll(__ballot(live && kind == fhtv::TV_FLAT));
    if ((threadIdx.x & 63) == 0) {
        tv_count(counters, FH_TV_REJECTED, rejected);
        tv_count(counters, FH_TV_FLAT, flat);
    }
}

// low: the prefix sums of the column counts modulo 2^32, n + 1 of them -> wrapped[t] = 1 where the sum passed 2^32 at triangle t
__global__ void __launch_bounds__(256) k_tv_wraps(const uint32_t* __restrict__ low, uint32_t n, uint32_t* __restrict__ wrapped) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) wrapped[t] = low[t + 1] < low[t] ? 1u : 0u;
}

__device__ __forceinline__ uint64_t tv_prefix(const uint32_t* __restrict__ low, const uint32_t* __restrict__ high, uint32_t t) {
    return ((uint64_t)high[t] << 32) | low[t];
}
// the triangle of item w: the t in [lo, hi) with prefix(t) <= w < prefix(t + 1), given prefix(lo) <= w < prefix(hi) (triangles without
// columns are passed over)
__device__ __forceinline__ uint32_t tv_bisect(const uint32_t* __restrict__ low, const uint32_t* __restrict__ high, uint32_t lo, uint32_t hi, uint64_t w) {
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (tv_prefix(low, high, mid) <= w) lo = mid;
        else hi = mid;
    }
    return lo;
}
// ... given only prefix(lo) <= w < prefix(n) = W: steps of 1, 2, 4, .. from lo until one passes w, then the bisection between the last two
__device__ __forceinline__ uint32_t tv_gallop(const uint32_t* __restrict__ low, const uint32_t* __restrict__ high, uint32_t lo, uint32_t n, uint64_t w) {
    uint32_t step = 1;
    while (n - lo > step && tv_prefix(low, high, lo + step) <= w) {
        lo += step;
        step <<= 1;
    }
    return tv_bisect(low, high, lo, n - lo > step ? lo + step : n, w);
}

// per_wave: a multiple of 64; the grid's waves times it cover n_items
__global__ void __launch_bounds__(256) k_tv_cross(const fhtv::Tri* __restrict__ records, const uint32_t* __restrict__ low, const uint32_t* __restrict__ high,
                                                  uint32_t n_triangles, uint64_t n_items, uint64_t per_wave, uint32_t depth, uint64_t* __restrict__ bricks,
                                                  uint64_t* __restrict__ exit_plane, uint64_t* __restrict__ counters) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t first = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * per_wave;          // (the same in every lane of a wave, as all of the loop's bounds)
    const uint64_t end = first + per_wave < n_items ? first + per_wave : n_items;
    uint32_t crossings = 0, clipped = 0;
    uint32_t t0 = first < end ? tv_bisect(low, high, 0, n_triangles, first) : 0;
    for (uint64_t w0 = first; w0 < end; w0 += 64) {
        const uint64_t w = w0 + lane;
        t0 = tv_gallop(low, high, t0, n_triangles, w0);
        if (w < end) {
            const uint32_t t = w < tv_prefix(low, high, t0 + 1) ? t0 : tv_gallop(low, high, t0 + 1, n_triangles, w);
            const fhtv::Tri T = records[t];
            const uint32_t local = (uint32_t)(w - tv_prefix(low, high, t));          // < nj nk <= 2^24
            const uint32_t j = T.j0 + local % T.nj, k = T.k0 + local / T.nj;
            int64_t i;
            if (fhtv::cover_cross(T, depth, j, k, i)) {
                crossings++;
                if (i == fhtv::TV_EXIT) {
                    clipped++;
                    const uint64_t at = fhtv::exit_index(depth, j, k);
                    (void)atomicXor((unsigned long long*)exit_plane + (at >> 6), (unsigned long long)1 << (at & 63));
                } else {
                    (void)atomicXor((unsigned long long*)bricks + fhtv::voxel_word(depth, (uint32_t)i, j, k), (unsigned long long)fhtv::voxel_bit((uint32_t)i, j, k));
                }
            }
        }
    }
    crossings = fhvox::wave_sum(crossings);
    clipped = fhvox::wave_sum(clipped);
    if (lane == 0) {
        tv_count(counters, FH_TV_CROSSINGS, crossings);
        tv_count(counters, FH_TV_CLIPPED, clipped);
    }
}

// In place on the B^3 words.  A wave holds 64 >> lg_width rows of width = min(B, 64) bricks each; with B > 64 it walks its one row in
// B / 64 chunks (k_flow_x's layout).
__global__ void __launch_bounds__(256) k_tv_fill(uint64_t* __restrict__ bricks, const uint64_t* __restrict__ exit_plane, uint32_t depth, uint64_t* __restrict__ counters) {
    const uint32_t B = 1u << depth, lg_width = depth < 6 ? depth : 6, width = 1u << lg_width;
    const uint32_t lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t pos0 = lane & (width - 1);                                    // the lane's place in its row's chunk
    const uint32_t row = (wave << (6 - lg_width)) + (lane >> lg_width);          // bz B + by
    const bool live = row < B * B;          // (a grid of fewer than 256 rows leaves lanes, and below depth 2 whole waves of its one block, without a row)
    const uint32_t n_chunks = B >> lg_width;
    uint64_t* const words = bricks + ((uint64_t)row << depth);
    uint64_t next = live ? words[pos0] : 0;
    uint64_t carry = 0;          // the parity that enters the chunk: the same in every lane of a row, at the X0 positions
    uint32_t n_set = 0, n_open = 0;
    for (uint32_t chunk = 0; chunk < n_chunks; chunk++) {
        const bool more = chunk + 1 < n_chunks;
        const uint64_t filled = fhtv::fill_word(next);
        if (live && more) next = words[(chunk + 1) * 64 + pos0];
        uint64_t acc = fhtv::fill_carry(filled);
        for (uint32_t step = 1; step < width; step <<= 1) {          // inclusive: after it `acc` is the parity of the row's words up to this lane's
            const uint64_t before = __shfl_up(acc, step, 64);
            if (pos0 >= step) acc ^= before;
        }
        uint64_t excl = __shfl_up(acc, 1, 64);
        if (pos0 == 0) excl = 0;
        const uint64_t res = fhtv::fill_apply(filled, excl ^ carry);
        if (live) {
            words[chunk * 64 + pos0] = res;
            n_set += (uint32_t)__popcll(res);
            if (!more && pos0 == width - 1) n_open = (uint32_t)__popcll(fhtv::open_ends(res, exit_plane, depth, row & (B - 1), row >> depth));
        }
        if (more) carry ^= __shfl(acc, 63, 64);          // (only with width == 64: the row's last brick of this chunk is in lane 63)
    }
    n_set = fhvox::wave_sum(n_set);
    n_open = fhvox::wave_sum(n_open);
    if (lane == 0) {
        tv_count(counters, FH_TV_SET, n_set);
        tv_count(counters, FH_TV_OPEN, n_open);
    }
}
}  // namespace fhm
