// A voxel bitmap along a direction (fhip_voxels_flow, fhip_voxels_overhangs, fhip_voxels_heights, include/fidget_hip.h; the host side is
// capi_flow.hpp).  The bit arithmetic is mesh_flow.hpp's, which the tests also build for the host.
//   k_flow_yz       flow along +-y and +-z.  A lane per column of bricks, which it marches in the direction of the flow, the carry in a
//                   register; the lanes of a wave lie along bx, so that a wave's loads and stores are contiguous runs of words.  The
//                   addresses do not depend on the carry: the loads of the next four bricks are issued before the arithmetic of these.
//   k_flow_x        flow along +-x.  The lanes of a wave lie along the row of bricks in the direction of the flow; every lane makes
//                   the pair (G, P) of its word, an inclusive scan across the wave composes them in six steps - a carry-lookahead
//                   adder - and with the carry that enters it the lane finishes its word.  A row longer than a wave is walked in
//                   chunks of 64 bricks, the last lane's carry handed on; rows shorter than a wave share one, the scan restarting
//                   at each row's first brick.
//   k_overhangs     a lane per brick: the nine words around it in the plane perpendicular to `up` and the nine one brick below,
//                   dilated by the disc, moved one step up, taken out of the brick's word
//   k_heights       a lane per column of voxels, marching the bricks along the axis; the lanes lie along the lower of the two other
//                   axes, so the three planes are stored contiguously.  Along y and z the loads are contiguous too
//   k_heights_x     along x from depth 6 on: a wave per row of bricks, a lane per brick; the row's 16 columns of voxels are reduced
//                   across the wave with ballots - the first and the last lane that hold a set voxel, the number of set bits
// No kernel uses scratch or atomics or waits for another workgroup; every word written has one writer.  Integers throughout.
// Included by mesh.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "mesh_flow.hpp"

namespace fhm {
constexpr uint32_t FH_FLOW_AHEAD = 4;          // bricks of a column whose loads are in flight while the four before them are worked on

// seeds, blockers (null: none), out: B^3 words each; dir = 2 .. 5
__global__ void __launch_bounds__(64) k_flow_yz(const uint64_t* __restrict__ seeds, const uint64_t* __restrict__ blockers, uint32_t depth, uint32_t dir,
                                                uint32_t with_seeds, uint64_t* __restrict__ out) {
    const uint32_t B = 1u << depth, t = blockIdx.x * 64 + threadIdx.x;
    if (t >= B * B) return;          // (depth <= 10: B^2 <= 2^20)
    const uint32_t bx = t & (B - 1), o = t >> depth;
    // along y the column is (bx, ., bz = o), along z (bx, by = o, .)
    const uint64_t stride = (dir >> 1) == 1 ? (uint64_t)B : (uint64_t)B * B;
    const uint64_t base = (dir >> 1) == 1 ? fhvox::word_index(depth, bx, 0, o) : fhvox::word_index(depth, bx, o, 0);
    const bool forward = dir & 1;
    auto word_at = [&](uint32_t i) { return base + (uint64_t)(forward ? i : B - 1 - i) * stride; };          // the i-th brick the flow meets, i < B
    uint64_t s[FH_FLOW_AHEAD], k[FH_FLOW_AHEAD];
#pragma unroll
    for (uint32_t u = 0; u < FH_FLOW_AHEAD; u++) {
        s[u] = u < B ? seeds[word_at(u)] : 0;
        k[u] = (u < B && blockers) ? blockers[word_at(u)] : 0;
    }
    uint64_t carry = 0;
    for (uint32_t i0 = 0; i0 < B; i0 += FH_FLOW_AHEAD) {
        uint64_t sn[FH_FLOW_AHEAD], kn[FH_FLOW_AHEAD];
#pragma unroll
        for (uint32_t u = 0; u < FH_FLOW_AHEAD; u++) {
            const uint32_t i = i0 + FH_FLOW_AHEAD + u;
            sn[u] = i < B ? seeds[word_at(i)] : 0;
            kn[u] = (i < B && blockers) ? blockers[word_at(i)] : 0;
        }
#pragma unroll
        for (uint32_t u = 0; u < FH_FLOW_AHEAD; u++) {
            const uint32_t i = i0 + u;
            if (i < B) {
                const uint64_t r = fhfl::flow_word(s[u], ~k[u], carry, dir), rs = r | s[u];
                carry = fhfl::carry_out(rs, dir);
                out[word_at(i)] = with_seeds ? rs : r;
            }
            s[u] = sn[u];
            k[u] = kn[u];
        }
    }
}

// the pair (G, P) in one word for the cross-lane moves: G at the X0 positions, P one bit above
__device__ __forceinline__ uint64_t gp_pack(fhfl::GP a) { return a.g | (a.p << 1); }
__device__ __forceinline__ fhfl::GP gp_unpack(uint64_t v) { return fhfl::GP{v & fhvm::X0, (v >> 1) & fhvm::X0}; }

// dir = 0, 1.  A wave holds 64 >> lg_width rows of width = min(B, 64) bricks each; with B > 64 it walks its one row in B / 64 chunks.
__global__ void __launch_bounds__(256) k_flow_x(const uint64_t* __restrict__ seeds, const uint64_t* __restrict__ blockers, uint32_t depth, uint32_t dir,
                                                uint32_t with_seeds, uint64_t* __restrict__ out) {
    const uint32_t B = 1u << depth, lg_width = depth < 6 ? depth : 6, width = 1u << lg_width;
    const uint32_t lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t pos0 = lane & (width - 1);                                    // the lane's place in its row's chunk, in the direction of the flow
    const uint32_t row = (wave << (6 - lg_width)) + (lane >> lg_width);          // bz B + by
    const bool live = row < B * B;          // (only the one wave of a grid of fewer than 64 bricks has lanes without a row, its last ones)
    const uint32_t n_chunks = B >> lg_width;
    auto word_at = [&](uint32_t chunk) {
        const uint32_t pos = chunk * 64 + pos0;
        return ((uint64_t)row << depth) + ((dir & 1) ? pos : B - 1 - pos);
    };
    uint64_t s = live ? seeds[word_at(0)] : 0, k = (live && blockers) ? blockers[word_at(0)] : 0;
    uint64_t carry = 0;          // what enters the chunk: the same in every lane of a row, at the X0 positions
    for (uint32_t chunk = 0; chunk < n_chunks; chunk++) {
        const bool more = chunk + 1 < n_chunks;
        const uint64_t s_next = (live && more) ? seeds[word_at(chunk + 1)] : 0;
        const uint64_t k_next = (live && more && blockers) ? blockers[word_at(chunk + 1)] : 0;
        const uint64_t open = ~k;
        fhfl::GP acc = fhfl::gp_of(s, open, dir);
        for (uint32_t step = 1; step < width; step <<= 1) {          // inclusive: after it `acc` composes the row's words up to this lane's
            const fhfl::GP before = gp_unpack(__shfl_up(gp_pack(acc), step, 64));
            if (pos0 >= step) acc = fhfl::gp_then(before, acc);
        }
        fhfl::GP excl = gp_unpack(__shfl_up(gp_pack(acc), 1, 64));
        if (pos0 == 0) excl = fhfl::gp_identity();
        const uint64_t carry_in = excl.g | (excl.p & carry);
        const uint64_t r = fhfl::flow_word(s, open, fhfl::carry_from_x0(carry_in, dir), dir);
        if (live) out[word_at(chunk)] = with_seeds ? (r | s) : r;
        if (more) {          // (only with width == 64: the row's last brick of this chunk is in lane 63)
            const fhfl::GP whole = gp_unpack(__shfl(gp_pack(acc), 63, 64));
            carry = whole.g | (whole.p & carry);
        }
        s = s_next;
        k = k_next;
    }
}

// a brick's word, 0 beyond the grid: a coordinate of -1 has wrapped to above B
__device__ __forceinline__ uint64_t fl_word(const uint64_t* __restrict__ bricks, uint32_t depth, const uint32_t c[3]) {
    const uint32_t B = 1u << depth;
    return (c[0] < B && c[1] < B && c[2] < B) ? bricks[fhvox::word_index(depth, c[0], c[1], c[2])] : 0;
}
// the solid dilated by the disc in the plane perpendicular to `axis`, at the brick `at` (inside the grid)
__device__ __forceinline__ uint64_t fl_dilated(const uint64_t* __restrict__ bricks, uint32_t depth, const uint32_t at[3], uint32_t axis, uint32_t reach2) {
    const uint32_t U = fhfl::perp_u(axis), V = fhfl::perp_v(axis);
    uint64_t W[9], any = 0;
#pragma unroll
    for (uint32_t q = 0; q < 9; q++) {
        const uint32_t du = q % 3 - 1, dv = q / 3 - 1;          // (0 - 1 wraps, and so does the sum: selects, no index that depends on the axis)
        const uint32_t c[3] = {at[0] + (U == 0 ? du : 0), at[1] + (U == 1 ? du : 0) + (V == 1 ? dv : 0), at[2] + (V == 2 ? dv : 0)};
        W[q] = fl_word(bricks, depth, c);
        any |= W[q];
    }
    return any ? fhfl::dilate_disc(W, U, V, reach2) : 0;
}
__global__ void __launch_bounds__(256) k_overhangs(const uint64_t* __restrict__ bricks, uint32_t depth, uint32_t up, uint32_t reach2, uint32_t bed,
                                                   uint64_t* __restrict__ out) {
    const uint64_t n_words = (uint64_t)1 << (3 * depth);
    const uint32_t B = 1u << depth, axis = up >> 1;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < n_words; t += (uint64_t)gridDim.x * 256) {
        const uint64_t w = bricks[t];
        uint64_t res = 0;
        if (w != 0) {
            const uint32_t at[3] = {(uint32_t)t & (B - 1), (uint32_t)(t >> depth) & (B - 1), (uint32_t)(t >> (2 * depth))};
            const uint32_t step = (up & 1) ? ~0u : 1u;          // to the brick at -e(up); beyond the grid it has wrapped to above B or is B
            const uint32_t under[3] = {at[0] + (axis == 0 ? step : 0), at[1] + (axis == 1 ? step : 0), at[2] + (axis == 2 ? step : 0)};
            const uint64_t here = fl_dilated(bricks, depth, at, axis, reach2);
            const uint64_t below = (under[0] < B && under[1] < B && under[2] < B) ? fl_dilated(bricks, depth, under, axis, reach2) : (bed ? ~(uint64_t)0 : 0);
            res = fhfl::unsupported(w, here, below, up);
        }
        out[t] = res;
    }
}

// out: int32 [3][N][N], the lowest, the highest and the number of set voxels of every column along `axis`; thread q N + p is the
// column whose two other coordinates are p (the lower axis) and q
__global__ void __launch_bounds__(256) k_heights(const uint64_t* __restrict__ bricks, uint32_t depth, uint32_t axis, int32_t* __restrict__ out) {
    const uint32_t B = 1u << depth, N = 4u << depth, lgN = depth + 2;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;          // (N^2 <= 2^24)
    if (t >= N * N) return;
    const uint32_t p = t & (N - 1), q = t >> lgN, c = (p & 3) + 4 * (q & 3);
    const uint32_t U = fhfl::perp_u(axis), V = fhfl::perp_v(axis);
    const uint64_t base = fhvox::word_index(depth, U == 0 ? p >> 2 : 0, U == 1 ? p >> 2 : (V == 1 ? q >> 2 : 0), V == 2 ? q >> 2 : 0), stride = (uint64_t)1 << (axis * depth);
    int32_t lo = -1, hi = -1, n = 0;
    uint64_t next = bricks[base];
    for (uint32_t b = 0; b < B; b++) {
        const uint64_t col = fhfl::column(next, axis, c);
        if (b + 1 < B) next = bricks[base + (uint64_t)(b + 1) * stride];
        if (col) {
            if (lo < 0) lo = (int32_t)(4 * b + fhfl::column_lowest(col, axis));
            hi = (int32_t)(4 * b + fhfl::column_highest(col, axis));
            n += (int32_t)fhfl::column_count(col);
        }
    }
    const size_t plane = (size_t)N * N;
    out[t] = lo;
    out[plane + t] = hi;
    out[2 * plane + t] = n;
}

// axis x, depth >= 6: wave `row` = bz B + by takes the row's B bricks 64 at a time, a lane each.  Column c = ly + 4 lz of the row is
// voxel row (j, k) = (4 by + ly, 4 bz + lz); lane c keeps its three numbers and stores them at the end: 16 lanes, three runs of four.
__global__ void __launch_bounds__(256) k_heights_x(const uint64_t* __restrict__ bricks, uint32_t depth, int32_t* __restrict__ out) {
    const uint32_t B = 1u << depth, N = 4u << depth;
    const uint32_t lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B * B) return;          // (the same in every lane of a wave)
    const uint64_t* const words = bricks + ((uint64_t)row << depth);
    int32_t lo = -1, hi = -1, n = 0;
    uint64_t next = words[lane];
    for (uint32_t chunk = 0; chunk < B / 64; chunk++) {
        const uint64_t w = next;
        if (chunk + 1 < B / 64) next = words[(chunk + 1) * 64 + lane];
        if (__ballot(w != 0) == 0) continue;
#pragma unroll
        for (uint32_t c = 0; c < 16; c++) {
            const uint32_t bits = (uint32_t)(w >> (4 * c)) & 0xFu;
            int32_t c_lo = -1, c_hi = -1, c_n = 0;
#pragma unroll
            for (uint32_t lx = 0; lx < 4; lx++) {
                const uint64_t has = __ballot((bits >> lx) & 1u);          // the lanes - bricks of this chunk - whose voxel lx of the column is set
                if (has) {
                    const int32_t first = (int32_t)(4 * (chunk * 64 + (uint32_t)__builtin_ctzll(has)) + lx);
                    const int32_t last = (int32_t)(4 * (chunk * 64 + 63 - (uint32_t)__builtin_clzll(has)) + lx);
                    c_lo = (c_lo < 0 || first < c_lo) ? first : c_lo;
                    c_hi = last > c_hi ? last : c_hi;
                    c_n += (int32_t)__builtin_popcountll(has);
                }
            }
            if (lane == c && c_n) {
                if (lo < 0) lo = c_lo;          // (chunks ascend)
                hi = c_hi;
                n += c_n;
            }
        }
    }
    if (lane < 16) {
        const uint32_t by = row & (B - 1), bz = row >> depth;
        const size_t plane = (size_t)N * N, at = (size_t)(4 * bz + (lane >> 2)) * N + 4 * by + (lane & 3);
        out[at] = lo;
        out[plane + at] = hi;
        out[2 * plane + at] = n;
    }
}
}  // namespace fhm
