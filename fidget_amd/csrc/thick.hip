// The local thickness of a distance field (fhip_distance_thickness, include/fidget_hip.h; the host side is capi_thick.hpp): from the
// field F of edt.hip - squared distances, 0 on the foreground - T[k][j][i] = max { F(c) : F(c) > |p - c|^2 }, the squared radius of the
// largest ball that fits and holds the voxel, by the integer arithmetic of mesh_thick.hpp:
//   k_lt_shells, k_lt_need   the three tables of the domination bound up to the field's largest value: a thread per pair a >= b walks the
//                    lattice points (a, b, c <= b) and raises its shells' maxima with atomicMax; one block per table then scans it
//   k_lt_ridge       a thread per voxel: a centre (F > 0) is kept unless the ball of one of its 26 neighbours holds its own.  A wave
//                    writes its 64 keep flags as one word - the list of kept centres, in place of a compacted one - and a block adds its
//                    count to the total
//   k_lt_paint       the hot path, a scatter: a wave takes a word of keep flags and paints the balls of its centres, clipped to the grid,
//                    with `if (T[p] < f) atomicMax(&T[p], f)`, lanes consecutive along i.  Balls of squared radius up to 16 - at most 7
//                    voxels a row - go eight at a time, 8 lanes each; larger ones one after the other, a group of 8, 16, 32 or 64 lanes
//                    a row and several rows a step, rows wider than 64 voxels in several steps; gridDim.y splits a ball's rows
//   k_lt_reduce, k_lt_reduce_sum   the largest and the smallest positive T, each at its smallest index, and the voxels with T > 0
//   k_lt_hist        counts per [e_i, e_i+1) over ascending edges: bins in LDS, then one add per used bin and block
// All on one stream, none waits for another workgroup.  Max is commutative and the values are integers: the field is the same in any
// order of arrival, bit for bit.  Included by mesh.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "mesh_thick.hpp"

namespace fhm {
constexpr uint32_t FH_LT_PAINT_BLOCKS = 8192;       // blocks of k_lt_paint along x at most (four words of keep flags a step each)
constexpr uint32_t FH_LT_PAINT_SPLIT = 32;          // ... and along y at most: the parts a large ball's rows are dealt into
constexpr uint32_t FH_LT_REDUCE_BLOCKS = 2048, FH_LT_HIST_BLOCKS = 1024;
constexpr uint32_t FH_LT_MAX_EDGES = 1024;

// tables: [3][vmax + 1], zeroed; A = isqrt(vmax - 1), the largest coordinate on a shell below vmax.  Thread t is (a, b) = (t / (A + 1), t % (A + 1)).
__global__ void __launch_bounds__(256) k_lt_shells(uint32_t vmax, uint32_t A, uint32_t* __restrict__ tables) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t a = (uint32_t)(t / (A + 1)), b = (uint32_t)(t % (A + 1));
    if (a > A || b > a || a * a + b * b >= vmax) return;
    for (uint32_t c = 0; c <= b; c++) {
        const uint32_t n = a * a + b * b + c * c;
        if (n >= vmax) break;
        for (uint32_t cls = 1; cls <= 3; cls++) atomicMax(tables + (size_t)(cls - 1) * (vmax + 1) + n, fhlt::shell_value(cls, a, b, c));
    }
}
// fhlt::need_scan of table blockIdx.x in place: a thread takes a run of entries, the runs' maxima are scanned in LDS
__global__ void __launch_bounds__(1024) k_lt_need(uint32_t vmax, uint32_t* __restrict__ tables) {
    __shared__ uint32_t sh_max[1024];
    uint32_t* const table = tables + (size_t)blockIdx.x * (vmax + 1);
    const uint32_t n = vmax + 1, tid = threadIdx.x, per = (n + 1023) / 1024;
    const uint32_t lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
    uint32_t m = 0;
    for (uint32_t v = lo; v < hi; v++) m = table[v] > m ? table[v] : m;
    sh_max[tid] = m;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint32_t other = tid >= d ? sh_max[tid - d] : 0u;
        __syncthreads();
        if (other > sh_max[tid]) sh_max[tid] = other;
        __syncthreads();
    }
    uint32_t run = tid ? sh_max[tid - 1] : 0u;          // the maximum of everything before this run
    for (uint32_t v = lo; v < hi; v++) {
        const uint32_t s = table[v];
        table[v] = 1 + run;
        if (s > run) run = s;
    }
}

// keep[w]: bit b says that voxel 64 w + b is a kept centre.  N^3 is a multiple of 64, so a wave's 64 voxels are one word; the last
// block of the smallest grid (N = 4) has three idle waves.  kept: the number of set bits, added up.
__global__ void __launch_bounds__(256) k_lt_ridge(const uint32_t* __restrict__ field, uint32_t depth, const uint32_t* __restrict__ need, uint32_t vmax,
                                                  uint64_t* __restrict__ keep, unsigned long long* __restrict__ kept) {
    __shared__ uint32_t sh_count[4];
    const uint32_t N = 4u << depth, lg = depth + 2, tid = threadIdx.x;
    const uint64_t n = (uint64_t)1 << (3 * lg), idx = (uint64_t)blockIdx.x * 256 + tid;
    bool k = false;
    if (idx < n) {
        const uint32_t f = field[idx];
        if (f != 0) k = fhlt::keep_centre(field, N, (uint32_t)idx & (N - 1), (uint32_t)(idx >> lg) & (N - 1), (uint32_t)(idx >> (2 * lg)), f, need, vmax);
    }
    const uint64_t m = __ballot(k);
    if ((tid & 63) == 0) {
        if (idx < n) keep[idx >> 6] = m;
        sh_count[tid >> 6] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (tid == 0) {
        const uint32_t c = sh_count[0] + sh_count[1] + sh_count[2] + sh_count[3];
        if (c) atomicAdd(kept, (unsigned long long)c);
    }
}

// T[p] = max(T[p], f).  The plain load first: it can only return a value that T[p] held at some earlier time - T never falls - so a line
// gone stale in this CU's L1 or in another XCD's L2 costs one needless atomic and never a wrong skip.
__device__ __forceinline__ void lt_raise(uint32_t* p, uint32_t f) {
    if (*p < f) atomicMax(p, f);
}
// A wave per word of keep flags, striding over the words; blockIdx.y = part of gridDim.y of the rows of a large ball.  Every index into T
// is formed from coordinates checked against 0 .. N - 1.
__global__ void __launch_bounds__(256) k_lt_paint(const uint32_t* __restrict__ field, const uint64_t* __restrict__ keep, uint32_t depth, uint32_t* __restrict__ T) {
    const uint32_t N = 4u << depth, lg = depth + 2, lane = threadIdx.x & 63;
    const uint64_t n_words = (uint64_t)1 << (3 * lg - 6);
    for (uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < n_words; w += (uint64_t)gridDim.x * 4) {
        const uint64_t kw = keep[w];
        // (the builtin returns an int: without the casts the low half's sign would spill over the high half's flags)
        const uint64_t m = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(kw >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)kw);
        if (m == 0) continue;
        const uint32_t f_lane = field[w * 64 + lane];
        const bool large = __ballot(((m >> lane) & 1) != 0 && f_lane > fhlt::SMALL_F) != 0;
        if (!large) {
            // ---- eight balls a step, 8 lanes each: lane l of a group takes the voxels at dx = l - R of every row ----
            if (blockIdx.y != 0) continue;
            const uint32_t g = lane >> 3, l = lane & 7;
            uint64_t rest = m;
            while (rest) {
                uint32_t src = 64;          // this group's centre: the g-th set bit of `rest`, if there is one
                for (uint32_t q = 0; q < 8 && rest; q++) {
                    if (q == g) src = (uint32_t)__builtin_ctzll(rest);
                    rest &= rest - 1;
                }
                if (src == 64) continue;
                const uint64_t c = w * 64 + src;
                const uint32_t f = field[c];
                if (f == 0) continue;          // (never kept; isqrt(f - 1) would not end)
                const int32_t cx = (int32_t)((uint32_t)c & (N - 1)), cy = (int32_t)((uint32_t)(c >> lg) & (N - 1)), cz = (int32_t)(c >> (2 * lg));
                const int32_t R = (int32_t)fhlt::reach(f), dx = (int32_t)l - R, x = cx + dx;          // (R <= 3)
                if (dx > R || x < 0 || x >= (int32_t)N) continue;
                for (int32_t dz = -R; dz <= R; dz++) {
                    const int32_t z = cz + dz;
                    if (z < 0 || z >= (int32_t)N) continue;
                    for (int32_t dy = -R; dy <= R; dy++) {
                        const int32_t y = cy + dy;
                        if (y < 0 || y >= (int32_t)N || (uint32_t)(dx * dx + dy * dy + dz * dz) >= f) continue;
                        lt_raise(T + (((((size_t)z << lg) + (uint32_t)y) << lg) + (uint32_t)x), f);
                    }
                }
            }
            continue;
        }
        // ---- one ball after the other: groups of G lanes take a row each, 64 / G rows a step ----
        for (uint64_t rest = m; rest; rest &= rest - 1) {
            const uint32_t src = (uint32_t)__builtin_ctzll(rest);
            const uint64_t c = w * 64 + src;
            const uint32_t f = (uint32_t)__builtin_amdgcn_readfirstlane(field[c]);          // (the same address in every lane)
            if (f == 0) continue;          // (never kept; isqrt(f - 1) would not end)
            const int32_t cx = (int32_t)((uint32_t)c & (N - 1)), cy = (int32_t)((uint32_t)(c >> lg) & (N - 1)), cz = (int32_t)(c >> (2 * lg));
            const uint32_t R = fhlt::reach(f), side = 2 * R + 1, rows = side * side;
            const uint32_t lgG = side > 32 ? 6 : side > 16 ? 5 : side > 8 ? 4 : 3, G = 1u << lgG, per = 64u >> lgG;
            const uint32_t g = lane >> lgG, l = lane & (G - 1);
            for (uint32_t q0 = blockIdx.y * per; q0 < rows; q0 += gridDim.y * per) {
                const uint32_t q = q0 + g;
                if (q >= rows) continue;
                const int32_t dz = (int32_t)(q / side) - (int32_t)R, dy = (int32_t)(q % side) - (int32_t)R, z = cz + dz, y = cy + dy;
                const uint32_t dd = (uint32_t)(dy * dy + dz * dz);
                if (z < 0 || z >= (int32_t)N || y < 0 || y >= (int32_t)N || !fhlt::row_present(f, dd)) continue;
                uint32_t lo, hi;
                fhlt::row_span(f, (uint32_t)cx, dd, N, lo, hi);          // 0 <= lo <= hi <= N - 1
                uint32_t* const row = T + ((((size_t)z << lg) + (uint32_t)y) << lg);
                for (uint32_t x = lo + l; x <= hi; x += G) lt_raise(row + x, f);
            }
        }
    }
}

// The summary.  Two keys per voxel with T > 0, index = (k N + j) N + i < 2^30: T << 32 | (0xFFFFFFFF - index), whose maximum is the largest
// T at the smallest index (0 says: nothing positive), and T << 32 | index, whose minimum is the smallest positive T at the smallest index
// (all ones says: nothing positive).  parts: [gridDim.x][3] = {largest key, smallest key, voxels with T > 0}.
__device__ __forceinline__ void lt_block_reduce(uint64_t hi, uint64_t lo, uint64_t count, uint64_t* __restrict__ out) {
    __shared__ uint64_t sh_hi[256], sh_lo[256], sh_count[256];
    const uint32_t tid = threadIdx.x;
    sh_hi[tid] = hi; sh_lo[tid] = lo; sh_count[tid] = count;
    __syncthreads();
    for (uint32_t d = 128; d > 0; d >>= 1) {
        if (tid < d) {
            if (sh_hi[tid + d] > sh_hi[tid]) sh_hi[tid] = sh_hi[tid + d];
            if (sh_lo[tid + d] < sh_lo[tid]) sh_lo[tid] = sh_lo[tid + d];
            sh_count[tid] += sh_count[tid + d];
        }
        __syncthreads();
    }
    if (tid == 0) { out[0] = sh_hi[0]; out[1] = sh_lo[0]; out[2] = sh_count[0]; }
}
__global__ void __launch_bounds__(256) k_lt_reduce(const uint32_t* __restrict__ T, uint32_t depth, uint64_t* __restrict__ parts) {
    const uint64_t n_runs = (uint64_t)16 << (3 * depth);          // runs of four voxels
    uint64_t hi = 0, lo = ~(uint64_t)0, count = 0;
    for (uint64_t run = (uint64_t)blockIdx.x * 256 + threadIdx.x; run < n_runs; run += (uint64_t)gridDim.x * 256) {
        const uint4 v = ((const uint4*)T)[run];
        const uint32_t t[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            if (t[u] == 0) continue;
            const uint32_t index = (uint32_t)(4 * run + u);
            const uint64_t kh = ((uint64_t)t[u] << 32) | (0xFFFFFFFFu - index), kl = ((uint64_t)t[u] << 32) | index;
            count++;
            if (kh > hi) hi = kh;
            if (kl < lo) lo = kl;
        }
    }
    lt_block_reduce(hi, lo, count, parts + 3 * (size_t)blockIdx.x);
}
__global__ void __launch_bounds__(256) k_lt_reduce_sum(const uint64_t* __restrict__ parts, uint32_t n_parts, uint64_t* __restrict__ out) {
    uint64_t hi = 0, lo = ~(uint64_t)0, count = 0;
    for (uint32_t p = threadIdx.x; p < n_parts; p += 256) {
        if (parts[3 * (size_t)p] > hi) hi = parts[3 * (size_t)p];
        if (parts[3 * (size_t)p + 1] < lo) lo = parts[3 * (size_t)p + 1];
        count += parts[3 * (size_t)p + 2];
    }
    lt_block_reduce(hi, lo, count, out);
}

// counts[b] += the values v of the field with edges[b] <= v < edges[b + 1], b < n_edges - 1; 2 <= n_edges <= 1024, the edges ascending
// (equal neighbours make an empty bin).  counts are zeroed before.  A thread gathers a run of equal bins before it touches LDS: most of a
// field is 0.
__global__ void __launch_bounds__(256) k_lt_hist(const uint32_t* __restrict__ T, uint64_t n, const uint32_t* __restrict__ edges, uint32_t n_edges,
                                                 unsigned long long* __restrict__ counts) {
    __shared__ uint32_t sh_edges[FH_LT_MAX_EDGES], sh_bins[FH_LT_MAX_EDGES];
    for (uint32_t e = threadIdx.x; e < n_edges; e += 256) { sh_edges[e] = edges[e]; sh_bins[e] = 0; }
    __syncthreads();
    const uint32_t first = sh_edges[0], last = sh_edges[n_edges - 1];
    uint32_t bin = 0, pending = 0;
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256) {
        const uint32_t v = T[p];
        if (v < first || v >= last) continue;
        uint32_t lo = 0, hi = n_edges - 1;          // edges[lo] <= v < edges[hi]
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (sh_edges[mid] <= v) lo = mid; else hi = mid;
        }
        if (lo != bin && pending) { atomicAdd(&sh_bins[bin], pending); pending = 0; }
        bin = lo;
        pending++;
    }
    if (pending) atomicAdd(&sh_bins[bin], pending);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b + 1 < n_edges; b += 256)
        if (sh_bins[b]) atomicAdd(counts + b, (unsigned long long)sh_bins[b]);
}
}  // namespace fhm
