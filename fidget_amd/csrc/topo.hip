// The check of a triangle mesh (fhip_triangles_topology, fhip_mesh_topology, include/fidget_hip.h; the host side is capi_topo.hpp): weld,
// edges, shells.  The arithmetic and the two inserts are mesh_topo.hpp's, which the tests also build for the host.  Corner c = 3 t + k.
//   k_mt_check      a lane per triangle: rejected if a coordinate is not finite or an index lies at or beyond n_vertices (never read)
//   k_mt_weld       a lane per corner: fhtopo::vertex_insert -> the corner's slot
//   k_mt_vflag      flag[c] = 1 where c is the first corner of its vertex; (prefix sums: k_scan_block / k_scan_add of mesh.hip)
//   k_mt_vemit      the first corners write their positions, bits unchanged, at their rank; every corner gets its vertex's rank
//   k_mt_ids        without the weld: a corner's vertex is its index; a byte per vertex in use, counted by k_mt_used
//   k_mt_edges      a lane per triangle: its row of `triangles`, parent[t] = t, degenerate or three fhtopo::edge_insert -> the slots
//   k_mt_link       a lane per triangle: per corner, whether it is the first use of its edge and the edge's classes - one byte, kept by
//                   the handle for the edge lists - the classes counted at the first use, and the triangle united with the triangle of
//                   the first use (cc_unite of mesh.hip: towards the smaller root, so a shell's root is its first triangle)
//   (k_cc_flatten of mesh.hip; then the roots that are not degenerate flagged - k_mt_roots - and their prefix sums)
//   k_mt_number     triangle_shell[t] = the rank of its root, EMPTY for a degenerate triangle; a root writes `first`
//   k_mt_table      the shells' triangles, unbalanced edges (counted at the first use), bounds (atomicMin / Max on the ordered-integer
//                   form) and the two float64 sums (atomic adds).  The triangles in equal contiguous shares, one per wave, walked 64
//                   at a time.  Consecutive triangles nearly always lie in one shell: while the 64 of a turn do, and it is the shell of
//                   the turn before, the lanes only add to sums of their own; the wave reduces and one lane sends them when the
//                   shell changes and at the end of the share.  A turn with several shells sends each of up to MT_ROUNDS of them
//                   reduced over the wave, and what is still left lane by lane.  (One lane per triangle and a send per wave, to one
//                   address for a mesh of one shell, took 11.3 ms at 59 M triangles: profiles/mesh_topology/README.md.)
//   k_mt_eflag / k_mt_eemit   the edge list of one class: the first uses of that class flagged, ranked, written as (a, b)
// Everything but the two float64 sums is an integer that does not depend on the order of arrival: a vertex's first corner and an
// edge's first use are minima, the counts are sums, a shell's root is the minimum of its triangles, and no list is written in slot
// order - which slot a key gets does depend on who won a race.  The float64 sums add the same terms in an order that may differ from
// run to run.  No kernel waits for another workgroup; the only loops over memory that other waves write are the probe sequences,
// which visit every slot at most once, and cc_find / cc_unite, bounded as mesh.hip says.  Included by mesh.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "mesh_topo.hpp"

namespace fhm {
// the counters of a call, uint64 each: FH_MT_ROWS rows of FH_MT_COUNTERS, the row chosen by the wave's number, summed by the host
constexpr uint32_t FH_MT_REJECTED = 0, FH_MT_DEGENERATE = 1, FH_MT_USED = 2, FH_MT_EDGES = 3, FH_MT_BOUNDARY = 4, FH_MT_FLIPPED = 5, FH_MT_NONMANIFOLD = 6,
                   FH_MT_UNBALANCED = 7, FH_MT_OVERFLOW = 8, FH_MT_COUNTERS = 16, FH_MT_ROWS = 256;
constexpr uint32_t MT_ROUNDS = 4;
constexpr uint32_t FH_MT_TABLE_BLOCKS = 4096;          // k_mt_table: at most so many blocks of 256 - 16 waves to each of 256 CUs, four shares to each

struct MtAtomic {          // fhtopo's memory operations on the device: relaxed, agent scope
    __device__ static uint32_t load32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ static uint32_t cas32(uint32_t* p, uint32_t expect, uint32_t v) { return atomicCAS(p, expect, v); }
    __device__ static void min32(uint32_t* p, uint32_t v) { (void)atomicMin(p, v); }
    __device__ static uint64_t load64(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ static uint64_t cas64(uint64_t* p, uint64_t expect, uint64_t v) { return atomicCAS((unsigned long long*)p, (unsigned long long)expect, (unsigned long long)v); }
    __device__ static void add64(uint64_t* p, uint64_t v) { (void)atomicAdd((unsigned long long*)p, (unsigned long long)v); }
    __device__ static void max64(uint64_t* p, uint64_t v) { (void)atomicMax((unsigned long long*)p, (unsigned long long)v); }
};

__device__ __forceinline__ void mt_count(uint64_t* counters, uint32_t which, uint32_t in_wave) {          // (called by one lane of the wave)
    const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (in_wave) atomicAdd((unsigned long long*)counters + (wave & (FH_MT_ROWS - 1)) * FH_MT_COUNTERS + which, (unsigned long long)in_wave);
}
__device__ __forceinline__ void mt_count_if(uint64_t* counters, uint32_t which, bool mine) {          // (called by every lane of the wave)
    const uint32_t n = (uint32_t)__popcll(__ballot(mine));
    if ((threadIdx.x & 63) == 0) mt_count(counters, which, n);
}

__global__ void __launch_bounds__(256) k_mt_check(const float* __restrict__ vertices, uint64_t n_vertices, const uint64_t* __restrict__ triangles, uint32_t n_triangles,
                                                  uint64_t* __restrict__ counters) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;          // (64 bits: n_triangles rounded up to 256 may pass 2^32)
    bool rejected = false;
    if (t < n_triangles) {
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) {
            const uint64_t at = triangles ? triangles[3 * t + k] : 3 * t + k;
            if (at >= n_vertices) rejected = true;
            else if (!fhtopo::finite3(vertices + 3 * at)) rejected = true;
        }
    }
    mt_count_if(counters, FH_MT_REJECTED, rejected);
}

__global__ void __launch_bounds__(256) k_mt_weld(fhtopo::Corners in, uint32_t n_corners, uint32_t* table, uint32_t log2, uint32_t* __restrict__ corner_slot,
                                                 uint64_t* __restrict__ counters) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool lost = false;
    if (c < n_corners) {
        uint64_t slot = 0;
        lost = !fhtopo::vertex_insert<MtAtomic>(in, table, log2, (uint32_t)c, slot);
        corner_slot[c] = (uint32_t)slot;          // (a slot index is below 2^32)
    }
    mt_count_if(counters, FH_MT_OVERFLOW, lost);
}
__global__ void __launch_bounds__(256) k_mt_vflag(const uint32_t* __restrict__ corner_slot, const uint32_t* __restrict__ table, uint32_t n_corners, uint32_t* __restrict__ flag) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < n_corners) flag[c] = fhtopo::vertex_first(table, corner_slot[c]) == (uint32_t)c ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_mt_vemit(fhtopo::Corners in, const uint32_t* __restrict__ corner_slot, const uint32_t* __restrict__ table,
                                                  const uint32_t* __restrict__ rank, uint32_t n_corners, float* __restrict__ out_vertices, uint32_t* __restrict__ vid) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_corners) return;
    const uint32_t f = fhtopo::vertex_first(table, corner_slot[c]), v = rank[f];
    vid[c] = v;
    if (f == (uint32_t)c) {
        const float* const p = fhtopo::position(in, (uint32_t)c);
        out_vertices[3 * (uint64_t)v] = p[0]; out_vertices[3 * (uint64_t)v + 1] = p[1]; out_vertices[3 * (uint64_t)v + 2] = p[2];
    }
}
// used: a byte per vertex, all zero before; every lane that uses a vertex stores the same 1 - no atomic: a bit per vertex set by atomicOr,
// 32 vertices to a word and six corners to a vertex, took 12.8 ms at 59 M triangles (profiles/mesh_topology/README.md)
__global__ void __launch_bounds__(256) k_mt_ids(const uint64_t* __restrict__ triangles, uint32_t n_corners, uint32_t* __restrict__ vid, uint8_t* used) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_corners) return;
    const uint32_t v = (uint32_t)triangles[c];          // (checked: below n_vertices <= 2^32 - 2)
    vid[c] = v;
    used[v] = 1;
}
// ... counted four at a time: n_words words of four bytes, the bytes past the last vertex zero
__global__ void __launch_bounds__(256) k_mt_used(const uint32_t* __restrict__ used, uint32_t n_words, uint64_t* __restrict__ counters) {
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t n = fhvox::wave_sum(w < n_words ? (uint32_t)__popc(used[w] & 0x01010101u) : 0u);
    if ((threadIdx.x & 63) == 0) mt_count(counters, FH_MT_USED, n);
}

__global__ void __launch_bounds__(256) k_mt_edges(const uint32_t* __restrict__ vid, uint32_t n_triangles, uint64_t* table, uint32_t log2,
                                                  uint64_t* __restrict__ out_triangles, uint32_t* __restrict__ parent, uint32_t* __restrict__ corner_slot,
                                                  uint64_t* __restrict__ counters) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool lost = false, flat = false;
    if (t < n_triangles) {
        const uint32_t v[3] = {vid[3 * t], vid[3 * t + 1], vid[3 * t + 2]};
        out_triangles[3 * t] = v[0]; out_triangles[3 * t + 1] = v[1]; out_triangles[3 * t + 2] = v[2];
        parent[t] = (uint32_t)t;
        flat = fhtopo::degenerate(v[0], v[1], v[2]);
        if (!flat) {
#pragma unroll
            for (uint32_t k = 0; k < 3; k++) {
                uint64_t slot = 0;
                lost = !fhtopo::edge_insert<MtAtomic>(table, log2, v[k], v[(k + 1) % 3], (uint32_t)(3 * t + k), slot) || lost;
                corner_slot[3 * t + k] = (uint32_t)slot;
            }
        }
    }
    mt_count_if(counters, FH_MT_DEGENERATE, flat);
    mt_count_if(counters, FH_MT_OVERFLOW, lost);
}

__global__ void __launch_bounds__(256) k_mt_link(const uint64_t* __restrict__ triangles, uint32_t n_triangles, const uint64_t* __restrict__ table,
                                                 const uint32_t* __restrict__ corner_slot, uint8_t* __restrict__ corner_class,
                                                 uint32_t* parent, uint64_t* __restrict__ counters) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t n[fhtopo::N_KINDS + 1] = {0, 0, 0, 0, 0};          // first uses; of them boundary, flipped, nonmanifold, unbalanced
    if (t < n_triangles) {
        const bool flat = fhtopo::degenerate((uint32_t)triangles[3 * t], (uint32_t)triangles[3 * t + 1], (uint32_t)triangles[3 * t + 2]);
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) {
            const uint64_t c = 3 * t + k;
            uint32_t cls = 0;
            if (!flat) {
                const uint32_t s = corner_slot[c], f = fhtopo::edge_first(table, s);
                if (f == (uint32_t)c) {
                    cls = fhtopo::FIRST_USE | fhtopo::edge_class(fhtopo::edge_counts(table, s));
                    n[0]++;
#pragma unroll
                    for (uint32_t kind = 0; kind < fhtopo::N_KINDS; kind++) n[kind + 1] += (cls >> kind) & 1u;
                } else {
                    cc_unite(parent, (uint32_t)t, f / 3);
                }
            }
            corner_class[c] = (uint8_t)cls;
        }
    }
#pragma unroll
    for (uint32_t i = 0; i <= fhtopo::N_KINDS; i++) {
        const uint32_t sum = fhvox::wave_sum(n[i]);
        if ((threadIdx.x & 63) == 0) mt_count(counters, FH_MT_EDGES + i, sum);
    }
}
static_assert(FH_MT_BOUNDARY == FH_MT_EDGES + 1 && FH_MT_FLIPPED == FH_MT_EDGES + 2 && FH_MT_NONMANIFOLD == FH_MT_EDGES + 3 && FH_MT_UNBALANCED == FH_MT_EDGES + 4 &&
              fhtopo::BOUNDARY == 1 && fhtopo::FLIPPED == 2 && fhtopo::NONMANIFOLD == 4 && fhtopo::UNBALANCED == 8, "k_mt_link counts the classes by their bits' places");

__global__ void __launch_bounds__(256) k_mt_roots(const uint32_t* __restrict__ parent, const uint64_t* __restrict__ triangles, uint32_t n_triangles, uint32_t* __restrict__ flag) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n_triangles)
        flag[t] = parent[t] == (uint32_t)t && !fhtopo::degenerate((uint32_t)triangles[3 * t], (uint32_t)triangles[3 * t + 1], (uint32_t)triangles[3 * t + 2]) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_mt_number(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ flag,
                                                   uint32_t n_triangles, uint32_t* __restrict__ shell, uint32_t* __restrict__ shell_first) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_triangles) return;
    const uint32_t root = parent[t];          // (flattened: a degenerate triangle was united with nothing and is its own root, not flagged)
    const bool in_shell = flag[root] != 0;
    shell[t] = in_shell ? rank[root] : fhtopo::EMPTY;
    if (in_shell && root == (uint32_t)t) shell_first[rank[root]] = (uint32_t)t;
}

struct MtShellTable {          // the per-shell columns on the device; lo all ones and everything else zero before
    unsigned long long* triangles;
    unsigned long long* unbalanced;
    double* volume6;
    double* area2;
    uint32_t* lo;          // [shells][3], ordered-integer form
    uint32_t* hi;
};
__device__ __forceinline__ uint32_t mt_wave_min(uint32_t v) {
#pragma unroll
    for (uint32_t step = 32; step > 0; step >>= 1) { const uint32_t o = __shfl_xor(v, step, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ uint32_t mt_wave_max(uint32_t v) {
#pragma unroll
    for (uint32_t step = 32; step > 0; step >>= 1) { const uint32_t o = __shfl_xor(v, step, 64); v = o > v ? o : v; }
    return v;
}
// what a lane, and after mt_reduce a wave, holds of one shell
struct MtPart {
    uint32_t n, unbalanced, lo[3], hi[3];
    double v6, a2;
};
__device__ __forceinline__ void mt_clear(MtPart& p) {
    p.n = p.unbalanced = 0;
    p.lo[0] = p.lo[1] = p.lo[2] = 0xFFFFFFFFu;
    p.hi[0] = p.hi[1] = p.hi[2] = 0;
    p.v6 = p.a2 = 0;
}
__device__ __forceinline__ void mt_add(MtPart& p, const MtPart& q) {
    p.n += q.n; p.unbalanced += q.unbalanced;
#pragma unroll
    for (uint32_t a = 0; a < 3; a++) { p.lo[a] = q.lo[a] < p.lo[a] ? q.lo[a] : p.lo[a]; p.hi[a] = q.hi[a] > p.hi[a] ? q.hi[a] : p.hi[a]; }
    p.v6 += q.v6; p.a2 += q.a2;
}
__device__ __forceinline__ MtPart mt_reduce(MtPart p) {          // over the wave; every lane gets the result
    p.n = fhvox::wave_sum(p.n); p.unbalanced = fhvox::wave_sum(p.unbalanced);
#pragma unroll
    for (uint32_t a = 0; a < 3; a++) { p.lo[a] = mt_wave_min(p.lo[a]); p.hi[a] = mt_wave_max(p.hi[a]); }
    p.v6 = fhvox::wave_sum(p.v6); p.a2 = fhvox::wave_sum(p.a2);
    return p;
}
__device__ __forceinline__ void mt_send(const MtShellTable& T, uint32_t s, const MtPart& p) {
    atomicAdd(T.triangles + s, (unsigned long long)p.n);
    if (p.unbalanced) atomicAdd(T.unbalanced + s, (unsigned long long)p.unbalanced);
#pragma unroll
    for (uint32_t a = 0; a < 3; a++) {          // (a look first: the bounds only move one way, and the current value is never better than the true one)
        if (p.lo[a] < __hip_atomic_load(T.lo + 3 * (uint64_t)s + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) (void)atomicMin(T.lo + 3 * (uint64_t)s + a, p.lo[a]);
        if (p.hi[a] > __hip_atomic_load(T.hi + 3 * (uint64_t)s + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) (void)atomicMax(T.hi + 3 * (uint64_t)s + a, p.hi[a]);
    }
    (void)unsafeAtomicAdd(T.volume6 + s, p.v6);          // (the hardware's float64 add: the table is ordinary device memory)
    (void)unsafeAtomicAdd(T.area2 + s, p.a2);
}
// per_wave: a multiple of 64; the grid's waves times it cover n_triangles
__global__ void __launch_bounds__(256) k_mt_table(const float* __restrict__ vertices, const uint64_t* __restrict__ triangles, const uint32_t* __restrict__ shell,
                                                  const uint8_t* __restrict__ corner_class, uint32_t n_triangles, uint64_t per_wave, MtShellTable T) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t first = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * per_wave;          // (the same in every lane of a wave, as all of the loop's bounds)
    const uint64_t end = first + per_wave < n_triangles ? first + per_wave : n_triangles;
    uint32_t held = fhtopo::EMPTY;          // the shell the lanes' `sum` belongs to: the same in every lane
    MtPart sum;
    mt_clear(sum);
    for (uint64_t t0 = first; t0 < end; t0 += 64) {
        const uint64_t t = t0 + lane;
        const uint32_t s = t < end ? shell[t] : fhtopo::EMPTY;
        bool todo = s != fhtopo::EMPTY;
        MtPart mine;
        mt_clear(mine);
        if (todo) {
            const float* p[3];
            mine.n = 1;
#pragma unroll
            for (uint32_t k = 0; k < 3; k++) {
                p[k] = vertices + 3 * triangles[3 * t + k];
                mine.unbalanced += (corner_class[3 * t + k] & fhtopo::UNBALANCED) ? 1u : 0u;          // (set at the edge's first use only)
#pragma unroll
                for (uint32_t a = 0; a < 3; a++) {
                    const uint32_t o = fhtopo::ordered(fhtopo::canon(p[k][a]));
                    mine.lo[a] = o < mine.lo[a] ? o : mine.lo[a];
                    mine.hi[a] = o > mine.hi[a] ? o : mine.hi[a];
                }
            }
            mine.v6 = fhtopo::volume6_term(p[0], p[1], p[2]);
            mine.a2 = fhtopo::area2_term(p[0], p[1], p[2]);
        }
        const uint64_t left = __ballot(todo);          // (the same in every lane: the turns below are the wave's)
        if (!left) continue;
        const uint32_t s0 = __shfl(s, (uint32_t)__ffsll((unsigned long long)left) - 1, 64);
        if (__ballot(todo && s != s0) == 0) {          // one shell in these 64 triangles: the lanes keep adding, nothing is sent
            if (s0 != held) {
                if (held != fhtopo::EMPTY) { const MtPart w = mt_reduce(sum); if (lane == 0) mt_send(T, held, w); }
                held = s0;
                mt_clear(sum);
            }
            mt_add(sum, mine);
            continue;
        }
        for (uint32_t round = 0; round < MT_ROUNDS; round++) {          // several: the shell of the first lane left, reduced and sent, a few times
            const uint64_t now = __ballot(todo);
            if (!now) break;
            const uint32_t leader = (uint32_t)__ffsll((unsigned long long)now) - 1, sr = __shfl(s, leader, 64);
            const bool in = todo && s == sr;
            MtPart part;
            mt_clear(part);
            if (in) part = mine;
            const MtPart w = mt_reduce(part);
            if (lane == leader) mt_send(T, sr, w);
            todo = todo && !in;
        }
        if (todo) mt_send(T, s, mine);          // ... and what is still left, every lane its own
    }
    if (held != fhtopo::EMPTY) { const MtPart w = mt_reduce(sum); if (lane == 0) mt_send(T, held, w); }
}

__global__ void __launch_bounds__(256) k_mt_eflag(const uint8_t* __restrict__ corner_class, uint32_t n_corners, uint32_t kind_bit, uint32_t* __restrict__ flag) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < n_corners) flag[c] = (corner_class[c] & fhtopo::FIRST_USE) && (corner_class[c] & kind_bit) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_mt_eemit(const uint64_t* __restrict__ triangles, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank,
                                                  uint32_t n_corners, uint32_t* __restrict__ out) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_corners || !flag[c]) return;
    const uint64_t key = fhtopo::edge_key((uint32_t)triangles[c], (uint32_t)triangles[fhtopo::next_corner((uint32_t)c)]);
    out[2 * (uint64_t)rank[c]] = (uint32_t)(key >> 32);
    out[2 * (uint64_t)rank[c] + 1] = (uint32_t)key;
}
}  // namespace fhm
