// The slices of a triangle mesh (fhip_topology_slices, include/fidget_hip.h; the host side is capi_slice.hpp): the closed polygons in
// which planes z = const cut the welded indexed mesh of a topology.  The arithmetic is mesh_slice.hpp's, which the tests also build for
// the host; the table's insert is mesh_topo.hpp's, with the memory operations of topo.hip (MtAtomic).  Corner c = 3 t + k.
//   k_ms_levels     a lane per vertex: a(v), an upper bound search in the planes
//   k_ms_count      a lane per triangle: the planes it crosses - its segments - and how many of its corners' edges cross any: the
//                   crossing corners, which size the table.  64-bit totals of both
//   k_ms_insert     a lane per triangle: each corner whose edge crosses a plane into the edge table (fhtopo::edge_insert) -> its slot
//   k_ms_first      a lane per corner: the first corner of a crossing edge counts the edge's planes, every other corner nothing; the
//                   64-bit total.  (Prefix sums over the corners: k_scan_block / k_scan_add of mesh.hip)
//   k_ms_ids        a lane per corner: the table look-up, once per triangle edge - the prefix sum at the first corner of its edge
//   k_ms_emit       a lane per CROSSING: the corner that owns it by a search in the prefix sums, its plane, edge and position
//   k_ms_segments   a lane per SEGMENT: its triangle by a search in the triangles' prefix sums, its plane, the lone corner, the two
//                   crossings' ids; the record, out and in (a 64-bit add), next (a 64-bit max of the complement: the smallest triangle),
//                   and the union of the two crossings (cc_unite of mesh.hip: towards the smaller root, so a loop's root is its leader)
//   (k_cc_flatten, k_cc_roots, the prefix sums, k_cc_number of mesh.hip: loop_of)
//   k_ms_measure_x  a lane per crossing: next and the degree byte from their words; into its loop's row its count, whether it is
//                   irregular, its bounds (atomicMin / Max on the ordered-integer form); the root writes leader and plane
//   k_ms_measure_s  a lane per segment: its count and its area2 term into its loop's row (a float64 add: the one order of arrival)
// The work of the three passes that write records is dealt by the prefix sums, not one lane per edge or per triangle: twelve triangles
// under 4096 planes are 16384 crossings and as many lanes, and consecutive lanes store consecutive records.  A wave whose live lanes
// all belong to one loop adds their shares up first and sends one set of atomics.  Everything but area2 is an integer, or a float
// computed from the input alone, that does not depend on the order of arrival.  No kernel waits for another workgroup; the loops over
// memory that other waves write are the probe sequence, which visits every slot at most once, and cc_find / cc_unite, bounded as
// mesh.hip says.  Included by mesh.hip, after topo.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "mesh_slice.hpp"

namespace fhm {
// the counters of a call, in the rows of topo.hip's (FH_MT_ROWS x FH_MT_COUNTERS, the row by the wave's number, summed by the host)
constexpr uint32_t FH_MS_CORNERS = 0, FH_MS_SEGMENTS = 1, FH_MS_CROSSINGS = 2, FH_MS_OVERFLOW = 3;

__device__ __forceinline__ void ms_count(uint64_t* counters, uint32_t which, uint64_t mine) {          // (called by every lane of the wave)
    const uint64_t sum = fhvox::wave_sum(mine);
    const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd((unsigned long long*)counters + (wave & (FH_MT_ROWS - 1)) * FH_MT_COUNTERS + which, (unsigned long long)sum);
}
// triangle t: its vertex ids and their levels; false: degenerate
__device__ __forceinline__ bool ms_corners(const uint64_t* __restrict__ triangles, const uint32_t* __restrict__ level, uint64_t t, uint32_t v[3], uint32_t a[3]) {
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) { v[k] = (uint32_t)triangles[3 * t + k]; a[k] = level[v[k]]; }
    return !fhtopo::degenerate(v[0], v[1], v[2]);
}

__global__ void __launch_bounds__(256) k_ms_levels(const float* __restrict__ vertices, uint64_t n_vertices, const float* __restrict__ zs, uint32_t n_planes,
                                                   uint32_t* __restrict__ level) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n_vertices) level[v] = fhslice::level(zs, n_planes, vertices[3 * v + 2]);
}
__global__ void __launch_bounds__(256) k_ms_count(const uint64_t* __restrict__ triangles, const uint32_t* __restrict__ level, uint32_t n_triangles,
                                                  uint32_t* __restrict__ seg_count, uint64_t* __restrict__ counters) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t corners = 0, segments = 0;
    if (t < n_triangles) {
        uint32_t v[3], a[3];
        if (ms_corners(triangles, level, t, v, a)) {
            corners = (a[0] != a[1] ? 1u : 0u) + (a[1] != a[2] ? 1u : 0u) + (a[2] != a[0] ? 1u : 0u);
            segments = fhslice::n_planes(fhslice::triangle_range(a));
        }
        seg_count[t] = segments;
    }
    ms_count(counters, FH_MS_CORNERS, corners);
    ms_count(counters, FH_MS_SEGMENTS, segments);
}
__global__ void __launch_bounds__(256) k_ms_insert(const uint64_t* __restrict__ triangles, const uint32_t* __restrict__ level, uint32_t n_triangles, uint64_t* table,
                                                   uint32_t log2, uint32_t* __restrict__ corner_slot, uint64_t* __restrict__ counters) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool lost = false;
    if (t < n_triangles) {
        uint32_t v[3], a[3];
        const bool live = ms_corners(triangles, level, t, v, a);
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) {
            uint32_t slot = fhslice::NONE;
            if (live) lost = !fhslice::corner_insert<MtAtomic>(table, log2, v[k], v[(k + 1) % 3], a[k], a[(k + 1) % 3], (uint32_t)(3 * t + k), slot) || lost;
            corner_slot[3 * t + k] = slot;
        }
    }
    ms_count(counters, FH_MS_OVERFLOW, lost ? 1u : 0u);
}
__global__ void __launch_bounds__(256) k_ms_first(const uint64_t* __restrict__ table, const uint32_t* __restrict__ corner_slot, const uint32_t* __restrict__ level,
                                                  uint32_t n_corners, uint32_t* __restrict__ count, uint64_t* __restrict__ counters) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t n = 0;
    if (c < n_corners) {
        const uint32_t s = corner_slot[c];
        if (s != fhslice::NONE && fhtopo::edge_first(table, s) == (uint32_t)c) {
            const uint64_t key = fhslice::edge_key_at(table, s);
            n = fhslice::n_planes(fhslice::edge_range(level[(uint32_t)(key >> 32)], level[(uint32_t)key]));
        }
        count[c] = n;
    }
    ms_count(counters, FH_MS_CROSSINGS, n);
}
// corner_slot -> the id of the edge's first crossing, in place; NONE stays
__global__ void __launch_bounds__(256) k_ms_ids(const uint64_t* __restrict__ table, const uint32_t* __restrict__ base, uint32_t n_corners, uint32_t* corner_slot) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_corners) return;
    const uint32_t s = corner_slot[c];
    if (s != fhslice::NONE) corner_slot[c] = base[fhtopo::edge_first(table, s)];
}
// base: the exclusive prefix sums of k_ms_first's counts, n_corners + 1 of them; n = base[n_corners] crossings
__global__ void __launch_bounds__(256) k_ms_emit(const float* __restrict__ vertices, const uint64_t* __restrict__ triangles, const uint32_t* __restrict__ level,
                                                 const float* __restrict__ zs, const uint32_t* __restrict__ base, uint32_t n_corners, uint32_t n,
                                                 float2* __restrict__ xy, uint32_t* __restrict__ plane, uint2* __restrict__ edge) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= n) return;
    const uint32_t c = (uint32_t)fhslice::owner(base, n_corners, (uint32_t)x);
    const uint64_t key = fhtopo::edge_key((uint32_t)triangles[c], (uint32_t)triangles[fhtopo::next_corner(c)]);
    const uint32_t u = (uint32_t)(key >> 32), v = (uint32_t)key;
    const uint32_t p = fhslice::edge_range(level[u], level[v]).lo + ((uint32_t)x - base[c]);
    float out[2];
    fhslice::position(vertices + 3 * (uint64_t)u, vertices + 3 * (uint64_t)v, zs[p], out);
    xy[x] = make_float2(out[0], out[1]);
    plane[x] = p;
    edge[x] = make_uint2(u, v);
}
// seg_base: the exclusive prefix sums of k_ms_count's segments, n_triangles + 1 of them; m = seg_base[n_triangles] segments.
// next_words and degree: n words each, zeros before; parent[x] = x
__global__ void __launch_bounds__(256) k_ms_segments(const uint64_t* __restrict__ triangles, const uint32_t* __restrict__ level, const uint32_t* __restrict__ seg_base,
                                                     uint32_t n_triangles, uint32_t m, const uint32_t* __restrict__ corner_base, uint32_t n,
                                                     uint2* __restrict__ segments, uint64_t* next_words, uint64_t* degree, uint32_t* parent) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= m) return;
    const uint64_t t = fhslice::owner(seg_base, n_triangles, (uint32_t)s);
    uint32_t v[3], a[3], id[2];
    (void)ms_corners(triangles, level, t, v, a);          // (not degenerate: it has segments)
    const uint32_t p = fhslice::triangle_range(a).lo + ((uint32_t)s - seg_base[t]);
    const fhslice::SegmentEdges e = fhslice::segment_edges(a, p);
    const uint32_t k[2] = {e.from, e.to};
#pragma unroll
    for (uint32_t q = 0; q < 2; q++) id[q] = fhslice::crossing_id(corner_base[3 * t + k[q]], fhslice::edge_range(a[k[q]], a[(k[q] + 1) % 3]), p);
    segments[s] = make_uint2(id[0], id[1]);
    if (id[0] >= n || id[1] >= n) return;          // (never: both edges cross p, and their crossings were counted)
    MtAtomic::add64(degree + id[0], 1);
    MtAtomic::add64(degree + id[1], (uint64_t)1 << 32);
    MtAtomic::max64(next_words + id[0], fhslice::next_word((uint32_t)t, id[1]));
    cc_unite(parent, id[0], id[1]);
}

struct MsLoopTable {          // the per-loop columns on the device; lo all ones and everything else zero before
    double* area2;
    uint32_t *leader, *plane, *crossings, *segments, *irregular;
    uint32_t *lo, *hi;          // [loops][2], ordered-integer form
};
__global__ void __launch_bounds__(256) k_ms_measure_x(const float2* __restrict__ xy, const uint32_t* __restrict__ plane, const uint32_t* __restrict__ parent,
                                                      const uint32_t* __restrict__ loop_of, const uint64_t* __restrict__ next_words, const uint64_t* __restrict__ degree,
                                                      uint32_t n, uint32_t* __restrict__ next, uint8_t* __restrict__ degree_byte, MsLoopTable T) {
    const uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = x < n;
    if (__ballot(live) == 0) return;          // (ids ascend with the lanes: lane 0 of every other wave is live)
    uint32_t l = 0, count = 0, odd = 0, lo_x = ~0u, lo_y = ~0u, hi_x = 0, hi_y = 0;
    if (live) {
        const uint64_t d = degree[x];
        const float2 p = xy[x];
        l = loop_of[x];
        next[x] = fhslice::next_of(next_words[x]);
        degree_byte[x] = fhslice::degree_byte(d);
        count = 1;
        odd = fhslice::irregular(d) ? 1u : 0u;
        lo_x = hi_x = fhtopo::ordered(fhtopo::canon(p.x));
        lo_y = hi_y = fhtopo::ordered(fhtopo::canon(p.y));
        if (parent[x] == (uint32_t)x) { T.leader[l] = (uint32_t)x; T.plane[l] = plane[x]; }
    }
    // the crossings of a long loop would all meet in its one row: where a wave's live lanes all belong to one loop, lane 0 sends their sums
    const uint32_t l0 = (uint32_t)__shfl((int)l, 0, 64);
    if (__ballot(live && l != l0) == 0) {
        count = fhvox::wave_sum(count);
        odd = fhvox::wave_sum(odd);
        lo_x = mt_wave_min(lo_x); lo_y = mt_wave_min(lo_y);
        hi_x = mt_wave_max(hi_x); hi_y = mt_wave_max(hi_y);
        if ((threadIdx.x & 63) != 0) return;
    } else if (!live) {
        return;
    }
    atomicAdd(T.crossings + l, count);
    if (odd) atomicAdd(T.irregular + l, odd);
    uint32_t* const lo = T.lo + 2 * (size_t)l;
    uint32_t* const hi = T.hi + 2 * (size_t)l;
    // (a look first: the bounds only move one way, and the current value is never better than the true one)
    if (lo_x < __hip_atomic_load(lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) (void)atomicMin(lo, lo_x);
    if (lo_y < __hip_atomic_load(lo + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) (void)atomicMin(lo + 1, lo_y);
    if (hi_x > __hip_atomic_load(hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) (void)atomicMax(hi, hi_x);
    if (hi_y > __hip_atomic_load(hi + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) (void)atomicMax(hi + 1, hi_y);
}
__global__ void __launch_bounds__(256) k_ms_measure_s(const float2* __restrict__ xy, const uint2* __restrict__ segments, const uint32_t* __restrict__ loop_of, uint32_t m,
                                                      MsLoopTable T) {
    const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = s < m;
    if (__ballot(live) == 0) return;
    uint32_t l = 0, count = 0;
    double term = 0;
    if (live) {
        const uint2 e = segments[s];
        const float2 a = xy[e.x], b = xy[e.y];
        const float from[2] = {a.x, a.y}, to[2] = {b.x, b.y};
        l = loop_of[e.x];
        term = fhslice::area2_term(from, to);
        count = 1;
    }
    const uint32_t l0 = (uint32_t)__shfl((int)l, 0, 64);
    if (__ballot(live && l != l0) == 0) {
        count = fhvox::wave_sum(count);
        term = fhvox::wave_sum(term);
        if ((threadIdx.x & 63) != 0) return;
    } else if (!live) {
        return;
    }
    atomicAdd(T.segments + l, count);
    (void)unsafeAtomicAdd(T.area2 + l, term);          // (the hardware's float64 add: the table is ordinary device memory)
}
}  // namespace fhm
