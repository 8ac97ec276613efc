// The arithmetic of slicing a triangle mesh with planes z = const (fhip_topology_slices; include/fidget_hip.h, where the definition stands
// in full): a vertex's level among the planes, the planes an edge and a triangle cross, the lone corner of a crossing triangle and the
// two edges that hold its segment, a crossing's position and its id, the owner of an item under a prefix sum, the term of a loop's
// area - written over the memory operations `A` of mesh_topo.hpp, whose edge key, edge insert and probe it reuses.  No HIP and no
// memory of its own: slice.hip runs it on the device, tests/host_build/mesh_slice_host.cpp the whole pipeline with fhtopo::Serial.
// There is no counterpart in the reference, which never cuts a mesh.
//
//   level     a(v) = the number of planes with zs[p] <= z_v, by float comparison (-0 equals +0): an upper bound search in the ascending zs.
//             Vertex v is above plane p iff a(v) > p; everything after the levels is integer arithmetic
//   ranges    edge {u, v} crosses the planes min(a_u, a_v) <= p < max(a_u, a_v); a triangle those from the smallest to the largest level
//             of its corners
//   segment   corners (A, B, C) in the triangle's order, A the one alone on its side of the plane: A above, from the crossing on edge
//             A -> B to the one on edge C -> A; A below, the other way.  Edge i is the one from corner i to corner i + 1
//   position  u the end with the smaller vertex id: t = (zs[p] - z_u) / (z_v - z_u), x = x_u + t (x_v - x_u), y likewise, in binary64 from
//             the floats converted, every operation rounded on its own, the result rounded to float32
//   id        the crossings of an edge are consecutive, in ascending order of the plane, from the prefix sum at the edge's first corner
//   table     the crossing edges alone: the least power of two at or above 4/3 of the crossing corners, at least 2 slots
#pragma once
#include "mesh_topo.hpp"

namespace fhslice {
constexpr uint32_t NONE = 0xFFFFFFFFu;                  // no successor; a corner whose edge crosses no plane
constexpr uint64_t MAX_ITEMS = 0xFFFFFFFEull;           // crossings, and segments: ids are uint32 and NONE is none
constexpr uint32_t MAX_PLANES = 0xFFFFFFFEu;

FHV_HD uint32_t level(const float* zs, uint32_t n_planes, float z) {
    uint32_t lo = 0, hi = n_planes;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (zs[mid] <= z) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the host's check of the planes: finite and strictly ascending
FHV_HD bool planes_ok(const float* zs, uint32_t n_planes) {
    for (uint32_t p = 0; p < n_planes; p++)
        if (!fhtopo::finite(zs[p]) || (p > 0 && !(zs[p - 1] < zs[p]))) return false;
    return true;
}

struct Range { uint32_t lo, hi; };          // the planes lo <= p < hi
FHV_HD uint32_t n_planes(Range r) { return r.hi - r.lo; }
FHV_HD Range edge_range(uint32_t au, uint32_t av) { return au < av ? Range{au, av} : Range{av, au}; }
FHV_HD Range triangle_range(const uint32_t a[3]) {
    Range r = edge_range(a[0], a[1]);
    if (a[2] < r.lo) r.lo = a[2];
    if (a[2] > r.hi) r.hi = a[2];
    return r;
}

// A triangle that crosses plane p (triangle_range(a).lo <= p < .hi): the edges - by their first corners' places 0 .. 2 in the triangle -
// on which its segment starts and ends
struct SegmentEdges { uint32_t from, to; };
FHV_HD SegmentEdges segment_edges(const uint32_t a[3], uint32_t p) {
    const bool above[3] = {a[0] > p, a[1] > p, a[2] > p};
    const uint32_t lone = above[0] != above[1] ? (above[0] != above[2] ? 0u : 1u) : 2u;
    const uint32_t before = (lone + 2) % 3;          // C: edge C -> A
    return above[lone] ? SegmentEdges{lone, before} : SegmentEdges{before, lone};
}

// pu, pv: the ends' three coordinates, u the end with the smaller vertex id; z_u != z_v, as for every edge that crosses a plane
FHV_HD void position(const float* pu, const float* pv, float z_plane, float out[2]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double zu = pu[2], zv = pv[2];
    const double num = (double)z_plane - zu, den = zv - zu;
    const double t = num / den;
    const double dx = (double)pv[0] - (double)pu[0], dy = (double)pv[1] - (double)pu[1];
    const double tx = t * dx, ty = t * dy;
    out[0] = (float)((double)pu[0] + tx);
    out[1] = (float)((double)pu[1] + ty);
}
FHV_HD uint32_t crossing_id(uint32_t edge_base, Range edge, uint32_t p) { return edge_base + (p - edge.lo); }
// the term of a loop's area2 for the segment s -> d, from the float32 positions converted
FHV_HD double area2_term(const float* s, const float* d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double a = (double)s[0] * (double)d[1], b = (double)d[0] * (double)s[1];
    return a - b;
}

// base: the exclusive prefix sums of n counts, n + 1 of them, i < base[n]: the k with base[k] <= i < base[k + 1]
FHV_HD uint64_t owner(const uint32_t* base, uint64_t n, uint32_t i) {
    uint64_t lo = 0, hi = n;          // base[lo] <= i < base[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (base[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

FHV_HD uint32_t default_log2(uint64_t n_crossing_corners) {
    uint32_t l = 1;
    while (l < fhtopo::MAX_LOG2 && 3 * fhtopo::n_slots(l) < 4 * n_crossing_corners) l++;
    return l;
}
// Corner c of a triangle that is not degenerate, its edge from -> to: into the table if the edge crosses a plane -> its slot, or NONE.
// false: the table is full
template <class A>
FHV_HD bool corner_insert(uint64_t* table, uint32_t log2, uint32_t from, uint32_t to, uint32_t a_from, uint32_t a_to, uint32_t c, uint32_t& slot) {
    slot = NONE;
    if (a_from == a_to) return true;
    uint64_t s = 0;
    if (!fhtopo::edge_insert<A>(table, log2, from, to, c, s)) return false;
    slot = (uint32_t)s;          // (a slot index is below 2^32, and NONE is none: fhtopo::MAX_LOG2 slots hold 2^32 - 2 keys at the most)
    return true;
}
FHV_HD uint64_t edge_key_at(const uint64_t* table, uint64_t slot) { return table[fhtopo::EDGE_SLOT_WORDS * slot]; }

// a crossing's successor word: the complement of the smallest (triangle << 32 | end) of the segments that leave it, by A::max64 as an
// edge's first corner is kept, zero before - then next_of gives NONE; its degree word: the segments that leave it in the low and those
// that arrive in the high half, by A::add64
FHV_HD uint64_t next_word(uint32_t triangle, uint32_t end) { return ~(((uint64_t)triangle << 32) | end); }
FHV_HD uint32_t next_of(uint64_t word) { return ~(uint32_t)word; }
FHV_HD bool irregular(uint64_t degree) { return degree != (((uint64_t)1 << 32) | 1u); }
FHV_HD uint8_t degree_byte(uint64_t degree) {
    const uint64_t out = degree & 0xFFFFFFFFull, in = degree >> 32;
    return (uint8_t)((out > 15 ? 15 : out) | ((in > 15 ? 15 : in) << 4));
}
}  // namespace fhslice
