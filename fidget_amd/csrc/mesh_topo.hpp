// The arithmetic of the check of a triangle mesh (fhip_triangles_topology, fhip_mesh_topology; include/fidget_hip.h, where the definition
// stands in full): the canonical key of a corner's position, the hash and the probe sequence of the two tables, the key and the direction
// of an edge, the class of an edge's two counts, the two float64 terms of a triangle, the ordered-integer form of a float, and the two
// inserts themselves - written over a set of memory operations `A`, atomic on the device (topo.hip) and plain in a serial host build
// (fhtopo::Serial; tests/host_build/mesh_topo_host.cpp runs the whole pipeline with it).  No HIP and no memory of its own.  There is
// no counterpart in the reference: it never asks what kind of mesh it made.
//
//   key       the three coordinates' bits after x + 0.0f: -0 becomes +0, everything else keeps its bits (no NaN reaches a key: a
//             triangle with a coordinate that is not finite is rejected first)
//   probe     slot (hash + i) mod 2^log2 for i = 0, 1, .. 2^log2 - 1: every slot once, then the insert gives up - the call returns
//             FHIP_ERR_OVERFLOW - and nothing spins
//   vertex    a slot is two words side by side: the corner that claimed it (CAS from EMPTY) and the smallest corner with its key
//             (atomicMin); a corner that meets a claimed slot compares its key with the claimant's, read from the input.  The table
//             starts as all ones
//   edge      a slot is 32 bytes, one sector: the key a << 32 | b with a < b, claimed by a 64-bit CAS - b >= 1, so no key is 0 and 0 is
//             the empty slot; the counts f (uses a -> b) in the low and r (b -> a) in the high half of one word, a 64-bit add of 1 or
//             1 << 32; the complement of the smallest corner that uses it, by atomicMax.  The table starts as zeros
//   class     boundary f + r == 1; flipped f + r == 2 and f != r; nonmanifold f + r >= 3; unbalanced f != r
//   volume6   a . (b x c) with n = (b.y c.z - b.z c.y, b.z c.x - b.x c.z, b.x c.y - b.y c.x), (a.x n.x + a.y n.y) + a.z n.z
//   area2     |u x v|, u = b - a, v = c - a, m = u x v in the same component order, sqrt((m.x m.x + m.y m.y) + m.z m.z)
//             both in binary64 from the corners converted to binary64, in that order, no contraction
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "mesh_vox.hpp"

namespace fhtopo {
constexpr uint32_t EMPTY = 0xFFFFFFFFu;                 // a vertex slot nobody claimed; `first` words before any atomicMin; no shell
constexpr uint64_t EMPTY_KEY = 0;                       // an edge slot nobody claimed (a < b: b >= 1 and no key is 0)
constexpr uint32_t VERTEX_SLOT_WORDS = 2, EDGE_SLOT_WORDS = 4;          // uint32 {owner, first}; uint64 {key, counts, ~first, unused}
constexpr uint64_t MAX_CORNERS = 0xFFFFFFFEull;       // 3 T and, indexed, n_vertices: corners and vertex ids are uint32, EMPTY is neither
constexpr uint32_t MAX_LOG2 = 32;
constexpr uint32_t BOUNDARY = 1, FLIPPED = 2, NONMANIFOLD = 4, UNBALANCED = 8, FIRST_USE = 16;          // a corner's byte: FIRST_USE | the classes of its edge
constexpr uint32_t N_KINDS = 4;

FHV_HD uint32_t float_bits(float x) { uint32_t b; memcpy(&b, &x, 4); return b; }
FHV_HD float bits_float(uint32_t b) { float x; memcpy(&x, &b, 4); return x; }
FHV_HD uint32_t canon(float x) { const uint32_t b = float_bits(x); return b == 0x80000000u ? 0u : b; }          // the bits of x + 0.0f
FHV_HD bool finite(float x) { return (float_bits(x) & 0x7F800000u) != 0x7F800000u; }
FHV_HD bool finite3(const float* v) { return finite(v[0]) && finite(v[1]) && finite(v[2]); }

// the ordered-integer form: a < b as floats iff ordered(a) < ordered(b) as uint32 (of canonical bits: no -0)
FHV_HD uint32_t ordered(uint32_t canon_bits) { return (canon_bits & 0x80000000u) ? ~canon_bits : (canon_bits | 0x80000000u); }
FHV_HD uint32_t unordered(uint32_t o) { return (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o; }

FHV_HD uint64_t mix64(uint64_t x) {          // (the finalizer of MurmurHash3)
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return x;
}
FHV_HD uint64_t hash_vertex(const uint32_t k[3]) { return mix64(mix64(((uint64_t)k[1] << 32) | k[0]) ^ ((uint64_t)k[2] * 0x9E3779B97F4A7C15ull)); }
FHV_HD uint64_t hash_edge(uint64_t key) { return mix64(key); }
FHV_HD uint64_t n_slots(uint32_t log2) { return (uint64_t)1 << log2; }
FHV_HD uint64_t probe(uint64_t hash, uint64_t i, uint32_t log2) { return ((hash >> 16) + i) & (n_slots(log2) - 1); }
// the library's choice: the least power of two at or above 4 T, at least 2 slots - 3 T keys at the most, a load of at most 3/4 - capped
// at 2^32, which still holds the 2^32 - 2 keys
FHV_HD uint32_t default_log2(uint64_t n_triangles) {
    uint32_t l = 1;
    while (l < MAX_LOG2 && n_slots(l) < 4 * n_triangles) l++;
    return l;
}

// where the corners' positions are: by index, or three in a row for a soup
struct Corners {
    const float* vertices;
    const uint64_t* triangles;          // null: a soup
};
FHV_HD const float* position(const Corners& in, uint32_t c) { return in.vertices + 3 * (in.triangles ? in.triangles[c] : (uint64_t)c); }
FHV_HD void corner_key(const Corners& in, uint32_t c, uint32_t k[3]) {
    const float* const p = position(in, c);
    k[0] = canon(p[0]); k[1] = canon(p[1]); k[2] = canon(p[2]);
}
FHV_HD uint32_t next_corner(uint32_t c) { return c % 3 == 2 ? c - 2 : c + 1; }

// the memory operations of a serial host build; topo.hip has the device's
struct Serial {
    static uint32_t load32(const uint32_t* p) { return *p; }
    static uint32_t cas32(uint32_t* p, uint32_t expect, uint32_t v) { const uint32_t old = *p; if (old == expect) *p = v; return old; }
    static void min32(uint32_t* p, uint32_t v) { if (v < *p) *p = v; }
    static uint64_t load64(const uint64_t* p) { return *p; }
    static uint64_t cas64(uint64_t* p, uint64_t expect, uint64_t v) { const uint64_t old = *p; if (old == expect) *p = v; return old; }
    static void add64(uint64_t* p, uint64_t v) { *p += v; }
    static void max64(uint64_t* p, uint64_t v) { if (v > *p) *p = v; }
};

FHV_HD uint32_t vertex_first(const uint32_t* table, uint64_t slot) { return table[VERTEX_SLOT_WORDS * slot + 1]; }
// Corner c into the vertex table (2^log2 slots, all ones before) -> its slot; false: every slot holds another key
template <class A>
FHV_HD bool vertex_insert(const Corners& in, uint32_t* table, uint32_t log2, uint32_t c, uint64_t& slot) {
    uint32_t k[3], other[3];
    corner_key(in, c, k);
    const uint64_t h = hash_vertex(k), n = n_slots(log2);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t s = probe(h, i, log2);
        uint32_t* const owner = table + VERTEX_SLOT_WORDS * s;
        uint32_t cur = A::load32(owner);
        if (cur == EMPTY) {
            cur = A::cas32(owner, EMPTY, c);
            if (cur == EMPTY) cur = c;
        }
        if (cur != c) {
            corner_key(in, cur, other);
            if (other[0] != k[0] || other[1] != k[1] || other[2] != k[2]) continue;
        }
        A::min32(owner + 1, c);
        slot = s;
        return true;
    }
    return false;
}

FHV_HD uint64_t edge_key(uint32_t from, uint32_t to) { return from < to ? ((uint64_t)from << 32) | to : ((uint64_t)to << 32) | from; }
FHV_HD uint64_t edge_use(uint32_t from, uint32_t to) { return from < to ? (uint64_t)1 : (uint64_t)1 << 32; }
FHV_HD uint32_t edge_class(uint64_t counts) {
    const uint64_t f = counts & 0xFFFFFFFFull, r = counts >> 32;
    return (f + r == 1 ? BOUNDARY : 0u) | (f + r == 2 && f != r ? FLIPPED : 0u) | (f + r >= 3 ? NONMANIFOLD : 0u) | (f != r ? UNBALANCED : 0u);
}
FHV_HD uint64_t edge_counts(const uint64_t* table, uint64_t slot) { return table[EDGE_SLOT_WORDS * slot + 1]; }
FHV_HD uint32_t edge_first(const uint64_t* table, uint64_t slot) { return ~(uint32_t)table[EDGE_SLOT_WORDS * slot + 2]; }
// The use from -> to (from != to) by corner c into the edge table (2^log2 slots, zeros before) -> its slot
template <class A>
FHV_HD bool edge_insert(uint64_t* table, uint32_t log2, uint32_t from, uint32_t to, uint32_t c, uint64_t& slot) {
    const uint64_t key = edge_key(from, to), h = hash_edge(key), n = n_slots(log2);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t s = probe(h, i, log2);
        uint64_t* const words = table + EDGE_SLOT_WORDS * s;
        uint64_t cur = A::load64(words);
        if (cur == EMPTY_KEY) {
            cur = A::cas64(words, EMPTY_KEY, key);
            if (cur == EMPTY_KEY) cur = key;
        }
        if (cur != key) continue;
        A::add64(words + 1, edge_use(from, to));
        A::max64(words + 2, (uint64_t)~c);
        slot = s;
        return true;
    }
    return false;
}

FHV_HD bool degenerate(uint32_t a, uint32_t b, uint32_t c) { return a == b || b == c || a == c; }

FHV_HD double volume6_term(const float* pa, const float* pb, const float* pc) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ax = pa[0], ay = pa[1], az = pa[2], bx = pb[0], by = pb[1], bz = pb[2], cx = pc[0], cy = pc[1], cz = pc[2];
    const double nx = by * cz - bz * cy, ny = bz * cx - bx * cz, nz = bx * cy - by * cx;
    const double xy = ax * nx + ay * ny;
    return xy + az * nz;
}
FHV_HD double area2_term(const float* pa, const float* pb, const float* pc) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ux = (double)pb[0] - (double)pa[0], uy = (double)pb[1] - (double)pa[1], uz = (double)pb[2] - (double)pa[2];
    const double vx = (double)pc[0] - (double)pa[0], vy = (double)pc[1] - (double)pa[1], vz = (double)pc[2] - (double)pa[2];
    const double mx = uy * vz - uz * vy, my = uz * vx - ux * vz, mz = ux * vy - uy * vx;
    const double xy = mx * mx + my * my;
    return sqrt(xy + mz * mz);
}
}  // namespace fhtopo
