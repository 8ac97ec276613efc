// The arithmetic of the solid voxelization of a triangle mesh (fhip_triangles_voxels, fhip_mesh_voxels; include/fidget_hip.h, where the
// definition stands in full): the snap of a vertex to the lattice of 1/256 voxel, the set-up of a triangle - rejected, flat, oriented,
// its box of columns - the cover test of a column with the crossing's voxel, and the prefix XOR along x inside a brick's word.  Integers
// throughout after the snap, all of them in int64.  No HIP and no memory of its own: compiled for the device by trivox.hip and for the
// host by tests/host_build/mesh_trivox_host.cpp.  There is no counterpart in the reference: it has no voxel bitmap.
//
//   snap      w = ((m0 x + m1 y) + m2 z) + m3 in binary64, uncontracted (identity without a matrix); q = llrint(w 128 N + 128 N), to
//             nearest-even: voxel i has its centre at 256 i + 128.  A triangle with a coordinate w that is not finite or lies outside
//             [-1.5, 1.5] is rejected - decided on w, before any conversion to an integer - so q lies in [-64 N, 320 N]
//   flat      D = (b.y - a.y)(c.z - a.z) - (b.z - a.z)(c.y - a.y) == 0; with D < 0 b and c change places and D its sign
//   cover     column (j, k) is the point P = (256 j + 128, 256 k + 128); for the directed edges p -> r of b -> c, c -> a, a -> b
//             e = (r.y - p.y)(P.z - p.z) - (r.z - p.z)(P.y - p.y); P is covered iff every e > 0, or e == 0 and the edge owns its points:
//             r.y - p.y > 0, or r.y - p.y == 0 and r.z - p.z < 0
//   crossing  with the three e as weights of a, b, c (their sum is D), xmin the least x and num = sum of e (x - xmin), the crossing
//             lies at xmin + num / D and toggles every voxel whose centre is at or beyond it, the first of them
//             i* = ceil((num - (128 - xmin) D) / (256 D)); i* <= 0: voxel 0; i* >= N: the column's bit in the exit plane
//   bits      spans <= 384 N = 1.5 2^20 at depth 10; D <= span^2 < 2^41.2, an edge value off the triangle < 2^42.2; num <= span^3 <
//             2^61.8, |(128 - xmin) D| < 2^61.5, their difference below 2^63; 256 D < 2^50
#pragma once
#include <math.h>
#include <stdint.h>

#include "mesh_vmesh.hpp"

namespace fhtv {
constexpr uint32_t TV_OK = 0, TV_REJECTED = 1, TV_FLAT = 2;
constexpr double TV_RANGE = 1.5;
constexpr int64_t TV_EXIT = -1;          // cover_cross: the crossing lies beyond the last voxel's centre

// a triangle ready for the columns: the snapped corners, oriented so that the inside lies to the left of every edge in the yz plane,
// and its box of columns clipped to the grid - nj x nk columns from (j0, k0), none where either is 0
struct alignas(16) Tri {
    int32_t a[3], b[3], c[3];
    uint16_t j0, k0, nj, nk;
    uint32_t pad;
};
static_assert(sizeof(Tri) == 48, "three 16-byte loads");

// one coordinate of the vertex in world space: row `r` of the 3 x 4 matrix (null: the identity) applied in binary64, no contraction
FHV_HD double world(const double* m, uint32_t r, const float v[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!m) return (double)v[r];
    const double x = (double)v[0], y = (double)v[1], z = (double)v[2];
    const double xy = m[4 * r] * x + m[4 * r + 1] * y;
    const double xyz = xy + m[4 * r + 2] * z;
    return xyz + m[4 * r + 3];
}
FHV_HD bool in_range(double w) { return w >= -TV_RANGE && w <= TV_RANGE; }          // (false for a NaN)
// w in [-1.5, 1.5] -> lattice units; 128 N is a power of two, so the product is exact and the sum rounds once
FHV_HD int32_t snap(double w, uint32_t depth) {
    const double s = (double)((uint64_t)512 << depth);
    return (int32_t)llrint(w * s + s);
}
// the vertex `v` -> q[3]; false: rejected
FHV_HD bool snap_vertex(const float v[3], const double* m, uint32_t depth, int32_t q[3]) {
    bool ok = true;
    for (uint32_t r = 0; r < 3; r++) {
        const double w = world(m, r, v);
        ok = ok && in_range(w);
        q[r] = in_range(w) ? snap(w, depth) : 0;
    }
    return ok;
}
// the columns' centres 256 j + 128 within [lo, hi], clipped to 0 .. N - 1: the first and how many
FHV_HD void column_range(int32_t lo, int32_t hi, uint32_t N, uint16_t& first, uint16_t& n) {
    int32_t j0 = (lo - 128 + 255) >> 8, j1 = (hi - 128) >> 8;          // ceil and floor: the shifts are arithmetic
    if (j0 < 0) j0 = 0;
    if (j1 > (int32_t)N - 1) j1 = (int32_t)N - 1;
    first = (uint16_t)(j1 >= j0 ? j0 : 0);
    n = (uint16_t)(j1 >= j0 ? j1 - j0 + 1 : 0);
}
FHV_HD int32_t min3(int32_t a, int32_t b, int32_t c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
FHV_HD int32_t max3(int32_t a, int32_t b, int32_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }
// the snapped corners -> T, oriented and with its box; TV_OK or TV_FLAT (then T has no columns)
FHV_HD uint32_t setup(const int32_t a[3], const int32_t b[3], const int32_t c[3], uint32_t depth, Tri& T) {
    const int64_t D = (int64_t)(b[1] - a[1]) * (c[2] - a[2]) - (int64_t)(b[2] - a[2]) * (c[1] - a[1]);
    const bool swap = D < 0;
    for (uint32_t r = 0; r < 3; r++) {
        T.a[r] = a[r];
        T.b[r] = swap ? c[r] : b[r];
        T.c[r] = swap ? b[r] : c[r];
    }
    T.j0 = T.k0 = T.nj = T.nk = 0;
    T.pad = 0;
    if (D == 0) return TV_FLAT;
    const uint32_t N = 4u << depth;
    column_range(min3(a[1], b[1], c[1]), max3(a[1], b[1], c[1]), N, T.j0, T.nj);
    column_range(min3(a[2], b[2], c[2]), max3(a[2], b[2], c[2]), N, T.k0, T.nk);
    return TV_OK;
}
FHV_HD uint32_t n_columns(const Tri& T) { return (uint32_t)T.nj * T.nk; }

// the edge p -> r at P = (py, pz): the value, and whether P counts as inside of it.  (All four differences fit 32 bits - a centre lies
// in [128, 256 N), a corner in [-64 N, 320 N] - so each product is one of 32 x 32 -> 64 bits.)
FHV_HD int64_t edge_value(const int32_t p[3], const int32_t r[3], int32_t py, int32_t pz) {
    return (int64_t)(r[1] - p[1]) * (int64_t)(pz - p[2]) - (int64_t)(r[2] - p[2]) * (int64_t)(py - p[1]);
}
FHV_HD bool edge_inside(const int32_t p[3], const int32_t r[3], int64_t e) {
    const int32_t dy = r[1] - p[1], dz = r[2] - p[2];
    return e > 0 || (e == 0 && (dy > 0 || (dy == 0 && dz < 0)));
}
// Column (j, k) against the triangle: false where it is not covered; where it is, `i` is the voxel the crossing toggles, 0 .. N - 1,
// or TV_EXIT.  The one division is made for a covered column whose crossing falls between the first and the last centre.
FHV_HD bool cover_cross(const Tri& T, uint32_t depth, uint32_t j, uint32_t k, int64_t& i) {
    const int32_t py = 256 * (int32_t)j + 128, pz = 256 * (int32_t)k + 128;          // j, k < N <= 4096
    const int64_t wa = edge_value(T.b, T.c, py, pz), wb = edge_value(T.c, T.a, py, pz), wc = edge_value(T.a, T.b, py, pz);
    if (!(edge_inside(T.b, T.c, wa) && edge_inside(T.c, T.a, wb) && edge_inside(T.a, T.b, wc))) return false;
    const int64_t D = wa + wb + wc, N = (int64_t)4 << depth;
    const int64_t xmin = min3(T.a[0], T.b[0], T.c[0]);
    const int64_t num = wa * (T.a[0] - xmin) + wb * (T.b[0] - xmin) + wc * (T.c[0] - xmin);
    const int64_t t = num - (128 - xmin) * D, den = 256 * D;          // i* = ceil(t / den), den > 0
    if (t <= 0) { i = 0; return true; }
    if (t > (N - 1) * den) { i = TV_EXIT; return true; }
    const int64_t q = t / den;
    i = q + (t - q * den > 0 ? 1 : 0);
    return true;
}
// where a toggle goes: the word of the bitmap and the bit in it; for the exit plane bit k N + j of N N bits in words of 64
FHV_HD uint64_t voxel_word(uint32_t depth, uint32_t i, uint32_t j, uint32_t k) { return fhvox::word_index(depth, i >> 2, j >> 2, k >> 2); }
FHV_HD uint64_t voxel_bit(uint32_t i, uint32_t j, uint32_t k) { return (uint64_t)1 << ((i & 3) + 4 * (j & 3) + 16 * (k & 3)); }
FHV_HD uint64_t exit_words(uint32_t depth) { return depth == 0 ? 1 : (uint64_t)1 << (2 * depth - 2); }          // N N / 64, at least one
FHV_HD uint64_t exit_index(uint32_t depth, uint32_t j, uint32_t k) { return ((uint64_t)k << (depth + 2)) + j; }

// ---- the fill inside a word ------------------------------------------------------------------------------------------------------------------
// the prefix XOR along lx of all 16 rows of four voxels at once: two shift-and-XOR steps that do not cross a row's border
FHV_HD uint64_t fill_word(uint64_t toggles) {
    uint64_t w = toggles;
    w ^= (w << 1) & ~fhvm::X0;
    w ^= (w << 2) & ~(fhvm::X0 | (fhvm::X0 << 1));
    return w;
}
// the parity that leaves a filled word along +x: one bit per row, at the X0 positions; and what a parity entering does to the word
FHV_HD uint64_t fill_carry(uint64_t filled) { return (filled >> 3) & fhvm::X0; }
FHV_HD uint64_t fill_apply(uint64_t filled, uint64_t carry_in) { return filled ^ (carry_in * 15u); }
// the four columns (4 by .. 4 by + 3, k) of the exit plane as a nibble, for the rows' open ends
FHV_HD uint64_t exit_nibble(const uint64_t* exit_plane, uint32_t depth, uint32_t by, uint32_t k) {
    const uint64_t at = exit_index(depth, 4 * by, k);
    return (exit_plane[at >> 6] >> (at & 63)) & 15u;
}
// the rows of brick row (by, bz) that end inside: the last word's parity against the exit plane, a bit per row at the X0 positions
FHV_HD uint64_t open_ends(uint64_t last_filled, const uint64_t* exit_plane, uint32_t depth, uint32_t by, uint32_t bz) {
    uint64_t out = fill_carry(last_filled);
    for (uint32_t lz = 0; lz < 4; lz++) {
        const uint64_t nib = exit_nibble(exit_plane, depth, by, 4 * bz + lz);
        for (uint32_t ly = 0; ly < 4; ly++) out ^= ((nib >> ly) & 1u) << (4 * ly + 16 * lz);
    }
    return out;
}
}  // namespace fhtv
