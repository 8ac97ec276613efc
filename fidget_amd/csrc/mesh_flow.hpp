// The bit arithmetic of a voxel bitmap along a direction (fhip_voxels_flow, fhip_voxels_overhangs, fhip_voxels_heights;
// include/fidget_hip.h): the flow of seeds past blockers inside a brick's word, with the carry that enters and the one that leaves; for
// the flow along x the pair (G, P) of a word and the composition of pairs, which a scan across a wave folds; the move of a word by up
// to four voxels with the neighbouring brick's bits coming in, and the dilation by a disc that is made of such moves; the lowest, the
// highest and the number of set voxels of a word's columns.  No HIP and no memory of its own: compiled for the device by flow.hip and
// for the host by tests/host_build/mesh_flow_host.cpp.  There is no counterpart in the reference: it has no voxel bitmap.
//
// Bricks as in mesh_vmesh.hpp: word (bz B + by) B + bx holds the voxels (4 bx + lx, 4 by + ly, 4 bz + lz) at bit lx + 4 ly + 16 lz; a word
// outside the grid is 0.  A direction d = 0 .. 5 is -x, +x, -y, +y, -z, +z; its axis is d >> 1, e(d) its unit vector.  The plane of a
// word that a flow towards d enters first is its entry plane (lx == 0 for +x, lx == 3 for -x, ...); the one it leaves last its exit plane.
#pragma once
#include <stdint.h>

#include "mesh_vmesh.hpp"

namespace fhfl {
constexpr uint32_t MAX_REACH2 = 16;          // with it every supporter lies in the brick or in one next to it
constexpr uint32_t FLOW_WITH_SEEDS = 1u;

// the word whose bit p is the voxel at p - e(d): `cur` moved one step towards d, its entry plane the exit plane of `behind`, the brick
// at -e(d)
FHV_HD uint64_t toward(uint32_t d, uint64_t cur, uint64_t behind) {
    switch (d) {
        case 0: return fhvm::above_x(cur, behind);
        case 1: return fhvm::below_x(cur, behind);
        case 2: return fhvm::above_y(cur, behind);
        case 3: return fhvm::below_y(cur, behind);
        case 4: return fhvm::above_z(cur, behind);
        default: return fhvm::below_z(cur, behind);
    }
}

// ---- flow ------------------------------------------------------------------------------------------------------------------------------------
// R(p) = (R(p - e) | S(p - e)) & ~K(p) inside one word.  `open` is ~K; `carry` holds R | S of the brick behind, already moved onto this
// word's entry plane (carry_out of that brick; 0 at the grid's border).  One move brings the seeds and the carry one step on; what they
// reach spreads over the three further voxels of a row in three more moves.
FHV_HD uint64_t flow_word(uint64_t seeds, uint64_t open, uint64_t carry, uint32_t d) {
    uint64_t r = (toward(d, seeds, 0) | carry) & open;
    r |= toward(d, r, 0) & open;
    r |= toward(d, r, 0) & open;
    r |= toward(d, r, 0) & open;
    return r;
}
// what the next brick towards d takes in: the exit plane of rs = R | S, on that brick's entry plane
FHV_HD uint64_t carry_out(uint64_t rs, uint32_t d) { return toward(d, 0, rs); }

// Along x a carry is one bit per row of four voxels: 16 bits, kept at the X0 positions whatever the sign of the direction.
//   G: the carry out of the word when none comes in;  P: a carry in passes the whole row - no blocker among its four voxels.
// The carry out is G | (P & carry in).
struct GP {
    uint64_t g, p;
};
FHV_HD uint64_t carry_to_x0(uint64_t carry, uint32_t d) { return d == 0 ? carry >> 3 : carry; }          // from the entry plane; d = 0, 1
FHV_HD uint64_t carry_from_x0(uint64_t c, uint32_t d) { return d == 0 ? c << 3 : c; }                    // ... and back onto it
FHV_HD GP gp_of(uint64_t seeds, uint64_t open, uint32_t d) {
    const uint64_t r = flow_word(seeds, open, 0, d);
    const uint64_t pairs = open & (open >> 1);
    return GP{carry_to_x0(carry_out(r | seeds, d), d), pairs & (pairs >> 2) & fhvm::X0};
}
// first `a`, then `b`, the word after it in the direction of the flow: associative, with identity (0, X0)
FHV_HD GP gp_then(GP a, GP b) { return GP{b.g | (b.p & a.g), a.p & b.p}; }
FHV_HD GP gp_identity() { return GP{0, fhvm::X0}; }

// ---- moves and the disc ----------------------------------------------------------------------------------------------------------------------
// the word whose bit p is the voxel at p - s e_axis, -4 <= s <= 4: below_* / above_* are s = 1 / -1.  `lower` and `upper` are the bricks
// next to `cur` at -e_axis and +e_axis.
FHV_HD uint64_t moved(uint32_t axis, uint64_t cur, uint64_t lower, uint64_t upper, int32_t s) {
    if (s == 0) return cur;
    const uint32_t k = (uint32_t)(s < 0 ? -s : s);
    if (k >= 4) return s > 0 ? lower : upper;
    const uint32_t unit = 1u << (2 * axis), sh = k * unit, back = (4 - k) * unit;          // (at most 48: no shift by the word's width)
    const uint64_t every = axis == 0 ? fhvm::X0 : axis == 1 ? 0x0001000100010001ull : 1ull;
    const uint64_t lo = every * ((1ull << sh) - 1);          // the bits whose coordinate along the axis is below k
    if (s > 0) return ((cur << sh) & ~lo) | ((lower >> back) & lo);
    const uint64_t hi = lo << back;                          // ... is 4 - k and above
    return ((cur >> sh) & ~hi) | ((upper << back) & hi);
}
// the largest w with w^2 <= r, r <= 16
FHV_HD uint32_t isqrt_small(uint32_t r) {
    uint32_t w = 0;
    while ((w + 1) * (w + 1) <= r) w++;
    return w;
}
// W[3 b + a] is the brick at offset a - 1 along axis U and b - 1 along axis V from the brick in the middle.  Bit p of the result: some
// voxel at p + u e_U + v e_V with u^2 + v^2 <= reach2 is set.  For every |v| the words moved by v and by -v along V, for the three
// bricks along U; then the OR of their moves by -w .. w along U, w = isqrt(reach2 - v^2).
FHV_HD uint64_t dilate_disc(const uint64_t W[9], uint32_t U, uint32_t V, uint32_t reach2) {
    uint64_t out = 0;
    for (uint32_t v = 0; v <= 4 && v * v <= reach2; v++) {
        // (the three bricks along U written out: no index that depends on a loop)
        const uint64_t m0 = moved(V, W[3], W[0], W[6], (int32_t)v) | moved(V, W[3], W[0], W[6], -(int32_t)v);
        const uint64_t m1 = moved(V, W[4], W[1], W[7], (int32_t)v) | moved(V, W[4], W[1], W[7], -(int32_t)v);
        const uint64_t m2 = moved(V, W[5], W[2], W[8], (int32_t)v) | moved(V, W[5], W[2], W[8], -(int32_t)v);
        const uint32_t w = isqrt_small(reach2 - v * v);
        uint64_t acc = m1;
        for (uint32_t s = 1; s <= w; s++) acc |= moved(U, m1, m0, m2, (int32_t)s) | moved(U, m1, m0, m2, -(int32_t)s);
        out |= acc;
    }
    return out;
}
// the two axes perpendicular to `axis`, the lower first
FHV_HD uint32_t perp_u(uint32_t axis) { return axis == 0 ? 1 : 0; }
FHV_HD uint32_t perp_v(uint32_t axis) { return axis == 2 ? 1 : 2; }
// the set voxels of `w` without support.  `here` is the dilated solid at the brick itself and `below` the one at the brick at -e(up):
// all ones or 0, as the bed says, where that brick lies beyond the grid.
FHV_HD uint64_t unsupported(uint64_t w, uint64_t here, uint64_t below, uint32_t up) { return w & ~toward(up, here, below); }

// ---- heights ---------------------------------------------------------------------------------------------------------------------------------
// A word has 16 columns along an axis; column c is numbered by the two remaining local coordinates, the lower axis fastest: c = p + 4 q.
// Its four voxels, at the bits 0, unit, 2 unit, 3 unit with unit = 1 << 2 axis:
FHV_HD uint64_t column(uint64_t w, uint32_t axis, uint32_t c) {
    const uint32_t p = c & 3, q = c >> 2;
    if (axis == 0) return (w >> (4 * p + 16 * q)) & 0xFull;
    if (axis == 1) return (w >> (p + 16 * q)) & 0x1111ull;
    return (w >> (p + 4 * q)) & 0x0001000100010001ull;
}
// of a column that is not empty: the local coordinate of its lowest and of its highest set voxel; of any: the number of set voxels
FHV_HD uint32_t column_lowest(uint64_t col, uint32_t axis) { return (uint32_t)__builtin_ctzll(col) >> (2 * axis); }
FHV_HD uint32_t column_highest(uint64_t col, uint32_t axis) { return (63u - (uint32_t)__builtin_clzll(col)) >> (2 * axis); }
FHV_HD uint32_t column_count(uint64_t col) { return fhvm::popcount64(col); }
}  // namespace fhfl
