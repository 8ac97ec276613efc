// The bit arithmetic of the outlines of a voxel bitmap's layers (fhip_voxels_outlines, include/fidget_hip.h, where the definitions stand):
// the rows of a layer image as bit vectors, the eight masks of a lattice row - where an outline leaves and where it arrives, by heading -
// the vertices among them, their ranks in the row, and the successor of a vertex along its heading.  No HIP and no memory of its own:
// compiled for the device by outline.hip and for the host by tests/host_build/mesh_outline_host.cpp.
//
// A layer k is the image P(i, j) = voxel (i, j, k), clear beyond the grid.  Corner (a, b), 0 <= a, b <= N, touches the pixels
//   A = P(a - 1, b - 1), B = P(a, b - 1), C = P(a, b), D = P(a - 1, b)          (the corner mask m = A | B << 1 | C << 2 | D << 3)
// and the four unit edges around it, each directed with the inside on its left (headings 0 = -x, 1 = +x, 2 = -y, 3 = +y):
//   the edge to the right, between B below and C above:   C & ~B leaves with 1,   B & ~C arrives with 0
//   the edge to the left,  between A below and D above:   D & ~A arrives with 1,  A & ~D leaves with 0
//   the edge above, between D on the left and C right:    D & ~C leaves with 3,   C & ~D arrives with 2
//   the edge below, between A on the left and B right:    A & ~B arrives with 3,  B & ~A leaves with 2
// A corner that is no saddle has one edge in and one out, or none; it holds a vertex where the two headings differ.  A saddle (A, C or
// B, D alone) has two of each, every heading different, and holds two vertices.  So in both cases
//   a vertex leaves with heading d where   out_d & ~in_d,          and a vertex is arrived at with heading d where   in_d & ~out_d.
// A lattice row is worked on in chunks of 32 corners, a = 32 c + s; the masks are 32-bit words indexed by s.
#pragma once
#include <stdint.h>

#include "mesh_vox.hpp"

namespace fhol {
constexpr uint32_t CHUNK = 32;
constexpr uint64_t MAX_VERTICES = 0xFFFFFFFFull;          // ids are uint32: 2^32 vertices or more is an overflow

FHV_HD bool conn_ok(uint32_t c) { return c == 4 || c == 8; }
FHV_HD uint32_t n_chunks(uint32_t depth) { return ((4u << depth) + CHUNK) / CHUNK; }          // over the N + 1 corners of a row
FHV_HD uint32_t popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// bit t, 0 <= t <= 32: pixel (32 c - 1 + t, j) of layer k; clear beyond the grid (j = -1 has wrapped to above N)
FHV_HD uint64_t row_bits(const uint64_t* bricks, uint32_t depth, uint32_t j, uint32_t k, uint32_t c) {
    const uint32_t B = 1u << depth, N = 4u << depth;
    if (j >= N) return 0;
    const uint32_t sh = 4 * (j & 3) + 16 * (k & 3), bx0 = 8 * c;
    const uint64_t* const row = bricks + fhvox::word_index(depth, 0, j >> 2, k >> 2);
    uint64_t r = c > 0 ? (row[bx0 - 1] >> (sh + 3)) & 1u : 0;          // (c <= N / 32: brick 8 c - 1 is inside)
    for (uint32_t u = 0; u < 8; u++)
        if (bx0 + u < B) r |= ((row[bx0 + u] >> sh) & 15u) << (1 + 4 * u);
    return r;
}
FHV_HD uint32_t pixel(const uint64_t* bricks, uint32_t depth, uint32_t i, uint32_t j, uint32_t k) {
    const uint32_t N = 4u << depth;
    if (i >= N || j >= N) return 0;
    return (uint32_t)(bricks[fhvox::word_index(depth, i >> 2, j >> 2, k >> 2)] >> fhvox::voxel_bit(i & 3, j & 3, k & 3)) & 1u;
}

struct Masks {
    uint32_t out[4], in[4];          // an edge leaves / arrives with heading d
    uint32_t leave[4], arrive[4];    // a vertex leaves / is arrived at with heading d
    uint32_t any, saddle, saddle5;   // corners with a vertex; with two; those of them with A and C set (m = 5; the others m = 10)
};
FHV_HD Masks masks_of(uint32_t A, uint32_t B, uint32_t C, uint32_t D) {
    Masks M;
    M.out[0] = A & ~D; M.out[1] = C & ~B; M.out[2] = B & ~A; M.out[3] = D & ~C;
    M.in[0] = B & ~C; M.in[1] = D & ~A; M.in[2] = C & ~D; M.in[3] = A & ~B;
    M.any = 0;
    for (uint32_t d = 0; d < 4; d++) {
        M.leave[d] = M.out[d] & ~M.in[d];
        M.arrive[d] = M.in[d] & ~M.out[d];
        M.any |= M.leave[d];
    }
    M.saddle5 = A & C & ~B & ~D;
    M.saddle = M.saddle5 | (B & D & ~A & ~C);
    return M;
}
// the masks of chunk c of lattice row b of layer k
FHV_HD Masks row_masks(const uint64_t* bricks, uint32_t depth, uint32_t k, uint32_t b, uint32_t c) {
    const uint64_t lo = row_bits(bricks, depth, b - 1, k, c), up = row_bits(bricks, depth, b, k, c);
    return masks_of((uint32_t)lo, (uint32_t)(lo >> 1), (uint32_t)(up >> 1), (uint32_t)up);
}
// ... and of the one corner (a, b), in bit 0
FHV_HD Masks corner_masks(const uint64_t* bricks, uint32_t depth, uint32_t k, uint32_t a, uint32_t b) {
    return masks_of(pixel(bricks, depth, a - 1, b - 1, k), pixel(bricks, depth, a, b - 1, k), pixel(bricks, depth, a, b, k), pixel(bricks, depth, a - 1, b, k));
}
FHV_HD uint32_t count(const Masks& M) { return popc(M.any) + popc(M.saddle); }
FHV_HD uint32_t below(uint32_t s) { return (1u << s) - 1u; }          // the corners of a chunk before s, s < 32
// the rank in its chunk of the vertex that leaves corner s with heading d: a saddle's two are in ascending order of that heading,
// 0 before 1 and 2 before 3
FHV_HD uint32_t rank_leaving(const Masks& M, uint32_t s, uint32_t d) {
    return popc(M.any & below(s)) + popc(M.saddle & below(s)) + (((M.saddle >> s) & 1u) & d);
}
// ... of the vertex arrived at with heading d.  At a saddle the connectivity pairs the headings: with 4 both loops turn left,
// m = 5: (3, 0), (2, 1), m = 10: (0, 2), (1, 3); with 8 both turn right, m = 5: (2, 0), (3, 1), m = 10: (1, 2), (0, 3).
FHV_HD uint32_t rank_arriving(const Masks& M, uint32_t s, uint32_t d, uint32_t conn) {
    const uint32_t second5 = conn == 4 ? 2u : 3u, second10 = conn == 4 ? 1u : 0u;
    const uint32_t second = ((M.saddle >> s) & 1u) & (((M.saddle5 >> s) & 1u) ? (uint32_t)(d == second5) : (uint32_t)(d == second10));
    return popc(M.any & below(s)) + popc(M.saddle & below(s)) + second;
}
// the entry of chunk c of row b of the layer-th layer in the arrays of counts and base ids: ids ascend with it
FHV_HD uint64_t entry(uint32_t depth, uint32_t layer, uint32_t b, uint32_t c) {
    return ((uint64_t)layer * ((4u << depth) + 1) + b) * n_chunks(depth) + c;
}

// The successor of the vertex that leaves corner (32 c + s, b) of layer k (the layer-th of the call) with heading d: the nearest corner
// along d at which a vertex is arrived at with d - in between lie straight corners alone, and since every outline is closed there is
// one before the lattice ends.  `base`: the first id of every entry.  `M`: the masks of the vertex's own chunk.
FHV_HD uint32_t successor(const uint64_t* bricks, uint32_t depth, uint32_t k, uint32_t layer, uint32_t conn, const uint32_t* base, const Masks& M, uint32_t b, uint32_t c,
                          uint32_t s, uint32_t d) {
    const uint32_t N = 4u << depth, C = n_chunks(depth);
    if (d == 1) {
        const uint32_t own = M.arrive[1] & ~below(s) & ~(1u << s);
        if (own) return base[entry(depth, layer, b, c)] + rank_arriving(M, (uint32_t)__builtin_ctz(own), 1, conn);
        for (uint32_t c2 = c + 1; c2 < C; c2++) {
            const Masks M2 = row_masks(bricks, depth, k, b, c2);
            if (M2.arrive[1]) return base[entry(depth, layer, b, c2)] + rank_arriving(M2, (uint32_t)__builtin_ctz(M2.arrive[1]), 1, conn);
        }
    } else if (d == 0) {
        const uint32_t own = M.arrive[0] & below(s);
        if (own) return base[entry(depth, layer, b, c)] + rank_arriving(M, 31u - (uint32_t)__builtin_clz(own), 0, conn);
        for (uint32_t c2 = c; c2-- > 0;) {
            const Masks M2 = row_masks(bricks, depth, k, b, c2);
            if (M2.arrive[0]) return base[entry(depth, layer, b, c2)] + rank_arriving(M2, 31u - (uint32_t)__builtin_clz(M2.arrive[0]), 0, conn);
        }
    } else {
        const uint32_t a = CHUNK * c + s;
        for (uint32_t step = 1; step <= N; step++) {
            const uint32_t b2 = d == 3 ? b + step : b - step;
            if (b2 > N) break;          // (b - step has wrapped)
            if (corner_masks(bricks, depth, k, a, b2).arrive[d] & 1u)
                return base[entry(depth, layer, b2, c)] + rank_arriving(row_masks(bricks, depth, k, b2, c), s, d, conn);
        }
    }
    return 0xFFFFFFFFu;          // not reached: an outline that ends
}
}  // namespace fhol
