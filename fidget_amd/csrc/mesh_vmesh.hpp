// The bit arithmetic of the boundary mesh of a voxel bitmap (fhip_voxels_mesh, fhip_voxels_surface; include/fidget_hip.h): which faces
// of a brick's voxels are exposed, from its word and its six neighbours; which lattice corners and lattice edges of a corner brick are
// used, from the eight words around it; a face's four corners; where a corner lies in the numbering of the vertices.  No HIP and no
// memory of its own: compiled for the device by vmesh.hip and for the host by tests/host_build/mesh_vmesh_host.cpp.  There is no
// counterpart in the reference: it has no voxel bitmap.
//
// Bricks.  Word (bz B + by) B + bx holds the voxels (4 bx + lx, 4 by + ly, 4 bz + lz) at bit lx + 4 ly + 16 lz; a word outside the
// grid is 0.  Corner bricks.  Lattice corner (a, b, c), 0 <= a, b, c <= N, lies in corner brick (a >> 2, b >> 2, c >> 2) of a grid of
// (B + 1)^3 at bit (a & 3) + 4 (b & 3) + 16 (c & 3) - the same layout, one brick more per axis.  The eight voxels around corner
// (a, b, c) are (a - 1 .. a, b - 1 .. b, c - 1 .. c): those of a corner brick's 64 corners lie in brick (cx, cy, cz) and in the last
// planes of the seven bricks below it, the words W[dx + 2 dy + 4 dz] = brick (cx - dx, cy - dy, cz - dz).
#pragma once
#include <stdint.h>

#include "mesh_vox.hpp"

namespace fhvm {
constexpr uint64_t X0 = 0x1111111111111111ull, X3 = 0x8888888888888888ull;          // the bits with lx == 0; lx == 3
constexpr uint64_t Y0 = 0x000F000F000F000Full, Y3 = 0xF000F000F000F000ull;          // ly == 0; ly == 3
// (lz == 0 is the low 16 bits and lz == 3 the high 16: a shift by 16 drops exactly the plane that leaves the word)

// the word whose bit (lx, ly, lz) is the voxel one step below along an axis: `cur` moved up by one, its first plane the last plane of
// `prev`, the brick below along that axis
FHV_HD uint64_t below_x(uint64_t cur, uint64_t prev) { return ((cur << 1) & ~X0) | ((prev >> 3) & X0); }
FHV_HD uint64_t below_y(uint64_t cur, uint64_t prev) { return ((cur << 4) & ~Y0) | ((prev >> 12) & Y0); }
FHV_HD uint64_t below_z(uint64_t cur, uint64_t prev) { return (cur << 16) | (prev >> 48); }
// ... one step above: `next` is the brick above along that axis
FHV_HD uint64_t above_x(uint64_t cur, uint64_t next) { return ((cur >> 1) & ~X3) | ((next << 3) & X3); }
FHV_HD uint64_t above_y(uint64_t cur, uint64_t next) { return ((cur >> 4) & ~Y3) | ((next << 12) & Y3); }
FHV_HD uint64_t above_z(uint64_t cur, uint64_t next) { return (cur >> 16) | (next << 48); }

// ---- faces ---------------------------------------------------------------------------------------------------------------------------------
// out[d], d = 0 .. 5 = -x, +x, -y, +y, -z, +z: the set voxels of `w` whose neighbour in direction d is clear.  nb[d] is the brick next
// to it in direction d, 0 beyond the grid.
FHV_HD void face_masks(uint64_t w, const uint64_t nb[6], uint64_t out[6]) {
    out[0] = w & ~below_x(w, nb[0]);
    out[1] = w & ~above_x(w, nb[1]);
    out[2] = w & ~below_y(w, nb[2]);
    out[3] = w & ~above_y(w, nb[3]);
    out[4] = w & ~below_z(w, nb[4]);
    out[5] = w & ~above_z(w, nb[5]);
}
// a brick without faces at a compare: empty, or full among full neighbours
FHV_HD bool faces_none(uint64_t w, const uint64_t nb[6]) {
    return w == 0 || (w & nb[0] & nb[1] & nb[2] & nb[3] & nb[4] & nb[5]) == ~(uint64_t)0;
}

// the four lattice corners of the face of voxel (i, j, k) in direction d, counter-clockwise seen from outside: with (u, v) the unit
// vectors of the next two axes cyclically, o, o + u, o + u + v, o + v from o = voxel + e_a on the + side, and o, o + v, o + u + v, o + u
// from o = voxel on the - side
FHV_HD void face_corners(uint32_t i, uint32_t j, uint32_t k, uint32_t d, uint32_t c[4][3]) {
    const uint32_t a = d >> 1, ua = a == 2 ? 0 : a + 1, va = ua == 2 ? 0 : ua + 1, plus = d & 1;
    const uint32_t p[3] = {i, j, k};
    for (uint32_t x = 0; x < 3; x++) {          // per coordinate, so that no index into c depends on d
        const uint32_t eu = ua == x, ev = va == x, o = p[x] + (plus & (uint32_t)(a == x));
        c[0][x] = o;
        c[1][x] = o + (plus ? eu : ev);
        c[2][x] = o + eu + ev;
        c[3][x] = o + (plus ? ev : eu);
    }
}

// ---- corners and edges ------------------------------------------------------------------------------------------------------------------------
// "all of" / "any of" the two voxels on either side of a lattice plane, for both words at once: bit = voxel & the voxel below it
struct Pair {
    uint64_t all, any;
};
FHV_HD Pair pair_x(Pair cur, Pair prev) { return Pair{cur.all & below_x(cur.all, prev.all), cur.any | below_x(cur.any, prev.any)}; }
FHV_HD Pair pair_y(Pair cur, Pair prev) { return Pair{cur.all & below_y(cur.all, prev.all), cur.any | below_y(cur.any, prev.any)}; }
FHV_HD Pair pair_z(Pair cur, Pair prev) { return Pair{cur.all & below_z(cur.all, prev.all), cur.any | below_z(cur.any, prev.any)}; }
FHV_HD Pair pair_of(uint64_t w) { return Pair{w, w}; }
FHV_HD uint64_t mixed(Pair p) { return p.any & ~p.all; }

// a corner brick whose eight words are all 0 or all ones uses nothing
FHV_HD bool corners_none(const uint64_t W[8]) {
    const uint64_t any = W[0] | W[1] | W[2] | W[3] | W[4] | W[5] | W[6] | W[7], all = W[0] & W[1] & W[2] & W[3] & W[4] & W[5] & W[6] & W[7];
    return any == 0 || all == ~(uint64_t)0;
}
// W[dx + 2 dy + 4 dz] = brick (cx - dx, cy - dy, cz - dz).  corners: bit (la, lb, lc) set iff the eight voxels around lattice corner
// (4 cx + la, 4 cy + lb, 4 cz + lc) are not all equal.  edges[t]: bit set iff the four voxels around the lattice edge from that corner
// one step along axis t are not all equal - an edge belongs to the corner brick of its lower end.
FHV_HD void corner_masks(const uint64_t W[8], uint64_t& corners, uint64_t edges[3]) {
    // along x the edge's voxels are (a, b - 1 .. b, c - 1 .. c): the words with dx == 0, paired along y and z
    const Pair ex = pair_z(pair_y(pair_of(W[0]), pair_of(W[2])), pair_y(pair_of(W[4]), pair_of(W[6])));
    // along y: (a - 1 .. a, b, c - 1 .. c), dy == 0
    const Pair ey = pair_z(pair_x(pair_of(W[0]), pair_of(W[1])), pair_x(pair_of(W[4]), pair_of(W[5])));
    // along z: (a - 1 .. a, b - 1 .. b, c), dz == 0
    const Pair xy0 = pair_y(pair_x(pair_of(W[0]), pair_of(W[1])), pair_x(pair_of(W[2]), pair_of(W[3])));
    const Pair xy1 = pair_y(pair_x(pair_of(W[4]), pair_of(W[5])), pair_x(pair_of(W[6]), pair_of(W[7])));
    edges[0] = mixed(ex);
    edges[1] = mixed(ey);
    edges[2] = mixed(xy0);
    corners = mixed(pair_z(xy0, xy1));
}

// ---- numbering ----------------------------------------------------------------------------------------------------------------------------
FHV_HD uint32_t popcount64(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }
// the position of the r-th set bit of m, r counted from 0 (r < popcount64(m)): by halves
FHV_HD uint32_t select_bit(uint64_t m, uint32_t r) {
    uint32_t pos = 0;
    for (uint32_t width = 32; width > 0; width >>= 1) {
        const uint32_t low = popcount64(m & (((uint64_t)1 << width) - 1));
        if (r >= low) { r -= low; m >>= width; pos += width; }
    }
    return pos;
}
// the corner bricks per axis; their number; the one of lattice corner (a, b, c) and the corner's bit in it
FHV_HD uint32_t corner_side(uint32_t depth) { return (1u << depth) + 1; }
FHV_HD uint64_t n_corner_bricks(uint32_t depth) { const uint64_t s = corner_side(depth); return s * s * s; }          // (1025^3 < 2^31)
FHV_HD uint32_t corner_brick(uint32_t depth, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t s = corner_side(depth);
    return ((c >> 2) * s + (b >> 2)) * s + (a >> 2);
}
FHV_HD uint32_t corner_bit(uint32_t a, uint32_t b, uint32_t c) { return (a & 3) + 4 * (b & 3) + 16 * (c & 3); }
// how many used corners of a corner brick come before bit `bit`
FHV_HD uint32_t rank_below(uint64_t flags, uint32_t bit) { return popcount64(flags & (((uint64_t)1 << bit) - 1)); }
// a lattice coordinate in the frame the bitmap was sampled in, the cube [-1, 1]^3: both factors and the product are exact in f32
FHV_HD float corner_coord(uint32_t a, uint32_t N) { return (float)(2 * (int32_t)a - (int32_t)N) * (1.0f / (float)N); }
}  // namespace fhvm
