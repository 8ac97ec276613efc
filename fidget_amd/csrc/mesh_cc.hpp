// The bit arithmetic of connected-component labelling on the voxel bitmap (fhip_voxels_components, include/fidget_hip.h): the components
// of one 4 x 4 x 4 brick taken alone, by flood fill inside its 64-bit word, and which positions of a neighbouring brick touch a set of
// voxels of this one.  No HIP and no memory access: compiled for the device by mesh.hip and for the host by
// tests/host_build/mesh_cc_host.cpp.  There is no counterpart in the reference: it has no voxel bitmap.
//
// Bit lx + 4 ly + 16 lz of a word is voxel (lx, ly, lz) of its brick (mesh_vox.hpp).  Connectivity 6: neighbours share a face;
// connectivity 26: a face, an edge or a corner.
#pragma once
#include <stdint.h>

#include "mesh_vox.hpp"

namespace fhcc {
constexpr uint32_t MAX_LOCAL = 32;       // components of one brick at most (local_components)
constexpr uint32_t N_DIRS = 13;          // the "positive half" of the 26 directions; the first 3 are the faces +x, +y, +z
FHV_HD bool conn_ok(uint32_t conn) { return conn == 6 || conn == 26; }
FHV_HD uint32_t n_dirs(uint32_t conn) { return conn == 26 ? N_DIRS : 3; }

// the voxels with lx = 0 / 3, ly = 0 / 3, lz = 0 / 3
constexpr uint64_t X0 = 0x1111111111111111ull, X3 = 0x8888888888888888ull;
constexpr uint64_t Y0 = 0x000F000F000F000Full, Y3 = 0xF000F000F000F000ull;
constexpr uint64_t Z0 = 0x000000000000FFFFull, Z3 = 0xFFFF000000000000ull;

// A set of voxels and its neighbours along one axis.  x: a shift by 1, without the bit that would wrap into the next row (lx = 0 after
// a shift up, lx = 3 after a shift down); y: a shift by 4 within the planes of 16; z: a shift by 16, where what leaves the word is gone.
FHV_HD uint64_t dilate_x(uint64_t m) { return m | ((m << 1) & ~X0) | ((m >> 1) & ~X3); }
FHV_HD uint64_t dilate_y(uint64_t m) { return m | ((m << 4) & ~Y0) | ((m >> 4) & ~Y3); }
FHV_HD uint64_t dilate_z(uint64_t m) { return m | (m << 16) | (m >> 16); }
// one step of the flood fill: 6 - the three axes side by side; 26 - one after the other (x, then y, then z: the 3 x 3 x 3 box)
FHV_HD uint64_t dilate(uint64_t m, uint32_t conn) {
    return conn == 26 ? dilate_z(dilate_y(dilate_x(m))) : (dilate_x(m) | dilate_y(m) | dilate_z(m));
}
// the component of `word` (alone) that holds the lowest bit of `rest`, a non-empty subset of word made of whole components.  At most 64
// steps: every step but the last adds a voxel.
FHV_HD uint64_t lowest_component(uint64_t rest, uint64_t word, uint32_t conn) {
    if (word == ~(uint64_t)0) return word;      // a full brick is one component either way
    uint64_t m = rest & (~rest + 1);
    for (;;) {
        const uint64_t g = dilate(m, conn) & word;
        if (g == m) return m;
        m = g;
    }
}
// The components of one brick, as bit masks in the order of their lowest set bits; -> their number.
// At most 32, MAX_LOCAL: pair the voxels (2 q, ly, lz), (2 q + 1, ly, lz) - 32 pairs.  The two voxels of a pair share a face, so under
// either connectivity a pair never holds voxels of two components, and every component holds a voxel of some pair.  The 3-D checkerboard
// (lx + ly + lz even) has no two voxels that share a face: 32 components under connectivity 6 (one under 26, where all of them touch
// along edges).
FHV_HD uint32_t local_components(uint64_t word, uint32_t conn, uint64_t masks[MAX_LOCAL]) {
    if (word == 0) return 0;
    if (word == ~(uint64_t)0) { masks[0] = word; return 1; }
    uint32_t n = 0;
    for (uint64_t rest = word; rest != 0;) {
        const uint64_t m = lowest_component(rest, word, conn);
        masks[n++] = m;
        rest &= ~m;
    }
    return n;
}
// ... their number alone (no array: what the kernels use, which walk the components with lowest_component as they need them)
FHV_HD uint32_t local_count(uint64_t word, uint32_t conn) {
    if (word == 0) return 0;
    if (word == ~(uint64_t)0) return 1;
    uint32_t n = 0;
    for (uint64_t rest = word; rest != 0; n++) rest &= ~lowest_component(rest, word, conn);
    return n;
}

// Direction d < N_DIRS as (dx, dy, dz) in {-1, 0, 1}: the 13 whose last non-zero component (z, else y, else x) is +1 - together with their
// opposites all 26.  0..2: the faces +x, +y, +z; 3..8: the edges; 9..12: the corners.  (packed two bits a direction, the value + 1)
FHV_HD void direction(uint32_t d, int& dx, int& dy, int& dz) {
    //                              d = 12 11 10  9  8  7  6  5  4  3  2  1  0
    constexpr uint32_t DX = 0x0894896;  // -1  1 -1  1  0  0 -1  1 -1  1  0  0  1
    constexpr uint32_t DY = 0x0289699;  // -1 -1  1  1 -1  1  0  0  1  1  0  1  0
    constexpr uint32_t DZ = 0x2AAA965;  //  1  1  1  1  1  1  1  1  0  0  1  0  0
    dx = (int)((DX >> (2 * d)) & 3u) - 1; dy = (int)((DY >> (2 * d)) & 3u) - 1; dz = (int)((DZ >> (2 * d)) & 3u) - 1;
}

// For the voxels `mask` of a brick and the brick one step along (dx, dy, dz), any of the 26 directions: the positions of that brick, in
// its own bit numbering, that are neighbours of some voxel of mask.  Per axis with a step, only the layer that touches counts and lands
// on the opposite layer (3 -> 0 for +1, 0 -> 3 for -1): a face direction moves a layer, an edge direction a row, a corner direction one
// voxel.  Under connectivity 26 the image is then dilated along the axes without a step - within the plane for a face, along the row for
// an edge.  Under connectivity 6 only faces touch: edge and corner directions give 0.
FHV_HD uint64_t carry(uint64_t mask, int dx, int dy, int dz, uint32_t conn) {
    if (conn != 26 && (dx != 0) + (dy != 0) + (dz != 0) != 1) return 0;
    uint64_t m = mask;
    if (dx > 0) m = (m & X3) >> 3; else if (dx < 0) m = (m & X0) << 3;
    if (dy > 0) m = (m & Y3) >> 12; else if (dy < 0) m = (m & Y0) << 12;
    if (dz > 0) m = (m & Z3) >> 48; else if (dz < 0) m = (m & Z0) << 48;
    if (conn == 26) {
        if (dx == 0) m = dilate_x(m);
        if (dy == 0) m = dilate_y(m);
        if (dz == 0) m = dilate_z(m);
    }
    return m;
}

// Local bounds of a non-empty mask: lo / hi [axis] in 0..3, inclusive.  (Which layers hold a voxel: 4 bits an axis.)
FHV_HD void local_bounds(uint64_t mask, uint32_t lo[3], uint32_t hi[3]) {
    uint32_t occ[3] = {0, 0, 0};
    for (uint32_t v = 0; v < 4; v++) {
        if (mask & (X0 << v)) occ[0] |= 1u << v;
        if (mask & (Y0 << (4 * v))) occ[1] |= 1u << v;
        if (mask & (Z0 << (16 * v))) occ[2] |= 1u << v;
    }
    for (uint32_t a = 0; a < 3; a++) {
        lo[a] = (occ[a] & 1u) ? 0 : (occ[a] & 2u) ? 1 : (occ[a] & 4u) ? 2 : 3;
        hi[a] = (occ[a] & 8u) ? 3 : (occ[a] & 4u) ? 2 : (occ[a] & 2u) ? 1 : 0;
    }
}
// whether some voxel of `mask`, in brick (bx, by, bz) of a bitmap of B bricks per axis, has a coordinate equal to 0 or 4 B - 1
FHV_HD bool touches_border(uint64_t mask, uint32_t bx, uint32_t by, uint32_t bz, uint32_t B) {
    uint64_t edge = 0;
    if (bx == 0) edge |= X0;
    if (by == 0) edge |= Y0;
    if (bz == 0) edge |= Z0;
    if (bx == B - 1) edge |= X3;
    if (by == B - 1) edge |= Y3;
    if (bz == B - 1) edge |= Z3;
    return (mask & edge) != 0;
}
// the key of a voxel, word * 64 + bit, as (i, j, k)
FHV_HD void key_voxel(uint64_t key, uint32_t depth, uint32_t v[3]) {
    const uint64_t w = key >> 6;
    const uint32_t bit = (uint32_t)key & 63u, Bm = (1u << depth) - 1;
    v[0] = 4 * ((uint32_t)w & Bm) + (bit & 3u);
    v[1] = 4 * ((uint32_t)(w >> depth) & Bm) + ((bit >> 2) & 3u);
    v[2] = 4 * ((uint32_t)(w >> (2 * depth)) & Bm) + (bit >> 4);
}
}  // namespace fhcc
