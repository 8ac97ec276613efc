// The arithmetic of the nesting of a mesh's slices (fhip_slices_nesting; include/fidget_hip.h, where the definitions stand in full): which
// regular loop of a plane contains which, by a ray cast from each loop's leader towards -x against the float32 polygons themselves -
// the straddle rule, the binary64 predicate, the band of a y and of a segment, the parity reduction of a hit list, the parent choice.
// No HIP and no memory of its own: slice_nest.hip runs it on the device, tests/host_build/slice_nest_host.cpp the whole pipeline
// serially.  There is no counterpart in the reference, which never cuts a mesh.
//
//   hit       leader position q, segment s -> d of another regular loop of q's plane: (s.y <= q.y) != (d.y <= q.y) by float comparison -
//             each end's y compared once, so of two segments that share a vertex on q's row exactly one straddles where the loop passes
//             through the row and none or both where it turns back - and c = (d.x - s.x) (q.y - s.y) - (q.x - s.x) (d.y - s.y), in
//             binary64 from the floats converted, every operation rounded on its own: c < 0 for an upward segment (s.y <= q.y), c > 0
//             for a downward one.  c == 0 is no hit.  Not exact for arbitrary float32 input - the differences may round - but a function
//             of the six floats alone: a leader within rounding of another loop's boundary falls either side, always the same side
//   band      band(y) = clamp(floor((y - y0) * scale), 0, nb - 1) in float32, the subtraction and the product each rounded on its own;
//             NaN -> 0.  With scale >= 0 every step is monotone non-decreasing in y, so band(min) <= band(q.y) <= band(max) for a
//             segment that straddles q's row, whatever y0, scale and nb are: no rounding argument is needed.  scale = nb / (y1 - y0)
//             over the plane's y-extent [y0, y1], 0 where that is empty or not finite - then every y is in band 0
//   parity    a leader's hit list holds a loop's id once per hit segment; the loops of odd multiplicity contain the leader's loop
//   parent    the containing loop of the largest depth, the smallest id among equals
#pragma once
#include <stdint.h>

#include "mesh_slice.hpp"

namespace fhsn {
constexpr uint32_t NONE = 0xFFFFFFFFu;                  // no parent; the parent and depth of an irregular loop
constexpr uint64_t MAX_ENTRIES = 0xFFFFFFFEull;         // band entries, hits, bands: prefix sums are uint32
constexpr uint32_t IRREGULAR = 1u, POSITIVE = 2u;       // a loop's flags on the device: it takes no part; area2 > 0
// The host's rule for the bands of a plane: one per SEGMENTS_PER_BAND regular segments, between 1 and MAX_BANDS - a band then holds about
// that many segments and a leader's wave reads them in one step.  (8 a band was tried first: on a fine mesh, whose segments are as long as
// a cell of the mesher, the count then ran three times, 17 + 9 + 5 ms, to arrive at what 32 a band gives at once.)  Where the count pass
// finds more than ENTRY_MULTIPLE entries per regular segment - long segments, each in many bands - every plane's number is halved and
// the count repeated, until it fits or all are 1
constexpr uint32_t SEGMENTS_PER_BAND = 32, MAX_BANDS = 1u << 20, ENTRY_MULTIPLE = 4;

struct Band { float y0, scale; uint32_t nb, base; };          // a plane's bands: base .. base + nb of the call's

FHV_HD uint32_t default_bands(uint64_t regular_segments) {
    const uint64_t nb = regular_segments / SEGMENTS_PER_BAND;
    return nb < 1 ? 1u : nb > MAX_BANDS ? MAX_BANDS : (uint32_t)nb;
}
FHV_HD float band_scale(float y0, float y1, uint32_t nb) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float extent = y1 - y0;
    if (!(extent > 0.0f) || !fhtopo::finite(extent)) return 0.0f;
    const float s = (float)nb / extent;
    return fhtopo::finite(s) ? s : 0.0f;
}
FHV_HD uint32_t band(float y, const Band& B) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (B.nb <= 1) return 0;
    const float dy = y - B.y0;
    const float t = dy * B.scale;
    if (!(t > 0.0f)) return 0;          // (NaN too)
    if (t >= (float)B.nb) return B.nb - 1;
    const uint32_t b = (uint32_t)t;
    return b < B.nb ? b : B.nb - 1;
}
struct BandRange { uint32_t lo, hi; };          // the bands lo <= b <= hi
FHV_HD BandRange segment_bands(float sy, float dy, const Band& B) {
    const uint32_t a = band(sy, B), b = band(dy, B);          // (monotone: the bands of the ends are the ends of the bands)
    return a < b ? BandRange{a, b} : BandRange{b, a};
}

FHV_HD bool straddles(float sy, float dy, float qy) { return (sy <= qy) != (dy <= qy); }
FHV_HD double side(const float* s, const float* d, const float* q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double ax = (double)d[0] - (double)s[0], ay = (double)q[1] - (double)s[1];
    const double bx = (double)q[0] - (double)s[0], by = (double)d[1] - (double)s[1];
    const double a = ax * ay, b = bx * by;
    return a - b;
}
FHV_HD bool hit(const float* s, const float* d, const float* q) {
    if (!straddles(s[1], d[1], q[1])) return false;
    const double c = side(s, d, q);
    return s[1] <= q[1] ? c < 0.0 : c > 0.0;
}

// hits[0 .. h): is hits[i] the first of its value, and is that value there an odd number of times?  Any length; reads the list alone
FHV_HD bool odd_first(const uint32_t* hits, uint32_t h, uint32_t i) {
    const uint32_t mine = hits[i];
    uint32_t times = 0;
    for (uint32_t j = 0; j < h; j++) {
        if (hits[j] != mine) continue;
        if (j < i) return false;
        times++;
    }
    return (times & 1u) != 0;
}
// the list of the loops that contain l -> its parent; ids at or beyond n_loops and loops without a depth are passed over
FHV_HD uint32_t parent_of(const uint32_t* contain, uint32_t n, const uint32_t* depth, uint32_t n_loops) {
    uint32_t best = NONE, best_depth = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t c = contain[k];
        if (c >= n_loops) continue;
        const uint32_t d = depth[c];
        if (d == NONE) continue;
        if (best == NONE || d > best_depth || (d == best_depth && c < best)) { best = c; best_depth = d; }
    }
    return best;
}
FHV_HD bool improper(uint32_t depth_l, uint32_t parent, const uint32_t* depth) { return parent != NONE && depth[parent] != depth_l - 1; }
FHV_HD bool misoriented(uint32_t depth_l, uint32_t flags) { return ((depth_l & 1u) == 0) != ((flags & POSITIVE) != 0); }
}  // namespace fhsn
