// The arithmetic of 2D contouring (fhip_contour2d, include/fidget_hip.h): which lattice edge has which index, where a vertex sits on a
// crossing edge, which segments a cell emits, how a crossing edge finds its vertex id, and how the link array is followed into loops.
// No HIP and no memory access but through the pointers it is given: compiled for the device by mesh.hip (k_ctr_*) and for the host by
// tests/host_build/contour_host.cpp.  (A directory of its own: the render-source hash of tools/src_hash.py covers the files directly in
// csrc/, and nothing here can alter a render kernel.)
//
// The image is v[j * W + i], W x H, `inside` = v < 0 (NaN: outside); the centre of pixel (i, j) is the point (float(i), float(j)).
//   horizontal edge h(i, j): (i, j) - (i + 1, j), 0 <= i < W - 1, 0 <= j < H;      index j * (W - 1) + i
//   vertical edge   u(i, j): (i, j) - (i, j + 1), 0 <= i < W,     0 <= j < H - 1;  index (W - 1) * H + j * W + i
//   cell            c(i, j): 0 <= i < W - 1, 0 <= j < H - 1, index j * (W - 1) + i; corners bit 0 (i, j), 1 (i + 1, j), 2 (i + 1, j + 1),
//                            3 (i, j + 1); edges B = h(i, j), R = u(i + 1, j), T = h(i, j + 1), L = u(i, j)
// An edge crosses when `inside` differs at its ends; vertex k sits on the k-th crossing edge in index order.  Segments are directed with
// the inside on their left (x to the right, j upward).
#pragma once
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define FHC_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define FHC_HD __attribute__((always_inline)) inline
#endif

namespace fhctr {
constexpr uint32_t NONE = 0xFFFFFFFFu;        // next[k]: no segment leaves vertex k
constexpr uint32_t EDGE_BLOCK = 256;          // edges (and cells) per block of the kernels: four ballot words, one count

// (W - 1) * H and W * (H - 1) in 64 bits; an image without pixels has no edges
FHC_HD uint64_t n_hedges(uint32_t W, uint32_t H) { return (W && H) ? (uint64_t)(W - 1) * H : 0; }
FHC_HD uint64_t n_vedges(uint32_t W, uint32_t H) { return (W && H) ? (uint64_t)W * (H - 1) : 0; }
FHC_HD uint64_t n_edges(uint32_t W, uint32_t H) { return n_hedges(W, H) + n_vedges(W, H); }
FHC_HD uint64_t n_cells(uint32_t W, uint32_t H) { return (W && H) ? (uint64_t)(W - 1) * (H - 1) : 0; }
// what fhip_contour2d takes: pixel and edge indices fit 32 bits
FHC_HD bool size_ok(uint32_t W, uint32_t H) { return (uint64_t)W * H < ((uint64_t)1 << 32) && n_edges(W, H) < ((uint64_t)1 << 32); }

FHC_HD bool inside(float v) { return v < 0.0f; }

// (everything below: W, H with size_ok)
FHC_HD uint32_t h_index(uint32_t i, uint32_t j, uint32_t W) { return j * (W - 1) + i; }
FHC_HD uint32_t u_index(uint32_t i, uint32_t j, uint32_t W, uint32_t H) { return (W - 1) * H + j * W + i; }
struct Edge { uint32_t i, j, vertical; };       // its first end (i, j); the other end (i + 1, j), or (i, j + 1) when vertical
FHC_HD Edge edge_at(uint32_t e, uint32_t W, uint32_t H) {
    const uint32_t nh = (W - 1) * H;
    Edge E;
    if (e < nh) { E.j = e / (W - 1); E.i = e - E.j * (W - 1); E.vertical = 0; }
    else { e -= nh; E.j = e / W; E.i = e - E.j * W; E.vertical = 1; }
    return E;
}
// the pixels of an edge's two ends
FHC_HD uint32_t edge_pixel0(const Edge& E, uint32_t W) { return E.j * W + E.i; }
FHC_HD uint32_t edge_pixel1(const Edge& E, uint32_t W) { return E.j * W + E.i + (E.vertical ? W : 1u); }

// where the vertex sits between the first end (value a) and the other (b): one subtraction, one correctly rounded division; anything
// that is not in [0, 1] - NaN and infinite ends - becomes the middle
FHC_HD float edge_t(float a, float b) {
    float t = a / (a - b);
    if (!(t >= 0.0f && t <= 1.0f)) t = 0.5f;
    return t;
}
FHC_HD void edge_vertex(const Edge& E, float a, float b, float xy[2]) {
    const float t = edge_t(a, b);
    xy[0] = E.vertical ? (float)E.i : (float)E.i + t;
    xy[1] = E.vertical ? (float)E.j + t : (float)E.j;
}

// ---- cells -----------------------------------------------------------------------------------------------------------------------------
FHC_HD uint32_t cell_mask(float v00, float v10, float v11, float v01) {
    return (inside(v00) ? 1u : 0u) | (inside(v10) ? 2u : 0u) | (inside(v11) ? 4u : 0u) | (inside(v01) ? 8u : 0u);
}
FHC_HD bool saddle_centre_inside(float v00, float v10, float v11, float v01) { return ((v00 + v10) + (v11 + v01)) * 0.25f < 0.0f; }
FHC_HD uint32_t cell_count(uint32_t mask) { return (mask == 0 || mask == 15) ? 0u : ((mask == 5 || mask == 10) ? 2u : 1u); }
enum : uint32_t { EB = 0, ER = 1, ET = 2, EL = 3 };
// The segments of a cell, packed: n | from0 << 2 | to0 << 4 | from1 << 6 | to1 << 8 (edge codes EB .. EL).  A saddle's two segments in
// the order the table of the header gives them; `centre_in` matters to masks 5 and 10 alone.
FHC_HD uint32_t cell_case(uint32_t mask, bool centre_in) {
#define FHC_S1(f, t) (1u | ((f) << 2) | ((t) << 4))
#define FHC_S2(f0, t0, f1, t1) (2u | ((f0) << 2) | ((t0) << 4) | ((f1) << 6) | ((t1) << 8))
    switch (mask) {
        case 1: return FHC_S1(EB, EL);
        case 2: return FHC_S1(ER, EB);
        case 3: return FHC_S1(ER, EL);
        case 4: return FHC_S1(ET, ER);
        case 5: return centre_in ? FHC_S2(EB, ER, ET, EL) : FHC_S2(EB, EL, ET, ER);
        case 6: return FHC_S1(ET, EB);
        case 7: return FHC_S1(ET, EL);
        case 8: return FHC_S1(EL, ET);
        case 9: return FHC_S1(EB, ET);
        case 10: return centre_in ? FHC_S2(EL, EB, ER, ET) : FHC_S2(ER, EB, EL, ET);
        case 11: return FHC_S1(ER, ET);
        case 12: return FHC_S1(EL, ER);
        case 13: return FHC_S1(EB, ER);
        case 14: return FHC_S1(EL, EB);
        default: return 0u;
    }
#undef FHC_S1
#undef FHC_S2
}
FHC_HD uint32_t case_count(uint32_t c) { return c & 3u; }
FHC_HD uint32_t case_from(uint32_t c, uint32_t s) { return (c >> (2 + 4 * s)) & 3u; }
FHC_HD uint32_t case_to(uint32_t c, uint32_t s) { return (c >> (4 + 4 * s)) & 3u; }
// the lattice edge behind edge code `code` of cell (i, j)
FHC_HD uint32_t cell_edge(uint32_t code, uint32_t i, uint32_t j, uint32_t W, uint32_t H) {
    return (code & 1u) ? u_index(i + (code == ER ? 1u : 0u), j, W, H) : h_index(i, j + (code == ET ? 1u : 0u), W);
}

// ---- vertex ids ------------------------------------------------------------------------------------------------------------------------
// k_ctr_edges leaves one bit per edge - word e / 64, bit e % 64: the edge crosses - and one count per EDGE_BLOCK edges; block_off is the
// exclusive prefix sum of the counts.  The id of crossing edge e is the number of crossing edges before it: 4 + 1/64 bytes per 256 edges
// held and at most four words read, against 4 bytes per edge for a table of ids.
FHC_HD uint32_t popc64(uint64_t w) { return (uint32_t)__builtin_popcountll(w); }
FHC_HD bool edge_crosses(const uint64_t* bits, uint32_t e) { return (bits[e >> 6] >> (e & 63u)) & 1u; }
FHC_HD uint32_t vertex_id(const uint64_t* bits, const uint32_t* block_off, uint32_t e) {
    const uint32_t w = e >> 6, w0 = w & ~3u;
    uint32_t id = block_off[e / EDGE_BLOCK] + popc64(bits[w] & (((uint64_t)1 << (e & 63u)) - 1));
    for (uint32_t k = w0; k < w; k++) id += popc64(bits[k]);
    return id;
}

// ---- loops (host) ----------------------------------------------------------------------------------------------------------------------
// Follows next[0 .. n - 1] into chains: open ones first - from every vertex no segment arrives at, in ascending order of that vertex -
// then the closed ones, each from its smallest vertex, in ascending order of that.  order (n ids, the chains one after the other),
// loop_start (where each begins in `order`, and n at the end) and closed (1 / 0 per chain) may each be null: the count alone.
// Returns false for an array no contour gives: an id >= n that is not NONE, or a vertex two segments arrive at.
inline bool follow_loops(const uint32_t* next, uint64_t n, uint32_t* order, uint64_t* loop_start, uint8_t* closed, uint64_t* n_loops) {
    std::vector<uint8_t> seen(n, 0);        // bit 0: a segment arrives; bit 1: already in a chain
    for (uint64_t k = 0; k < n; k++) {
        const uint32_t t = next[k];
        if (t == NONE) continue;
        if (t >= n || (seen[t] & 1)) return false;
        seen[t] |= 1;
    }
    uint64_t at = 0, loops = 0;
    for (int pass = 0; pass < 2; pass++)          // 0: the open chains, 1: what is left is closed
        for (uint64_t k = 0; k < n; k++) {
            if ((seen[k] & 2) || (pass == 0 && (seen[k] & 1))) continue;
            if (loop_start) loop_start[loops] = at;
            if (closed) closed[loops] = (uint8_t)pass;
            loops++;
            for (uint32_t v = (uint32_t)k; v != NONE && !(seen[v] & 2); v = next[v]) {
                seen[v] |= 2;
                if (order) order[at] = v;
                at++;
            }
        }
    if (loop_start) loop_start[loops] = at;
    if (n_loops) *n_loops = loops;
    return true;
}
}  // namespace fhctr
