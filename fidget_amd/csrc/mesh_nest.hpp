// The arithmetic of the nesting of a voxel bitmap's outlines (fhip_outlines_nesting, include/fidget_hip.h, where the definitions stand):
// from a loop's leader the nearest boundary edge to its left on the leader's pixel row, from that edge the corner where its straight
// run begins, from that corner the vertex id and so the loop; then the steps of the pointer doubling that turn the `left` links into
// parents and depths.  No HIP and no memory of its own: compiled for the device by nest.hip and for the host by
// tests/host_build/mesh_nest_host.cpp.  The rows as bit vectors and the corner masks are mesh_outline.hpp's.
//
// Every search here is bounded by its own arguments, whatever the bitmap holds: the row scan ends at a = 0, the column walk at the
// lattice's border, the lookup inside [lo, hi) of the layer's vertices - and the caller keeps of the loop found only one of the same
// layer with a smaller id, so every chain of links descends and ends.
#pragma once
#include <stdint.h>

#include "mesh_outline.hpp"

namespace fhnest {
constexpr uint32_t NONE = 0xFFFFFFFFu;

// The nearest vertical unit boundary edge left of corner (a0, b0) on pixel row b0 of layer k: the largest a < a0 with
// P(a - 1, b0) != P(a, b0).  The "differs from its left neighbour" mask of a chunk of 32 corners is the row's bits against themselves
// shifted by one; below a0 in its own chunk, whole in the chunks towards a = 0; the last set bit by a count of leading zeros.
// `d`: the edge's heading, 2 (-y) where P(a, b0) is set - the left side of a set pixel - and 3 (+y) where it is clear.
FHV_HD bool left_edge(const uint64_t* bricks, uint32_t depth, uint32_t k, uint32_t a0, uint32_t b0, uint32_t& a, uint32_t& d) {
    const uint32_t N = 4u << depth;
    if (a0 > N || b0 >= N) return false;
    uint32_t keep = fhol::below(a0 % fhol::CHUNK);
    for (uint32_t c = a0 / fhol::CHUNK + 1; c-- > 0; keep = 0xFFFFFFFFu) {
        const uint64_t r = fhol::row_bits(bricks, depth, b0, k, c);
        const uint32_t differs = (uint32_t)(r ^ (r >> 1)) & keep;
        if (differs) {
            const uint32_t s = 31u - (uint32_t)__builtin_clz(differs);
            a = fhol::CHUNK * c + s;
            d = ((r >> (s + 1)) & 1u) ? 2u : 3u;
            return true;
        }
    }
    return false;
}
// The corner at which the straight run through the unit edge (a, b0)-(a, b0 + 1) of heading d begins: walked against the heading - down
// from b0 for +y, up from b0 + 1 for -y - the nearest corner of the column that holds a vertex leaving with d.
FHV_HD bool run_start(const uint64_t* bricks, uint32_t depth, uint32_t k, uint32_t a, uint32_t b0, uint32_t d, uint32_t& b) {
    const uint32_t N = 4u << depth;
    if (d == 3) {
        for (uint32_t b2 = b0 + 1; b2-- > 0;)
            if (fhol::corner_masks(bricks, depth, k, a, b2).leave[3] & 1u) { b = b2; return true; }
    } else {
        for (uint32_t b2 = b0 + 1; b2 <= N; b2++)
            if (fhol::corner_masks(bricks, depth, k, a, b2).leave[2] & 1u) { b = b2; return true; }
    }
    return false;
}
// The id of the vertex that leaves corner (a, b) with the vertical heading d, among the layer's vertices [lo, hi): their words
// a | b << 16 ascend with the id, so the first one equal is a lower bound search.  A saddle's two vertices share the word; only
// m = 10 has vertical outgoing headings, 2 then 3.  NONE where the layer holds no vertex there.
FHV_HD uint32_t vertex_at(const uint32_t* xy, uint32_t lo, uint32_t hi, uint32_t a, uint32_t b, uint32_t d) {
    const uint32_t word = a | (b << 16);
    uint32_t first = lo, n = hi - lo;
    while (n > 0) {
        const uint32_t half = n / 2;
        if (xy[first + half] < word) { first += half + 1; n -= half + 1; } else n = half;
    }
    if (first >= hi || xy[first] != word) return NONE;
    return d == 3 && first + 1 < hi && xy[first + 1] == word ? first + 1 : first;
}
// the layer of the call (0 <= layer < K) that holds id `i`, from the K + 1 ascending starts; start[layer] <= i < start[layer + 1]
FHV_HD uint32_t layer_of(const uint32_t* start, uint32_t K, uint32_t i) {
    uint32_t lo = 0, n = K;          // the last layer whose start is <= i
    while (n > 1) {
        const uint32_t half = n / 2;
        if (start[lo + half] <= i) { lo += half; n -= half; } else n = half;
    }
    return lo;
}
// left[l] for loop l of layer k (the layer-th of the call), whose leader is vertex `leader`: the three steps above and loop_of; kept
// only where it is a loop of the same layer before l.
FHV_HD uint32_t left_of(const uint64_t* bricks, uint32_t depth, uint32_t k, const uint32_t* xy, const uint32_t* loop_of, uint32_t v_lo, uint32_t v_hi, uint32_t l_lo,
                        uint32_t l, uint32_t leader) {
    if (leader < v_lo || leader >= v_hi) return NONE;
    const uint32_t p = xy[leader];
    uint32_t a = 0, b = 0, d = 0;
    if (!left_edge(bricks, depth, k, p & 0xFFFFu, p >> 16, a, d)) return NONE;
    if (!run_start(bricks, depth, k, a, p >> 16, d, b)) return NONE;
    const uint32_t v = vertex_at(xy, v_lo, v_hi, a, b, d);
    if (v == NONE) return NONE;
    const uint32_t e = loop_of[v];
    return e >= l_lo && e < l ? e : NONE;
}

// ---- pointer doubling ---------------------------------------------------------------------------------------------------------------------
// Parents.  link[l] is a loop of l's chain left[l], left[left[l]], ... such that every loop of the chain before it has l's sign; at
// the start it is left[l].  While link[l] has l's sign, link[link[l]] is such a loop too - twice as far, or the chain's end.  A link
// that is NONE or of the other sign stays: it is the parent.
FHV_HD uint32_t resolve_step(const uint32_t* link, const int64_t* area2, uint32_t l) {
    const uint32_t e = link[l];
    if (e == NONE || ((area2[e] < 0) != (area2[l] < 0))) return e;
    return link[e];
}
// Depths.  (anc[l], hops[l]): an ancestor and the number of parent links up to it, (parent[l], 1) at the start, (NONE, depth) at the
// end; a step adds the ancestor's own pair.
FHV_HD void depth_step(const uint32_t* anc, const uint32_t* hops, uint32_t l, uint32_t& anc_out, uint32_t& hops_out) {
    const uint32_t e = anc[l];
    anc_out = e == NONE ? NONE : anc[e];
    hops_out = hops[l] + (e == NONE ? 0u : hops[e]);
}
// the rounds after which every chain of a layer with `n` loops has ended: its links number n - 1 at the most, a round doubles the reach
FHV_HD uint32_t rounds(uint64_t n) {
    uint32_t r = 0;
    while (((uint64_t)1 << r) < n) r++;
    return r;
}
}  // namespace fhnest
