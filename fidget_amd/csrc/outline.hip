// The outlines of a voxel bitmap's layers (fhip_voxels_outlines, include/fidget_hip.h; the host side is capi_outline.hpp).  The bit
// arithmetic is mesh_outline.hpp's, which the tests also build for the host.  An entry is a chunk of 32 corners of a lattice row of a
// layer; entries ascend the way the vertex ids do - layer, row b, corner a.
//   k_ol_count      a lane per entry: the two image rows around the lattice row as bit vectors, nine words each, the masks from shifts
//                   and ANDs, the number of vertices from two popcounts.  Lanes of a wave lie along the row, then along b.
//   k_ol_layers     a block per layer: the 64-bit sum of its entries' counts, for vertex_start and the overflow check on the host
//   k_ol_emit       a lane per entry that has vertices (the others leave after one look at the scanned bases): for each vertex its
//                   corner as one 32-bit store and its successor - along x the next or the previous set bit of the "arrived at" mask,
//                   in the chunk's own word or in the following chunks'; along y a walk over the corners of the column
//   k_ol_unite      a lane per vertex: cc_unite(v, next[v]) (mesh.hip) - the smaller root wins, so a loop's root is its leader
//   k_ol_measure    a lane per vertex: its cross product and step length added to its loop's row, the bounds by atomic min / max, the
//                   leader written by the root.  A wave whose vertices all belong to one loop adds them up first and sends one set of
//                   atomics.  Integer atomics alone: the sums do not depend on the order of arrival.
// Between them k_cc_init, k_cc_flatten, k_cc_roots, k_cc_number and the prefix sums (k_scan_*) of mesh.hip.  No kernel uses LDS beyond
// k_ol_layers' four partial sums, none waits for another workgroup.  Included by mesh.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "mesh_outline.hpp"

namespace fhm {
struct OlEntry { uint32_t layer, b, c; };
// entry e of a call over `layers` layers; false beyond the last
__device__ __forceinline__ bool ol_entry(uint64_t e, uint32_t depth, uint32_t layers, OlEntry& E) {
    const uint32_t C = fhol::n_chunks(depth), rows = (4u << depth) + 1;
    const uint64_t row = e / C;
    E.c = (uint32_t)(e - row * C);
    E.layer = (uint32_t)(row / rows);
    E.b = (uint32_t)(row - (uint64_t)E.layer * rows);
    return E.layer < layers;
}
__global__ void __launch_bounds__(256) k_ol_count(const uint64_t* __restrict__ bricks, uint32_t depth, uint32_t k0, uint32_t layers, uint32_t* __restrict__ cnt) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    OlEntry E;
    if (!ol_entry(e, depth, layers, E)) return;
    cnt[e] = fhol::count(fhol::row_masks(bricks, depth, k0 + E.layer, E.b, E.c));
}
__global__ void __launch_bounds__(256) k_ol_layers(const uint32_t* __restrict__ cnt, uint32_t depth, unsigned long long* __restrict__ per_layer) {
    __shared__ unsigned long long sh[256 / WAVE];
    const uint64_t per = (uint64_t)((4u << depth) + 1) * fhol::n_chunks(depth);
    const uint32_t* const mine = cnt + (uint64_t)blockIdx.x * per;
    unsigned long long s = 0;
    for (uint64_t i = threadIdx.x; i < per; i += 256) s += mine[i];
    for (int d = WAVE / 2; d > 0; d >>= 1) s += __shfl_down(s, d);
    if ((threadIdx.x & (WAVE - 1)) == 0) sh[threadIdx.x / WAVE] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int k = 0; k < 256 / WAVE; k++) t += sh[k];
        per_layer[blockIdx.x] = t;
    }
}
// base: the exclusive prefix sums of cnt, n_entries + 1 of them.  xy: (a, b) as two uint16 in one word; next: the successor's id
__global__ void __launch_bounds__(256) k_ol_emit(const uint64_t* __restrict__ bricks, uint32_t depth, uint32_t k0, uint32_t layers, uint32_t conn,
                                                 const uint32_t* __restrict__ base, uint32_t* __restrict__ xy, uint32_t* __restrict__ next) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    OlEntry E;
    if (!ol_entry(e, depth, layers, E)) return;
    const uint32_t first = base[e];
    if (base[e + 1] == first) return;
    const uint32_t k = k0 + E.layer;
    const fhol::Masks M = fhol::row_masks(bricks, depth, k, E.b, E.c);
#pragma unroll
    for (uint32_t d = 0; d < 4; d++)
        for (uint32_t rest = M.leave[d]; rest != 0; rest &= rest - 1) {
            const uint32_t s = (uint32_t)__builtin_ctz(rest), v = first + fhol::rank_leaving(M, s, d);
            xy[v] = (fhol::CHUNK * E.c + s) | (E.b << 16);
            next[v] = fhol::successor(bricks, depth, k, E.layer, conn, base, M, E.b, E.c, s, d);
        }
}
__global__ void __launch_bounds__(256) k_ol_unite(const uint32_t* __restrict__ next, uint32_t n, uint32_t* parent) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const uint32_t w = next[v];
    if (w < n) cc_unite(parent, (uint32_t)v, w);          // (always: fhol::successor finds one on a closed outline)
}
struct OlLoopTable {
    unsigned long long *area2, *perimeter;          // area2: an int64 in two's complement
    uint32_t *n_vertices, *leader, *lo, *hi;        // lo, hi: [loop][2]
};
__global__ void __launch_bounds__(256) k_ol_measure(const uint32_t* __restrict__ xy, const uint32_t* __restrict__ next, const uint32_t* __restrict__ parent,
                                                    const uint32_t* __restrict__ loop_of, uint32_t n, OlLoopTable T) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    if (__ballot(live) == 0) return;          // (ids ascend with the lanes: lane 0 of every other wave is live)
    uint32_t l = 0, count = 0, lo_x = ~0u, lo_y = ~0u, hi_x = 0, hi_y = 0;
    long long cross = 0;
    unsigned long long length = 0;
    if (live) {
        const uint32_t v = (uint32_t)i, w = next[v], p = xy[v], q = xy[w < n ? w : v];
        const int64_t x = p & 0xFFFFu, y = p >> 16, x2 = q & 0xFFFFu, y2 = q >> 16;
        l = loop_of[v];
        cross = x * y2 - x2 * y;
        length = (unsigned long long)((x2 > x ? x2 - x : x - x2) + (y2 > y ? y2 - y : y - y2));
        count = 1;
        lo_x = hi_x = (uint32_t)x;
        lo_y = hi_y = (uint32_t)y;
        if (parent[v] == v) T.leader[l] = v;
    }
    // The vertices of a long loop would all meet in its one row.  Consecutive ids mostly belong to one loop - an outline comes back to
    // a lattice row again and again - so where a wave's live lanes all do, it adds their terms up and lane 0 sends them once.
    const uint32_t l0 = (uint32_t)__shfl((int)l, 0, WAVE);
    const bool one = __ballot(live && l != l0) == 0;
    if (one) {
        for (int d = WAVE / 2; d > 0; d >>= 1) {
            cross += __shfl_down(cross, d, WAVE);
            length += __shfl_down(length, d, WAVE);
            count += (uint32_t)__shfl_down((int)count, d, WAVE);
            lo_x = min(lo_x, (uint32_t)__shfl_down((int)lo_x, d, WAVE));
            lo_y = min(lo_y, (uint32_t)__shfl_down((int)lo_y, d, WAVE));
            hi_x = max(hi_x, (uint32_t)__shfl_down((int)hi_x, d, WAVE));
            hi_y = max(hi_y, (uint32_t)__shfl_down((int)hi_y, d, WAVE));
        }
        if ((threadIdx.x & (WAVE - 1)) != 0) return;
    } else if (!live) {
        return;
    }
    atomicAdd(T.area2 + l, (unsigned long long)cross);
    atomicAdd(T.perimeter + l, length);
    atomicAdd(T.n_vertices + l, count);
    // the bounds move one way: a look at the current value - never better than the true one - says whether this one would change it
    uint32_t* const lo = T.lo + 2 * (size_t)l;
    uint32_t* const hi = T.hi + 2 * (size_t)l;
    if (lo_x < lo[0]) atomicMin(lo, lo_x);
    if (lo_y < lo[1]) atomicMin(lo + 1, lo_y);
    if (hi_x > hi[0]) atomicMax(hi, hi_x);
    if (hi_y > hi[1]) atomicMax(hi + 1, hi_y);
}
}  // namespace fhm
