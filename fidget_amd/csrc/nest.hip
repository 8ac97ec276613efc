// The nesting of a voxel bitmap's outlines (fhip_outlines_nesting, include/fidget_hip.h; the host side is capi_nest.hpp).  The arithmetic
// is mesh_nest.hpp's, which the tests also build for the host.  A lane per loop throughout; loops are three orders of magnitude fewer
// than vertices.
//   k_on_left       the loop's layer from loop_start, its leader's corner, then the row scan to the nearest edge on the left, the column
//                   walk to the corner where that edge's run begins and the lower bound search for the vertex there: left[l], which is
//                   also the first link of the doubling
//   k_on_resolve    one round of pointer doubling over the links of equal sign, from one buffer into the other; the host fixes the number
//                   of rounds from the largest layer's loop count, and the last round lands in the handle's parent array
//   k_on_depth0     (parent, has a parent) as the first (ancestor, hops)
//   k_on_depth      one round of the same doubling over (ancestor, hops); the last round's hops are the depths
//   k_on_sums       1 and area2[l] added to the parent's row, area2[l] to the loop's own; the layer's outer and top by atomicAdd, its
//                   max_depth by atomicMax.  Integer atomics alone: the sums do not depend on the order of arrival.
// No LDS, no kernel waits for another workgroup.  Included by mesh.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "mesh_nest.hpp"

namespace fhm {
struct OnLoops {
    const uint32_t *loop_start, *vertex_start;          // [K + 1] each
    const uint32_t* leader;                             // [n]
    const int64_t* area2;                               // [n]
    uint32_t n, K, k0;
};
__global__ void __launch_bounds__(256) k_on_left(const uint64_t* __restrict__ bricks, uint32_t depth, const uint32_t* __restrict__ xy, const uint32_t* __restrict__ loop_of,
                                                 OnLoops L, uint32_t* __restrict__ left, uint32_t* __restrict__ link) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.n) return;
    const uint32_t l = (uint32_t)i, layer = fhnest::layer_of(L.loop_start, L.K, l);
    const uint32_t e = fhnest::left_of(bricks, depth, L.k0 + layer, xy, loop_of, L.vertex_start[layer], L.vertex_start[layer + 1], L.loop_start[layer], l, L.leader[l]);
    left[l] = e;
    link[l] = e;
}
__global__ void __launch_bounds__(256) k_on_resolve(const uint32_t* __restrict__ link, const int64_t* __restrict__ area2, uint32_t n, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = fhnest::resolve_step(link, area2, (uint32_t)i);
}
__global__ void __launch_bounds__(256) k_on_depth0(const uint32_t* __restrict__ parent, uint32_t n, uint32_t* __restrict__ anc, uint32_t* __restrict__ hops) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = parent[i];
    anc[i] = p;
    hops[i] = p != fhnest::NONE;
}
__global__ void __launch_bounds__(256) k_on_depth(const uint32_t* __restrict__ anc, const uint32_t* __restrict__ hops, uint32_t n, uint32_t* __restrict__ anc_out,
                                                  uint32_t* __restrict__ hops_out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t a, h;
    fhnest::depth_step(anc, hops, (uint32_t)i, a, h);
    anc_out[i] = a;
    hops_out[i] = h;
}
struct OnSums {
    uint32_t* n_children;                          // [n], zero at the start, as everything here
    unsigned long long* region_area2;              // [n]: an int64 in two's complement
    unsigned long long *outer, *top;               // [K]
    uint32_t* max_depth;                           // [K]
};
__global__ void __launch_bounds__(256) k_on_sums(OnLoops L, const uint32_t* __restrict__ parent, const uint32_t* __restrict__ depth, OnSums S) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= L.n) return;
    const uint32_t l = (uint32_t)i, layer = fhnest::layer_of(L.loop_start, L.K, l), p = parent[l];
    const int64_t a = L.area2[l];
    atomicAdd(S.region_area2 + l, (unsigned long long)a);
    if (p < L.n) {          // (NONE is not)
        atomicAdd(S.n_children + p, 1u);
        atomicAdd(S.region_area2 + p, (unsigned long long)a);
    } else {
        atomicAdd(S.top + layer, 1ull);
    }
    if (a > 0) atomicAdd(S.outer + layer, 1ull);
    atomicMax(S.max_depth + layer, depth[l]);
}
}  // namespace fhm
