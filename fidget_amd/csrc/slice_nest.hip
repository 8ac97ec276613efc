// The nesting of a mesh's slices (fhip_slices_nesting, include/fidget_hip.h; the host side is capi_slice_nest.hpp): per regular loop the
// loops of its plane that contain it, by a ray cast from its leader towards -x against the float32 polygons.  The arithmetic is
// mesh_slice_nest.hpp's, which the tests also build for the host.  Nothing lies under these loops - no bitmap whose rows nest.hip could
// scan - so the segments of every plane are indexed by bands of y, as CSR over all planes' bands.
//   k_sn_count     a lane per crossing v of a regular loop, the segment v -> next[v]: one more in each band from that of its lower to that
//                  of its upper end (an integer add per band); the 64-bit total of the entries
//                  (the prefix sums over the bands: k_scan_block / k_scan_add of mesh.hip)
//   k_sn_fill      the same lanes: the segment - its ends' four floats and its loop - into each of those bands, at a cursor that starts at
//                  the band's first entry: 20 bytes an entry, which the leaders' waves then read in order, gathering nothing.  The order
//                  within a band is one of arrival; no result depends on it - parity and counts are free of order
//   k_sn_hits      a WAVE per loop, twice.  Its lanes stride over the entries of the band of the leader's y and apply fhsn::hit; entries of
//                  the leader's own loop are passed over.  First the number of hits, their 64-bit total and the number of lists too long
//                  for LDS; after the prefix sums over the loops the hit loops' ids at places from ballot and popcount, no atomics: a
//                  list of at most FH_SN_LDS_HITS into the wave's part of LDS, where the same wave reduces it at once - the ids of odd
//                  multiplicity (fhsn::odd_first: for each entry a pass over the list) into the loop's part of `contain`, depth = their
//                  number - and a longer one into the loop's part of `hits`
//   k_sn_contain   launched where a list was longer: a wave per loop, the same reduction from `hits` in global memory - any length, no
//                  buffer of its own, quadratic in that one list.  (Measured on the fine mesh, 86 hits a leader: writing every list out
//                  cost 26 ms and reducing it from global memory 35 ms; the writing pass with the reduction in LDS takes 32 ms, and
//                  this kernel 2 ms for the lists beyond 512: profiles/slice_nesting/README.md)
//   k_sn_parent    a lane per loop, after every depth is known: the deepest of its containing loops, n_children and the planes' counts by
//                  integer adds and one integer max
// Irregular loops get NONE twice and are in no band.  Everything is an integer that does not depend on the order of arrival.  No kernel
// waits for another workgroup and nothing spins; every loop here runs over a range that is clamped to the arrays' sizes first, so a
// handle whose arrays are garbage yields garbage and no access outside them.  Included by mesh.hip, after slice.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "mesh_slice_nest.hpp"

namespace fhm {
constexpr uint32_t FH_SN_ENTRIES = 0, FH_SN_HITS = 1, FH_SN_LONG = 2;          // the counters of a call, in the rows of topo.hip's
// a plane's counts on the device, uint32 each
constexpr uint32_t FH_SN_REGULAR = 0, FH_SN_OUTER = 1, FH_SN_TOP = 2, FH_SN_MAX_DEPTH = 3, FH_SN_IMPROPER = 4, FH_SN_MISORIENTED = 5, FH_SN_PLANE_WORDS = 6;

struct SnIn {          // the arrays of a fhip_slices and what the host sends up of its loops' table
    const float2* xy;
    const uint32_t *plane, *next, *loop_of;
    uint32_t n;          // crossings
    const uint32_t *leader, *loop_plane, *flags;
    uint32_t L;          // loops
    const fhsn::Band* bands;
    uint32_t P, n_bands;
};
// crossing v: does a regular segment leave it -> its plane's bands and its range among them
__device__ __forceinline__ bool sn_segment(const SnIn& I, uint64_t v, fhsn::Band& B, fhsn::BandRange& r) {
    if (v >= I.n) return false;
    const uint32_t l = I.loop_of[v], p = I.plane[v], w = I.next[v];
    if (l >= I.L || p >= I.P || w >= I.n || (I.flags[l] & fhsn::IRREGULAR)) return false;
    B = I.bands[p];
    r = fhsn::segment_bands(I.xy[v].y, I.xy[w].y, B);
    return r.hi < B.nb && (uint64_t)B.base + B.nb <= I.n_bands;
}
__global__ void __launch_bounds__(256) k_sn_count(SnIn I, uint32_t* __restrict__ band_count, uint64_t* __restrict__ counters) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    fhsn::Band B;
    fhsn::BandRange r;
    uint64_t mine = 0;
    if (sn_segment(I, v, B, r)) {
        for (uint32_t b = r.lo; b <= r.hi; b++) atomicAdd(band_count + B.base + b, 1u);
        mine = (uint64_t)(r.hi - r.lo) + 1;
    }
    ms_count(counters, FH_SN_ENTRIES, mine);
}
// cursor: the bands' first entries before, their ends after.  An entry is the segment itself - its ends' four floats and its loop - so
// that the leaders' waves read consecutive records and gather nothing
__global__ void __launch_bounds__(256) k_sn_fill(SnIn I, uint32_t* __restrict__ cursor, uint32_t n_entries, float4* __restrict__ entry_ends,
                                                 uint32_t* __restrict__ entry_loop) {
    const uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    fhsn::Band B;
    fhsn::BandRange r;
    if (!sn_segment(I, v, B, r)) return;
    const float2 s = I.xy[v], d = I.xy[I.next[v]];
    const float4 ends = make_float4(s.x, s.y, d.x, d.y);
    const uint32_t m = I.loop_of[v];
    for (uint32_t b = r.lo; b <= r.hi; b++) {
        const uint32_t at = atomicAdd(cursor + B.base + b, 1u);
        if (at < n_entries) { entry_ends[at] = ends; entry_loop[at] = m; }
    }
}
// A leader's hits, twice.  !WRITE: hit_count[l], the 64-bit total, and the number of leaders with more than FH_SN_LDS_HITS hits.  WRITE,
// with hit_base - the exclusive prefix sums of the counts: a list of at most FH_SN_LDS_HITS hits stays in the wave's part of LDS, its
// ids of odd multiplicity go to contain[hit_base[l] ..] and their number to depth[l]; a longer one goes to hits[hit_base[l] ..
// hit_base[l + 1]) for k_sn_contain.  A wave's part of LDS is its own: written and read by the same wave, in program order - no barrier
// of the workgroup, whose waves do not all get here
constexpr uint32_t FH_SN_LDS_HITS = 512;
template <bool WRITE>
__global__ void __launch_bounds__(256) k_sn_hits(SnIn I, const uint32_t* __restrict__ band_start, const float4* __restrict__ entry_ends,
                                                 const uint32_t* __restrict__ entry_loop, uint32_t n_entries, uint32_t* __restrict__ hit_count,
                                                 const uint32_t* __restrict__ hit_base, uint32_t n_hits, uint32_t* __restrict__ hits, uint32_t* __restrict__ contain,
                                                 uint32_t* __restrict__ depth, uint64_t* __restrict__ counters) {
    __shared__ uint32_t lists[WRITE ? 4 : 1][WRITE ? FH_SN_LDS_HITS : 1];
    const uint64_t l = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);          // (the same for the whole wave)
    const uint32_t lane = threadIdx.x & 63;
    if (l >= I.L) return;
    uint32_t* const mine = lists[WRITE ? threadIdx.x >> 6 : 0];
    uint32_t found = 0, at = 0, room = 0;
    const uint32_t v0 = I.leader[l], p = I.loop_plane[l];
    const bool regular = !(I.flags[l] & fhsn::IRREGULAR);
    if (WRITE) {
        at = hit_base[l] < n_hits ? hit_base[l] : n_hits;
        const uint32_t stop = hit_base[l + 1] < n_hits ? hit_base[l + 1] : n_hits;
        room = stop > at ? stop - at : 0;
    }
    const bool in_lds = room <= FH_SN_LDS_HITS;
    if (regular && v0 < I.n && p < I.P) {
        const fhsn::Band B = I.bands[p];
        const float2 qq = I.xy[v0];
        const float q[2] = {qq.x, qq.y};
        const uint64_t b = (uint64_t)B.base + fhsn::band(q[1], B);
        if (b < I.n_bands) {
            uint32_t first = band_start[b], end = band_start[b + 1];
            if (end > n_entries) end = n_entries;
            if (first > end) first = end;
            for (uint32_t e0 = first; e0 < end; e0 += 64) {          // (e0 is the wave's: every lane takes every turn)
                bool is_hit = false;
                uint32_t m = 0;
                if (e0 + lane < end && e0 + lane >= e0) {
                    m = entry_loop[e0 + lane];
                    if (m != (uint32_t)l) {
                        const float4 ends = entry_ends[e0 + lane];
                        const float s[2] = {ends.x, ends.y}, d[2] = {ends.z, ends.w};
                        is_hit = fhsn::hit(s, d, q);
                    }
                }
                const uint64_t mask = __ballot(is_hit);
                if (WRITE && is_hit) {
                    const uint32_t k = found + (uint32_t)__popcll(mask & (((uint64_t)1 << lane) - 1));
                    if (k < room) { if (in_lds) mine[k] = m; else hits[at + k] = m; }
                }
                found += (uint32_t)__popcll(mask);
                if (e0 + 64 < e0) break;          // (the end of uint32)
            }
        }
    }
    if (!WRITE) {
        if (lane == 0) {
            hit_count[l] = found;
            uint64_t* const row = counters + (l & (FH_MT_ROWS - 1)) * FH_MT_COUNTERS;
            if (found) atomicAdd((unsigned long long*)row + FH_SN_HITS, (unsigned long long)found);
            if (found > FH_SN_LDS_HITS) atomicAdd((unsigned long long*)row + FH_SN_LONG, 1ull);
        }
        return;
    }
    if (!regular) { if (lane == 0) depth[l] = fhsn::NONE; return; }
    if (!in_lds) return;          // (k_sn_contain's)
    const uint32_t h = found < room ? found : room;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    uint32_t kept = 0;
    for (uint32_t i0 = 0; i0 < h; i0 += 64) {
        const bool keep = i0 + lane < h && fhsn::odd_first(mine, h, i0 + lane);
        const uint64_t mask = __ballot(keep);
        if (keep) contain[at + kept + (uint32_t)__popcll(mask & (((uint64_t)1 << lane) - 1))] = mine[i0 + lane];
        kept += (uint32_t)__popcll(mask);
    }
    if (lane == 0) depth[l] = kept;
}
// the lists that were too long for LDS: hits -> contain, in each loop's own part; depth
__global__ void __launch_bounds__(256) k_sn_contain(const uint32_t* __restrict__ flags, uint32_t L, const uint32_t* __restrict__ hit_base, uint32_t n_hits,
                                                    const uint32_t* __restrict__ hits, uint32_t* __restrict__ contain, uint32_t* __restrict__ depth) {
    const uint64_t l = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (l >= L || (flags[l] & fhsn::IRREGULAR)) return;
    const uint32_t at = hit_base[l] < n_hits ? hit_base[l] : n_hits, stop = hit_base[l + 1] < n_hits ? hit_base[l + 1] : n_hits;
    const uint32_t h = stop > at ? stop - at : 0;
    if (h <= FH_SN_LDS_HITS) return;
    uint32_t kept = 0;
    for (uint32_t i0 = 0; i0 < h; i0 += 64) {
        const bool keep = i0 + lane < h && i0 + lane >= i0 && fhsn::odd_first(hits + at, h, i0 + lane);
        const uint64_t mask = __ballot(keep);
        if (keep) contain[at + kept + (uint32_t)__popcll(mask & (((uint64_t)1 << lane) - 1))] = hits[at + i0 + lane];
        kept += (uint32_t)__popcll(mask);
        if (i0 + 64 < i0) break;
    }
    if (lane == 0) depth[l] = kept;
}
// n_children and plane_counts (FH_SN_PLANE_WORDS words per plane): zeros before
__global__ void __launch_bounds__(256) k_sn_parent(SnIn I, const uint32_t* __restrict__ hit_base, uint32_t n_hits, const uint32_t* __restrict__ contain,
                                                   const uint32_t* __restrict__ depth, uint32_t* __restrict__ parent, uint32_t* __restrict__ n_children,
                                                   uint32_t* __restrict__ plane_counts) {
    const uint64_t l = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= I.L) return;
    const uint32_t flags = I.flags[l], d = depth[l], p = I.loop_plane[l];
    if ((flags & fhsn::IRREGULAR) || d == fhsn::NONE || p >= I.P) { parent[l] = fhsn::NONE; return; }
    const uint32_t at = hit_base[l] < n_hits ? hit_base[l] : n_hits;
    const uint32_t n = d < n_hits - at ? d : n_hits - at;
    const uint32_t up = fhsn::parent_of(contain + at, n, depth, I.L);
    parent[l] = up;
    if (up != fhsn::NONE) atomicAdd(n_children + up, 1u);
    uint32_t* const row = plane_counts + (size_t)FH_SN_PLANE_WORDS * p;
    atomicAdd(row + FH_SN_REGULAR, 1u);
    if ((d & 1u) == 0) atomicAdd(row + FH_SN_OUTER, 1u);
    if (up == fhsn::NONE) atomicAdd(row + FH_SN_TOP, 1u);
    if (d) (void)atomicMax(row + FH_SN_MAX_DEPTH, d);
    if (fhsn::improper(d, up, depth)) atomicAdd(row + FH_SN_IMPROPER, 1u);
    if (fhsn::misoriented(d, flags)) atomicAdd(row + FH_SN_MISORIENTED, 1u);
}
}  // namespace fhm
