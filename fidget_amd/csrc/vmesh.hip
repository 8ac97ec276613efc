// The boundary mesh of a voxel bitmap (fhip_voxels_mesh, fhip_voxels_surface, include/fidget_hip.h; the host side is capi_vmesh.hpp):
// the exposed faces of the set voxels as two triangles each, over shared vertices at the used lattice corners.  The bit arithmetic is
// mesh_vmesh.hpp's, which the tests also build for the host.
//   k_vm_count      a thread per corner brick of the (B + 1)^3 grid, which below B per axis is also brick (cx, cy, cz): the eight words
//                   around it give the used-corner flag word and the used-edge count, three more neighbours the six exposed-face masks.
//                   The popcounts go to a per-brick face count, a per-corner-brick vertex count and per-block partial sums
//   k_vm_sum        the partials to the nine totals, in 64 bits
//   (two prefix sums over the counts, k_scan_block / k_scan_add of mesh.hip)
//   k_vm_vertices   a block per 256 corner bricks: their vertices dealt out over the threads, one V3 each, consecutive threads
//                   consecutive vertices
//   k_vm_faces      a block per 256 bricks: their faces dealt out likewise, so that the 48-byte records of consecutive faces are
//                   stored by consecutive lanes
// No kernel waits for another workgroup; every word written has one writer; no atomics.  Integers throughout but for the vertices'
// coordinates, which are exact.  Included by mesh.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "mesh_collapse.hpp"
#include "mesh_vmesh.hpp"

namespace fhm {
constexpr uint32_t FH_VM_COUNT_BLOCKS = 2048;          // blocks of k_vm_count at most (one row of partials each)
constexpr uint32_t FH_VM_SUMS = 9;                     // faces -x, +x, -y, +y, -z, +z; used corners; used edges; set voxels
constexpr uint32_t FH_VM_PER_BLOCK = 256;              // (corner) bricks a block of k_vm_vertices / k_vm_faces expands

// a brick's word, 0 beyond the grid: a coordinate of -1 has wrapped to above B
__device__ __forceinline__ uint64_t vm_word(const uint64_t* __restrict__ bricks, uint32_t depth, uint32_t bx, uint32_t by, uint32_t bz) {
    const uint32_t B = 1u << depth;
    return (bx < B && by < B && bz < B) ? bricks[fhvox::word_index(depth, bx, by, bz)] : 0;
}
__device__ __forceinline__ void vm_face_masks(const uint64_t* __restrict__ bricks, uint32_t depth, uint32_t bx, uint32_t by, uint32_t bz, uint64_t w, uint64_t m[6]) {
    const uint64_t nb[6] = {vm_word(bricks, depth, bx - 1, by, bz), vm_word(bricks, depth, bx + 1, by, bz), vm_word(bricks, depth, bx, by - 1, bz),
                            vm_word(bricks, depth, bx, by + 1, bz), vm_word(bricks, depth, bx, by, bz - 1), vm_word(bricks, depth, bx, by, bz + 1)};
    fhvm::face_masks(w, nb, m);
}

// face_count [B^3], corner_flags and vertex_count [(B + 1)^3]: null for the summary alone.  parts: [gridDim.x][FH_VM_SUMS].
__global__ void __launch_bounds__(256) k_vm_count(const uint64_t* __restrict__ bricks, uint32_t depth, uint32_t* __restrict__ face_count,
                                                  uint64_t* __restrict__ corner_flags, uint32_t* __restrict__ vertex_count, uint64_t* __restrict__ parts) {
    __shared__ uint32_t sh_sum[4][FH_VM_SUMS];
    const uint32_t B = 1u << depth, S = B + 1, n = S * S * S;          // (1025^3 < 2^31, and so is the last index plus a stride)
    uint32_t acc[FH_VM_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};            // (a thread sees at most 1025^3 / 2^19 + 1 bricks of 64 voxels)
    for (uint32_t t = blockIdx.x * 256 + threadIdx.x; t < n; t += gridDim.x * 256) {
        const uint32_t cx = t % S, cy = t / S % S, cz = t / (S * S);
        uint64_t W[8];
#pragma unroll
        for (uint32_t q = 0; q < 8; q++) W[q] = vm_word(bricks, depth, cx - (q & 1), cy - ((q >> 1) & 1), cz - (q >> 2));
        uint64_t used = 0;
        if (!fhvm::corners_none(W)) {
            uint64_t edges[3];
            fhvm::corner_masks(W, used, edges);
            acc[6] += fhvm::popcount64(used);
            acc[7] += fhvm::popcount64(edges[0]) + fhvm::popcount64(edges[1]) + fhvm::popcount64(edges[2]);
        }
        if (corner_flags) { corner_flags[t] = used; vertex_count[t] = fhvm::popcount64(used); }
        if (cx < B && cy < B && cz < B) {
            const uint64_t nb[6] = {W[1], vm_word(bricks, depth, cx + 1, cy, cz), W[2], vm_word(bricks, depth, cx, cy + 1, cz), W[4], vm_word(bricks, depth, cx, cy, cz + 1)};
            uint32_t faces = 0;
            if (!fhvm::faces_none(W[0], nb)) {
                uint64_t m[6];
                fhvm::face_masks(W[0], nb, m);
#pragma unroll
                for (uint32_t d = 0; d < 6; d++) { const uint32_t c = fhvm::popcount64(m[d]); acc[d] += c; faces += c; }
            }
            acc[8] += fhvm::popcount64(W[0]);
            if (face_count) face_count[fhvox::word_index(depth, cx, cy, cz)] = faces;
        }
    }
    // a block's sums stay below 2^32: 256 threads of at most 2^11 bricks of at most 64 (3 * 64 for the edges)
#pragma unroll
    for (uint32_t j = 0; j < FH_VM_SUMS; j++) {
        uint32_t v = acc[j];
        for (uint32_t d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
        if ((threadIdx.x & 63) == 0) sh_sum[threadIdx.x >> 6][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < FH_VM_SUMS)
        parts[(size_t)blockIdx.x * FH_VM_SUMS + threadIdx.x] = (uint64_t)sh_sum[0][threadIdx.x] + sh_sum[1][threadIdx.x] + sh_sum[2][threadIdx.x] + sh_sum[3][threadIdx.x];
}
// block j sums column j of the partials
__global__ void __launch_bounds__(256) k_vm_sum(const uint64_t* __restrict__ parts, uint32_t n_parts, uint64_t* __restrict__ out) {
    __shared__ uint64_t sh[256];
    uint64_t s = 0;
    for (uint32_t p = threadIdx.x; p < n_parts; p += 256) s += parts[(size_t)p * FH_VM_SUMS + blockIdx.x];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t d = 128; d > 0; d >>= 1) {
        if (threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// which of a block's 256 items holds element v: the largest b with off[b] <= v, off ascending with off[256] > v - an item without
// elements shares its offset with the next and is never the largest
__device__ __forceinline__ uint32_t vm_find(const uint32_t* off, uint32_t v) {
    uint32_t b = 0;
#pragma unroll
    for (uint32_t step = FH_VM_PER_BLOCK / 2; step > 0; step >>= 1)
        if (off[b + step] <= v) b += step;
    return b;
}

// base: the exclusive prefix sums of vertex_count, n + 1 of them.  Vertex base[t] + r is the r-th flagged corner of corner brick t.
__global__ void __launch_bounds__(256) k_vm_vertices(const uint64_t* __restrict__ corner_flags, const uint32_t* __restrict__ base, uint32_t depth,
                                                     fhmesh::V3* __restrict__ verts) {
    __shared__ uint32_t sh_off[FH_VM_PER_BLOCK + 1];
    __shared__ uint64_t sh_flags[FH_VM_PER_BLOCK];
    const uint32_t S = (1u << depth) + 1, n = S * S * S, N = 4u << depth, tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * FH_VM_PER_BLOCK, t_end = min(t0 + FH_VM_PER_BLOCK, n);
    const uint32_t first = base[t0], last = base[t_end];
    if (first == last) return;          // (the same in every thread)
    sh_off[tid] = base[min(t0 + tid, n)];
    sh_flags[tid] = t0 + tid < n ? corner_flags[t0 + tid] : 0;
    if (tid == 0) sh_off[FH_VM_PER_BLOCK] = last;
    __syncthreads();
    for (uint32_t e = tid; e < last - first; e += 256) {          // (at most 64 rounds; first + e cannot wrap)
        const uint32_t v = first + e;
        const uint32_t b = vm_find(sh_off, v), bit = fhvm::select_bit(sh_flags[b], v - sh_off[b]), t = t0 + b;
        const uint32_t cx = t % S, cy = t / S % S, cz = t / (S * S);
        verts[v] = fhmesh::V3{fhvm::corner_coord(4 * cx + (bit & 3), N), fhvm::corner_coord(4 * cy + ((bit >> 2) & 3), N), fhvm::corner_coord(4 * cz + (bit >> 4), N)};
    }
}

// face_base: the exclusive prefix sums of face_count, B^3 + 1 of them.  Face face_base[w] + r is the r-th exposed face of brick w, its
// faces ordered by direction, then by bit; it writes triangles 2 f and 2 f + 1, six vertex ids.
__global__ void __launch_bounds__(256) k_vm_faces(const uint64_t* __restrict__ bricks, uint32_t depth, const uint32_t* __restrict__ face_base,
                                                  const uint64_t* __restrict__ corner_flags, const uint32_t* __restrict__ vertex_base, uint64_t* __restrict__ tris) {
    __shared__ uint32_t sh_off[FH_VM_PER_BLOCK + 1];
    __shared__ uint64_t sh_mask[6][FH_VM_PER_BLOCK];
    const uint32_t B = 1u << depth, tid = threadIdx.x;
    const uint64_t n_words = (uint64_t)1 << (3 * depth);
    const uint64_t w0 = (uint64_t)blockIdx.x * FH_VM_PER_BLOCK, w_end = min(w0 + FH_VM_PER_BLOCK, n_words), w = w0 + tid;
    const uint32_t first = face_base[w0], last = face_base[w_end];
    if (first == last) return;          // (the same in every thread)
    const uint32_t mine = face_base[min(w, n_words)];
    sh_off[tid] = mine;
    if (tid == 0) sh_off[FH_VM_PER_BLOCK] = last;
    if (w < n_words && face_base[w + 1] != mine) {
        const uint32_t bx = (uint32_t)w & (B - 1), by = (uint32_t)(w >> depth) & (B - 1), bz = (uint32_t)(w >> (2 * depth));
        uint64_t m[6];
        vm_face_masks(bricks, depth, bx, by, bz, bricks[w], m);
#pragma unroll
        for (uint32_t d = 0; d < 6; d++) sh_mask[d][tid] = m[d];
    }
    __syncthreads();
    for (uint32_t e = tid; e < last - first; e += 256) {          // (at most 384 rounds)
        const uint32_t f = first + e;
        const uint32_t b = vm_find(sh_off, f);
        uint32_t r = f - sh_off[b], d = 0;
        uint64_t m = sh_mask[0][b];
        for (uint32_t c = fhvm::popcount64(m); r >= c; c = fhvm::popcount64(m)) { r -= c; m = sh_mask[++d][b]; }          // (r is below the six counts' sum: d stays below 6)
        const uint32_t bit = fhvm::select_bit(m, r);
        const uint64_t wb = w0 + b;
        const uint32_t bx = (uint32_t)wb & (B - 1), by = (uint32_t)(wb >> depth) & (B - 1), bz = (uint32_t)(wb >> (2 * depth));
        uint32_t c[4][3];
        fhvm::face_corners(4 * bx + (bit & 3), 4 * by + ((bit >> 2) & 3), 4 * bz + (bit >> 4), d, c);
        uint64_t id[4];
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            const uint32_t t = fhvm::corner_brick(depth, c[q][0], c[q][1], c[q][2]);
            id[q] = (uint64_t)vertex_base[t] + fhvm::rank_below(corner_flags[t], fhvm::corner_bit(c[q][0], c[q][1], c[q][2]));
        }
        ulonglong2* const out = (ulonglong2*)(tris + (size_t)f * 6);          // (48-byte records from a hipMalloc: 16-byte aligned)
        out[0] = make_ulonglong2(id[0], id[1]);
        out[1] = make_ulonglong2(id[2], id[0]);
        out[2] = make_ulonglong2(id[2], id[3]);
    }
}
}  // namespace fhm
