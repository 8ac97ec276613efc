// fidget-hip: the evaluation side of fidget-mesh's octree construction on the device (fidget-mesh/src/octree.rs).
//
//   k_mesh_cells  one lane per octree cell of a level: cell bounds (cell.rs:184-194 midpoint splitting), interval
//                 evaluation of the shape's tape (octree.rs:521-544), classification Full / Empty / ambiguous; the ambiguous
//                 cells are appended to the next level's list (or, at the last level, to the leaf list);
//   k_mesh_corners / k_mesh_edges / k_mesh_grads   the ambiguous leaf cells sampled (octree.rs:590-862) in passes over a chunk of them,
//                 every lane a point of its own: the 8 corners (bulk f32) -> corner mask -> edges of the Manifold Dual Contouring
//                 table -> 4 rounds of 16-point search per edge (one wave per four edges) -> intersections (u16 cell
//                 coordinates) -> gradients there (one lane per edge);
//   k_mesh_leaf   the same with one wavefront per leaf cell (FHIP_MESH_LEAF_PASSES=0; what the passes are checked against);
//   k_mesh_leaf_qef  one lane per leaf record: one QEF per cell vertex (qef.rs).
//
// Tapes of 256 ops and more are simplified once down the octree (FhMeshParams::sub_tab: at the split level every ambiguous cell gets the root
// tape simplified under its own choices, and everything below it is evaluated with that - values do not depend on which ancestor's tape
// evaluates a cell); small tapes are evaluated as they are, the leaf samples through the assembly bulk interpreter.
//
//   k_oct_kind / k_oct_collapse / k_oct_place / k_oct_leaf_verts   the octree assembled from those results without leaving HBM
//                 (octree.rs:256-470 check_done / collapsible, 866-1035 merged Hermite data; mesh_collapse.hpp): level by level
//                 bottom-up what every ambiguous cell becomes, top-down where its vertices and its block of eight cells go.
//   k_walk_* / k_scan_*   Octree::walk_dual (dc.rs, builder.rs) on that octree: the recursion's calls as level arrays in call order, the
//                 mesh's vertices numbered by first use through atomic minima and prefix sums (mesh_walk.hpp).
//   k_mesh_stl    Mesh::write_stl (fidget-mesh/src/output.rs:14-36): the binary STL file of a mesh, 256 triangles per block, the records
//                 put together in LDS and stored as whole dwords;
//   k_vox_full / k_vox_leaves / k_vox_slices / k_vox_layer_counts   the inside voxels themselves (fhip_shape_voxels): the octree of occupancy
//                 written down as a bitmap of 4 x 4 x 4 bricks, and what is made of the bitmap - layer images, voxels per layer;
//   k_cc_*        the connected parts of such a bitmap (fhip_voxels_components): flood fill inside each brick's word, a lock-free union-find
//                 over the brick faces (edges, corners), the components numbered by their seeds, their table, label images (mesh_cc.hpp);
//   k_ctr_edges / k_ctr_vertices / k_ctr_cells / k_ctr_segments   the outlines of a 2D slice (fhip_contour2d): marching squares over the
//                 pixel-perfect distance image render2d leaves in device memory - vertices on the crossing lattice edges, directed segments,
//                 the link array (contour/contour.hpp);
//   k_mesh_vertex_grads   the tape's value and gradient at every vertex of a mesh (VmGradSliceEval::eval, vm/mod.rs:1091-1397): one
//                 vertex per lane, read from the V3 array where the dual walk left it.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_ops.hpp"
#include "mesh_collapse.hpp"
#include "mesh_walk.hpp"
#include "mesh_edges.hpp"
#include "mesh_qef.hpp"
#include "mesh_vox.hpp"
#include "mesh_cc.hpp"
#include "contour/contour.hpp"
// (included by capi.hip after kernels.hip: Regs, step, ballot, uni, ctape_t)

struct FhMeshParams {
    const uint64_t* tape;
    uint32_t len, n_regs;
    float mat[16];
    uint32_t has_mat;
    uint32_t in_kind[FH_MAX_INPUTS];
    float in_value[FH_MAX_INPUTS];
    // Tape simplification down the octree (octree.rs:546-553, RenderHints::simplify_tree_during_meshing): once, at `split_level` - every
    // ambiguous cell there has a simplified tape of its own (VmData::simplify of the root tape under the cell's choices), which all the
    // cells and leaf samples below it use.  sub_tab[path of the ancestor at split_level - 8^split_level] = {offset into sub_ops, ops};
    // ops == 0 / sub_tab == null: the root tape.  (Values do not depend on which of an ancestor's tapes evaluates a cell: a min / max
    // decided over the ancestor's region is decided the same way everywhere inside it.)
    const uint64_t* sub_ops;
    const uint2* sub_tab;
    uint32_t split_level, pad_;
    // ... and a second time, further down (round 5: split_level2 = depth - 2, at most 7): the cells of that level get their ancestor's tape
    // simplified once more under their own choices - a 4^3-times smaller region, tapes a few times shorter again - for the levels and the leaf
    // samples below.  Same layout; an entry without a tape of its own (ops == 0) falls back to the first table.
    const uint64_t* sub_ops2;
    const uint2* sub_tab2;
    uint32_t split_level2, pad2_;
};
// shape occupancy (k_occ_full, k_occ_leaves): one block's partial sums
struct FhOccPart {
    uint64_t n, s1[3], s2[6];       // inside voxels; sum i, j, k; sum i^2, j^2, k^2, ij, ik, jk
    uint32_t lo[3], hi[3];          // inclusive bounds of the inside voxels per axis (n == 0: lo = 0xFFFFFFFF, hi = 0)
};
constexpr uint32_t FH_OCC_FULL_BLOCKS = 256, FH_OCC_LEAF_BLOCKS = 4096;      // the grids' upper bounds: blocks stride over their cells

namespace fhm {
using namespace fhd;

using fhmesh::lerp_pos;

// the tape of the cell with this path (3 bits per level below a leading 1)
__device__ __forceinline__ void mesh_tape(const FhMeshParams& P, uint64_t path, const uint64_t*& ops, uint32_t& len) {
    ops = P.tape; len = P.len;
    if (!P.sub_tab) return;
    if (P.sub_tab2) {
        const int up2 = (63 - __clzll((long long)path)) - 3 * (int)P.split_level2;
        if (up2 > 0) {
            const uint2 e2 = P.sub_tab2[(uint32_t)((path >> up2) - (1ull << (3 * P.split_level2)))];
            if (e2.y) { ops = P.sub_ops2 + e2.x; len = e2.y; return; }
        }
    }
    const int up = (63 - __clzll((long long)path)) - 3 * (int)P.split_level;
    if (up <= 0) return;          // (at the split level itself a cell is still evaluated with the tape it inherited)
    const uint2 e = P.sub_tab[(uint32_t)((path >> up) - (1ull << (3 * P.split_level)))];
    if (e.y) { ops = P.sub_ops + e.x; len = e.y; }
}

// interval evaluation + classification of the cells of one level.  expand: cell i is child (i & 7) of in[i >> 3]
__global__ void __launch_bounds__(WAVE) k_mesh_cells(FhMeshParams P, const FhMeshCell* in, uint32_t n, int expand, FhMeshCell* out, uint32_t* counters /* amb, full, empty */,
                                                      uint32_t out_cap, uint8_t* cls /* per cell: 1 empty 2 full 3 ambiguous, 0 another part's */, uint32_t* slot /* of an ambiguous cell in out */,
                                                      uint32_t child_mask /* expand: the corners evaluated here (0xFF but below the root of a sharded build) */) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x * WAVE + lane;
    const bool act = i < n && (!expand || ((child_mask >> (i & 7)) & 1u));
    FhMeshCell c;
    {
        const FhMeshCell p = in[expand ? min(i, n - 1) >> 3 : min(i, n - 1)];
        c = p;
        if (expand) {
            const int corner = i & 7;
            for (int k = 0; k < 3; k++) {
                const float mid = (p.b[2 * k] + p.b[2 * k + 1]) / 2.0f;
                if (corner & (1 << k)) { c.b[2 * k] = mid; c.b[2 * k + 1] = p.b[2 * k + 1]; } else { c.b[2 * k] = p.b[2 * k]; c.b[2 * k + 1] = mid; }
            }
            c.path = (p.path << 3) | (uint64_t)corner;
        }
    }
    IV X = iv(c.b[0], c.b[1]), Y = iv(c.b[2], c.b[3]), Z = iv(c.b[4], c.b[5]);
    if (P.has_mat) {
        Mat4 m;
#pragma unroll
        for (int k = 0; k < 16; k++) m.m[k] = P.mat[k];
        xf_interval(m, X, Y, Z, X, Y, Z);
    }
    Regs<IV, WAVE> R{(IV*)smem, lane};
    IV result = iv_nan();
    auto in_iv = [&](uint32_t slot) { const uint32_t kd = P.in_kind[slot]; return kd == 0 ? X : (kd == 1 ? Y : (kd == 2 ? Z : iv1(P.in_value[slot]))); };
    if (P.sub_tab) {       // every lane its cell's tape (a wave's cells mostly share an ancestor: their parents were neighbours)
        const uint64_t* ops; uint32_t len;
        mesh_tape(P, c.path, ops, len);
        for (uint32_t k = 0; k < len; k++) step<IVAL, WAVE, true>(ops[k], R, in_iv, [&](uint32_t, IV v) { result = v; }, [&](int) {});
    } else {
        const ctape_t tape = (ctape_t)P.tape;
        for (uint32_t k = 0; k < P.len; k++) step<IVAL, WAVE, true>(tape[k], R, in_iv, [&](uint32_t, IV v) { result = v; }, [&](int) {});
    }
    const bool full = act && result.hi < 0.0f, empty = act && !full && result.lo > 0.0f, amb = act && !full && !empty;
    const uint64_t am = ballot(amb);
    const uint32_t nf = (uint32_t)__popcll(ballot(full)), ne = (uint32_t)__popcll(ballot(empty));    // (every lane votes: outside the branch)
    uint32_t base = 0;
    if (lane == 0) {
        if (am) base = atomicAdd(&counters[0], (uint32_t)__popcll(am));
        if (nf) atomicAdd(&counters[1], nf);
        if (ne) atomicAdd(&counters[2], ne);
    }
    base = uni(base);
    uint32_t sl = 0xFFFFFFFFu;
    if (amb) {
        sl = base + (uint32_t)__popcll(am & ((1ull << lane) - 1));
        if (sl < out_cap) out[sl] = c;
    }
    if (i < n && cls) { cls[i] = !act ? 0 : (full ? 2 : (empty ? 1 : 3)); slot[i] = sl; }
}

// The choices of the root tape over each of n cells (the ambiguous cells of the split level): choices[cell * n_choices + ordinal] = what the
// interval evaluation decided at that min / max / and / or (vm/mod.rs:436-517), for VmData::simplify on the host (capi_mesh.hpp)
__global__ void __launch_bounds__(WAVE) k_mesh_choices(FhMeshParams P, const FhMeshCell* cells, uint32_t n, uint32_t n_choices, uint8_t* choices) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const uint32_t i = blockIdx.x * WAVE + lane;
    const FhMeshCell c = cells[min(i, n - 1)];
    IV X = iv(c.b[0], c.b[1]), Y = iv(c.b[2], c.b[3]), Z = iv(c.b[4], c.b[5]);
    if (P.has_mat) {
        Mat4 m;
#pragma unroll
        for (int k = 0; k < 16; k++) m.m[k] = P.mat[k];
        xf_interval(m, X, Y, Z, X, Y, Z);
    }
    Regs<IV, WAVE> R{(IV*)smem, lane};
    uint8_t* const mine = choices + (size_t)min(i, n - 1) * n_choices;
    uint32_t ci = 0;
    auto in_iv = [&](uint32_t slot) { const uint32_t kd = P.in_kind[slot]; return kd == 0 ? X : (kd == 1 ? Y : (kd == 2 ? Z : iv1(P.in_value[slot]))); };
    if (P.sub_tab) {       // (the second split: every lane the choices of the tape its cell inherited - the first split's; n_choices = the row length)
        const uint64_t* ops; uint32_t len;
        mesh_tape(P, c.path, ops, len);
        for (uint32_t k = 0; k < len; k++)
            step<IVAL, WAVE, true>(ops[k], R, in_iv, [&](uint32_t, IV) {}, [&](int ch) { if (i < n && ci < n_choices) mine[ci] = (uint8_t)ch; ci++; });
        return;
    }
    const ctape_t tape = (ctape_t)P.tape;
    for (uint32_t k = 0; k < P.len; k++) {
        step<IVAL, WAVE, true>(tape[k], R, in_iv, [&](uint32_t, IV) {}, [&](int ch) { if (i < n) mine[ci] = (uint8_t)ch; ci++; });
    }
}

// f32 value of the tape at this lane's point (lanes evaluate different points of the same leaf)
// (path: the leaf cell's, which says whose simplified tape to take when the octree was split, FhMeshParams)
__device__ __forceinline__ float eval_point(const FhMeshParams& P, const Regs<float, WAVE>& R, float x, float y, float z, uint64_t path) {
    if (P.has_mat) {
        Mat4 m;
#pragma unroll
        for (int k = 0; k < 16; k++) m.m[k] = P.mat[k];
        xf_point(m, x, y, z, x, y, z);
    }
    float result = qnan();
    auto in_f = [&](uint32_t slot) { const uint32_t kd = P.in_kind[slot]; return kd == 0 ? x : (kd == 1 ? y : (kd == 2 ? z : P.in_value[slot])); };
    if (P.sub_tab) {
        const uint64_t* ops; uint32_t len;
        mesh_tape(P, path, ops, len);
        for (uint32_t k = 0; k < len; k++) step<F32, WAVE, true>(ops[k], R, in_f, [&](uint32_t, float v) { result = v; }, [&](int) {});
    } else {
        const ctape_t tape = (ctape_t)P.tape;
        for (uint32_t k = 0; k < P.len; k++) step<F32, WAVE, true>(tape[k], R, in_f, [&](uint32_t, float v) { result = v; }, [&](int) {});
    }
    return result;
}
// ... and its gradient there
template <class GX>
__device__ __forceinline__ GR eval_grad(const FhMeshParams& P, const Regs<GR, WAVE>& G, const GX& gx, const GX& gy, const GX& gz, uint64_t path) {
    GR result = gr1(qnan());
    auto in_g = [&](uint32_t slot) { const uint32_t kd = P.in_kind[slot]; return kd == 0 ? gx : (kd == 1 ? gy : (kd == 2 ? gz : gr1(P.in_value[slot]))); };
    if (P.sub_tab) {
        const uint64_t* ops; uint32_t len;
        mesh_tape(P, path, ops, len);
        for (uint32_t k = 0; k < len; k++) step<GRAD, WAVE, true>(ops[k], G, in_g, [&](uint32_t, GR v) { result = v; }, [&](int) {});
    } else {
        const ctape_t tape = (ctape_t)P.tape;
        for (uint32_t k = 0; k < P.len; k++) step<GRAD, WAVE, true>(tape[k], G, in_g, [&](uint32_t, GR v) { result = v; }, [&](int) {});
    }
    return result;
}

__global__ void __launch_bounds__(WAVE) k_mesh_leaf(FhMeshParams P, const FhMeshCell* cells, uint32_t n, const FhMdcTable* T, FhMeshLeaf* out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ uint16_t s_start[12][3], s_end[12][3];
    const int lane = threadIdx.x;
    const uint32_t li = blockIdx.x;
    if (li >= n) return;
    const FhMeshCell c = cells[li];
    Regs<float, WAVE> R{(float*)smem, lane};
    // corners (cell.rs:196-206): bit 0 x, 1 y, 2 z
    const int cr = lane & 7;
    const float v = eval_point(P, R, (cr & 1) ? c.b[1] : c.b[0], (cr & 2) ? c.b[3] : c.b[2], (cr & 4) ? c.b[5] : c.b[4], c.path);
    const uint32_t mask = (uint32_t)(ballot(v < 0.0f) & 0xFFull);
    FhMeshLeaf* o = &out[li];
    if (lane < 6) o->b[lane] = c.b[lane];
    if (lane == 0) { o->path = c.path; o->mask = mask; o->n_edges = 0; o->n_verts = 0; o->pad = 0; }
    if (mask == 0 || mask == 255) return;      // Cell::Empty / Cell::Full (octree.rs:633-637)
    const uint32_t ne = T->n_edges[mask], nv = T->n_verts[mask];
    if (lane < (int)ne) {
        const int st = T->edge[mask][lane][0], en = T->edge[mask][lane][1];
        const int axis = st ^ en, ai = axis == 1 ? 0 : (axis == 2 ? 1 : 2);
        const uint16_t a = (en & axis) ? 0 : 65535, b = (en & axis) ? 65535 : 0;
        uint16_t p[3] = {0, 0, 0};
        const int i = (ai + 1) % 3, j = (ai + 2) % 3;
        p[i] = (st & (1 << i)) ? 65535 : 0;
        p[j] = (st & (1 << j)) ? 65535 : 0;
        for (int k = 0; k < 3; k++) { s_start[lane][k] = p[k]; s_end[lane][k] = p[k]; }
        s_start[lane][ai] = a; s_end[lane][ai] = b;
    }
    __syncthreads();
    // N-ary search: 4 rounds of 16 points per edge, 4 edges per pass (octree.rs:697-768)
    for (int round = 0; round < 4; round++) {
        for (uint32_t e0 = 0; e0 < ne; e0 += 4) {
            const uint32_t e = e0 + (lane >> 4), j = lane & 15;
            const bool valid = e < ne;
            const uint32_t ee = valid ? e : 0;
            uint32_t p[3];
            for (int k = 0; k < 3; k++) p[k] = ((uint32_t)s_start[ee][k] * (15u - j) + (uint32_t)s_end[ee][k] * j) / 15u;
            const float r = eval_point(P, R, lerp_pos(c.b[0], c.b[1], p[0]), lerp_pos(c.b[2], c.b[3], p[1]), lerp_pos(c.b[4], c.b[5], p[2]), c.path);
            const uint64_t nonneg = ballot(r >= 0.0f);
            const uint32_t m16 = (uint32_t)(nonneg >> ((lane >> 4) * 16)) & 0xFFFFu;
            uint32_t frac = m16 ? (uint32_t)__builtin_ctz(m16) : 16u;
            if (frac == 0) frac = 1;
            if (frac > 15) frac = 15;
            __syncthreads();
            if (valid && j == 0) {
                uint16_t a[3], b[3];
                for (int k = 0; k < 3; k++) {
                    a[k] = (uint16_t)(((uint32_t)s_start[e][k] * (15u - (frac - 1)) + (uint32_t)s_end[e][k] * (frac - 1)) / 15u);
                    b[k] = (uint16_t)(((uint32_t)s_start[e][k] * (15u - frac) + (uint32_t)s_end[e][k] * frac) / 15u);
                }
                for (int k = 0; k < 3; k++) { s_start[e][k] = a[k]; s_end[e][k] = b[k]; }
            }
            __syncthreads();
        }
    }
    // intersections, gradients (octree.rs:771-803)
    {
        const uint32_t e = lane < (int)ne ? lane : 0;
        uint16_t q[3];
        for (int k = 0; k < 3; k++) q[k] = (uint16_t)(((uint32_t)s_start[e][k] + (uint32_t)s_end[e][k]) / 2u);
        const float px = lerp_pos(c.b[0], c.b[1], q[0]), py = lerp_pos(c.b[2], c.b[3], q[1]), pz = lerp_pos(c.b[4], c.b[5], q[2]);
        GR gx = gr(px, 1.0f, 0.0f, 0.0f), gy = gr(py, 0.0f, 1.0f, 0.0f), gz = gr(pz, 0.0f, 0.0f, 1.0f);
        if (P.has_mat) {
            Mat4 m;
#pragma unroll
            for (int k = 0; k < 16; k++) m.m[k] = P.mat[k];
            xf_grad(m, gx, gy, gz, gx, gy, gz);
        }
        __syncthreads();
        Regs<GR, WAVE> G{(GR*)smem, lane};
        const GR result = eval_grad(P, G, gx, gy, gz, c.path);
        if (lane < (int)ne) {
            for (int k = 0; k < 3; k++) o->inter[lane][k] = q[k];
            o->pos[lane][0] = px; o->pos[lane][1] = py; o->pos[lane][2] = pz;
            o->grad[lane][0] = result.dx; o->grad[lane][1] = result.dy; o->grad[lane][2] = result.dz; o->grad[lane][3] = result.v;
        }
    }
    // (the QEFs of the cell vertices: k_mesh_leaf_qef, one LANE per record - here they kept a whole wavefront waiting on lane 0)
    if (lane == 0) { o->n_edges = ne; o->n_verts = nv; }
}

// ---- the same leaf sampling as passes over all leaf cells of a chunk (what fhip_mesh_* run; FHIP_MESH_LEAF_PASSES=0: k_mesh_leaf) --------------------------------------
// k_mesh_leaf gives a leaf a wavefront and leaves most of its lanes idle most of the time: 8 of 64 at the corners, 16 x (edges mod 4)
// in the last pass of a search round, one per edge in the gradient pass - about half of its lane-evaluations are wasted, and every one
// is ~90 f64 operations for a sin / cos.  Here every lane of every pass has a point of its own: corners 8 cells per wave; the edge
// search one wave per FOUR EDGES, of whatever cells (the cells' edges are appended to a list as the corners find them; the 16 lanes of an
// edge keep its bracket in registers through the four rounds: no LDS, no barriers); gradients one lane per edge.  Per lane the arithmetic
// is k_mesh_leaf's, operation for operation: the records are the same, bit for bit.
__global__ void __launch_bounds__(WAVE) k_mesh_corners(FhMeshParams P, const FhMeshCell* cells, uint32_t n, const FhMdcTable* T, FhMeshLeaf* out,
                                                        uint32_t* edge_count, uint32_t* edge_list /* (cell << 4) | edge */) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x, cr = lane & 7;
    const uint32_t li = blockIdx.x * 8 + (lane >> 3);
    const bool act = li < n;
    const FhMeshCell c = cells[act ? li : n - 1];
    Regs<float, WAVE> R{(float*)smem, lane};
    const float v = eval_point(P, R, (cr & 1) ? c.b[1] : c.b[0], (cr & 2) ? c.b[3] : c.b[2], (cr & 4) ? c.b[5] : c.b[4], c.path);
    const uint32_t mask = (uint32_t)((ballot(v < 0.0f) >> (lane & ~7)) & 0xFFull);
    const uint32_t ne = (mask == 0 || mask == 255) ? 0u : T->n_edges[mask];
    // this wave's edges: one reservation in the list, the cells' shares in cell order
    uint32_t before = 0, total = 0;
    for (int g = 0; g < 8; g++) {
        const uint32_t ng = (uint32_t)__shfl((int)(act ? ne : 0u), g * 8);
        if (g < (lane >> 3)) before += ng;
        total += ng;
    }
    uint32_t base = 0;
    if (lane == 0 && total) base = atomicAdd(edge_count, total);
    base = uni(base);
    if (!act) return;
    FhMeshLeaf* o = &out[li];
    if (cr < 6) o->b[cr] = c.b[cr];
    if (cr == 0) { o->path = c.path; o->mask = mask; o->n_edges = ne; o->n_verts = ne ? T->n_verts[mask] : 0u; o->pad = 0; }
    for (uint32_t e = cr; e < ne; e += 8) edge_list[base + before + e] = (li << 4) | e;
}

// The corners as passes around the assembly bulk interpreter, like the edge search (capi_mesh.hpp sample_chunk): k_mesh_corner_points writes the
// chunk's 8 n corner points as the interpreter's [slot][8 n] arrays (after xf_point when there is a matrix: what eval_point does), the
// interpreter evaluates them, k_mesh_corner_masks does the rest of k_mesh_corners from the values - same points, same f32 evaluator
// semantics (tests/test_render_random.py drives every opcode through both), so the same masks and records.
__global__ void __launch_bounds__(256) k_mesh_corner_points(FhMeshParams P, const FhMeshCell* cells, uint32_t n, float* vars) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * 8u) return;
    const FhMeshCell c = cells[i >> 3];
    const uint32_t cr = i & 7u;
    float x = (cr & 1) ? c.b[1] : c.b[0], y = (cr & 2) ? c.b[3] : c.b[2], z = (cr & 4) ? c.b[5] : c.b[4];
    if (P.has_mat) {
        Mat4 m;
#pragma unroll
        for (int q = 0; q < 16; q++) m.m[q] = P.mat[q];
        xf_point(m, x, y, z, x, y, z);
    }
    const size_t np = (size_t)n * 8;
    for (uint32_t s = 0; s < FH_MAX_INPUTS; s++) {
        const uint32_t kd = P.in_kind[s];
        if (kd < 3) vars[(size_t)s * np + i] = kd == 0 ? x : (kd == 1 ? y : z);
    }
}
__global__ void __launch_bounds__(WAVE) k_mesh_corner_masks(const FhMeshCell* cells, uint32_t n, const float* values, const FhMdcTable* T, FhMeshLeaf* out,
                                                             uint32_t* edge_count, uint32_t* edge_list /* (cell << 4) | edge */) {
    const int lane = threadIdx.x, cr = lane & 7;
    const uint32_t li = blockIdx.x * 8 + (lane >> 3);
    const bool act = li < n;
    const FhMeshCell c = cells[act ? li : n - 1];
    const float v = values[(size_t)(act ? li : n - 1) * 8 + cr];
    const uint32_t mask = (uint32_t)((ballot(v < 0.0f) >> (lane & ~7)) & 0xFFull);
    const uint32_t ne = (mask == 0 || mask == 255) ? 0u : T->n_edges[mask];
    uint32_t before = 0, total = 0;
    for (int g = 0; g < 8; g++) {
        const uint32_t ng = (uint32_t)__shfl((int)(act ? ne : 0u), g * 8);
        if (g < (lane >> 3)) before += ng;
        total += ng;
    }
    uint32_t base = 0;
    if (lane == 0 && total) base = atomicAdd(edge_count, total);
    base = uni(base);
    if (!act) return;
    FhMeshLeaf* o = &out[li];
    if (cr < 6) o->b[cr] = c.b[cr];
    if (cr == 0) { o->path = c.path; o->mask = mask; o->n_edges = ne; o->n_verts = ne ? T->n_verts[mask] : 0u; o->pad = 0; }
    for (uint32_t e = cr; e < ne; e += 8) edge_list[base + before + e] = (li << 4) | e;
}

__global__ void __launch_bounds__(WAVE) k_mesh_edges(FhMeshParams P, const FhMdcTable* T, FhMeshLeaf* out, const uint32_t* edge_list, uint32_t n_edges) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x, grp = lane >> 4;
    const uint32_t j = lane & 15;
    const uint32_t k = blockIdx.x * 4 + grp;
    const bool valid = k < n_edges;
    const uint32_t ent = edge_list[valid ? k : 0];
    FhMeshLeaf* o = &out[ent >> 4];
    const uint32_t e = ent & 15u, mask = o->mask;
    float b[6];
    for (int q = 0; q < 6; q++) b[q] = o->b[q];
    // the edge's end points in u16 cell coordinates (octree.rs:662-695), as k_mesh_leaf sets them up
    uint32_t s[3] = {0, 0, 0}, t[3];
    {
        const int st = T->edge[mask][e][0], en = T->edge[mask][e][1];
        const int axis = st ^ en, ai = axis == 1 ? 0 : (axis == 2 ? 1 : 2);
        const int i1 = (ai + 1) % 3, i2 = (ai + 2) % 3;
        s[i1] = (st & (1 << i1)) ? 65535u : 0u;
        s[i2] = (st & (1 << i2)) ? 65535u : 0u;
        for (int q = 0; q < 3; q++) t[q] = s[q];
        s[ai] = (en & axis) ? 0u : 65535u;
        t[ai] = (en & axis) ? 65535u : 0u;
    }
    Regs<float, WAVE> R{(float*)smem, lane};
    for (int round = 0; round < 4; round++) {       // N-ary search: 16 points per round (octree.rs:697-768)
        uint32_t p[3];
        for (int q = 0; q < 3; q++) p[q] = (s[q] * (15u - j) + t[q] * j) / 15u;
        const float r = eval_point(P, R, lerp_pos(b[0], b[1], p[0]), lerp_pos(b[2], b[3], p[1]), lerp_pos(b[4], b[5], p[2]), o->path);
        const uint32_t m16 = (uint32_t)(ballot(r >= 0.0f) >> (grp * 16)) & 0xFFFFu;
        uint32_t frac = m16 ? (uint32_t)__builtin_ctz(m16) : 16u;
        if (frac == 0) frac = 1;
        if (frac > 15) frac = 15;
        for (int q = 0; q < 3; q++) {
            const uint32_t lo = (uint32_t)(uint16_t)((s[q] * (15u - (frac - 1)) + t[q] * (frac - 1)) / 15u);
            const uint32_t hi = (uint32_t)(uint16_t)((s[q] * (15u - frac) + t[q] * frac) / 15u);
            s[q] = lo; t[q] = hi;
        }
    }
    if (valid && j == 0) {
        uint16_t qq[3];
        for (int q = 0; q < 3; q++) qq[q] = (uint16_t)((s[q] + t[q]) / 2u);
        for (int q = 0; q < 3; q++) o->inter[e][q] = qq[q];
        o->pos[e][0] = lerp_pos(b[0], b[1], qq[0]); o->pos[e][1] = lerp_pos(b[2], b[3], qq[1]); o->pos[e][2] = lerp_pos(b[4], b[5], qq[2]);
    }
}

// ---- ... and with the values from the assembly bulk interpreter (fh_float_eval_*[_t]: 256 or 128 samples per wave at ~22 instructions per op,
// where eval_point's generic interpreter spends ~40 per op on 64): the four rounds as passes over the chunk's edges - this round's 16 sample
// points per edge written as the interpreter's [slot][n] input arrays, the interpreter, the brackets narrowed by the signs (mesh_edges.hpp).
__global__ void __launch_bounds__(256) k_mesh_edge_begin(const FhMdcTable* T, const FhMeshLeaf* recs, const uint32_t* edge_list, uint32_t n_edges, fhmesh::EdgeBracket* br) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_edges) return;
    const uint32_t ent = edge_list[k], mask = recs[ent >> 4].mask, e = ent & 15u;
    br[k] = fhmesh::edge_ends(T->edge[mask][e][0], T->edge[mask][e][1]);
}
// one lane per sample: sample i = 16 * edge + j; vars[slot * n + i] for the tape's x / y / z slots (constant slots are filled once per chunk)
__global__ void __launch_bounds__(256) k_mesh_edge_points(FhMeshParams P, const FhMeshLeaf* recs, const uint32_t* edge_list, const fhmesh::EdgeBracket* br, uint32_t n_edges,
                                                           float* vars, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_edges * 16u) return;
    const uint32_t k = i >> 4, j = i & 15u;
    const FhMeshLeaf* o = &recs[edge_list[k] >> 4];
    uint32_t p[3];
    fhmesh::edge_sample(br[k], j, p);
    float x = lerp_pos(o->b[0], o->b[1], p[0]), y = lerp_pos(o->b[2], o->b[3], p[1]), z = lerp_pos(o->b[4], o->b[5], p[2]);
    if (P.has_mat) {
        Mat4 m;
#pragma unroll
        for (int q = 0; q < 16; q++) m.m[q] = P.mat[q];
        xf_point(m, x, y, z, x, y, z);
    }
    for (uint32_t s = 0; s < FH_MAX_INPUTS; s++) {
        const uint32_t kd = P.in_kind[s];
        if (kd < 3) vars[(size_t)s * n + i] = kd == 0 ? x : (kd == 1 ? y : z);
    }
}
__global__ void __launch_bounds__(256) k_mesh_fill(float* p, float v, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
__global__ void __launch_bounds__(256) k_mesh_edge_narrow(fhmesh::EdgeBracket* br, const float* values, uint32_t n_edges) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_edges) return;
    uint32_t m16 = 0;
    for (uint32_t j = 0; j < 16; j++) m16 |= (values[(size_t)k * 16 + j] >= 0.0f ? 1u : 0u) << j;
    br[k] = fhmesh::edge_narrow(br[k], m16);
}
__global__ void __launch_bounds__(256) k_mesh_edge_end(FhMeshLeaf* recs, const uint32_t* edge_list, const fhmesh::EdgeBracket* br, uint32_t n_edges) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_edges) return;
    const uint32_t ent = edge_list[k], e = ent & 15u;
    FhMeshLeaf* o = &recs[ent >> 4];
    uint16_t q[3];
    fhmesh::edge_mid(br[k], q);
    for (int a = 0; a < 3; a++) o->inter[e][a] = q[a];
    o->pos[e][0] = lerp_pos(o->b[0], o->b[1], q[0]); o->pos[e][1] = lerp_pos(o->b[2], o->b[3], q[1]); o->pos[e][2] = lerp_pos(o->b[4], o->b[5], q[2]);
}

// gradients at the intersections (octree.rs:771-803): one lane per edge
__global__ void __launch_bounds__(WAVE) k_mesh_grads(FhMeshParams P, FhMeshLeaf* out, const uint32_t* edge_list, uint32_t n_edges) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const uint32_t k = blockIdx.x * WAVE + lane;
    const bool valid = k < n_edges;
    const uint32_t ent = edge_list[valid ? k : 0];
    FhMeshLeaf* o = &out[ent >> 4];
    const uint32_t e = ent & 15u;
    const float px = o->pos[e][0], py = o->pos[e][1], pz = o->pos[e][2];
    GR gx = gr(px, 1.0f, 0.0f, 0.0f), gy = gr(py, 0.0f, 1.0f, 0.0f), gz = gr(pz, 0.0f, 0.0f, 1.0f);
    if (P.has_mat) {
        Mat4 m;
#pragma unroll
        for (int q = 0; q < 16; q++) m.m[q] = P.mat[q];
        xf_grad(m, gx, gy, gz, gx, gy, gz);
    }
    Regs<GR, WAVE> G{(GR*)smem, lane};
    const GR result = eval_grad(P, G, gx, gy, gz, o->path);
    if (valid) { o->grad[e][0] = result.dx; o->grad[e][1] = result.dy; o->grad[e][2] = result.dz; o->grad[e][3] = result.v; }
}

// one QEF per cell vertex (octree.rs:805-848), vertices in order: a NaN gradient snaps the vertex to that intersection and
// stops its loop WITHOUT consuming the edge (the reference's `break` comes before `i += 1`), so the next vertex starts there.
// One lane per leaf record: the Jacobi sweeps of fhq::Qef::solve are a few thousand dependent f64 operations, which at the end of
// k_mesh_leaf occupied a wavefront for the sake of one lane.
__global__ void __launch_bounds__(WAVE) k_mesh_leaf_qef(const FhMdcTable* T, FhMeshLeaf* recs, uint32_t n) {
    const uint32_t li = blockIdx.x * WAVE + threadIdx.x;
    if (li >= n) return;
    FhMeshLeaf* o = &recs[li];
    const uint32_t mask = o->mask;
    if (mask == 0 || mask == 255) return;
    const uint32_t nv = T->n_verts[mask];
    uint32_t i = 0;
    for (uint32_t vtx = 0; vtx < nv; vtx++) {
        fhq::Qef q;
        q.init();
        bool forced = false;
        float pos[3] = {0, 0, 0}, err = -1.0f;
        for (uint32_t k = 0; k < T->per_vert[mask][vtx]; k++) {
            const uint32_t ii = i < 12 ? i : 11;
            float g[4], p[3];
            for (int a = 0; a < 4; a++) g[a] = o->grad[ii][a];
            for (int a = 0; a < 3; a++) p[a] = o->pos[ii][a];
            if (g[0] != g[0] || g[1] != g[1] || g[2] != g[2] || g[3] != g[3]) {
                forced = true;
                for (int a = 0; a < 3; a++) pos[a] = p[a];
                err = -2.0f;
                break;
            }
            q.add(p, g);
            i++;
        }
        if (!forced) q.solve(pos, &err);
        for (int a = 0; a < 3; a++) o->vert[vtx][a] = pos[a];
        o->qef_err[vtx] = err;
    }
}

// ---- Mesh::write_stl (fidget-mesh/src/output.rs:14-36) ----------------------------------------------------------------------------------
// The file: 80 bytes of header (44 of text, zeros), the triangle count as a little-endian u32, then 50 bytes per triangle: normal =
// (b - a) x (c - a) in f32, the corners a, b, c, two zero bytes.  The cross product is nalgebra's, which is not vendored here: the operand
// order below - x = u.y v.z - u.z v.y, y = u.z v.x - u.x v.z, z = u.x v.y - u.y v.x, every product and every difference rounded to f32
// (the library is built with -ffp-contract=off) - is RECALLED from its source and could not be verified against it; another order of the
// same products can only change the sign of a zero.  The normal is not normalised (output.rs:20).
// A block packs 256 triangles: every thread gathers its three vertices and writes its record into LDS (12 800 bytes), the block then
// stores its span as coalesced dwords - 84 and 12 800 are multiples of 4, so every block starts on a dword of `out` (which must be
// 4-byte aligned).  A last block with an odd number of triangles ends with a 16-bit store; nothing is written at or beyond
// 84 + 50 n_tris.  Block 0 writes the header and the count (the 21 dwords of H).
constexpr uint32_t FH_STL_TRIS = 256, FH_STL_HEADER = 84, FH_STL_RECORD = 50;
struct FhStlHeader { uint32_t w[FH_STL_HEADER / 4]; };
__global__ void __launch_bounds__(256) k_mesh_stl(const fhmesh::V3* __restrict__ verts, const uint64_t* __restrict__ tris, uint32_t n_tris, FhStlHeader H,
                                                   uint32_t* __restrict__ out) {
    __shared__ uint32_t rec32[FH_STL_TRIS * FH_STL_RECORD / 4];
    uint16_t* const rec = (uint16_t*)rec32;
    const uint32_t tid = threadIdx.x, first = blockIdx.x * FH_STL_TRIS;        // (first <= n_tris: the grid is ceil(n_tris / 256), one block for none)
    const uint32_t cnt = min(FH_STL_TRIS, n_tris - first);
    if (blockIdx.x == 0 && tid < FH_STL_HEADER / 4) out[tid] = H.w[tid];
    if (tid < cnt) {
        const uint64_t* q = tris + (size_t)(first + tid) * 3;
        const fhmesh::V3 a = verts[q[0]], b = verts[q[1]], c = verts[q[2]];
        const float ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
        const float vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
        const float f[12] = {uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
        uint16_t* r = rec + tid * (FH_STL_RECORD / 2);      // (a record starts on an even byte, every second one not on a dword: halves)
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const uint32_t bits = __float_as_uint(f[k]);
            r[2 * k] = (uint16_t)(bits & 0xFFFFu); r[2 * k + 1] = (uint16_t)(bits >> 16);
        }
        r[24] = 0;      // the attribute byte count
    }
    __syncthreads();
    const uint32_t bytes = cnt * FH_STL_RECORD, n_dw = bytes >> 2;
    uint32_t* const dst = out + FH_STL_HEADER / 4 + (size_t)blockIdx.x * (FH_STL_TRIS * FH_STL_RECORD / 4);
    for (uint32_t i = tid; i < n_dw; i += 256) dst[i] = rec32[i];
    if ((bytes & 2u) && tid == 0) *(uint16_t*)(dst + n_dw) = rec[2 * n_dw];
}

// ---- gradients at a mesh's vertices -----------------------------------------------------------------------------------------------------
// out[i] = {v, dx, dy, dz} of the tape at vertex i (model space: octree.rs:58-65 has already taken the vertices there), x / y / z seeded
// (1,0,0) / (0,1,0) / (0,0,1) in registers, every other input slot the constant values[slot] with a zero gradient.  The interpreter is
// k_eval_grad's (step<GRAD>), the register file in LDS, or - GREGS - this block's region of a global slab when n_regs x 64 x 16 bytes
// exceed LDS; a block takes 64 vertices at a time, as many times as the grid needs to cover them (the slab bounds the grid).
template <bool GREGS>
__global__ void __launch_bounds__(WAVE) k_mesh_vertex_grads(const uint64_t* __restrict__ tape_g, uint32_t len, uint32_t n_regs, const fhmesh::V3* __restrict__ verts, uint64_t n,
                                                             int sx, int sy, int sz, const float* __restrict__ values, float4* __restrict__ out, GR* gregs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ctape_t tape = (ctape_t)tape_g;
    const int lane = threadIdx.x;
    Regs<GR, WAVE> R{GREGS ? gregs + (size_t)blockIdx.x * n_regs * WAVE : (GR*)smem, lane};
    for (uint64_t base = (uint64_t)blockIdx.x * WAVE; base < n; base += (uint64_t)gridDim.x * WAVE) {
        const uint64_t i = base + (uint64_t)lane;
        const bool act = i < n;
        const fhmesh::V3 p = verts[act ? i : n - 1];
        const GR gx = gr(p.x, 1.0f, 0.0f, 0.0f), gy = gr(p.y, 0.0f, 1.0f, 0.0f), gz = gr(p.z, 0.0f, 0.0f, 1.0f);
        for (uint32_t k = 0; k < len; k++) {
            const uint64_t w = tape[k];
            step<GRAD, WAVE, true>(
                w, R,
                [&](uint32_t slot) { return (int)slot == sz ? gz : ((int)slot == sy ? gy : ((int)slot == sx ? gx : gr(values[slot], 0.0f, 0.0f, 0.0f))); },     // (bind_inputs: a slot two axes share is the later axis')
                [&](uint32_t, GR v) { if (act) out[i] = make_float4(v.v, v.dx, v.dy, v.dz); },
                [&](int) {});
        }
    }
}

// ---- the octree assembled on the device (mesh_collapse.hpp: one thread per ambiguous cell / candidate / leaf record and pass) ----------
__global__ void __launch_bounds__(256) k_oct_kind(fhmesh::OctLevel D, fhmesh::OctLevel C, fhmesh::OctLeaves L, const FhMdcTable* T, uint32_t* counter, uint32_t n) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n) fhmesh::oct_kind(D, C, L, T, s, counter);
}
__global__ void __launch_bounds__(64) k_oct_collapse(fhmesh::OctLevel D, fhmesh::OctLevel C, fhmesh::OctLeaves L, const FhMdcTable* T, uint32_t n) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) fhmesh::oct_collapse(D, C, L, T, k);
}
__global__ void __launch_bounds__(256) k_oct_place(fhmesh::OctLevel D, fhmesh::OctLevel C, fhmesh::OctLeaves L, const FhMdcTable* T, fhmesh::Cell* cells, fhmesh::V3* verts,
                                                    const float* mat, uint32_t n) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n) fhmesh::oct_place(D, C, L, T, s, cells, verts, mat);
}
__global__ void __launch_bounds__(256) k_oct_leaf_verts(fhmesh::OctLeaves L, fhmesh::V3* verts, const float* mat, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fhmesh::oct_leaf_verts(L, i, verts, mat);
}

// the mesh's vertices out of the octree's (for the dual walk on the HOST, option mesh_device_walk 0: it says which - first uses, in its order)
__global__ void __launch_bounds__(256) k_oct_gather(const fhmesh::V3* verts, const uint32_t* idx, fhmesh::V3* out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = verts[idx[i]];
}


// ---- Octree::walk_dual on the device (mesh_walk.hpp: the recursion as level arrays, MeshBuilder's numbering by atomic minima) ----------
__global__ void __launch_bounds__(256) k_walk_count(fhmesh::WalkTree o, const fhmesh::WalkItem* items, uint32_t n, uint32_t* cnt, uint32_t* live) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const fhmesh::WalkItem k = items[i];
    cnt[i] = fhmesh::wk_count(o, k);
    if ((k.hdr & 3u) != fhmesh::WK_REC) *live = 1;      // (every writer writes the same value)
}
__global__ void __launch_bounds__(256) k_walk_expand(fhmesh::WalkTree o, const fhmesh::WalkItem* items, uint32_t n, const uint32_t* off, fhmesh::WalkItem* next) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t at = off[i];
    if (off[i + 1] == at) return;
    fhmesh::wk_expand(o, items[i], next + at);
}
__global__ void __launch_bounds__(256) k_walk_first(const fhmesh::WalkItem* recs, uint32_t n, uint32_t* first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;       // one thread per reference: 5 per record
    if (i >= n * 5u) return;
    atomicMin(&first[recs[i / 5u].a[i % 5u]], i);
}
__global__ void __launch_bounds__(256) k_walk_rec_counts(const fhmesh::WalkItem* recs, uint32_t n, const uint32_t* first, uint32_t* nn, uint32_t* nt) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fhmesh::wk_rec_counts(recs[i], i, first, &nn[i], &nt[i]);
}
__global__ void __launch_bounds__(256) k_walk_rec_number(const fhmesh::WalkItem* recs, uint32_t n, uint32_t* first, const uint32_t* vb, const fhmesh::V3* octree_verts, fhmesh::V3* verts) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fhmesh::wk_rec_number(recs[i], i, first, vb[i], octree_verts, verts);
}
__global__ void __launch_bounds__(256) k_walk_rec_triangles(const fhmesh::WalkItem* recs, uint32_t n, const uint32_t* first, const uint32_t* tb, uint64_t* tris) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fhmesh::wk_rec_triangles(recs[i], first, tb[i], tris);
}
// exclusive prefix sums: out[i] = in[0] + .. + in[i - 1] for i in [0, n] (in[n] is not read), a block of 256 threads over 2048 elements;
// sums[block] = the block's total; k_scan_add adds the (already scanned) block totals back
constexpr uint32_t FH_SCAN_PER_BLOCK = 2048;
__global__ void __launch_bounds__(256) k_scan_block(const uint32_t* in, uint32_t n, uint32_t* out, uint32_t* sums) {
    __shared__ uint32_t part[256];
    const uint32_t base = blockIdx.x * FH_SCAN_PER_BLOCK + threadIdx.x * 8u;
    uint32_t v[8], s = 0;
    for (uint32_t k = 0; k < 8; k++) { v[k] = base + k < n ? in[base + k] : 0u; s += v[k]; }
    part[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t add = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - s;
    for (uint32_t k = 0; k < 8; k++) { if (base + k <= n) out[base + k] = run; run += v[k]; }
    if (threadIdx.x == 255 && sums) sums[blockIdx.x] = part[255];
}
__global__ void __launch_bounds__(256) k_scan_add(uint32_t* out, uint32_t n, const uint32_t* block_off) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) out[i] += block_off[i / FH_SCAN_PER_BLOCK];
}

// ---- shape occupancy: the inside voxels of the regular grid of N = 4 << depth per axis, as integer sums -------------------------------
// The octree of k_mesh_cells with another leaf: a Full cell counts all its voxels (closed forms, k_occ_full), an Empty one none, an
// ambiguous cell of the last level is sampled at the centres of its 4 x 4 x 4 voxels (k_occ_leaves).  Voxel (i, j, k) is inside iff the
// tape is < 0 at c(i) = float(2 i + 1 - N) * (1.0f / N) (both factors and the product exact in f32), likewise j, k.  Every block writes
// one partial record; the host adds them up - integers, so the result does not depend on the order.
FH_DEV void occ_zero(FhOccPart& a) {
    a.n = 0;
    for (int k = 0; k < 3; k++) { a.s1[k] = 0; a.lo[k] = 0xFFFFFFFFu; a.hi[k] = 0; }
    for (int k = 0; k < 6; k++) a.s2[k] = 0;
}
// the origin (in cells of its level) of the cell with this path: 3 bits per level below a leading 1, bit 0 x, 1 y, 2 z, the last level lowest
// (mesh_vox.hpp: the voxel bitmap's index arithmetic starts from the same origin, on the device and in its host build)
FH_DEV void occ_origin(uint64_t path, uint32_t level, uint32_t o[3]) { fhvox::cell_origin(path, level, o); }
// all the voxels of the box [X, X + w) x [Y, Y + w) x [Z, Z + w): with S1(X) = sum of a over [X, X + w) = w X + w (w - 1) / 2 and
// S2(X) = sum of a^2 = w X^2 + X w (w - 1) + (w - 1) w (2 w - 1) / 6:  n = w^3, sum i = w^2 S1(X), sum i^2 = w^2 S2(X), sum ij = w S1(X) S1(Y).
// (N <= 4096: the largest, sum i^2 of the whole grid, is below N^5 = 2^60)
FH_DEV void occ_add_box(FhOccPart& a, const uint32_t org[3], uint32_t w32) {
    const uint64_t w = w32, t1 = w * (w - 1) / 2, t2 = (w - 1) * w * (2 * w - 1) / 6;
    uint64_t S1[3], S2[3];
    for (int k = 0; k < 3; k++) {
        const uint64_t X = org[k];
        S1[k] = w * X + t1;
        S2[k] = w * X * X + X * w * (w - 1) + t2;
        a.lo[k] = min(a.lo[k], org[k]);
        a.hi[k] = max(a.hi[k], org[k] + w32 - 1);
    }
    a.n += w * w * w;
    for (int k = 0; k < 3; k++) { a.s1[k] += w * w * S1[k]; a.s2[k] += w * w * S2[k]; }
    a.s2[3] += w * S1[0] * S1[1]; a.s2[4] += w * S1[0] * S1[2]; a.s2[5] += w * S1[1] * S1[2];
}
FH_DEV uint64_t occ_shfl_down(uint64_t v, int d) { return (uint64_t)__shfl_down((unsigned long long)v, d); }
// the sum of the lanes' records, valid in lane 0
FH_DEV void occ_wave_reduce(FhOccPart& a) {
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        a.n += occ_shfl_down(a.n, d);
        for (int k = 0; k < 3; k++) {
            a.s1[k] += occ_shfl_down(a.s1[k], d);
            a.lo[k] = min(a.lo[k], (uint32_t)__shfl_down((int)a.lo[k], d));
            a.hi[k] = max(a.hi[k], (uint32_t)__shfl_down((int)a.hi[k], d));
        }
        for (int k = 0; k < 6; k++) a.s2[k] += occ_shfl_down(a.s2[k], d);
    }
}

// The Full cells of one level (cls as k_mesh_cells left it: cell i is child (i & 7) of in[i >> 3] when expand): one lane per cell, the
// closed forms of a cell of edge w = N >> level voxels; one partial record per block.  The grid is bounded: a block strides over the cells.
__global__ void __launch_bounds__(256) k_occ_full(const FhMeshCell* in, const uint8_t* cls, uint32_t n, int expand, uint32_t level, uint32_t depth, FhOccPart* out) {
    __shared__ FhOccPart part[256 / WAVE];
    FhOccPart a;
    occ_zero(a);
    const uint32_t w = (4u << depth) >> level;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        if (cls[i] != 2) continue;
        const uint64_t path = expand ? ((in[i >> 3].path << 3) | (i & 7)) : in[i].path;
        uint32_t o[3];
        occ_origin(path, level, o);
        for (int k = 0; k < 3; k++) o[k] *= w;
        occ_add_box(a, o, w);
    }
    occ_wave_reduce(a);
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < 256 / WAVE; v++) {
            const FhOccPart b = part[v];
            a.n += b.n;
            for (int k = 0; k < 3; k++) { a.s1[k] += b.s1[k]; a.lo[k] = min(a.lo[k], b.lo[k]); a.hi[k] = max(a.hi[k], b.hi[k]); }
            for (int k = 0; k < 6; k++) a.s2[k] += b.s2[k];
        }
        out[blockIdx.x] = a;
    }
}

// The ambiguous cells of the last level: one wave takes one cell at a time, lane (lx, ly, lz) = (lane & 3, (lane >> 2) & 3, lane >> 4)
// the voxel (4 ox + lx, 4 oy + ly, 4 oz + lz) of the cell at origin (ox, oy, oz), evaluated as k_mesh_leaf's samples are (eval_point: the
// f32 point transform, the cell's own tape, the register file in LDS - a lane only ever touches its own column, so cells need no barrier
// between them).  The inside mask is one ballot; what the cell adds follows from it with X = 4 ox:
//   sum i = n X + sum lx,   sum i^2 = n X^2 + 2 X sum lx + sum lx^2,   sum ij = n X Y + X sum ly + Y sum lx + sum lx ly,
// the local sums being popcounts of the mask against constant lane masks - wave-uniform, scalar work.  The block's sums stay in
// registers across its cells; one store of the record at the end, no atomics.
__global__ void __launch_bounds__(WAVE) k_occ_leaves(FhMeshParams P, const FhMeshCell* cells, uint32_t n, uint32_t depth, FhOccPart* out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const uint32_t lx = lane & 3, ly = (lane >> 2) & 3, lz = lane >> 4;
    const int32_t N = (int32_t)(4u << depth);
    const float inv = 1.0f / (float)N;
    Regs<float, WAVE> R{(float*)smem, lane};
    FhOccPart a;
    occ_zero(a);
    constexpr uint64_t MX = 0x1111111111111111ull, MY = 0x000F000F000F000Full, MZ = 0xFFFFull;
    for (uint32_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
        const uint64_t pv = cells[ci].path;
        const uint64_t path = ((uint64_t)uni((uint32_t)(pv >> 32)) << 32) | (uint64_t)uni((uint32_t)pv);      // (wave-uniform, and known to be)
        uint32_t o[3];
        occ_origin(path, depth, o);
        const uint32_t X = 4 * o[0], Y = 4 * o[1], Z = 4 * o[2];
        const float x = (float)(2 * (int32_t)(X + lx) + 1 - N) * inv, y = (float)(2 * (int32_t)(Y + ly) + 1 - N) * inv, z = (float)(2 * (int32_t)(Z + lz) + 1 - N) * inv;
        const float v = eval_point(P, R, x, y, z, path);
        const uint64_t m = ballot(v < 0.0f);       // (NaN: not inside)
        if (m == 0) continue;
        const uint64_t cnt = (uint64_t)__popcll(m);
        const uint32_t org[3] = {X, Y, Z};
        uint64_t M[3][4];                           // the inside voxels with local coordinate v along axis k
        for (int q = 0; q < 4; q++) { M[0][q] = m & (MX << q); M[1][q] = m & (MY << (4 * q)); M[2][q] = m & (MZ << (16 * q)); }
        uint64_t S[3];
        for (int k = 0; k < 3; k++) {
            const uint64_t c1 = (uint64_t)__popcll(M[k][1]), c2 = (uint64_t)__popcll(M[k][2]), c3 = (uint64_t)__popcll(M[k][3]);
            const uint64_t s = c1 + 2 * c2 + 3 * c3, ss = c1 + 4 * c2 + 9 * c3, O = org[k];
            S[k] = s;
            a.s1[k] += cnt * O + s;
            a.s2[k] += cnt * O * O + 2 * O * s + ss;
            const uint32_t first = M[k][0] ? 0u : (M[k][1] ? 1u : (M[k][2] ? 2u : 3u)), last = M[k][3] ? 3u : (M[k][2] ? 2u : (M[k][1] ? 1u : 0u));
            a.lo[k] = min(a.lo[k], org[k] + first);
            a.hi[k] = max(a.hi[k], org[k] + last);
        }
        int pi = 3;
        for (int k = 0; k < 3; k++)
            for (int j = k + 1; j < 3; j++, pi++) {
                uint64_t cross = 0;
                for (int p = 1; p < 4; p++) for (int q = 1; q < 4; q++) cross += (uint64_t)(p * q) * (uint64_t)__popcll(M[k][p] & M[j][q]);
                a.s2[pi] += cnt * org[k] * org[j] + (uint64_t)org[k] * S[j] + (uint64_t)org[j] * S[k] + cross;
            }
        a.n += cnt;
    }
    if (lane == 0) out[blockIdx.x] = a;
}

// ---- the voxel bitmap: occupancy's inside voxels written down, one 64-bit word per brick of 4 x 4 x 4 (layout: mesh_vox.hpp) ----------
// The same octree with the same leaf: a Full cell becomes a box of all-ones words (k_vox_full), an Empty one stays as the one clearing pass
// before level 0 left it, an ambiguous cell of the last level stores the ballot k_occ_leaves counts (k_vox_leaves).  Cells of one octree are
// disjoint, so every word has one writer after the clearing pass: plain stores, no atomics, the same bitmap in any order.
constexpr uint32_t FH_VOX_FULL_BLOCKS = 4096, FH_VOX_SLICE_BLOCKS = 1u << 16, FH_VOX_COUNT_PARTS = 64;

// The Full cells of one level (cls / in / expand as for k_occ_full).  A lane takes one slot of fhvox::full_slots at a time - 16 bytes (8 for
// single-word rows and a bitmap off 16-byte alignment) at the same place of up to 8 rows of one cell - and the blocks stride over the
// n << lg_per_cell slots of ALL the level's cells; the slots of a cell that is not Full cost its class byte, which the lanes around share.
// Neighbouring lanes hold neighbouring pieces of a row: rows of 32 words and more are stored as whole 256-byte lines per 16 lanes, shorter
// ones (r = 2: 16 bytes per row) as the pieces the layout leaves.  Nothing is read but classes and paths and nothing computed but
// addresses: what bounds the kernel is the store path to HBM (a plain streaming store pass, as the clearing memset is), for short rows
// the partial lines it writes.
__global__ void __launch_bounds__(256) k_vox_full(const FhMeshCell* in, const uint8_t* cls, uint32_t n, int expand, uint32_t level, uint32_t depth, int aligned16, uint64_t* out) {
    const fhvox::FullSlots S = fhvox::full_slots(depth, level, aligned16 != 0);
    const uint64_t total = (uint64_t)n << S.lg_per_cell;
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < total; s += (uint64_t)gridDim.x * 256) {
        const uint32_t i = (uint32_t)(s >> S.lg_per_cell), k = (uint32_t)s & ((1u << S.lg_per_cell) - 1);
        if (cls[i] != 2) continue;
        const uint64_t path = expand ? ((in[i >> 3].path << 3) | (i & 7)) : in[i].path;
        uint32_t o[3];
        occ_origin(path, level, o);
        const uint32_t sh = depth - level;
        const uint64_t cell = fhvox::word_index(depth, o[0] << sh, o[1] << sh, o[2] << sh);
        for (uint32_t q = 0; q < S.rows; q++) {
            uint64_t* const w = out + fhvox::slot_word(S, depth, cell, k, q);
            if (S.vec == 2) *(ulonglong2*)w = make_ulonglong2(~0ull, ~0ull);       // (16-byte aligned: `out` is, the row starts at a multiple of r >= 2 words, the piece at an even word)
            else *w = ~0ull;
        }
    }
}

// k_occ_leaves' loop with the sums replaced by the store of the ballot: bit lane = lx + 4 ly + 16 lz of the cell's word is its voxel
// (lx, ly, lz), which is the bitmap's bit numbering.  One ordinary 8-byte vector store from lane 0; a zero ballot is what the clearing
// pass left.
__global__ void __launch_bounds__(WAVE) k_vox_leaves(FhMeshParams P, const FhMeshCell* cells, uint32_t n, uint32_t depth, uint64_t* out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const uint32_t lx = lane & 3, ly = (lane >> 2) & 3, lz = lane >> 4;
    const int32_t N = (int32_t)(4u << depth);
    const float inv = 1.0f / (float)N;
    Regs<float, WAVE> R{(float*)smem, lane};
    for (uint32_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
        const uint64_t pv = cells[ci].path;
        const uint64_t path = ((uint64_t)uni((uint32_t)(pv >> 32)) << 32) | (uint64_t)uni((uint32_t)pv);      // (wave-uniform, and known to be)
        uint32_t o[3];
        occ_origin(path, depth, o);
        const uint32_t X = 4 * o[0], Y = 4 * o[1], Z = 4 * o[2];
        const float x = (float)(2 * (int32_t)(X + lx) + 1 - N) * inv, y = (float)(2 * (int32_t)(Y + ly) + 1 - N) * inv, z = (float)(2 * (int32_t)(Z + lz) + 1 - N) * inv;
        const float v = eval_point(P, R, x, y, z, path);
        const uint64_t m = ballot(v < 0.0f);       // (NaN: not inside)
        if (m != 0 && lane == 0) out[fhvox::word_index(depth, o[0], o[1], o[2])] = m;
    }
}

// Layer images out of the bitmap: out[(k - k0) * N * N + j * N + i] = 255 where voxel (i, j, k) is inside, 0 where not, for k0 <= k < k1.
// A lane takes a run of `nb` bricks (4; all B of a row where B < 4) of one (k, j): per brick one 8-byte load - the same word serves the
// 16 (ly, lz) of its bricks' rows, from cache after the first - the nibble at 4 ly + 16 lz spread into four bytes, and the run stored as
// one 16-byte vector (`out` 16-byte aligned, N >= 16) or dword by dword.  Bounded grid; a block strides over the runs.
__global__ void __launch_bounds__(256) k_vox_slices(const uint64_t* __restrict__ bricks, uint32_t depth, uint32_t k0, uint32_t k1, uint8_t* __restrict__ out) {
    const uint32_t B = 1u << depth, N = 4u << depth;
    const uint32_t nb = B < 4 ? B : 4, lg_runs = depth < 2 ? 0 : depth - 2;       // runs per row: B / nb
    const uint64_t total = ((uint64_t)(k1 - k0) * N) << lg_runs;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256) {
        const uint32_t g = (uint32_t)t & ((1u << lg_runs) - 1);
        const uint64_t row = t >> lg_runs;                 // (k - k0) * N + j
        const uint32_t j = (uint32_t)(row & (N - 1)), k = k0 + (uint32_t)(row >> (depth + 2));
        const uint32_t shift = 4 * (j & 3) + 16 * (k & 3);
        const uint64_t* const src = bricks + fhvox::word_index(depth, g * nb, j >> 2, k >> 2);
        uint32_t px[4] = {0, 0, 0, 0};
        for (uint32_t q = 0; q < nb; q++) {
            const uint32_t nib = (uint32_t)(src[q] >> shift) & 0xFu;
            px[q] = ((nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21)) * 0xFFu;
        }
        uint8_t* const dst = out + row * N + (size_t)g * 16;
        if (nb == 4) *(uint4*)dst = make_uint4(px[0], px[1], px[2], px[3]);
        else for (uint32_t q = 0; q < nb; q++) ((uint32_t*)dst)[q] = px[q];
    }
}

// Inside voxels per layer: layer k = 4 bz + lz holds the bits 16 lz .. 16 lz + 15 of the bricks of slab bz - popcounts against the
// constant masks k_occ_leaves uses.  Block (part, bz) adds up its share of the slab's B^2 words and writes one partial of four counts;
// k_vox_layer_sum adds a layer's partials.  Integers throughout: the same counts in any order.
__global__ void __launch_bounds__(256) k_vox_layer_counts(const uint64_t* __restrict__ bricks, uint32_t depth, uint64_t* __restrict__ parts /* [B][gridDim.x][4] */) {
    __shared__ uint32_t sh[256 / WAVE][4];
    const uint32_t bz = blockIdx.y;
    const uint64_t per_slab = (uint64_t)1 << (2 * depth);
    const uint64_t* const slab = bricks + bz * per_slab;
    constexpr uint64_t MZ = 0xFFFFull;
    uint32_t c[4] = {0, 0, 0, 0};                   // (a thread sees at most 2^20 / 256 words of 16 bits per layer: far below 2^32)
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < per_slab; i += (uint64_t)gridDim.x * 256) {
        const uint64_t w = slab[i];
        for (int q = 0; q < 4; q++) c[q] += (uint32_t)__popcll(w & (MZ << (16 * q)));
    }
    for (int q = 0; q < 4; q++)
        for (int d = WAVE / 2; d > 0; d >>= 1) c[q] += (uint32_t)__shfl_down((int)c[q], d);
    if ((threadIdx.x & (WAVE - 1)) == 0) for (int q = 0; q < 4; q++) sh[threadIdx.x / WAVE][q] = c[q];
    __syncthreads();
    if (threadIdx.x < 4) {
        uint64_t s = 0;
        for (int v = 0; v < 256 / WAVE; v++) s += sh[v][threadIdx.x];
        parts[((uint64_t)bz * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = s;
    }
}
__global__ void __launch_bounds__(256) k_vox_layer_sum(const uint64_t* __restrict__ parts, uint32_t n_parts, uint32_t n_layers, uint64_t* __restrict__ out) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_layers) return;
    uint64_t s = 0;
    for (uint32_t p = 0; p < n_parts; p++) s += parts[((uint64_t)(k >> 2) * n_parts + p) * 4 + (k & 3)];
    out[k] = s;
}

// ---- contours of a 2D slice: marching squares over the f32 distance image of a pixel-perfect render2d (contour/contour.hpp) -------------
// Four passes over the image and nothing else: every kernel takes the image and its size, plus what the passes before it left.  A block
// of 256 threads takes 256 consecutive lattice edges (cells) at a time and the blocks stride over them, so the grid is bounded.  Edges
// and cells are numbered along rows: the lanes of a wave read consecutive pixels of a row (broken where a row ends), and the second end
// of a vertical edge, the upper corners of a cell, are the same reads one row on - lines the pass has just brought into L2.  Every word
// written has one writer - a ballot word by lane 0 of its wave, a vertex by its edge, a segment by its cell, next[from] by the one
// segment that leaves `from` - so the stores are plain vector stores and the result is the same in any order.
constexpr uint32_t FH_CTR_BLOCKS = 4096;
static_assert(fhctr::EDGE_BLOCK == 256 && WAVE == 64, "k_ctr_*: a block of 256 threads is four ballot words");

// Which edges cross: bits[e / 64] bit e % 64, and per block of 256 edges their number (the scan of these gives every crossing edge its
// vertex id, fhctr::vertex_id).  Edges beyond the last pad their word with zeros.
__global__ void __launch_bounds__(256) k_ctr_edges(const float* __restrict__ img, uint32_t W, uint32_t H, uint64_t* __restrict__ bits, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t part[256 / WAVE];
    const uint64_t E = fhctr::n_edges(W, H);
    const uint32_t n_blk = (uint32_t)((E + 255) / 256), lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    for (uint32_t blk = blockIdx.x; blk < n_blk; blk += gridDim.x) {
        const uint64_t e = (uint64_t)blk * 256 + threadIdx.x;
        bool cross = false;
        if (e < E) {
            const fhctr::Edge ed = fhctr::edge_at((uint32_t)e, W, H);
            cross = fhctr::inside(img[fhctr::edge_pixel0(ed, W)]) != fhctr::inside(img[fhctr::edge_pixel1(ed, W)]);
        }
        const uint64_t m = ballot(cross);
        if (lane == 0) { bits[(size_t)blk * 4 + wv] = m; part[wv] = (uint32_t)__popcll(m); }
        __syncthreads();
        if (threadIdx.x == 0) cnt[blk] = part[0] + part[1] + part[2] + part[3];
        __syncthreads();
    }
}

// One float2 per crossing edge, and its link cleared.  A wave whose ballot word is zero - nearly all of them - reads that word and
// nothing else.  (A lane per ballot word walking its set bits was measured and lost: 21 against 7.6 us at 1024^2, 42 against 49 at
// 4096^2 - the lanes of a wave that do have crossings then work through them one after the other.)
__global__ void __launch_bounds__(256) k_ctr_vertices(const float* __restrict__ img, uint32_t W, uint32_t H, const uint64_t* __restrict__ bits,
                                                      const uint32_t* __restrict__ block_off, float2* __restrict__ verts, uint32_t* __restrict__ next) {
    const uint64_t E = fhctr::n_edges(W, H);
    const uint32_t n_blk = (uint32_t)((E + 255) / 256);
    for (uint32_t blk = blockIdx.x; blk < n_blk; blk += gridDim.x) {
        const uint64_t e64 = (uint64_t)blk * 256 + threadIdx.x;
        if (e64 >= E) continue;
        const uint32_t e = (uint32_t)e64;
        if (!fhctr::edge_crosses(bits, e)) continue;
        const fhctr::Edge ed = fhctr::edge_at(e, W, H);
        float xy[2];
        fhctr::edge_vertex(ed, img[fhctr::edge_pixel0(ed, W)], img[fhctr::edge_pixel1(ed, W)], xy);
        const uint32_t id = fhctr::vertex_id(bits, block_off, e);
        verts[id] = make_float2(xy[0], xy[1]);
        next[id] = fhctr::NONE;
    }
}

// The case of cell c (its segments, packed: fhctr::cell_case), 0 beyond the last cell
FH_DEV uint32_t ctr_cell_case(const float* __restrict__ img, uint32_t W, uint64_t c, uint64_t n_cells, uint32_t& i, uint32_t& j) {
    i = j = 0;
    if (c >= n_cells) return 0u;
    j = (uint32_t)c / (W - 1); i = (uint32_t)c - j * (W - 1);
    const float* const p = img + (size_t)j * W + i;
    const float v00 = p[0], v10 = p[1], v01 = p[W], v11 = p[W + 1];
    return fhctr::cell_case(fhctr::cell_mask(v00, v10, v11, v01), fhctr::saddle_centre_inside(v00, v10, v11, v01));
}
// Segments per block of 256 cells (0, 1 or 2 a cell: two ballots)
__global__ void __launch_bounds__(256) k_ctr_cells(const float* __restrict__ img, uint32_t W, uint32_t H, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t part[256 / WAVE];
    const uint64_t NC = fhctr::n_cells(W, H);
    const uint32_t n_blk = (uint32_t)((NC + 255) / 256), lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    for (uint32_t blk = blockIdx.x; blk < n_blk; blk += gridDim.x) {
        uint32_t i, j;
        const uint32_t n = fhctr::case_count(ctr_cell_case(img, W, (uint64_t)blk * 256 + threadIdx.x, NC, i, j));
        const uint32_t s = (uint32_t)__popcll(ballot(n >= 1)) + (uint32_t)__popcll(ballot(n == 2));
        if (lane == 0) part[wv] = s;
        __syncthreads();
        if (threadIdx.x == 0) cnt[blk] = part[0] + part[1] + part[2] + part[3];
        __syncthreads();
    }
}
// The segments, in cell order: block_off of the cell counts, the waves before this one through LDS, the lanes before this one from the
// two ballots.  The ids of a segment's two edges come from the edge pass (fhctr::vertex_id); next[from] = to.
__global__ void __launch_bounds__(256) k_ctr_segments(const float* __restrict__ img, uint32_t W, uint32_t H, const uint64_t* __restrict__ bits,
                                                      const uint32_t* __restrict__ edge_off, const uint32_t* __restrict__ cell_off, uint2* __restrict__ segs,
                                                      uint32_t* __restrict__ next) {
    __shared__ uint32_t part[256 / WAVE];
    const uint64_t NC = fhctr::n_cells(W, H);
    const uint32_t n_blk = (uint32_t)((NC + 255) / 256), lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    for (uint32_t blk = blockIdx.x; blk < n_blk; blk += gridDim.x) {
        uint32_t i, j;
        const uint32_t cs = ctr_cell_case(img, W, (uint64_t)blk * 256 + threadIdx.x, NC, i, j), n = fhctr::case_count(cs);
        const uint64_t b1 = ballot(n >= 1), b2 = ballot(n == 2);
        if (lane == 0) part[wv] = (uint32_t)__popcll(b1) + (uint32_t)__popcll(b2);
        __syncthreads();
        uint32_t at = cell_off[blk] + (uint32_t)__popcll(b1 & below) + (uint32_t)__popcll(b2 & below);
        for (uint32_t k = 0; k < wv; k++) at += part[k];
        for (uint32_t s = 0; s < n; s++) {
            const uint32_t from = fhctr::vertex_id(bits, edge_off, fhctr::cell_edge(fhctr::case_from(cs, s), i, j, W, H));
            const uint32_t to = fhctr::vertex_id(bits, edge_off, fhctr::cell_edge(fhctr::case_to(cs, s), i, j, W, H));
            segs[at + s] = make_uint2(from, to);
            next[from] = to;
        }
        __syncthreads();
    }
}

// ---- connected components of a voxel bitmap (fhip_voxels_components; the bit arithmetic: mesh_cc.hpp) ------------------------------------
// Foreground: the word XOR `flip` (0, or all ones for the complement).  A node is one component of one brick taken alone
// (fhcc::lowest_component walks them in the order of their lowest bits, recomputed where needed: no array of masks, no scratch); node
// base[brick] + q is the brick's q-th.  Nodes are in the order of the smallest keys (word * 64 + bit) of their voxels, so the smallest
// node of a component holds its seed, and the components in the order of their seeds are the roots in ascending order.
//
// No kernel here waits for another workgroup: no flags, no spinning, no grid barrier.  The only loops over memory that other waves write
// are cc_find and the retry of cc_unite, and each of their steps moves to a strictly smaller node whatever the other waves do
// (parent[x] <= x always: it starts as x and only atomicMin changes it while k_cc_merge runs), so both end after at most `x` steps.
FH_DEV uint32_t cc_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
FH_DEV uint32_t cc_find(const uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = cc_load(parent + x);       // (relaxed, agent scope: past this CU's L1, which other CUs' atomics never refresh)
        if (p == x) return x;
        x = p;                                         // p < x
    }
}
// Lock-free union towards the smaller root (Komura; Playne and Hawick): the larger root's parent takes the minimum of itself and the
// smaller root.  If it was no longer a root - `old` is what another wave linked it to in the meantime - that link may just have been
// replaced, so old and b remain to be united: go on from there.  a + b falls with every turn.
FH_DEV void cc_unite(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

// Nodes per brick, and the totals {nodes, foreground voxels}: one atomic add each per block
__global__ void __launch_bounds__(256) k_cc_count(const uint64_t* __restrict__ bricks, uint64_t n_words, uint64_t flip, uint32_t conn, uint32_t* __restrict__ cnt,
                                                  unsigned long long* __restrict__ totals) {
    __shared__ uint32_t sh[256 / WAVE][2];
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t c = 0, v = 0;
    if (i < n_words) {
        const uint64_t w = bricks[i] ^ flip;
        c = fhcc::local_count(w, conn);
        v = (uint32_t)__popcll(w);
        cnt[i] = c;
    }
    for (int d = WAVE / 2; d > 0; d >>= 1) { c += (uint32_t)__shfl_down((int)c, d); v += (uint32_t)__shfl_down((int)v, d); }
    if ((threadIdx.x & (WAVE - 1)) == 0) { sh[threadIdx.x / WAVE][0] = c; sh[threadIdx.x / WAVE][1] = v; }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t s = 0;
        for (int k = 0; k < 256 / WAVE; k++) s += sh[k][threadIdx.x];
        if (s) atomicAdd(totals + threadIdx.x, (unsigned long long)s);
    }
}
__global__ void __launch_bounds__(256) k_cc_init(uint32_t* __restrict__ parent, uint64_t n_nodes) {
    const uint64_t n = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (n < n_nodes) parent[n] = (uint32_t)n;
}
// One lane per brick: its nodes against those of the bricks in the positive directions (3 faces; 13 for connectivity 26 - every pair of
// neighbouring bricks is seen once, from the brick the direction leaves).  Two nodes are united when the image of one's voxels in the
// other brick (fhcc::carry) meets the other's.  Full next to full - the inside of a solid - is one union without any flood fill.
__global__ void __launch_bounds__(256) k_cc_merge(const uint64_t* __restrict__ bricks, uint32_t depth, uint64_t flip, uint32_t conn, const uint32_t* __restrict__ base,
                                                  uint32_t* parent) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= fhvox::n_words(depth)) return;
    const uint64_t wa = bricks[i] ^ flip;
    if (wa == 0) return;
    const uint32_t B = 1u << depth, bx = (uint32_t)i & (B - 1), by = (uint32_t)(i >> depth) & (B - 1), bz = (uint32_t)(i >> (2 * depth));
    const uint32_t na = base[i], nd = fhcc::n_dirs(conn);
    for (uint32_t d = 0; d < nd; d++) {
        int dx, dy, dz;
        fhcc::direction(d, dx, dy, dz);
        const uint32_t x = bx + (uint32_t)dx, y = by + (uint32_t)dy, z = bz + (uint32_t)dz;       // (-1 wraps to above B: nothing lies beyond the grid)
        if (x >= B || y >= B || z >= B) continue;
        const uint64_t j = fhvox::word_index(depth, x, y, z);
        const uint64_t wb = bricks[j] ^ flip;
        if (wb == 0) continue;
        const uint32_t nb = base[j];
        if ((wa & wb) == ~(uint64_t)0) { cc_unite(parent, na, nb); continue; }
        uint32_t qa = 0;
        for (uint64_t ra = wa; ra != 0; qa++) {
            const uint64_t ma = fhcc::lowest_component(ra, wa, conn);
            ra &= ~ma;
            uint64_t c = fhcc::carry(ma, dx, dy, dz, conn) & wb;
            uint32_t qb = 0;
            for (uint64_t rb = wb; c != 0; qb++) {          // (c is part of wb: every bit of it is in some component of rb)
                const uint64_t mb = fhcc::lowest_component(rb, wb, conn);
                rb &= ~mb;
                if (c & mb) { cc_unite(parent, na + qa, nb + qb); c &= ~mb; }
            }
        }
    }
}
// parent[n] = the root of n.  A launch of its own: every union is in.  Other lanes store roots while this one climbs; whatever it reads -
// the old parent or the root - is an ancestor of the node it read it from, and the roots themselves are not stored to.
__global__ void __launch_bounds__(256) k_cc_flatten(uint32_t* parent, uint64_t n_nodes) {
    const uint64_t n = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= n_nodes) return;
    const uint32_t r = cc_find(parent, (uint32_t)n);
    if (r != (uint32_t)n) __hip_atomic_store(parent + n, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// flag[n] = 1 for a root; after the scan of the flags, comp[n] = the number of roots below n's root (comp may be the flags' array)
__global__ void __launch_bounds__(256) k_cc_roots(const uint32_t* __restrict__ parent, uint64_t n_nodes, uint32_t* __restrict__ flag) {
    const uint64_t n = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (n < n_nodes) flag[n] = parent[n] == (uint32_t)n ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_cc_number(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ rank, uint64_t n_nodes, uint32_t* comp) {
    const uint64_t n = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (n < n_nodes) comp[n] = rank[parent[n]];
}
// The table: a lane per brick adds each of its nodes to its component.  The lanes of a wave mostly meet in one component - the solid's -
// so where the nodes of a turn all belong to the same one, the wave adds their voxels up and makes one atomic add; bounds and the border
// flag are only sent where a look at the current value (never better than the true one: they move one way) says they would change it.
__global__ void __launch_bounds__(256) k_cc_table(const uint64_t* __restrict__ bricks, uint32_t depth, uint64_t flip, uint32_t conn, const uint32_t* __restrict__ base,
                                                  const uint32_t* __restrict__ comp_of_node, const uint32_t* __restrict__ parent, unsigned long long* size,
                                                  uint32_t* lo, uint32_t* hi, uint32_t* border, uint32_t* __restrict__ seed) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in_grid = i < fhvox::n_words(depth);
    const uint64_t w = in_grid ? bricks[i] ^ flip : 0;
    const uint32_t B = 1u << depth, b[3] = {(uint32_t)i & (B - 1), (uint32_t)(i >> depth) & (B - 1), (uint32_t)(i >> (2 * depth))};
    const uint32_t node0 = w != 0 ? base[i] : 0u;
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    uint64_t rest = w;
    for (uint32_t q = 0; ballot(rest != 0) != 0; q++) {          // (the same number of turns for every lane of the wave)
        const bool on = rest != 0;
        uint64_t m = 0;
        uint32_t comp = 0, cnt = 0;
        if (on) {
            m = fhcc::lowest_component(rest, w, conn);
            rest &= ~m;
            comp = comp_of_node[node0 + q];
            cnt = (uint32_t)__popcll(m);
        }
        const uint64_t who = ballot(on);
        const uint32_t c0 = (uint32_t)__shfl((int)comp, (int)__builtin_ctzll(who));
        if (ballot(on && comp != c0) == 0) {
            uint32_t s = cnt;
            for (int d = WAVE / 2; d > 0; d >>= 1) s += (uint32_t)__shfl_down((int)s, d);
            if (lane == 0) atomicAdd(size + c0, (unsigned long long)s);
        } else if (on) {
            atomicAdd(size + comp, (unsigned long long)cnt);
        }
        if (on) {
            uint32_t l[3], h[3];
            fhcc::local_bounds(m, l, h);
            for (uint32_t a = 0; a < 3; a++) {
                const uint32_t vl = 4 * b[a] + l[a], vh = 4 * b[a] + h[a];
                if (vl < cc_load(lo + 3 * (size_t)comp + a)) atomicMin(lo + 3 * (size_t)comp + a, vl);
                if (vh > cc_load(hi + 3 * (size_t)comp + a)) atomicMax(hi + 3 * (size_t)comp + a, vh);
            }
            if (fhcc::touches_border(m, b[0], b[1], b[2], B) && cc_load(border + comp) == 0) atomicOr(border + comp, 1u);
            if (parent[node0 + q] == node0 + q) {          // the root: the component's smallest node, whose lowest voxel is the seed
                uint32_t v[3];
                fhcc::key_voxel(i * 64 + (uint32_t)__builtin_ctzll(m), depth, v);
                for (uint32_t a = 0; a < 3; a++) seed[3 * (size_t)comp + a] = v[a];
            }
        }
    }
}
// Label images: k_vox_slices' layout - a lane takes a run of `nb` bricks (4; all B of a row where B < 4) of one (k, j) - with an int32 a
// voxel, one 16-byte store a brick: out[(k - k0) * N * N + j * N + i] = the component of voxel (i, j, k), -1 for background.  The brick's
// components are walked until the row's four voxels are all placed.
__global__ void __launch_bounds__(256) k_cc_label_slices(const uint64_t* __restrict__ bricks, uint32_t depth, uint64_t flip, uint32_t conn, const uint32_t* __restrict__ base,
                                                         const uint32_t* __restrict__ comp_of_node, uint32_t k0, uint32_t k1, int32_t* __restrict__ out) {
    const uint32_t B = 1u << depth, N = 4u << depth;
    const uint32_t nb = B < 4 ? B : 4, lg_runs = depth < 2 ? 0 : depth - 2;
    const uint64_t total = ((uint64_t)(k1 - k0) * N) << lg_runs;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256) {
        const uint32_t g = (uint32_t)t & ((1u << lg_runs) - 1);
        const uint64_t row = t >> lg_runs;                 // (k - k0) * N + j
        const uint32_t j = (uint32_t)(row & (N - 1)), k = k0 + (uint32_t)(row >> (depth + 2));
        const uint32_t shift = 4 * (j & 3) + 16 * (k & 3);
        const uint64_t first = fhvox::word_index(depth, g * nb, j >> 2, k >> 2);
        int4* const dst = (int4*)(out + row * N + (size_t)g * 16);
        for (uint32_t q = 0; q < nb; q++) {
            const uint64_t w = bricks[first + q] ^ flip;
            uint64_t want = w & ((uint64_t)0xF << shift);
            int32_t px[4] = {-1, -1, -1, -1};
            if (want != 0) {
                const uint32_t node0 = base[first + q];
                uint32_t c = 0;
                for (uint64_t rest = w; want != 0; c++) {
                    const uint64_t m = fhcc::lowest_component(rest, w, conn);
                    rest &= ~m;
                    if (m & want) {
                        const int32_t id = (int32_t)comp_of_node[node0 + c];
                        const uint32_t nib = (uint32_t)((m & want) >> shift);
                        for (uint32_t v = 0; v < 4; v++) if (nib & (1u << v)) px[v] = id;
                        want &= ~m;
                    }
                }
            }
            dst[q] = make_int4(px[0], px[1], px[2], px[3]);
        }
    }
}
// The bricks of the chosen components: the OR of the masks of the nodes whose component is flagged.  Every word is written.
__global__ void __launch_bounds__(256) k_cc_extract(const uint64_t* __restrict__ bricks, uint64_t n_words, uint64_t flip, uint32_t conn, const uint32_t* __restrict__ base,
                                                    const uint32_t* __restrict__ comp_of_node, const uint8_t* __restrict__ chosen, uint64_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_words) return;
    const uint64_t w = bricks[i] ^ flip;
    uint64_t o = 0;
    if (w != 0) {
        const uint32_t node0 = base[i];
        uint32_t c = 0;
        for (uint64_t rest = w; rest != 0; c++) {
            const uint64_t m = fhcc::lowest_component(rest, w, conn);
            rest &= ~m;
            if (chosen[comp_of_node[node0 + c]]) o |= m;
        }
    }
    out[i] = o;
}
}  // namespace fhm

// k_edt_*: the exact distance transform of such a bitmap (fhip_voxels_distance) - its own file
#include "edt.hip"
// k_lt_*: the local thickness of such a distance field (fhip_distance_thickness) - its own file
#include "thick.hip"
// k_vm_*: the boundary mesh of such a bitmap (fhip_voxels_mesh, fhip_voxels_surface) - its own file
#include "vmesh.hip"
// k_flow_*, k_overhangs, k_heights*: such a bitmap along a direction (fhip_voxels_flow, _overhangs, _heights) - its own file
#include "flow.hip"
// k_tv_*: a triangle mesh to such a bitmap (fhip_triangles_voxels, fhip_mesh_voxels) - its own file
#include "trivox.hip"
// k_mt_*: the check of a triangle mesh - weld, edges, shells (fhip_triangles_topology, fhip_mesh_topology) - its own file
#include "topo.hip"
// k_ol_*: the outlines of such a bitmap's layers - vertices, successors, loops (fhip_voxels_outlines) - its own file
#include "outline.hip"
// k_on_*: the nesting of those outlines - left links, parents, depths, regions (fhip_outlines_nesting) - its own file, after outline.hip
#include "nest.hip"
// k_ms_*: the slices of a triangle mesh - crossings, segments, loops per plane (fhip_topology_slices) - its own file, after topo.hip
#include "slice.hip"
// k_sn_*: the nesting of those slices - bands, hits, parity, parents (fhip_slices_nesting) - its own file, after slice.hip
#include "slice_nest.hip"
