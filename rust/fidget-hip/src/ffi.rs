//! The raw binding of `include/fidget_hip.h` (the C ABI of libfidget_hip.so): every function the crate calls, with the header's
//! argument order and types.  `tests/test_rust_binding.py` in the fidget-hip repository parses this file and the header and fails
//! on any drift (a function missing on either side of the list below, another arity, another pointer / integer type, another
//! struct field order).
#![allow(non_camel_case_types)]
#![allow(missing_docs)]
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)] pub struct fhip_ctx   { _p: [u8; 0] }
#[repr(C)] pub struct fhip_tape  { _p: [u8; 0] }
#[repr(C)] pub struct fhip_mesh  { _p: [u8; 0] }

/// The result of `fhip_shape_occupancy` (fidget_hip.h): integer sums over the inside voxels of the grid of `grid` per axis
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct fhip_occupancy {
    pub n: u64, pub s1: [u64; 3], pub s2: [u64; 6],
    pub lo: [u32; 3], pub hi: [u32; 3],
    pub grid: u32, pub pad: u32,
    pub cells: [u64; 4],
}

pub type fhip_status = c_int;           // 0 = OK, see fidget_hip.h
pub const FHIP_ERR_BAD_VAR_SLICE: c_int = 1;     // -> TracingEvalError / BulkEvalError::BadVarSlice
pub const FHIP_ERR_MISMATCHED_SLICES: c_int = 2; // -> BulkEvalError::MismatchedSlices
pub const FHIP_ERR_BAD_CHOICE_SLICE: c_int = 3;  // -> BadTrace::BadChoiceSlice

#[repr(C)]
pub struct fhip_render3d_config {
    pub width: u32, pub height: u32, pub depth: u32,
    pub world_to_model: *const f32,          // row-major 4x4 or null
    pub tile_sizes: *const u32, pub n_tile_sizes: u32,
    pub var_keys: *const u64, pub var_values: *const f32, pub n_vars: u32,
    pub axis_slots: *const i32,              // VarMap slots of X, Y, Z (-1 = absent)
}
#[repr(C)]
pub struct fhip_render2d_config {
    pub width: u32, pub height: u32,
    pub world_to_model: *const f32,          // row-major 3x3 or null
    pub z: f32, pub pixel_perfect: c_int,
    pub tile_sizes: *const u32, pub n_tile_sizes: u32,
    pub var_keys: *const u64, pub var_values: *const f32, pub n_vars: u32,
    pub axis_slots: *const i32,
}

#[link(name = "fidget_hip")]
extern "C" {
    pub fn fhip_ctx_create(device: c_int, stream: *mut c_void, out: *mut *mut fhip_ctx) -> fhip_status;
    pub fn fhip_ctx_destroy(ctx: *mut fhip_ctx);
    pub fn fhip_libm_probe(msg: *mut c_char, cap: usize) -> c_int;            // this host's libm against the routines the device restates
    pub fn fhip_last_error(ctx: *const fhip_ctx) -> *const c_char;
    pub fn fhip_cancel(ctx: *mut fhip_ctx);
    pub fn fhip_cancel_reset(ctx: *mut fhip_ctx);
    pub fn fhip_cancel_watch(ctx: *mut fhip_ctx, flag: *const c_void);    // the caller's one-byte cancel flag (CancelToken::into_raw), null: none
    pub fn fhip_ctx_sync(ctx: *mut fhip_ctx) -> fhip_status;     // waits for the asynchronous renders, reports their overflow flags
    pub fn fhip_ctx_trim(ctx: *mut fhip_ctx) -> fhip_status;     // caches kept for speed alone (mesh leaf records, frame lanes) go back
    pub fn fhip_ctx_reserve_arena(ctx: *mut fhip_ctx, megabytes: usize) -> fhip_status;     // a sequence of heavier frames to come: arenas sized ahead
    pub fn fhip_ctx_set_option(ctx: *mut fhip_ctx, name: *const c_char, value: c_int) -> fhip_status;   // behaviour switches: see below
    pub fn fhip_ctx_get_option(ctx: *const fhip_ctx, name: *const c_char, value: *mut c_int) -> fhip_status;

    pub fn fhip_tape_from_bytecode(ctx: *mut fhip_ctx, words: *const u32, n_words: usize,
                                   out: *mut *mut fhip_tape) -> fhip_status;
    pub fn fhip_tape_free(tape: *mut fhip_tape);
    pub fn fhip_tape_len(tape: *const fhip_tape) -> u32;
    pub fn fhip_tape_choice_count(tape: *const fhip_tape) -> u32;
    // RegTape::new::<N> + Bytecode::new of a tape, by the reference's own allocator (LRU eviction, Load / Store spills) on the host:
    // for callers that want VmData<N>'s view of a simplified tape back (len with spills, iter_asm, wire format); info = [len,
    // slot_count, reg_count, mem_count]
    pub fn fhip_tape_reg_tape(tape: *const fhip_tape, n_regs: u32, reg_ops: *mut u32, cap_ops: u32, words: *mut u32, cap_words: u32,
                              info: *mut u32) -> fhip_status;
    pub fn fhip_simplify(ctx: *mut fhip_ctx, tape: *const fhip_tape, choices: *const u8, n: u32,
                         child: *mut *mut fhip_tape) -> fhip_status;

    pub fn fhip_interval_eval(ctx: *mut fhip_ctx, tape: *const fhip_tape, vars: *const f32, n_vars: u32, n: u32,
                              out: *mut f32, choices: *mut u8, simplify: *mut u8) -> fhip_status;
    pub fn fhip_point_eval(ctx: *mut fhip_ctx, tape: *const fhip_tape, vars: *const f32, n_vars: u32, n: u32,
                           out: *mut f32, choices: *mut u8, simplify: *mut u8) -> fhip_status;
    pub fn fhip_float_eval(ctx: *mut fhip_ctx, tape: *const fhip_tape, vars: *const *const f32, lens: *const u32,
                           n_vars: u32, out: *const *mut f32) -> fhip_status;
    pub fn fhip_grad_eval(ctx: *mut fhip_ctx, tape: *const fhip_tape, vars: *const *const f32, lens: *const u32,
                          n_vars: u32, out: *const *mut f32) -> fhip_status;
    /// fidget::solver::solve (fidget-solver/src/lib.rs:191), batched over `n_instances` parameter sets
    pub fn fhip_solve(ctx: *mut fhip_ctx, constraints: *const *const fhip_tape, n_constraints: u32, param_axis: *const i32,
                      param_index: *const u64, param_free: *const u8, n_params: u32, values: *const f32, n_instances: u32,
                      max_iterations: u32, out: *mut f32, err: *mut f32, iterations: *mut u32, exit_reason: *mut i32) -> fhip_status;

    pub fn fhip_render2d(ctx: *mut fhip_ctx, tape: *const fhip_tape, cfg: *const fhip_render2d_config,
                         out: *mut f32, out_is_device: c_int) -> fhip_status;
    pub fn fhip_render3d(ctx: *mut fhip_ctx, tape: *const fhip_tape, cfg: *const fhip_render3d_config,
                         out: *mut c_void, out_is_device: c_int) -> fhip_status;
    pub fn fhip_render3d_shard(ctx: *mut fhip_ctx, tape: *const fhip_tape, cfg: *const fhip_render3d_config,
                               out: *mut c_void, out_is_device: c_int, shard: u32, n_shards: u32) -> fhip_status;
    pub fn fhip_render3d_block(ctx: *mut fhip_ctx, tape: *const fhip_tape, cfg: *const fhip_render3d_config,
                               out: *mut c_void, out_is_device: c_int, index: u32, split: *const u32) -> fhip_status;
    pub fn fhip_merge_depth(ctx: *mut fhip_ctx, front: *mut c_void, back: *const c_void, n_pixels: u64, image_depth: u32) -> fhip_status;

    // fidget_raster::effects on the image a render left in HBM (on_device = 1) or on host buffers
    pub fn fhip_denoise_normals(ctx: *mut fhip_ctx, image: *const c_void, w: u32, h: u32, out: *mut c_void, on_device: c_int) -> fhip_status;
    pub fn fhip_compute_ssao(ctx: *mut fhip_ctx, image: *const c_void, w: u32, h: u32, depth: u32, kernel: *const f32, n_kernel: u32,
                             noise: *const f32, n_noise: u32, out: *mut f32, on_device: c_int) -> fhip_status;
    pub fn fhip_blur_ssao(ctx: *mut fhip_ctx, ssao: *const f32, w: u32, h: u32, out: *mut f32, on_device: c_int) -> fhip_status;
    pub fn fhip_apply_shading(ctx: *mut fhip_ctx, image: *const c_void, w: u32, h: u32, depth: u32, ssao: *const f32,
                              out_rgb: *mut u8, on_device: c_int) -> fhip_status;
    pub fn fhip_to_rgba(ctx: *mut fhip_ctx, image: *const f32, w: u32, h: u32, mode: c_int, out_rgba: *mut u8, on_device: c_int) -> fhip_status;

    // fidget_mesh::Octree::build + walk_dual
    pub fn fhip_mesh_build(ctx: *mut fhip_ctx, tape: *const fhip_tape, depth: u32, world_to_model: *const f32, axis_slots: *const i32,
                           var_keys: *const u64, var_values: *const f32, n_vars: u32, out: *mut *mut fhip_mesh) -> fhip_status;
    pub fn fhip_mesh_counts(mesh: *const fhip_mesh, out: *mut u64);          // [6] vertices, [7] triangles
    pub fn fhip_mesh_vertices(mesh: *const fhip_mesh, out: *mut f32);
    pub fn fhip_mesh_triangles(mesh: *const fhip_mesh, out: *mut u64);
    pub fn fhip_mesh_vertices_ptr(mesh: *const fhip_mesh) -> *const f32;       // the arrays where the mesh holds them (valid until fhip_mesh_free)
    pub fn fhip_mesh_triangles_ptr(mesh: *const fhip_mesh) -> *const u64;
    pub fn fhip_mesh_free(mesh: *mut fhip_mesh);
    // the mesh where the device left it (context option "mesh_keep_device"), Mesh::write_stl and gradients at the vertices, on the device
    pub fn fhip_mesh_vertices_dev(mesh: *const fhip_mesh) -> *const f32;
    pub fn fhip_mesh_triangles_dev(mesh: *const fhip_mesh) -> *const u64;
    pub fn fhip_mesh_stl_bytes(mesh: *const fhip_mesh) -> u64;
    pub fn fhip_mesh_stl(ctx: *mut fhip_ctx, mesh: *const fhip_mesh, out: *mut c_void, out_is_device: c_int) -> fhip_status;
    pub fn fhip_mesh_vertex_grads(ctx: *mut fhip_ctx, tape: *const fhip_tape, mesh: *const fhip_mesh, axis_slots: *const i32,
                                  var_keys: *const u64, var_values: *const f32, n_vars: u32, out: *mut f32, out_is_device: c_int) -> fhip_status;
    // volume, centroid, second moments and bounds as exact integer sums; `out`: a `fhip_occupancy` (the header declares it void*)
    pub fn fhip_shape_occupancy(ctx: *mut fhip_ctx, tape: *const fhip_tape, depth: u32, world_to_model: *const f32, axis_slots: *const i32,
                                var_keys: *const u64, var_values: *const f32, n_vars: u32, out: *mut c_void) -> fhip_status;
    // the inside voxels as a bitmap of 4 x 4 x 4 bricks (one u64 each, `fhip_voxels_words(depth)` of them), layer images and voxels per layer
    pub fn fhip_voxels_words(depth: u32) -> u64;
    pub fn fhip_shape_voxels(ctx: *mut fhip_ctx, tape: *const fhip_tape, depth: u32, world_to_model: *const f32, axis_slots: *const i32,
                             var_keys: *const u64, var_values: *const f32, n_vars: u32, out: *mut u64, out_is_device: c_int,
                             cells: *mut u64) -> fhip_status;
    pub fn fhip_voxels_slices(ctx: *mut fhip_ctx, bricks: *const u64, depth: u32, k0: u32, k1: u32, out: *mut u8, on_device: c_int) -> fhip_status;
    pub fn fhip_voxels_layer_counts(ctx: *mut fhip_ctx, bricks: *const u64, depth: u32, out: *mut u64, on_device: c_int) -> fhip_status;
    // the outlines of a 2D slice (marching squares over the pixel-perfect render2d image); the handle - a `fhip_contours` - is void* in the header
    pub fn fhip_contour2d(ctx: *mut fhip_ctx, tape: *const fhip_tape, cfg: *const fhip_render2d_config, out: *mut *mut c_void) -> fhip_status;
    pub fn fhip_contours_counts(contours: *const c_void, out: *mut u64);         // vertices, segments, W, H
    pub fn fhip_contours_vertices(contours: *const c_void, out: *mut f32) -> fhip_status;
    pub fn fhip_contours_segments(contours: *const c_void, out: *mut u32) -> fhip_status;
    pub fn fhip_contours_next(contours: *const c_void, out: *mut u32) -> fhip_status;
    pub fn fhip_contours_vertices_dev(contours: *const c_void) -> *const f32;
    pub fn fhip_contours_segments_dev(contours: *const c_void) -> *const u32;
    pub fn fhip_contours_free(contours: *mut c_void);
    pub fn fhip_contour_loops(next: *const u32, n: u64, order: *mut u32, loop_start: *mut u64, closed: *mut u8, n_loops: *mut u64) -> fhip_status;
    // the connected parts of a voxel bitmap (6- or 26-connectivity, of the set or of the clear bits); the handle - a `fhip_components` - is void* in the header
    pub fn fhip_voxels_components(ctx: *mut fhip_ctx, bricks: *const u64, depth: u32, on_device: c_int, connectivity: u32, complement: c_int,
                                  out: *mut *mut c_void) -> fhip_status;
    pub fn fhip_components_counts(comps: *const c_void, out: *mut u64);         // components, nodes, foreground voxels, depth
    pub fn fhip_components_table(comps: *const c_void, size: *mut u64, seed: *mut u32, lo: *mut u32, hi: *mut u32, border: *mut u8) -> fhip_status;
    pub fn fhip_components_label_slices(ctx: *mut fhip_ctx, comps: *const c_void, bricks: *const u64, bricks_on_device: c_int, k0: u32, k1: u32,
                                        out: *mut i32, out_on_device: c_int) -> fhip_status;
    pub fn fhip_components_extract(ctx: *mut fhip_ctx, comps: *const c_void, bricks: *const u64, bricks_on_device: c_int, ids: *const u32, n_ids: u64,
                                   out: *mut u64, out_on_device: c_int) -> fhip_status;
    pub fn fhip_components_free(comps: *mut c_void);
    // the exact Euclidean distance transform of a voxel bitmap (squared distances, uint32); the handle - a `fhip_distance` - is void* in the header
    pub fn fhip_voxels_distance(ctx: *mut fhip_ctx, bricks: *const u64, depth: u32, on_device: c_int, complement: c_int, out: *mut *mut c_void) -> fhip_status;
    pub fn fhip_distance_info(dist: *const c_void, out: *mut u64);         // largest finite d2, its smallest index, foreground voxels, depth
    pub fn fhip_distance_slices(ctx: *mut fhip_ctx, dist: *const c_void, k0: u32, k1: u32, out: *mut u32, out_on_device: c_int) -> fhip_status;
    pub fn fhip_distance_dev(dist: *const c_void) -> *const u32;
    pub fn fhip_distance_threshold(ctx: *mut fhip_ctx, dist: *const c_void, t: u32, beyond: c_int, out_bricks: *mut u64, out_on_device: c_int) -> fhip_status;
    pub fn fhip_distance_free(dist: *mut c_void);
    // the local thickness of such a field: the result is a distance handle again, served by the functions above
    pub fn fhip_distance_thickness(ctx: *mut fhip_ctx, dist: *const c_void, out: *mut *mut c_void) -> fhip_status;
    pub fn fhip_thickness_info(thick: *const c_void, out: *mut u64);       // largest T, its index, smallest positive T, its index, voxels with T > 0, depth, centres, balls painted
    pub fn fhip_thickness_thin(ctx: *mut fhip_ctx, thick: *const c_void, t: u32, out_bricks: *mut u64, out_on_device: c_int) -> fhip_status;
    pub fn fhip_thickness_histogram(ctx: *mut fhip_ctx, thick: *const c_void, edges: *const u32, n_edges: u32, counts: *mut u64, on_device: c_int) -> fhip_status;
    // the boundary mesh of a voxel bitmap - a fhip_mesh like fhip_mesh_build's - and its surface summary {faces [6], V, E, F, n}
    pub fn fhip_voxels_surface(ctx: *mut fhip_ctx, bricks: *const u64, depth: u32, on_device: c_int, out: *mut u64) -> fhip_status;
    pub fn fhip_voxels_mesh(ctx: *mut fhip_ctx, bricks: *const u64, depth: u32, on_device: c_int, out: *mut *mut fhip_mesh) -> fhip_status;
    pub fn fhip_voxels_flow(ctx: *mut fhip_ctx, seeds: *const u64, blockers: *const u64, depth: u32, on_device: c_int, dir: u32, flags: u32, out: *mut u64, out_on_device: c_int) -> fhip_status;
    pub fn fhip_voxels_overhangs(ctx: *mut fhip_ctx, bricks: *const u64, depth: u32, on_device: c_int, up: u32, reach2: u32, bed: c_int, out: *mut u64, out_on_device: c_int) -> fhip_status;
    pub fn fhip_voxels_heights(ctx: *mut fhip_ctx, bricks: *const u64, depth: u32, on_device: c_int, axis: u32, out: *mut i32, out_on_device: c_int) -> fhip_status;
    // a triangle mesh to a voxel bitmap by parity along +x; info = {triangles, rejected, flat, crossings, clipped, open_rows, set voxels, W}
    pub fn fhip_triangles_voxels(ctx: *mut fhip_ctx, vertices: *const f32, n_vertices: u64, triangles: *const u64, n_triangles: u64, on_device: c_int,
                                 mesh_to_world: *const f64, depth: u32, out: *mut u64, out_on_device: c_int, info: *mut u64) -> fhip_status;
    pub fn fhip_mesh_voxels(ctx: *mut fhip_ctx, mesh: *const fhip_mesh, mesh_to_world: *const f64, depth: u32, out: *mut u64, out_on_device: c_int,
                            info: *mut u64) -> fhip_status;
    // the check of a triangle mesh: weld, edges, shells (the handle is a void* in the header)
    pub fn fhip_triangles_topology(ctx: *mut fhip_ctx, vertices: *const f32, n_vertices: u64, triangles: *const u64, n_triangles: u64, on_device: c_int,
                                   weld: c_int, table_log2: u32, out: *mut *mut c_void) -> fhip_status;
    pub fn fhip_mesh_topology(ctx: *mut fhip_ctx, mesh: *const fhip_mesh, weld: c_int, table_log2: u32, out: *mut *mut c_void) -> fhip_status;
    pub fn fhip_topology_counts(topo: *const c_void, out: *mut u64);
    pub fn fhip_topology_vertex_rows(topo: *const c_void) -> u64;
    pub fn fhip_topology_vertices(topo: *const c_void, out: *mut f32) -> fhip_status;
    pub fn fhip_topology_triangles(topo: *const c_void, out: *mut u64) -> fhip_status;
    pub fn fhip_topology_triangle_shells(topo: *const c_void, out: *mut u32) -> fhip_status;
    pub fn fhip_topology_vertices_dev(topo: *const c_void) -> *const f32;
    pub fn fhip_topology_triangles_dev(topo: *const c_void) -> *const u64;
    pub fn fhip_topology_triangle_shells_dev(topo: *const c_void) -> *const u32;
    pub fn fhip_topology_shells(topo: *const c_void, triangles: *mut u64, first: *mut u32, unbalanced: *mut u64, lo: *mut f32, hi: *mut f32, volume6: *mut f64,
                                area2: *mut f64) -> fhip_status;
    pub fn fhip_topology_edges(ctx: *mut fhip_ctx, topo: *const c_void, kind: u32, out: *mut u32, out_on_device: c_int) -> fhip_status;
    pub fn fhip_topology_free(topo: *mut c_void);
    // the outlines of a voxel bitmap's layers: vertices where the outline turns, their successors, the loops and their table
    pub fn fhip_voxels_outlines(ctx: *mut fhip_ctx, bricks: *const u64, depth: u32, on_device: c_int, k0: u32, k1: u32, connectivity: u32,
                                out: *mut *mut c_void) -> fhip_status;
    pub fn fhip_outlines_counts(outlines: *const c_void, out: *mut u64);
    pub fn fhip_outlines_layers(outlines: *const c_void, vertex_start: *mut u64, loop_start: *mut u64, area2: *mut i64, perimeter: *mut u64) -> fhip_status;
    pub fn fhip_outlines_vertices(outlines: *const c_void, first: u64, count: u64, xy: *mut u16, next: *mut u32, loop_of: *mut u32) -> fhip_status;
    pub fn fhip_outlines_loops(outlines: *const c_void, first: u64, count: u64, leader: *mut u32, n_vertices: *mut u32, area2: *mut i64, perimeter: *mut u64,
                               lo: *mut u16, hi: *mut u16) -> fhip_status;
    pub fn fhip_outlines_xy_dev(outlines: *const c_void) -> *const u16;
    pub fn fhip_outlines_next_dev(outlines: *const c_void) -> *const u32;
    pub fn fhip_outlines_loop_dev(outlines: *const c_void) -> *const u32;
    pub fn fhip_outlines_free(outlines: *mut c_void);
    // the nesting of those outlines: per loop its left neighbour, parent, depth, children and region sum; fhip_nesting_children is host code
    pub fn fhip_outlines_nesting(ctx: *mut fhip_ctx, outlines: *const c_void, bricks: *const u64, bricks_on_device: c_int, out: *mut *mut c_void) -> fhip_status;
    pub fn fhip_nesting_counts(nest: *const c_void, out: *mut u64);
    pub fn fhip_nesting_layers(nest: *const c_void, outer: *mut u64, top: *mut u64, max_depth: *mut u32) -> fhip_status;
    pub fn fhip_nesting_loops(nest: *const c_void, first: u64, count: u64, left: *mut u32, parent: *mut u32, depth: *mut u32, n_children: *mut u32,
                              region_area2: *mut i64) -> fhip_status;
    pub fn fhip_nesting_parent_dev(nest: *const c_void) -> *const u32;
    pub fn fhip_nesting_depth_dev(nest: *const c_void) -> *const u32;
    pub fn fhip_nesting_children(parent: *const u32, n: u64, child_start: *mut u64, children: *mut u32) -> fhip_status;
    pub fn fhip_nesting_free(nest: *mut c_void);
    // the slices of a checked mesh under planes z = const: crossings on the mesh's edges, their successors, the loops and their table
    pub fn fhip_topology_slices(ctx: *mut fhip_ctx, topology: *const c_void, zs: *const f32, n_planes: u32, table_log2: u32, out: *mut *mut c_void) -> fhip_status;
    pub fn fhip_slices_counts(slices: *const c_void, out: *mut u64);
    pub fn fhip_slices_planes(slices: *const c_void, zs: *mut f32, crossings: *mut u64, segments: *mut u64, loops: *mut u64) -> fhip_status;
    pub fn fhip_slices_loops(slices: *const c_void, leader: *mut u32, plane: *mut u32, crossings: *mut u32, segments: *mut u32, irregular: *mut u32, area2: *mut f64,
                             lo: *mut f32, hi: *mut f32) -> fhip_status;
    pub fn fhip_slices_vertices(slices: *const c_void, xy: *mut f32, plane: *mut u32, edge: *mut u32, next: *mut u32, loop_of: *mut u32, degree: *mut u8) -> fhip_status;
    pub fn fhip_slices_xy_dev(slices: *const c_void) -> *const f32;
    pub fn fhip_slices_next_dev(slices: *const c_void) -> *const u32;
    pub fn fhip_slices_loop_dev(slices: *const c_void) -> *const u32;
    pub fn fhip_slices_plane_dev(slices: *const c_void) -> *const u32;
    pub fn fhip_slices_free(slices: *mut c_void);
    // the nesting of those slices: per regular loop its parent, depth, children and region sum; children lists by fhip_nesting_children
    pub fn fhip_slices_nesting(ctx: *mut fhip_ctx, slices: *const c_void, bands: u32, out: *mut *mut c_void) -> fhip_status;
    pub fn fhip_slice_nesting_counts(nest: *const c_void, out: *mut u64);
    pub fn fhip_slice_nesting_planes(nest: *const c_void, regular: *mut u64, outer: *mut u64, top: *mut u64, max_depth: *mut u64, improper: *mut u64,
                                     misoriented: *mut u64, bands: *mut u32) -> fhip_status;
    pub fn fhip_slice_nesting_loops(nest: *const c_void, parent: *mut u32, depth: *mut u32, n_children: *mut u32, region_area2: *mut f64) -> fhip_status;
    pub fn fhip_slice_nesting_parent_dev(nest: *const c_void) -> *const u32;
    pub fn fhip_slice_nesting_depth_dev(nest: *const c_void) -> *const u32;
    pub fn fhip_slice_nesting_free(nest: *mut c_void);
    // the build sharded by the root's octants (Octree::build_inner_mt across GPUs): a part per process, merged in one
    pub fn fhip_mesh_sample_part(ctx: *mut fhip_ctx, tape: *const fhip_tape, depth: u32, world_to_model: *const f32, axis_slots: *const i32,
                                 var_keys: *const u64, var_values: *const f32, n_vars: u32, part: u32, n_parts: u32,
                                 out: *mut *mut fhip_mesh) -> fhip_status;
    pub fn fhip_mesh_part_bytes(mesh: *const fhip_mesh) -> u64;
    pub fn fhip_mesh_part_export(mesh: *const fhip_mesh, out: *mut c_void);
    pub fn fhip_mesh_merge(ctx: *mut fhip_ctx, parts: *const *const c_void, part_bytes: *const u64, n_parts: u32,
                           world_to_model: *const f32, out: *mut *mut fhip_mesh) -> fhip_status;
}
