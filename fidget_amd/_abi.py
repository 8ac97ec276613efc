"""The ctypes mirror of the C ABI (include/fidget_hip.h, include/fidget_hip_debug.h): the constants and structs the header names, the
signature of every entry point (`SIGNATURES`, one line each, in the header's order), the lazy loader `lib()`, and the small helpers
every subject's wrappers share.  Imports `_build` alone; loading the library waits for the first `lib()` call."""
import ctypes as C
import os

import numpy as np

from ._build import LIB_PATH

UNARY = ["neg", "abs", "recip", "sqrt", "square", "floor", "ceil", "round", "sin", "cos", "tan",
         "asin", "acos", "atan", "exp", "ln", "not", "rand"]          # context/op.rs:11-30
BINARY = ["add", "sub", "mul", "div", "atan2", "min", "max", "compare", "mod", "and", "or", "mix"]  # op.rs:35-48

FH_OPS = (["Output", "Input", "CopyReg", "CopyImm"] + [u.capitalize() for u in UNARY]
          + [b.capitalize() + "RR" for b in ["add", "sub", "mul", "div", "atan2", "compare", "mix", "mod", "min", "max", "and", "or"]]
          + [b.capitalize() + "RI" for b in ["add", "sub", "mul", "div", "atan2", "compare", "mix", "mod", "min", "max", "and", "or"]]
          + [b.capitalize() + "IR" for b in ["sub", "div", "atan2", "compare", "mix", "mod"]])

STATUS = {1: "BadVarSlice", 2: "MismatchedSlices", 3: "BadChoiceSlice", 4: "MissingVar", 5: "BadTape",
          6: "Unsupported", 7: "HipError", 8: "Cancelled", 9: "ParseError", 10: "Overflow"}

GEOMETRY_PIXEL = np.dtype([("normal", np.float32, 3), ("depth", np.uint32)])
# RenderHints of the HIP shape (capi.hip): 2D 128 / 16 as fidget-jit, 3D 128 / 32 / 8; the VM shape's for comparison
HIP_TILES_2D, HIP_TILES_3D = [128, 16], [128, 32, 8]
VM_TILES_2D, VM_TILES_3D = [128, 32, 8], [128, 64, 32, 16, 8]


class FidgetHipError(RuntimeError):
    def __init__(self, status, msg=""):
        self.status = status
        super().__init__(f"{STATUS.get(status, status)}: {msg}")


class _Cfg2D(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("world_to_model", C.c_void_p), ("z", C.c_float),
                ("pixel_perfect", C.c_int), ("tile_sizes", C.c_void_p), ("n_tile_sizes", C.c_uint32),
                ("var_keys", C.c_void_p), ("var_values", C.c_void_p), ("n_vars", C.c_uint32),
                ("axis_slots", C.c_void_p)]


class _Cfg3D(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("depth", C.c_uint32), ("world_to_model", C.c_void_p),
                ("tile_sizes", C.c_void_p), ("n_tile_sizes", C.c_uint32), ("var_keys", C.c_void_p),
                ("var_values", C.c_void_p), ("n_vars", C.c_uint32), ("axis_slots", C.c_void_p)]


vp, u32, i32, f32, u64 = C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_uint64
# name: (restype, argtypes) of every function the two headers declare, grouped as they are; EXPORTS and lib() are made of it, and
# tests/test_python_package.py holds the argument counts and the void returns against the headers
SIGNATURES = {
    # ---- context
    "fhip_ctx_create": (i32, [i32, vp, C.POINTER(vp)]),
    "fhip_ctx_destroy": (None, [vp]),
    "fhip_last_error": (C.c_char_p, [vp]),
    "fhip_ctx_sync": (i32, [vp]),
    "fhip_ctx_trim": (i32, [vp]),
    "fhip_ctx_reserve_arena": (i32, [vp, C.c_size_t]),
    "fhip_libm_probe": (i32, [C.c_char_p, C.c_size_t]),
    "fhip_cancel": (None, [vp]),
    "fhip_cancel_reset": (None, [vp]),
    "fhip_cancel_watch": (None, [vp, vp]),
    "fhip_ctx_set_option": (i32, [vp, C.c_char_p, i32]),
    "fhip_ctx_get_option": (i32, [vp, C.c_char_p, C.POINTER(i32)]),
    # ---- tapes
    "fhip_tape_from_bytecode": (i32, [vp, vp, C.c_size_t, C.POINTER(vp)]),
    "fhip_tape_free": (None, [vp]),
    "fhip_tape_len": (u32, [vp]),
    "fhip_tape_choice_count": (u32, [vp]),
    "fhip_tape_reg_count": (u32, [vp]),
    "fhip_tape_var_count": (u32, [vp]),
    "fhip_tape_output_count": (u32, [vp]),
    "fhip_tape_ops": (u32, [vp, vp, u32]),
    "fhip_tape_reg_tape": (i32, [vp, u32, vp, u32, vp, u32, vp]),
    "fhip_tape_group_count": (u32, [vp]),
    "fhip_tape_group_op": (i32, [vp]),
    "fhip_tape_group": (i32, [vp, vp, u32, vp]),
    "fhip_tape_term_plan": (u32, [vp, vp]),
    "fhip_tape_term_group": (i32, [vp, vp, u32, vp]),
    "fhip_tape_term_tree": (u32, [vp, vp, u32]),
    "fhip_tape_term_choice_src": (u32, [vp, vp, u32]),
    "fhip_simplify": (i32, [vp, vp, vp, u32, C.POINTER(vp)]),
    # ---- evaluators (trait surface; batched over n samples)
    "fhip_interval_eval": (i32, [vp, vp, vp, u32, u32, vp, vp, vp]),
    "fhip_point_eval": (i32, [vp, vp, vp, u32, u32, vp, vp, vp]),
    "fhip_float_eval": (i32, [vp, vp, vp, vp, u32, vp]),
    "fhip_grad_eval": (i32, [vp, vp, vp, vp, u32, vp]),
    # ---- constraint solver
    "fhip_solve": (i32, [vp, vp, u32, vp, vp, vp, u32, vp, u32, u32, vp, vp, vp, vp]),
    # ---- batched renders (the throughput path)
    "fhip_render2d": (i32, [vp, vp, C.POINTER(_Cfg2D), vp, i32]),
    "fhip_render3d": (i32, [vp, vp, C.POINTER(_Cfg3D), vp, i32]),
    "fhip_render3d_shard": (i32, [vp, vp, C.POINTER(_Cfg3D), vp, i32, u32, u32]),
    "fhip_render3d_block": (i32, [vp, vp, C.POINTER(_Cfg3D), vp, i32, u32, vp]),
    "fhip_merge_depth": (i32, [vp, vp, vp, u64, u32]),
    # ---- post-processing: fidget_raster::effects (fidget-raster/src/effects.rs)
    "fhip_denoise_normals": (i32, [vp, vp, u32, u32, vp, i32]),
    "fhip_compute_ssao": (i32, [vp, vp, u32, u32, u32, vp, u32, vp, u32, vp, i32]),
    "fhip_blur_ssao": (i32, [vp, vp, u32, u32, vp, i32]),
    "fhip_apply_shading": (i32, [vp, vp, u32, u32, u32, vp, vp, i32]),
    "fhip_to_rgba": (i32, [vp, vp, u32, u32, i32, vp, i32]),
    # ---- meshing: the evaluation side of fidget_mesh::Octree::build (fidget-mesh/src/octree.rs)
    "fhip_mesh_sample": (i32, [vp, vp, u32, vp, vp, vp, vp, u32, C.POINTER(vp)]),
    "fhip_mesh_build": (i32, [vp, vp, u32, vp, vp, vp, vp, u32, C.POINTER(vp)]),
    "fhip_mesh_vertices": (None, [vp, vp]),
    "fhip_mesh_triangles": (None, [vp, vp]),
    "fhip_mesh_vertices_ptr": (vp, [vp]),
    "fhip_mesh_triangles_ptr": (vp, [vp]),
    "fhip_mesh_free": (None, [vp]),
    "fhip_mesh_counts": (None, [vp, vp]),
    "fhip_mesh_leaves": (None, [vp, vp]),
    "fhip_mesh_sample_part": (i32, [vp, vp, u32, vp, vp, vp, vp, u32, u32, u32, C.POINTER(vp)]),
    "fhip_mesh_part_bytes": (C.c_uint64, [vp]),
    "fhip_mesh_part_export": (None, [vp, vp]),
    "fhip_mesh_merge": (i32, [vp, vp, vp, u32, vp, C.POINTER(vp)]),
    "fhip_mesh_vertices_dev": (vp, [vp]),
    "fhip_mesh_triangles_dev": (vp, [vp]),
    "fhip_mesh_stl_bytes": (u64, [vp]),
    "fhip_mesh_stl": (i32, [vp, vp, vp, i32]),
    "fhip_mesh_vertex_grads": (i32, [vp, vp, vp, vp, vp, vp, u32, vp, i32]),
    # ---- shape occupancy: volume, centroid, second moments and bounds of a solid, as exact integer sums
    "fhip_shape_occupancy": (i32, [vp, vp, u32, vp, vp, vp, vp, u32, vp]),
    # ---- shape voxels: the inside voxels themselves, as a packed bitmap, and what is made of one
    "fhip_voxels_words": (u64, [u32]),
    "fhip_shape_voxels": (i32, [vp, vp, u32, vp, vp, vp, vp, u32, vp, i32, vp]),
    "fhip_voxels_slices": (i32, [vp, vp, u32, u32, u32, vp, i32]),
    "fhip_voxels_layer_counts": (i32, [vp, vp, u32, vp, i32]),
    # ---- contours of a 2D slice: the outlines of the shape's cross-section at cfg->z, by marching squares
    "fhip_contour2d": (i32, [vp, vp, vp, vp]),
    "fhip_contours_counts": (None, [vp, vp]),
    "fhip_contours_vertices": (i32, [vp, vp]),
    "fhip_contours_segments": (i32, [vp, vp]),
    "fhip_contours_next": (i32, [vp, vp]),
    "fhip_contours_vertices_dev": (vp, [vp]),
    "fhip_contours_segments_dev": (vp, [vp]),
    "fhip_contours_free": (None, [vp]),
    "fhip_contour_loops": (i32, [vp, u64, vp, vp, vp, vp]),
    # ---- connected components of a voxel bitmap: is the solid one body or several, does it enclose voids
    "fhip_voxels_components": (i32, [vp, vp, u32, i32, u32, i32, vp]),
    "fhip_components_counts": (None, [vp, vp]),
    "fhip_components_table": (i32, [vp, vp, vp, vp, vp, vp]),
    "fhip_components_label_slices": (i32, [vp, vp, vp, i32, u32, u32, vp, i32]),
    "fhip_components_extract": (i32, [vp, vp, vp, i32, vp, u64, vp, i32]),
    "fhip_components_free": (None, [vp]),
    # ---- exact Euclidean distance transform of a voxel bitmap: how far, in voxels, from the nearest foreground voxel
    "fhip_voxels_distance": (i32, [vp, vp, u32, i32, i32, vp]),
    "fhip_distance_info": (None, [vp, vp]),
    "fhip_distance_slices": (i32, [vp, vp, u32, u32, vp, i32]),
    "fhip_distance_dev": (vp, [vp]),
    "fhip_distance_threshold": (i32, [vp, vp, u32, i32, vp, i32]),
    "fhip_distance_free": (None, [vp]),
    # ---- local thickness of a distance field: per voxel the largest ball that fits and holds it
    "fhip_distance_thickness": (i32, [vp, vp, vp]),
    "fhip_thickness_info": (None, [vp, vp]),
    "fhip_thickness_thin": (i32, [vp, vp, u32, vp, i32]),
    "fhip_thickness_histogram": (i32, [vp, vp, vp, u32, vp, i32]),
    # ---- boundary mesh of a voxel bitmap: the solid's faces as triangles, its surface area, its Euler number
    "fhip_voxels_surface": (i32, [vp, vp, u32, i32, vp]),
    "fhip_voxels_mesh": (i32, [vp, vp, u32, i32, vp]),
    # ---- a voxel bitmap along a direction: shadows, overhangs, supports, heights
    "fhip_voxels_flow": (i32, [vp, vp, vp, u32, i32, u32, u32, vp, i32]),
    "fhip_voxels_overhangs": (i32, [vp, vp, u32, i32, u32, u32, i32, vp, i32]),
    "fhip_voxels_heights": (i32, [vp, vp, u32, i32, u32, vp, i32]),
    # ---- a triangle mesh to a voxel bitmap: solid voxelization by parity along +x
    "fhip_triangles_voxels": (i32, [vp, vp, u64, vp, u64, i32, vp, u32, vp, i32, vp]),
    "fhip_mesh_voxels": (i32, [vp, vp, vp, u32, vp, i32, vp]),
    # ---- the check of a triangle mesh: weld, edges, shells, volume
    "fhip_triangles_topology": (i32, [vp, vp, u64, vp, u64, i32, i32, u32, vp]),
    "fhip_mesh_topology": (i32, [vp, vp, i32, u32, vp]),
    "fhip_topology_counts": (None, [vp, vp]),
    "fhip_topology_vertex_rows": (u64, [vp]),
    "fhip_topology_vertices": (i32, [vp, vp]),
    "fhip_topology_triangles": (i32, [vp, vp]),
    "fhip_topology_triangle_shells": (i32, [vp, vp]),
    "fhip_topology_vertices_dev": (vp, [vp]),
    "fhip_topology_triangles_dev": (vp, [vp]),
    "fhip_topology_triangle_shells_dev": (vp, [vp]),
    "fhip_topology_shells": (i32, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "fhip_topology_edges": (i32, [vp, vp, u32, vp, i32]),
    "fhip_topology_free": (None, [vp]),
    # ---- the outlines of a voxel bitmap's layers: closed rectilinear loops per layer
    "fhip_voxels_outlines": (i32, [vp, vp, u32, i32, u32, u32, u32, vp]),
    "fhip_outlines_counts": (None, [vp, vp]),
    "fhip_outlines_layers": (i32, [vp, vp, vp, vp, vp]),
    "fhip_outlines_vertices": (i32, [vp, u64, u64, vp, vp, vp]),
    "fhip_outlines_loops": (i32, [vp, u64, u64, vp, vp, vp, vp, vp, vp]),
    "fhip_outlines_xy_dev": (vp, [vp]),
    "fhip_outlines_next_dev": (vp, [vp]),
    "fhip_outlines_loop_dev": (vp, [vp]),
    "fhip_outlines_free": (None, [vp]),
    # ---- the nesting of those outlines: left links, parents, depths, regions
    "fhip_outlines_nesting": (i32, [vp, vp, vp, i32, vp]),
    "fhip_nesting_counts": (None, [vp, vp]),
    "fhip_nesting_layers": (i32, [vp, vp, vp, vp]),
    "fhip_nesting_loops": (i32, [vp, u64, u64, vp, vp, vp, vp, vp]),
    "fhip_nesting_parent_dev": (vp, [vp]),
    "fhip_nesting_depth_dev": (vp, [vp]),
    "fhip_nesting_children": (i32, [vp, u64, vp, vp]),
    "fhip_nesting_free": (None, [vp]),
    # ---- the slices of a triangle mesh: closed contour loops per plane z = const
    "fhip_topology_slices": (i32, [vp, vp, vp, u32, u32, vp]),
    "fhip_slices_counts": (None, [vp, vp]),
    "fhip_slices_planes": (i32, [vp, vp, vp, vp, vp]),
    "fhip_slices_loops": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "fhip_slices_vertices": (i32, [vp, vp, vp, vp, vp, vp, vp]),
    "fhip_slices_xy_dev": (vp, [vp]),
    "fhip_slices_next_dev": (vp, [vp]),
    "fhip_slices_loop_dev": (vp, [vp]),
    "fhip_slices_plane_dev": (vp, [vp]),
    "fhip_slices_free": (None, [vp]),
    # ---- the nesting of those slices: polygons with holes per plane
    "fhip_slices_nesting": (i32, [vp, vp, u32, vp]),
    "fhip_slice_nesting_counts": (None, [vp, vp]),
    "fhip_slice_nesting_planes": (i32, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "fhip_slice_nesting_loops": (i32, [vp, vp, vp, vp, vp]),
    "fhip_slice_nesting_parent_dev": (vp, [vp]),
    "fhip_slice_nesting_depth_dev": (vp, [vp]),
    "fhip_slice_nesting_free": (None, [vp]),
    # ---- profiling
    "fhip_profile_enable": (None, [vp, i32]),
    "fhip_profile_read": (i32, [vp, vp, vp]),
    "fhip_profile_read_kernels": (i32, [vp, vp, vp]),
    "fhip_render_counters": (i32, [vp, vp]),
    # ---- host mirror of fidget_core::Context (no Rust toolchain here; tests + demos)
    "fhip_graph_new": (vp, []),
    "fhip_graph_free": (None, [vp]),
    "fhip_graph_len": (u32, [vp]),
    "fhip_graph_var": (u32, [vp, i32, u64]),
    "fhip_graph_constant": (u32, [vp, f32]),
    "fhip_graph_unary": (u32, [vp, i32, u32]),
    "fhip_graph_binary": (u32, [vp, i32, u32, u32]),
    "fhip_graph_from_text": (u32, [vp, C.c_char_p]),
    "fhip_tape_from_graph": (i32, [vp, vp, vp, u32, C.POINTER(vp)]),
    "fhip_tape_axis_slot": (i32, [vp, i32]),
    "fhip_tape_var_slot": (i32, [vp, u64]),
    "fhip_screen_to_world": (None, [vp, i32, vp]),
    # ---- include/fidget_hip_debug.h
    "fhip_debug_stats": (i32, [vp, vp]),
    "fhip_debug_leaf_stats": (i32, [vp, vp]),
    "fhip_debug_tape_links": (u32, [vp, vp, u32]),
    "fhip_debug_tape_chain": (u32, [vp, vp, u32]),
    "fhip_debug_leaves": (u32, [vp, vp, u32]),
    "fhip_debug_probe": (i32, [vp, vp]),
    "fhip_debug_lane_frames": (u64, [vp]),
    "fhip_debug_rare_frames": (u64, [vp]),
    "fhip_debug_rare_launches": (u64, [vp]),
    "fhip_debug_lane_tune": (i32, [vp, vp, vp]),
    "fhip_debug_trans_probe": (i32, [vp, u32, u32, u32, u64, vp]),
    "fhip_debug_arena": (u32, [vp, u32, u32, vp]),
    "fhip_debug_bound_tape": (i32, [vp, vp, vp, vp, vp, u32, C.POINTER(vp)]),
    "fhip_debug_bench": (i32, [vp, vp, u32, u32, i32, vp]),
    "fhip_debug_ubench": (i32, [vp, u32, u32, u32, vp]),
    "fhip_debug_math_sweep": (i32, [vp, i32, u32, u32, u64, vp, vp]),
    "fhip_debug_groups": (u32, [vp, i32, u32, vp, u32, vp]),
    "fhip_debug_walk_dual": (None, [vp, u64, vp, vp, u64, i32, vp, vp, vp]),
    "fhip_debug_stl_pack": (i32, [vp, vp, u64, vp, u64, vp]),
}
del vp, u32, i32, f32, u64
EXPORTS = list(SIGNATURES)

_lib = None


def lib():
    """Load the HIP extension; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def libm_probe():
    """fhip_libm_probe: (number of probe arguments on which this host's libm differs from the routines the device restates, the first
    difference by name or "")"""
    buf = C.create_string_buffer(200)
    n = lib().fhip_libm_probe(buf, 200)
    return int(n), buf.value.decode()


class _Handle:
    """owner of one of the library's handles (a mesh, contours, components, a distance field, a topology, outlines), whose arrays the
    views and the later calls borrow: `.h`, freed with `free` when the last of them lets go"""
    def __init__(self, h, free):
        self.h = h
        self._free = free      # (held here: at interpreter shutdown the module's globals may be gone before the last view)

    def __del__(self):
        if self.h and self._free is not None:
            self._free(self.h)
            self.h = None


class _DeviceArray:
    """An array of a mesh in device memory, as `__cuda_array_interface__` (version 2) describes it; keeps the mesh's handle alive.
    The interface's read-only flag is False - torch refuses a read-only one - but the array is the mesh's: a consumer reads it."""
    def __init__(self, owner, ptr, shape, typestr):
        self._owner = owner
        self.ptr, self.shape = int(ptr), tuple(shape)
        self.__cuda_array_interface__ = {"shape": self.shape, "typestr": typestr, "data": (self.ptr, False), "version": 2, "strides": None}
