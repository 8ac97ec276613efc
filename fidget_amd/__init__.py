"""fidget_amd — Python binding of libfidget_hip.so (the MI355X / gfx950 backend).

Host-side mirror of the reference's user-facing surface for the evaluation hot path:

    reference (Rust)                                this module
    ---------------------------------------------   ------------------------------
    fidget_core::Context (+ from_text)              Context
    Shape<F> / F: Function + MathFunction           Shape (one device tape; simplify())
    TracingEvaluator / BulkEvaluator impls          Shape.eval_interval / eval_point /
                                                    eval_float_slice / eval_grad_slice
    fidget_raster::pixel::render / voxel::render    render2d / render3d

Everything that computes goes through the C ABI in include/fidget_hip.h (ctypes);
there is NO CPU fallback: importing works without a GPU (so the build and symbol
checks run anywhere), but creating a context without a HIP device raises.
"""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("FHIP_LIB") or os.path.join(_CSRC, "libfidget_hip.so")     # (FHIP_LIB: a variant build, tools/build_lib_variant.py - A/B runs)
_SOURCES = ["capi.hip", "capi_core.hpp", "capi_context.hpp", "capi_tapes.hpp", "capi_eval.hpp", "capi_bound.hpp", "capi_render.hpp", "frame_plan.hpp", "frame_schedule.hpp", "capi_effects.hpp", "capi_mesh.hpp", "capi_mesh_util.hpp", "capi_voxels.hpp", "capi_contour.hpp", "capi_cc.hpp", "capi_debug.hpp", "capi_solve.hpp", "solve.hip", "solve_lm.hpp", "kernels.hip", "prune2.hip", "effects.hip", "mesh.hip", "mesh_qef.hpp", "mesh_collapse.hpp", "mesh_edges.hpp", "mesh_walk.hpp", "mesh_split.hpp", "mesh_vox.hpp", "mesh_cc.hpp", "mesh_edt.hpp", "edt.hip", "capi_edt.hpp", "mesh_thick.hpp", "thick.hip", "capi_thick.hpp", "mesh_vmesh.hpp", "vmesh.hip", "capi_vmesh.hpp", "mesh_flow.hpp", "flow.hip", "capi_flow.hpp", "mesh_trivox.hpp", "trivox.hip", "capi_trivox.hpp", "mesh_topo.hpp", "topo.hip", "capi_topo.hpp", "mesh_outline.hpp", "outline.hip", "capi_outline.hpp", "mesh_slice.hpp", "slice.hip", "capi_slice.hpp", "contour/contour.hpp", "host_mesh.hpp", "dev_ops.hpp", "host_graph.hpp", "host_regtape.hpp", "render_state.h", "tape_format.h",
            "gen_interp.py", "gen_tiles.py", "gen_tilesv.py", "gen_normals.py", "gen_prune.py", "gen_ubench.py", "gen_trans.py", "trans_funcs.hip", "trans_libm.hpp", "offsets.cpp", "../../include/fidget_hip.h",
            "../../include/fidget_hip_debug.h"]

UNARY = ["neg", "abs", "recip", "sqrt", "square", "floor", "ceil", "round", "sin", "cos", "tan",
         "asin", "acos", "atan", "exp", "ln", "not", "rand"]          # context/op.rs:11-30
BINARY = ["add", "sub", "mul", "div", "atan2", "min", "max", "compare", "mod", "and", "or", "mix"]  # op.rs:35-48

FH_OPS = (["Output", "Input", "CopyReg", "CopyImm"] + [u.capitalize() for u in UNARY]
          + [b.capitalize() + "RR" for b in ["add", "sub", "mul", "div", "atan2", "compare", "mix", "mod", "min", "max", "and", "or"]]
          + [b.capitalize() + "RI" for b in ["add", "sub", "mul", "div", "atan2", "compare", "mix", "mod", "min", "max", "and", "or"]]
          + [b.capitalize() + "IR" for b in ["sub", "div", "atan2", "compare", "mix", "mod"]])

STATUS = {1: "BadVarSlice", 2: "MismatchedSlices", 3: "BadChoiceSlice", 4: "MissingVar", 5: "BadTape",
          6: "Unsupported", 7: "HipError", 8: "Cancelled", 9: "ParseError", 10: "Overflow"}

VM_TILES_3D = [128, 64, 32, 16, 8]
VM_TILES_2D = [128, 32, 8]
GEOMETRY_PIXEL = np.dtype([("normal", np.float32, 3), ("depth", np.uint32)])
# RenderHints of the HIP shape (capi.hip): 2D 128 / 16 as fidget-jit, 3D 128 / 32 / 8; the VM shape's for comparison
HIP_TILES_2D, HIP_TILES_3D = [128, 16], [128, 32, 8]
VM_TILES_2D, VM_TILES_3D = [128, 32, 8], [128, 64, 32, 16, 8]

EXPORTS = [
    "fhip_ctx_create", "fhip_ctx_destroy", "fhip_ctx_trim", "fhip_ctx_reserve_arena", "fhip_libm_probe", "fhip_last_error", "fhip_ctx_sync", "fhip_cancel", "fhip_cancel_reset", "fhip_cancel_watch", "fhip_ctx_set_option", "fhip_ctx_get_option",
    "fhip_tape_from_bytecode", "fhip_tape_free", "fhip_tape_len", "fhip_tape_reg_tape", "fhip_tape_choice_count", "fhip_tape_reg_count",
    "fhip_tape_var_count", "fhip_tape_output_count", "fhip_tape_ops", "fhip_simplify", "fhip_interval_eval",
    "fhip_point_eval", "fhip_float_eval", "fhip_grad_eval", "fhip_solve", "fhip_render2d", "fhip_render3d", "fhip_render3d_shard", "fhip_render3d_block", "fhip_merge_depth", "fhip_denoise_normals", "fhip_compute_ssao", "fhip_blur_ssao", "fhip_apply_shading", "fhip_to_rgba", "fhip_mesh_sample", "fhip_mesh_build", "fhip_mesh_vertices", "fhip_mesh_triangles", "fhip_mesh_vertices_ptr", "fhip_mesh_triangles_ptr", "fhip_mesh_free", "fhip_mesh_counts", "fhip_mesh_leaves", "fhip_mesh_sample_part", "fhip_mesh_part_bytes", "fhip_mesh_part_export", "fhip_mesh_merge", "fhip_mesh_vertices_dev", "fhip_mesh_triangles_dev", "fhip_mesh_stl_bytes", "fhip_mesh_stl", "fhip_mesh_vertex_grads", "fhip_shape_occupancy", "fhip_voxels_words", "fhip_shape_voxels", "fhip_voxels_slices", "fhip_voxels_layer_counts",
    "fhip_contour2d", "fhip_contours_counts", "fhip_contours_vertices", "fhip_contours_segments", "fhip_contours_next", "fhip_contours_vertices_dev", "fhip_contours_segments_dev", "fhip_contours_free", "fhip_contour_loops",
    "fhip_voxels_components", "fhip_components_counts", "fhip_components_table", "fhip_components_label_slices", "fhip_components_extract", "fhip_components_free",
    "fhip_voxels_distance", "fhip_distance_info", "fhip_distance_slices", "fhip_distance_dev", "fhip_distance_threshold", "fhip_distance_free",
    "fhip_distance_thickness", "fhip_thickness_info", "fhip_thickness_thin", "fhip_thickness_histogram",
    "fhip_voxels_surface", "fhip_voxels_mesh",
    "fhip_voxels_flow", "fhip_voxels_overhangs", "fhip_voxels_heights",
    "fhip_triangles_voxels", "fhip_mesh_voxels",
    "fhip_triangles_topology", "fhip_mesh_topology", "fhip_topology_counts", "fhip_topology_vertex_rows", "fhip_topology_vertices", "fhip_topology_triangles", "fhip_topology_triangle_shells",
    "fhip_topology_vertices_dev", "fhip_topology_triangles_dev", "fhip_topology_triangle_shells_dev", "fhip_topology_shells", "fhip_topology_edges", "fhip_topology_free",
    "fhip_voxels_outlines", "fhip_outlines_counts", "fhip_outlines_layers", "fhip_outlines_vertices", "fhip_outlines_loops", "fhip_outlines_xy_dev", "fhip_outlines_next_dev",
    "fhip_outlines_loop_dev", "fhip_outlines_free",
    "fhip_topology_slices", "fhip_slices_counts", "fhip_slices_planes", "fhip_slices_loops", "fhip_slices_vertices", "fhip_slices_xy_dev", "fhip_slices_next_dev", "fhip_slices_loop_dev",
    "fhip_slices_plane_dev", "fhip_slices_free",
    "fhip_profile_enable", "fhip_profile_read", "fhip_profile_read_kernels", "fhip_render_counters", "fhip_graph_new", "fhip_graph_free",
    "fhip_graph_len", "fhip_graph_var", "fhip_graph_constant", "fhip_graph_unary", "fhip_graph_binary",
    "fhip_graph_from_text", "fhip_tape_from_graph", "fhip_tape_axis_slot", "fhip_tape_var_slot",
    "fhip_screen_to_world", "fhip_debug_groups", "fhip_debug_ubench", "fhip_debug_math_sweep", "fhip_debug_stats", "fhip_debug_leaf_stats", "fhip_debug_tape_links", "fhip_debug_tape_chain", "fhip_debug_bench", "fhip_debug_leaves", "fhip_debug_arena", "fhip_debug_probe", "fhip_debug_trans_probe", "fhip_debug_bound_tape", "fhip_debug_lane_frames", "fhip_debug_rare_frames", "fhip_debug_lane_tune", "fhip_debug_walk_dual", "fhip_debug_stl_pack", "fhip_tape_group_count", "fhip_tape_group_op",
    "fhip_tape_group", "fhip_tape_term_plan", "fhip_tape_term_group", "fhip_tape_term_tree", "fhip_tape_term_choice_src",
]


class FidgetHipError(RuntimeError):
    def __init__(self, status, msg=""):
        self.status = status
        super().__init__(f"{STATUS.get(status, status)}: {msg}")


def build(force=False, verbose=False):
    """Compile libfidget_hip.so for gfx950 (cross-compiles without a GPU): the assembly
    interpreters (gen_interp.py -> .s -> code object, embedded in the library) and the HIP
    kernels + C ABI (capi.hip)."""
    srcs = [os.path.join(_CSRC, s) for s in _SOURCES]
    if os.environ.get("FHIP_LIB"):
        return LIB_PATH         # (a variant built elsewhere: never rebuilt from here)
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(s) <= os.path.getmtime(LIB_PATH) for s in srcs):
        return LIB_PATH
    gen = os.path.join(_CSRC, "_gen")
    os.makedirs(gen, exist_ok=True)
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
    co = os.path.join(gen, "interp_gfx950.co")

    def run(cmd, **kw):
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd, **kw)

    run(["g++", "-std=c++17", "-I", _CSRC, os.path.join(_CSRC, "offsets.cpp"), "-o", os.path.join(gen, "offsets")])
    with open(os.path.join(gen, "offsets.json"), "w") as f:
        subprocess.check_call([os.path.join(gen, "offsets")], stdout=f)
    # the transcendental routines the assembly interpreters call: trans_funcs.hip through LLVM IR, where the functions are limited to
    # 8 scalar registers + vcc / the return address ("amdgpu-num-sgpr": clang takes that attribute on kernels only; the handlers
    # that call them have ten free) -> llc -> assembly, embedded by gen_trans.py
    ll = os.path.join(gen, "trans_funcs.ll")
    run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "-emit-llvm", "--cuda-device-only", "-I", _CSRC,
         "-o", ll, os.path.join(_CSRC, "trans_funcs.hip")])
    ir = open(ll).read()
    groups = set()
    for fn in ("fh_t_sin", "fh_t_atan2", "fh_t_mod", "fh_t_sin4", "fh_t_ln4"):
        m = re.search(rf"^define [^\n]*@{fn}\([^\n]*\) (#\d+)", ir, re.M)
        assert m, f"trans_funcs.ll: {fn} not found"
        groups.add(m.group(1))
    for g in groups:
        ir, n = re.subn(rf"^attributes {g} = {{ ", f'attributes {g} = {{ "amdgpu-num-sgpr"="18" ', ir, flags=re.M)
        assert n == 1
    with open(ll, "w") as f:
        f.write(ir)
    run([os.path.join(llvm, "llc"), "-mtriple=amdgcn-amd-amdhsa", "-mcpu=gfx950", "-O3", "-o", os.path.join(gen, "trans_funcs.s"), ll])
    run([sys.executable, os.path.join(_CSRC, "gen_interp.py"), os.path.join(gen, "offsets.json"),
         os.path.join(gen, "interp_gfx950.s"), os.path.join(gen, "trans_funcs.s")])
    run([os.path.join(llvm, "clang"), "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950", "-c",
         os.path.join(gen, "interp_gfx950.s"), "-o", os.path.join(gen, "interp_gfx950.o")])
    run([os.path.join(llvm, "ld.lld"), "-shared", os.path.join(gen, "interp_gfx950.o"), "-o", co])
    run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
         f'-DFH_INTERP_CO="{co}"', "-o", LIB_PATH, os.path.join(_CSRC, "capi.hip")])
    return LIB_PATH


class _Cfg2D(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("world_to_model", C.c_void_p), ("z", C.c_float),
                ("pixel_perfect", C.c_int), ("tile_sizes", C.c_void_p), ("n_tile_sizes", C.c_uint32),
                ("var_keys", C.c_void_p), ("var_values", C.c_void_p), ("n_vars", C.c_uint32),
                ("axis_slots", C.c_void_p)]


class _Cfg3D(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("depth", C.c_uint32), ("world_to_model", C.c_void_p),
                ("tile_sizes", C.c_void_p), ("n_tile_sizes", C.c_uint32), ("var_keys", C.c_void_p),
                ("var_values", C.c_void_p), ("n_vars", C.c_uint32), ("axis_slots", C.c_void_p)]


_lib = None


def lib():
    """Load the HIP extension; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        vp, u32, i32, f32, u64 = C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_uint64
        sig = {
            "fhip_ctx_create": (i32, [i32, vp, C.POINTER(vp)]), "fhip_ctx_destroy": (None, [vp]),
            "fhip_libm_probe": (i32, [C.c_char_p, C.c_size_t]), "fhip_ctx_trim": (i32, [vp]), "fhip_ctx_reserve_arena": (i32, [vp, C.c_size_t]),
            "fhip_last_error": (C.c_char_p, [vp]), "fhip_ctx_sync": (i32, [vp]),
            "fhip_cancel": (None, [vp]), "fhip_cancel_reset": (None, [vp]), "fhip_cancel_watch": (None, [vp, vp]),
            "fhip_ctx_set_option": (i32, [vp, C.c_char_p, i32]), "fhip_ctx_get_option": (i32, [vp, C.c_char_p, C.POINTER(i32)]),
            "fhip_tape_from_bytecode": (i32, [vp, vp, C.c_size_t, C.POINTER(vp)]), "fhip_tape_free": (None, [vp]),
            "fhip_tape_len": (u32, [vp]), "fhip_tape_reg_tape": (i32, [vp, u32, vp, u32, vp, u32, vp]), "fhip_tape_choice_count": (u32, [vp]), "fhip_tape_reg_count": (u32, [vp]),
            "fhip_tape_var_count": (u32, [vp]), "fhip_tape_output_count": (u32, [vp]),
            "fhip_tape_ops": (u32, [vp, vp, u32]),
            "fhip_simplify": (i32, [vp, vp, vp, u32, C.POINTER(vp)]),
            "fhip_interval_eval": (i32, [vp, vp, vp, u32, u32, vp, vp, vp]),
            "fhip_point_eval": (i32, [vp, vp, vp, u32, u32, vp, vp, vp]),
            "fhip_float_eval": (i32, [vp, vp, vp, vp, u32, vp]),
            "fhip_grad_eval": (i32, [vp, vp, vp, vp, u32, vp]),
            "fhip_solve": (i32, [vp, vp, u32, vp, vp, vp, u32, vp, u32, u32, vp, vp, vp, vp]),
            "fhip_render2d": (i32, [vp, vp, C.POINTER(_Cfg2D), vp, i32]),
            "fhip_render3d": (i32, [vp, vp, C.POINTER(_Cfg3D), vp, i32]),
            "fhip_render3d_shard": (i32, [vp, vp, C.POINTER(_Cfg3D), vp, i32, u32, u32]),
            "fhip_render3d_block": (i32, [vp, vp, C.POINTER(_Cfg3D), vp, i32, u32, vp]),
            "fhip_merge_depth": (i32, [vp, vp, vp, u64, u32]),
            "fhip_denoise_normals": (i32, [vp, vp, u32, u32, vp, i32]),
            "fhip_compute_ssao": (i32, [vp, vp, u32, u32, u32, vp, u32, vp, u32, vp, i32]),
            "fhip_blur_ssao": (i32, [vp, vp, u32, u32, vp, i32]),
            "fhip_apply_shading": (i32, [vp, vp, u32, u32, u32, vp, vp, i32]),
            "fhip_to_rgba": (i32, [vp, vp, u32, u32, i32, vp, i32]),
            "fhip_mesh_sample": (i32, [vp, vp, u32, vp, vp, vp, vp, u32, C.POINTER(vp)]), "fhip_mesh_free": (None, [vp]),
            "fhip_mesh_counts": (None, [vp, vp]), "fhip_mesh_leaves": (None, [vp, vp]),
            "fhip_mesh_build": (i32, [vp, vp, u32, vp, vp, vp, vp, u32, C.POINTER(vp)]),
            "fhip_mesh_vertices": (None, [vp, vp]), "fhip_mesh_triangles": (None, [vp, vp]),
            "fhip_mesh_vertices_ptr": (vp, [vp]), "fhip_mesh_triangles_ptr": (vp, [vp]),
            "fhip_mesh_sample_part": (i32, [vp, vp, u32, vp, vp, vp, vp, u32, u32, u32, C.POINTER(vp)]),
            "fhip_mesh_part_bytes": (C.c_uint64, [vp]), "fhip_mesh_part_export": (None, [vp, vp]),
            "fhip_mesh_merge": (i32, [vp, vp, vp, u32, vp, C.POINTER(vp)]),
            "fhip_mesh_vertices_dev": (vp, [vp]), "fhip_mesh_triangles_dev": (vp, [vp]),
            "fhip_mesh_stl_bytes": (u64, [vp]), "fhip_mesh_stl": (i32, [vp, vp, vp, i32]),
            "fhip_mesh_vertex_grads": (i32, [vp, vp, vp, vp, vp, vp, u32, vp, i32]),
            "fhip_shape_occupancy": (i32, [vp, vp, u32, vp, vp, vp, vp, u32, vp]),
            "fhip_voxels_words": (u64, [u32]), "fhip_shape_voxels": (i32, [vp, vp, u32, vp, vp, vp, vp, u32, vp, i32, vp]),
            "fhip_voxels_slices": (i32, [vp, vp, u32, u32, u32, vp, i32]), "fhip_voxels_layer_counts": (i32, [vp, vp, u32, vp, i32]),
            "fhip_contour2d": (i32, [vp, vp, vp, vp]), "fhip_contours_counts": (None, [vp, vp]), "fhip_contours_vertices": (i32, [vp, vp]),
            "fhip_contours_segments": (i32, [vp, vp]), "fhip_contours_next": (i32, [vp, vp]), "fhip_contours_vertices_dev": (vp, [vp]),
            "fhip_contours_segments_dev": (vp, [vp]), "fhip_contours_free": (None, [vp]), "fhip_contour_loops": (i32, [vp, u64, vp, vp, vp, vp]),
            "fhip_voxels_components": (i32, [vp, vp, u32, i32, u32, i32, vp]), "fhip_components_counts": (None, [vp, vp]),
            "fhip_components_table": (i32, [vp, vp, vp, vp, vp, vp]), "fhip_components_label_slices": (i32, [vp, vp, vp, i32, u32, u32, vp, i32]),
            "fhip_components_extract": (i32, [vp, vp, vp, i32, vp, u64, vp, i32]), "fhip_components_free": (None, [vp]),
            "fhip_voxels_distance": (i32, [vp, vp, u32, i32, i32, vp]), "fhip_distance_info": (None, [vp, vp]), "fhip_distance_slices": (i32, [vp, vp, u32, u32, vp, i32]),
            "fhip_distance_dev": (vp, [vp]), "fhip_distance_threshold": (i32, [vp, vp, u32, i32, vp, i32]), "fhip_distance_free": (None, [vp]),
            "fhip_distance_thickness": (i32, [vp, vp, vp]), "fhip_thickness_info": (None, [vp, vp]), "fhip_thickness_thin": (i32, [vp, vp, u32, vp, i32]),
            "fhip_thickness_histogram": (i32, [vp, vp, vp, u32, vp, i32]),
            "fhip_voxels_surface": (i32, [vp, vp, u32, i32, vp]), "fhip_voxels_mesh": (i32, [vp, vp, u32, i32, vp]),
            "fhip_voxels_flow": (i32, [vp, vp, vp, u32, i32, u32, u32, vp, i32]), "fhip_voxels_overhangs": (i32, [vp, vp, u32, i32, u32, u32, i32, vp, i32]),
            "fhip_voxels_heights": (i32, [vp, vp, u32, i32, u32, vp, i32]),
            "fhip_triangles_voxels": (i32, [vp, vp, u64, vp, u64, i32, vp, u32, vp, i32, vp]), "fhip_mesh_voxels": (i32, [vp, vp, vp, u32, vp, i32, vp]),
            "fhip_triangles_topology": (i32, [vp, vp, u64, vp, u64, i32, i32, u32, vp]), "fhip_mesh_topology": (i32, [vp, vp, i32, u32, vp]),
            "fhip_topology_counts": (None, [vp, vp]), "fhip_topology_vertex_rows": (u64, [vp]), "fhip_topology_vertices": (i32, [vp, vp]),
            "fhip_topology_triangles": (i32, [vp, vp]), "fhip_topology_triangle_shells": (i32, [vp, vp]), "fhip_topology_vertices_dev": (vp, [vp]),
            "fhip_topology_triangles_dev": (vp, [vp]), "fhip_topology_triangle_shells_dev": (vp, [vp]),
            "fhip_topology_shells": (i32, [vp, vp, vp, vp, vp, vp, vp, vp]), "fhip_topology_edges": (i32, [vp, vp, u32, vp, i32]), "fhip_topology_free": (None, [vp]),
            "fhip_voxels_outlines": (i32, [vp, vp, u32, i32, u32, u32, u32, vp]), "fhip_outlines_counts": (None, [vp, vp]), "fhip_outlines_layers": (i32, [vp, vp, vp, vp, vp]),
            "fhip_outlines_vertices": (i32, [vp, u64, u64, vp, vp, vp]), "fhip_outlines_loops": (i32, [vp, u64, u64, vp, vp, vp, vp, vp, vp]),
            "fhip_outlines_xy_dev": (vp, [vp]), "fhip_outlines_next_dev": (vp, [vp]), "fhip_outlines_loop_dev": (vp, [vp]), "fhip_outlines_free": (None, [vp]),
            "fhip_topology_slices": (i32, [vp, vp, vp, u32, u32, vp]), "fhip_slices_counts": (None, [vp, vp]), "fhip_slices_planes": (i32, [vp, vp, vp, vp, vp]),
            "fhip_slices_loops": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp]), "fhip_slices_vertices": (i32, [vp, vp, vp, vp, vp, vp, vp]), "fhip_slices_xy_dev": (vp, [vp]),
            "fhip_slices_next_dev": (vp, [vp]), "fhip_slices_loop_dev": (vp, [vp]), "fhip_slices_plane_dev": (vp, [vp]), "fhip_slices_free": (None, [vp]),
            "fhip_debug_stl_pack": (i32, [vp, vp, u64, vp, u64, vp]),
            "fhip_profile_enable": (None, [vp, i32]), "fhip_profile_read": (i32, [vp, vp, vp]), "fhip_profile_read_kernels": (i32, [vp, vp, vp]),
            "fhip_render_counters": (i32, [vp, vp]),
            "fhip_debug_stats": (i32, [vp, vp]), "fhip_debug_leaf_stats": (i32, [vp, vp]), "fhip_debug_tape_links": (u32, [vp, vp, u32]), "fhip_debug_tape_chain": (u32, [vp, vp, u32]),
            "fhip_tape_group_count": (u32, [vp]), "fhip_tape_group_op": (i32, [vp]),
            "fhip_tape_group": (i32, [vp, vp, u32, vp]), "fhip_tape_term_plan": (u32, [vp, vp]), "fhip_tape_term_group": (i32, [vp, vp, u32, vp]),
            "fhip_tape_term_tree": (u32, [vp, vp, u32]), "fhip_tape_term_choice_src": (u32, [vp, vp, u32]),
            "fhip_debug_leaves": (u32, [vp, vp, u32]), "fhip_debug_arena": (u32, [vp, u32, u32, vp]), "fhip_debug_probe": (i32, [vp, vp]),
            "fhip_debug_bench": (i32, [vp, vp, u32, u32, i32, vp]),
            "fhip_debug_walk_dual": (None, [vp, u64, vp, vp, u64, i32, vp, vp, vp]),
            "fhip_debug_groups": (u32, [vp, i32, u32, vp, u32, vp]),
            "fhip_debug_ubench": (i32, [vp, u32, u32, u32, vp]),
            "fhip_debug_math_sweep": (i32, [vp, i32, u32, u32, u64, vp, vp]),
            "fhip_debug_trans_probe": (i32, [vp, u32, u32, u32, u64, vp]),
            "fhip_debug_lane_frames": (u64, [vp]),
            "fhip_debug_rare_frames": (u64, [vp]),
            "fhip_debug_lane_tune": (i32, [vp, vp, vp]),
            "fhip_debug_bound_tape": (i32, [vp, vp, vp, vp, vp, u32, C.POINTER(vp)]),
            "fhip_graph_new": (vp, []), "fhip_graph_free": (None, [vp]), "fhip_graph_len": (u32, [vp]),
            "fhip_graph_var": (u32, [vp, i32, u64]), "fhip_graph_constant": (u32, [vp, f32]),
            "fhip_graph_unary": (u32, [vp, i32, u32]), "fhip_graph_binary": (u32, [vp, i32, u32, u32]),
            "fhip_graph_from_text": (u32, [vp, C.c_char_p]),
            "fhip_tape_from_graph": (i32, [vp, vp, vp, u32, C.POINTER(vp)]),
            "fhip_tape_axis_slot": (i32, [vp, i32]), "fhip_tape_var_slot": (i32, [vp, u64]),
            "fhip_screen_to_world": (None, [vp, i32, vp]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class HipContext:
    """fhip_ctx: one device + stream.  `stream` may be a raw hipStream_t (e.g. torch's)."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        st = lib().fhip_ctx_create(device, C.c_void_p(stream or 0), C.byref(h))
        if st != 0:
            raise FidgetHipError(st, "no usable HIP device: fidget_amd has no CPU fallback")
        self._h = h

    def __del__(self):
        try:
            lib().fhip_ctx_destroy(self._h)
        except Exception:
            pass

    def check(self, st):
        if st != 0:
            raise FidgetHipError(st, (lib().fhip_last_error(self._h) or b"").decode())

    def sync(self):
        self.check(lib().fhip_ctx_sync(self._h))

    def trim(self):
        """fhip_ctx_trim: memory kept between calls for speed alone (mesh leaf records and the scratch of `voxelize_mesh` in the same buffer, frame lanes) goes back to the device"""
        self.check(lib().fhip_ctx_trim(self._h))

    def reserve_arena(self, megabytes):
        """fhip_ctx_reserve_arena: every buffer set's tape arena at least this large from the next frame on"""
        self.check(lib().fhip_ctx_reserve_arena(self._h, int(megabytes)))

    def cancel(self):
        lib().fhip_cancel(self._h)

    def cancel_watch(self, flag):
        """fhip_cancel_watch: `flag` = a numpy uint8 array of one element the context reads beside its own flag (None: stop watching)"""
        self._watched = flag          # (kept alive while it is watched)
        lib().fhip_cancel_watch(self._h, None if flag is None else flag.ctypes.data_as(C.c_void_p))

    def cancel_reset(self):
        lib().fhip_cancel_reset(self._h)

    def lane_tune(self):
        """What the frame arrangement tuner knows about the kind of 3D frame queued last (fhip_debug_lane_tune): phase 0 .. 2 measuring
        (stage pipeline, lanes, stage pipeline again), 3 waiting, 4 decided, -1 none; ms per frame of the three windows; the decision."""
        ms, ln = (C.c_float * 3)(), C.c_int(0)
        ph = lib().fhip_debug_lane_tune(self._h, ms, C.byref(ln))
        return {"phase": int(ph), "stage_pipeline_ms": [float(ms[0]), float(ms[2])], "frame_lanes_ms": float(ms[1]), "kept": "frame lanes" if ln.value else "stage pipeline"}

    def lane_frames(self):
        """Frames of this context that went to a frame lane so far (fhip_debug_lane_frames)"""
        return int(lib().fhip_debug_lane_frames(self._h))

    def rare_frames(self):
        """3D frames of this context rendered in rare mode so far - the launches for tapes beyond the assembly kernels' register files folded
        into the slab's other launches (fhip_debug_rare_frames; capi_render.hpp)"""
        return int(lib().fhip_debug_rare_frames(self._h))

    def set_option(self, name, value=1):
        """A behaviour switch of this context (fhip_ctx_set_option: "no_column_inv", "frame_lanes", ...).  The environment
        (FHIP_<NAME>) is read once, when the context is created; this is the only way to change a switch afterwards."""
        self.check(lib().fhip_ctx_set_option(self._h, name.encode(), int(value)))

    def option(self, name):
        v = C.c_int(0)
        self.check(lib().fhip_ctx_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def options(self, **kw):
        """Context manager: switches set for the duration of a block, then restored."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            old = {k: self.option(k) for k in kw}
            try:
                for k, v in kw.items():
                    self.set_option(k, v)
                yield self
            finally:
                for k, v in old.items():
                    self.set_option(k, v)
        return scope()

    def profile(self, on):
        lib().fhip_profile_enable(self._h, int(on))

    def profile_read(self):
        ms = np.zeros(4, np.float64)
        n = np.zeros(4, np.uint32)
        self.check(lib().fhip_profile_read(self._h, _p(ms), _p(n)))
        names = ["tiles", "points", "normals", "other"]
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(names)}

    def profile_read_kernels(self):
        """(ms, launches) of the last profiled frame per assembly kernel, every launch timed on its own."""
        ms = np.zeros(8, np.float64)
        n = np.zeros(8, np.uint32)
        self.check(lib().fhip_profile_read_kernels(self._h, _p(ms), _p(n)))
        # (fh_prune1: the root level's prune, i.e. k_prune2 with the scalar sweep behind it when option prune2 is on)
        names = ["fh_columns", "fh_float_eval_16x4", "fh_float_eval_32x2", "fh_tiles", "fh_prune1", "fh_tiles_v32", "fh_tiles_v64", "unused"]
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(names)}

    def counters(self):
        c = np.zeros(8, np.uint64)
        self.check(lib().fhip_render_counters(self._h, _p(c)))
        return {"arena_ops": int(c[0]), "arena_overflow": int(c[1]), "leaves_last_slab": int(c[2]),
                "queue_overflow": int(c[3]), "groups_last_slab": [int(v) for v in c[4:6]], "hip_tile_stage_frames": int(c[6]), "substituted_tile_lists": int(c[7])}

    def last_leaves(self, cap=1 << 20):
        """Leaf records of the last slab of the last 3D frame: structured array (off, len, regs, choices, x, y, z)."""
        dt = np.dtype([("off", np.uint32), ("len", np.uint32), ("regs", np.uint16), ("choices", np.uint16),
                       ("x", np.uint32), ("y", np.uint32), ("z", np.uint32)])
        buf = np.zeros(cap, dt)
        n = lib().fhip_debug_leaves(self._h, _p(buf), cap)
        return buf[:n]

    def groups(self, kind, index, cap=1 << 20):
        """Work-queue entries the last 3D frame left behind (kind 0: tile level `index`; 1: parked z-slab `index`):
        (structured array (off, len, regs, choices, x, y, z, ...), (n_small_layout, n_other))."""
        dt = np.dtype([("off", np.uint32), ("len", np.uint32), ("regs", np.uint16), ("choices", np.uint16),
                       ("x", np.uint32), ("y", np.uint32), ("z", np.uint32), ("first", np.uint32), ("n", np.uint32), ("stride", np.uint32)])
        assert dt.itemsize == 36  # sizeof(FhGroup)
        buf = np.zeros(cap, dt)
        cnt = np.zeros(2, np.uint32)
        n = lib().fhip_debug_groups(self._h, kind, index, _p(buf), cap, _p(cnt))
        return buf[:n], (int(cnt[0]), int(cnt[1]))

    def arena_ops(self, off, n):
        """`n` device-format ops of the tape arena from op `off` (diagnostics; see last_leaves)."""
        buf = np.zeros(n, np.uint64)
        got = lib().fhip_debug_arena(self._h, int(off), int(n), _p(buf))
        return buf[:got]

    def leaf_stats(self):
        """Leaf-stage counters of the last profiled 3D frame (render_state.h leaf_stat)."""
        c = np.zeros(8, np.uint64)
        self.check(lib().fhip_debug_leaf_stats(self._h, _p(c)))
        return {"leaves": int(c[0]), "tape_ops": int(c[1]), "tape_words_read": int(c[2]), "lane_ops": int(c[3]),
                "prune2_phase_clocks_max": [int(v) for v in c[4:8]]}

    def wave_stats(self):
        """Per kernel kind: mean / max busy microseconds of the waves that found work, their
        number and the units of work they pulled (frame totals)."""
        c = np.zeros(64, np.uint64)
        self.check(lib().fhip_debug_stats(self._h, _p(c)))
        names = ["tiles_l0", "tiles_l1", "tiles_l2", "tiles_l3", "tiles_l4", "columns_c0", "columns_c12", "tiles_2d"]
        self.tile_v = {f"l{l}": {"slots": int(c[8 + l]), "fwd_clocks": int(c[16 + l]), "prune_clocks": int(c[24 + l]), "max_slot_clocks": int(c[l])}
                       for l in range(8) if c[8 + l]}
        self.tile_phases = {f"l{l}": {"fwd_us": int(c[32 + l]) / 100.0, "prune_us": int(c[40 + l]) / 100.0,
                                      "ops": int(c[48 + l]), "ops_written": int(c[56 + l]), "fwd_shader_clocks": int(c[16 + l])} for l in range(8) if c[48 + l]}
        return {k: {"busy_us_sum": int(c[4 * i]) / 100.0, "busy_us_max": int(c[4 * i + 1]) / 100.0,
                    "waves": int(c[4 * i + 2]), "units": int(c[4 * i + 3])} for i, k in enumerate(names) if c[4 * i + 2]}


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = HipContext(int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("FHIP_USE_LOCAL_RANK") else 0)
    return _default_ctx


BAD_NODE = 0xFFFFFFFF


class BadNode(Exception):
    pass


class Node(int):
    pass


class Context:
    """Host mirror of fidget_core::Context (constructor identities, dedup, .vm text)."""

    def __init__(self):
        self._h = C.c_void_p(lib().fhip_graph_new())

    def __del__(self):
        try:
            lib().fhip_graph_free(self._h)
        except Exception:
            pass

    def __len__(self):
        return lib().fhip_graph_len(self._h)

    def _node(self, v):
        if isinstance(v, (float, int)) and not isinstance(v, Node):
            return self.constant(float(v))
        return v

    def x(self): return Node(lib().fhip_graph_var(self._h, 0, 0))
    def y(self): return Node(lib().fhip_graph_var(self._h, 1, 0))
    def z(self): return Node(lib().fhip_graph_var(self._h, 2, 0))
    def var(self, index): return Node(lib().fhip_graph_var(self._h, 3, int(index)))
    def constant(self, f): return Node(lib().fhip_graph_constant(self._h, float(f)))

    def _un(self, name, a):
        r = lib().fhip_graph_unary(self._h, UNARY.index(name), int(self._node(a)))
        if r == BAD_NODE:
            raise BadNode()
        return Node(r)

    def _bin(self, name, a, b):
        r = lib().fhip_graph_binary(self._h, BINARY.index(name), int(self._node(a)), int(self._node(b)))
        if r == BAD_NODE:
            raise BadNode()
        return Node(r)

    # derived constructors (context/mod.rs:701-780)
    def less_than(self, lhs, rhs):
        return self.max(self._bin("compare", rhs, lhs), 0.0)

    def less_than_or_equal(self, lhs, rhs):
        return self.min(self.add(self._bin("compare", rhs, lhs), 1.0), 1.0)

    def if_nonzero_else(self, cond, a, b):
        cond, a, b = self._node(cond), self._node(a), self._node(b)
        lhs = self.and_(cond, a)
        rhs = self.and_(self.not_(cond), b)
        return self.or_(lhs, rhs)

    @staticmethod
    def from_text(text):
        ctx = Context()
        if isinstance(text, str):
            text = text.encode()
        r = lib().fhip_graph_from_text(ctx._h, text)
        if r == BAD_NODE:
            raise ValueError("parse error")
        return ctx, Node(r)


def _mk_un(name):
    def f(self, a):
        return self._un(name, a)
    return f


def _mk_bin(name):
    def f(self, a, b):
        return self._bin(name, a, b)
    return f


for _n in UNARY:
    setattr(Context, {"not": "not_"}.get(_n, _n), _mk_un(_n))
for _n in BINARY:
    setattr(Context, {"and": "and_", "or": "or_", "mod": "modulo"}.get(_n, _n), _mk_bin(_n))


class Shape:
    """One function compiled to a device tape (the role of `Shape<HipFunction>`)."""

    def __init__(self, ctx=None, node=None, n_regs=255, _h=None, roots=None, hip=None, _vars=None):
        # n_regs is accepted for signature parity with GenericVmFunction<N>; device tapes
        # always use dense renumbering over up to 256 registers (no spills).
        self._hip = hip  # created lazily: tape construction and simplify are host-only
        self.n_regs = n_regs
        if _h is not None:
            self._h = _h
            self._vars = _vars
            return
        if roots is None:
            roots = [node]
        r = np.array([int(n) for n in roots], dtype=np.uint32)
        h = C.c_void_p()
        st = lib().fhip_tape_from_graph(None, ctx._h, _p(r), len(r), C.byref(h))
        if st != 0:
            raise FidgetHipError(st, "tape construction failed")
        self._h = h
        self._vars = None

    @property
    def hip(self):
        if self._hip is None:
            self._hip = default_context()
        return self._hip

    def __del__(self):
        try:
            lib().fhip_tape_free(self._h)
        except Exception:
            pass

    def groups(self):
        """Tape parallelism: (combining op name, [Shape of each independent sub-tape]); ('', []) if the
        root of the function is not a min / max of many parts."""
        n = lib().fhip_tape_group_count(self._h)
        out = []
        for g in range(n):
            h = C.c_void_p()
            st = lib().fhip_tape_group(None, self._h, g, C.byref(h))
            if st != 0:
                raise FidgetHipError(st, "tape group")
            out.append(Shape(_h=h, hip=self._hip, _vars=self._vars))
        op = lib().fhip_tape_group_op(self._h)
        return ({30: "min", 31: "max"}.get(op, ""), out)

    def term_parts(self):
        """(group Shapes, tree ops as an (n, 3) u32 array, choice sources as a u32 array) of term_plan()."""
        n = self.term_plan()
        gs = []
        for g in range(n["groups"]):
            h = C.c_void_p()
            st = lib().fhip_tape_term_group(None, self._h, g, C.byref(h))
            if st != 0:
                raise FidgetHipError(st, "term group")
            gs.append(Shape(_h=h, hip=self._hip, _vars=self._vars))
        tree = np.zeros((max(n["tree_ops"], 1), 3), np.uint32)
        lib().fhip_tape_term_tree(self._h, _p(tree), n["tree_ops"])
        src = np.zeros(max(n["choices"], 1), np.uint32)
        lib().fhip_tape_term_choice_src(self._h, _p(src), n["choices"])
        return gs, tree[:n["tree_ops"]], src[:n["choices"]]

    def term_plan(self):
        """The renderer's root-level split: dict(groups, terms, tree_ops, tree_regs, choices); groups = 0 if none."""
        info = (C.c_uint32 * 4)()
        n = lib().fhip_tape_term_plan(self._h, info)
        return dict(groups=n, terms=info[0], tree_ops=info[1], tree_regs=info[2], choices=info[3])

    @staticmethod
    def from_vm(path_or_text, n_regs=255, hip=None):
        text = open(path_or_text).read() if os.path.exists(path_or_text) else path_or_text
        ctx, root = Context.from_text(text)
        return Shape(ctx, root, n_regs, hip=hip)

    @staticmethod
    def from_bytecode(words, axis_slots=(0, 1, 2), hip=None):
        """The reference wire format (fidget_bytecode::Bytecode::data()); axis_slots = VarMap slots of X, Y, Z."""
        w = np.ascontiguousarray(words, dtype=np.uint32)
        h = C.c_void_p()
        st = lib().fhip_tape_from_bytecode(None, _p(w), len(w), C.byref(h))
        if st != 0:
            raise FidgetHipError(st, "bad bytecode")
        return Shape(_h=h, hip=hip, _vars=tuple(axis_slots))

    # sizes ---------------------------------------------------------------
    def device_len(self): return lib().fhip_tape_len(self._h)

    def size(self):
        """Function::size (eval/mod.rs:171) = VmData<N>::len(): the device tape's length - one op per SSA op - or, for a Shape made with
        fewer than 255 registers, the reference's RegTape under that limit with its loads and stores (fhip_tape_reg_tape)."""
        if self.n_regs == 255 and lib().fhip_tape_reg_count(self._h) <= 255:
            return self.device_len()
        return int(self.reg_tape()[1][0])     # (also for a tape that needs more than 255 registers: VmData<255>::len() counts its loads / stores)
    __len__ = size
    def ssa_len(self): return self.device_len()  # device tapes carry no load/store: one op per SSA op

    def reg_tape(self, n_regs=None, want_words=False):
        """RegTape::new::<N> + Bytecode::new of this tape (host side): ([(op, form, out, a, b, idx, imm bits)] in evaluation order - the
        oracle's asm_ops() records -, (len, slot_count, reg_count, mem_count)[, bytecode words])."""
        n_regs = self.n_regs if n_regs is None else n_regs
        info = np.zeros(4, np.uint32)
        st = lib().fhip_tape_reg_tape(self._h, n_regs, None, 0, None, 0, _p(info))
        if st not in (0, 6):
            raise FidgetHipError(st, "register allocation")
        n = int(info[0])
        rec = np.zeros((n, 4), np.uint32)
        words = np.zeros(2 * n + 4, np.uint32)
        st = lib().fhip_tape_reg_tape(self._h, n_regs, _p(rec), n, _p(words), len(words), _p(info))
        if want_words and st == 6:
            raise ValueError("ReservedRegister")
        NAMES = ["Output", "Input", "CopyReg", "CopyImm", "Neg", "Abs", "Recip", "Sqrt", "Square", "Floor", "Ceil", "Round", "Sin", "Cos", "Tan",
                 "Asin", "Acos", "Atan", "Exp", "Ln", "Not", "Rand"]
        BIN = ["Add", "Sub", "Mul", "Div", "Atan2", "Compare", "Mix", "Mod", "Min", "Max", "And", "Or"]
        ops = []
        for op, o, a, w in rec.tolist():
            if op == 52: ops.append(("Load", "", o, 0, 0, w, 0))
            elif op == 53: ops.append(("Store", "", 0, a, 0, w, 0))
            elif op == 0: ops.append(("Output", "", 0, a, 0, w, 0))
            elif op == 1: ops.append(("Input", "", o, 0, 0, w, 0))
            elif op == 3: ops.append(("CopyImm", "", o, 0, 0, 0, w))
            elif op < 22: ops.append((NAMES[op], "Reg", o, a, 0, 0, 0))
            elif op < 34: ops.append((BIN[op - 22], "RegReg", o, a, w, 0, 0))
            elif op < 46: ops.append((BIN[op - 34], "RegImm", o, a, 0, 0, w))
            else: ops.append((["Sub", "Div", "Atan2", "Compare", "Mix", "Mod"][op - 46], "ImmReg", o, a, 0, 0, w))
        out = (ops, tuple(int(v) for v in info))
        return out + (words,) if want_words else out

    def asm_ops(self): return self.reg_tape()[0]

    def bytecode(self):
        """fidget_bytecode::Bytecode::new of the tape as VmData<n_regs>: (words, reg_count, mem_count)"""
        _, info, words = self.reg_tape(want_words=True)
        return words, info[2], info[3]
    def choice_count(self): return lib().fhip_tape_choice_count(self._h)
    def output_count(self): return lib().fhip_tape_output_count(self._h)
    def slot_count(self): return lib().fhip_tape_reg_count(self._h)
    def var_count(self): return lib().fhip_tape_var_count(self._h)

    def axis_index(self, axis):
        if self._vars is not None:
            return self._vars[axis]
        return lib().fhip_tape_axis_slot(self._h, axis)

    def var_index(self, index): return lib().fhip_tape_var_slot(self._h, int(index))

    def words(self):
        """Device tape as raw 8-byte ops (tape_format.h), evaluation order."""
        n = self.device_len()
        w = np.zeros(max(n, 1), dtype=np.uint64)
        lib().fhip_tape_ops(self._h, _p(w), n)
        return w[:n]

    def links(self):
        """Per-op links for the linked prune (fhip_debug_tape_links; host_graph.hpp compute_links): [n, 5] = (opcode, class, choice ordinal,
        producer of a, producer of b) - a producer is an op index, 0x8000 | ordinal for a choice op, 0xFFFF for none; None when the tape
        does not qualify."""
        n = self.device_len()
        w = np.zeros(max(n, 1), dtype=np.uint64)
        if lib().fhip_debug_tape_links(self._h, _p(w), n) != n:
            return None
        w = w[:n]
        return np.stack([w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFFFF, (w >> 32) & 0xFFFF, (w >> 48) & 0xFFFF], axis=1).astype(np.int64)

    def chain(self):
        """The root chain for the linked prune's liveness pass (fhip_debug_tape_chain): [n, 2] = (choice ordinal, op index) per chain op in
        evaluation order; empty when the root tree is no chain"""
        w = np.zeros(65536, dtype=np.uint32)
        n = lib().fhip_debug_tape_chain(self._h, _p(w), len(w))
        return np.stack([w[:n] & 0xFFFF, w[:n] >> 16], axis=1).astype(np.int64)

    def ops(self):
        """Device tape as (name, out, a, b, imm_bits) tuples in evaluation order."""
        n = self.device_len()
        w = np.zeros(max(n, 1), dtype=np.uint64)
        lib().fhip_tape_ops(self._h, _p(w), n)
        out = []
        for v in w[:n]:
            v = int(v)
            out.append((FH_OPS[v & 0xFF], (v >> 8) & 0xFFF, (v >> 20) & 0xFFF, v >> 32, v >> 32))  # (name, out, a, b|imm, imm)
        return out

    def simplify(self, choices, n_regs=None):
        c = np.ascontiguousarray(choices, dtype=np.uint8)
        h = C.c_void_p()
        st = lib().fhip_simplify(None, self._h, _p(c), len(c), C.byref(h))
        if st != 0:
            raise ValueError(STATUS.get(st, str(st)))
        return Shape(_h=h, hip=self._hip, _vars=self._vars if self._vars is not None else tuple(self.axis_index(a) for a in range(3)),
                     n_regs=self.n_regs if n_regs is None else n_regs)._with_named(self)

    def _with_named(self, parent):
        self._named_parent = parent  # children keep the parent's Var::V slots
        return self

    def _named_slot(self, index):
        p = self
        while getattr(p, "_named_parent", None) is not None:
            p = p._named_parent
        return lib().fhip_tape_var_slot(p._h, int(index))

    # evaluators ------------------------------------------------------------
    def _xyz_vars(self, x, y, z, extra=None):
        n = max(self.var_count(), 1)
        vs = [None] * n
        for axis, v in enumerate((x, y, z)):
            i = self.axis_index(axis)
            if 0 <= i < n:
                vs[i] = v
        for k, v in (extra or {}).items():
            i = self._named_slot(k)
            if 0 <= i < n:
                vs[i] = v
        return vs

    def _tracing(self, fn, v, comp):
        n, nv = v.shape[0], v.shape[1]
        no, nc = self.output_count(), self.choice_count()
        out = np.zeros((n, max(no, 1)) + ((2,) if comp == 2 else ()), dtype=np.float32)
        ch = np.zeros((n, max(nc, 1)), dtype=np.uint8)
        simp = np.zeros(n, dtype=np.uint8)
        st = fn(self.hip._h, self._h, _p(v), nv, n, _p(out), _p(ch), _p(simp))
        if st in (1, 2, 3):
            raise ValueError(STATUS[st])
        self.hip.check(st)
        return out[:, :no], ch[:, :nc], simp

    def eval_interval_batch(self, batch):
        """batch: list of per-variable (lo, hi) lists (None = [0,0]).  Returns [((lo,hi), trace|None)]."""
        v = np.array([[(0.0, 0.0) if a is None else a for a in vs] for vs in batch], dtype=np.float32)
        if v.ndim != 3:
            v = v.reshape(len(batch), -1, 2)
        out, ch, simp = self._tracing(lib().fhip_interval_eval, np.ascontiguousarray(v), 2)
        return [((float(out[i, 0, 0]), float(out[i, 0, 1])), (ch[i].copy() if simp[i] else None)) for i in range(len(batch))]

    def eval_interval_raw(self, vars_):
        v = np.array(vars_, dtype=np.float32).reshape(1, -1, 2)
        out, ch, simp = self._tracing(lib().fhip_interval_eval, v, 2)
        return out[0], (ch[0].copy() if simp[0] else None)

    def eval_interval(self, x, y, z, extra=None):
        vs = self._xyz_vars(x, y, z, extra)
        vs = [(0.0, 0.0) if v is None else ((v, v) if np.isscalar(v) else tuple(v)) for v in vs]
        out, tr = self.eval_interval_raw(vs)
        return (float(out[0][0]), float(out[0][1])), tr

    def eval_point_raw(self, vars_):
        v = np.array(vars_, dtype=np.float32).reshape(1, -1)
        out, ch, simp = self._tracing(lib().fhip_point_eval, v, 1)
        return out[0], (ch[0].copy() if simp[0] else None)

    def eval_point(self, x, y, z, extra=None):
        vs = [0.0 if v is None else v for v in self._xyz_vars(x, y, z, extra)]
        out, tr = self.eval_point_raw(vs)
        return float(out[0]), tr

    def _bulk(self, fn, arrs, comp):
        n = len(arrs[0]) // comp if arrs else 0
        lens = np.array([len(a) // comp for a in arrs], dtype=np.uint32)
        ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        no = self.output_count()
        outs = [np.zeros(n * comp, dtype=np.float32) for _ in range(no)]
        optrs = (C.c_void_p * max(no, 1))(*[o.ctypes.data for o in outs])
        st = fn(self.hip._h, self._h, ptrs, _p(lens), len(arrs), optrs)
        if st in (1, 2, 3):
            raise ValueError(STATUS[st])
        self.hip.check(st)
        return outs

    def eval_float_slice_raw(self, arrays):
        arrs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in arrays]
        outs = self._bulk(lib().fhip_float_eval, arrs, 1)
        n = len(arrs[0]) if arrs else 0
        return np.array(outs, dtype=np.float32).reshape(self.output_count(), n)

    def eval_float_slice(self, x, y, z, extra=None):
        x, y, z = (np.asarray(a, dtype=np.float32) for a in (x, y, z))
        n = len(x)
        vs = self._xyz_vars(x, y, z, extra)
        vs = [np.zeros(n, np.float32) if v is None else (np.full(n, v, np.float32) if np.isscalar(v) else v) for v in vs]
        return self.eval_float_slice_raw(vs)[0]

    def eval_grad_slice_raw(self, arrays):
        arrs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in arrays]
        outs = self._bulk(lib().fhip_grad_eval, arrs, 4)
        n = len(arrs[0]) // 4 if arrs else 0
        return np.array(outs, dtype=np.float32).reshape(self.output_count(), n, 4)

    def eval_grad_slice(self, x, y, z, extra=None):
        x, y, z = (np.asarray(a, dtype=np.float32) for a in (x, y, z))
        n = len(x)

        def seed(v, k):
            g = np.zeros((n, 4), np.float32)
            g[:, 0] = v
            g[:, 1 + k] = 1.0
            return g
        vs = self._xyz_vars(seed(x, 0), seed(y, 1), seed(z, 2), extra)
        out = []
        for v in vs:
            if v is None:
                out.append(np.zeros((n, 4), np.float32))
            elif np.isscalar(v):
                g = np.zeros((n, 4), np.float32)
                g[:, 0] = v
                out.append(g)
            else:
                out.append(v)
        return self.eval_grad_slice_raw(out)[0]


# ---- geometry helpers (host f32, same operation order as the C++ driver) --------------
def screen_to_world(size):
    n = len(size)
    s = np.array(size, dtype=np.uint32)
    out = np.zeros((n + 1, n + 1), dtype=np.float32)
    lib().fhip_screen_to_world(_p(s), n, _p(out))
    return out


def mat_mul(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    d = a.shape[0]
    out = np.zeros((d, d), np.float32)
    for col in range(d):
        for row in range(d):
            acc = np.float32(a[row, 0] * b[0, col])
            for k in range(1, d):
                acc = np.float32(np.float32(a[row, k] * b[k, col]) + acc)
            out[row, col] = acc
    return out


def lift_2d(m3):
    m3 = np.asarray(m3, np.float32)
    m = np.zeros((4, 4), np.float32)
    m[0, :2] = m3[0, :2]; m[0, 3] = m3[0, 2]
    m[1, :2] = m3[1, :2]; m[1, 3] = m3[1, 2]
    m[2, 2] = 1.0
    m[3, :2] = m3[2, :2]; m[3, 3] = m3[2, 2]
    return m


def transform_point(mat4, x, y, z):
    m = np.asarray(mat4, np.float32)
    x, y, z = np.float32(x), np.float32(y), np.float32(z)
    r = [np.float32(np.float32(np.float32(m[i, 0] * x) + np.float32(m[i, 1] * y)) + np.float32(m[i, 2] * z)) + m[i, 3]
         for i in range(4)]
    r = [np.float32(v) for v in r]
    if r[3] != 0:
        return np.array([r[0] / r[3], r[1] / r[3], r[2] / r[3]], np.float32)
    return np.array(r[:3], np.float32)


def _var_arrays(shape, vars_):
    vars_ = vars_ or {}
    k = np.array(list(vars_.keys()), dtype=np.uint64)
    v = np.array(list(vars_.values()), dtype=np.float32)
    return k, v


def _dev_ptr(out):
    """Accept a torch CUDA tensor (device pointer) or None."""
    if out is None:
        return None
    return C.c_void_p(out.data_ptr())


def render2d(shape, width, height=None, z=0.0, pixel_perfect=False, world_to_model=None, tile_sizes=None,
             vars=None, out=None, mode=None, threads=None):
    """fidget_raster::pixel::render on the GPU.  Returns (float32 [h,w] RawDistancePixel image, stats, seconds);
    with `out` (a torch CUDA float32 tensor) the call is asynchronous and returns (out, None, None)."""
    height = width if height is None else height
    hip = shape.hip
    ts = np.array(tile_sizes, dtype=np.uint32) if tile_sizes else None
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    vk, vv = _var_arrays(shape, vars)
    ax = None
    if shape._vars is not None:
        ax = np.array(shape._vars, dtype=np.int32)
        vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
    cfg = _Cfg2D(width, height, _p(w2m), z, int(pixel_perfect), _p(ts), 0 if ts is None else len(ts), _p(vk), _p(vv),
                 len(vk), _p(ax))
    if out is not None:
        st = lib().fhip_render2d(hip._h, shape._h, C.byref(cfg), _dev_ptr(out), 1)
        if st == 4:
            raise ValueError("MissingVar")
        hip.check(st)
        return out, None, None
    img = np.zeros((height, width), dtype=np.float32)
    import time
    t0 = time.perf_counter()
    st = lib().fhip_render2d(hip._h, shape._h, C.byref(cfg), _p(img), 0)
    dt = time.perf_counter() - t0
    if st == 4:
        raise ValueError("MissingVar")
    hip.check(st)
    return img, {}, dt


def render3d(shape, width, height=None, depth=None, world_to_model=None, tile_sizes=None, vars=None, out=None,
             shard=0, n_shards=1, mode=None, threads=None, block=None, host_out=None):
    """fidget_raster::voxel::render on the GPU.  Returns (GeometryPixel [h,w] image, stats, seconds).
    Multi-GPU parts: (shard, n_shards) = root-tile columns round robin; block = (index, (nx, ny, nz)) = one block of an
    nx x ny x nz split of the volume (fhip_render3d_block)."""
    height = width if height is None else height
    depth = width if depth is None else depth
    hip = shape.hip
    if out is not None and world_to_model is None and not tile_sizes and not vars and shape._vars is None:
        # (the same frame again - what a caller that holds its RenderConfig does: the configuration struct is kept with the shape, the call
        # is the C call and nothing else; queued frames are bound by the thread that queues them)
        key = (width, height, depth, shard, n_shards, None if block is None else (int(block[0]), tuple(int(b) for b in block[1])))
        frames = shape.__dict__.setdefault("_frames", {})
        ent = frames.get(key)
        if ent is None:
            cfg = _Cfg3D(width, height, depth, None, None, 0, None, None, 0, None)
            split = None if block is None else np.array(block[1], dtype=np.uint32)
            ent = frames[key] = (cfg, C.byref(cfg), split, _p(split))
        if block is not None:
            st = lib().fhip_render3d_block(hip._h, shape._h, ent[1], C.c_void_p(out.data_ptr()), 1, key[5][0], ent[3])
        else:
            st = lib().fhip_render3d_shard(hip._h, shape._h, ent[1], C.c_void_p(out.data_ptr()), 1, shard, n_shards)
        if st:
            if st == 4:
                raise ValueError("MissingVar")
            hip.check(st)
        return out, None, None
    ts = np.array(tile_sizes, dtype=np.uint32) if tile_sizes else None
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    vk, vv = _var_arrays(shape, vars)
    ax = None
    if shape._vars is not None:
        ax = np.array(shape._vars, dtype=np.int32)
        vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
    cfg = _Cfg3D(width, height, depth, _p(w2m), _p(ts), 0 if ts is None else len(ts), _p(vk), _p(vv), len(vk), _p(ax))
    def call(ptr, dev):
        if block is not None:
            split = np.array(block[1], dtype=np.uint32)
            return lib().fhip_render3d_block(hip._h, shape._h, C.byref(cfg), ptr, dev, int(block[0]), _p(split))
        return lib().fhip_render3d_shard(hip._h, shape._h, C.byref(cfg), ptr, dev, shard, n_shards)
    if out is not None:
        st = call(_dev_ptr(out), 1)
        if st == 4:
            raise ValueError("MissingVar")
        hip.check(st)
        return out, None, None
    # (host_out: a caller's own [height, width] GEOMETRY_PIXEL array to land in - pinned memory, say)
    img = np.zeros((height, width), dtype=GEOMETRY_PIXEL) if host_out is None else host_out
    assert img.dtype == GEOMETRY_PIXEL and img.shape == (height, width) and img.flags.c_contiguous
    import time
    t0 = time.perf_counter()
    st = call(_p(img), 0)
    dt = time.perf_counter() - t0
    if st == 4:
        raise ValueError("MissingVar")
    hip.check(st)
    return img, {}, dt


def merge_depth(front, back, image_depth, hip=None):
    """fhip_merge_depth on torch CUDA tensors ([h, w, 4] int32 GeometryPixel words), in place on `front`."""
    hip = hip or default_context()
    hip.check(lib().fhip_merge_depth(hip._h, _dev_ptr(front), _dev_ptr(back), front.numel() // 4, int(image_depth)))
    return front


def pixel_inside(img):
    """RawDistancePixel::inside (fidget-raster/src/pixel.rs:187-193)."""
    img = np.asarray(img, np.float32)
    bits = img.view(np.uint32)
    is_fill = np.isnan(img) & ((bits & (0xFF << 9)) == (0xF6 << 9))
    return np.where(is_fill, (bits & 1) == 1, img < 0.0)


def pixel_fill_depth(img):
    img = np.asarray(img, np.float32)
    bits = img.view(np.uint32)
    is_fill = np.isnan(img) & ((bits & (0xFF << 9)) == (0xF6 << 9))
    return np.where(is_fill, ((bits >> 1) & 0xFF).astype(np.int32), -1)


# ---- fidget_raster::effects (fidget-raster/src/effects.rs), host arrays in / out -----------------------
def denoise_normals(image, hip=None):
    hip = hip or default_context()
    image = np.ascontiguousarray(image, GEOMETRY_PIXEL)
    out = np.zeros_like(image)
    hip.check(lib().fhip_denoise_normals(hip._h, _p(image), image.shape[1], image.shape[0], _p(out), 0))
    return out


def compute_ssao(image, depth, kernel, noise, hip=None):
    """kernel: 3 x n, noise: 2 x m (the matrices effects::ssao_kernel / ssao_noise return)"""
    hip = hip or default_context()
    image = np.ascontiguousarray(image, GEOMETRY_PIXEL)
    k = np.ascontiguousarray(np.asarray(kernel, np.float32).T)
    nz = np.ascontiguousarray(np.asarray(noise, np.float32).T)
    out = np.zeros(image.shape, np.float32)
    hip.check(lib().fhip_compute_ssao(hip._h, _p(image), image.shape[1], image.shape[0], depth, _p(k), len(k), _p(nz), len(nz), _p(out), 0))
    return out


def blur_ssao(ssao, hip=None):
    hip = hip or default_context()
    ssao = np.ascontiguousarray(ssao, np.float32)
    out = np.zeros_like(ssao)
    hip.check(lib().fhip_blur_ssao(hip._h, _p(ssao), ssao.shape[1], ssao.shape[0], _p(out), 0))
    return out


def apply_shading(image, depth, ssao=None, hip=None):
    hip = hip or default_context()
    image = np.ascontiguousarray(image, GEOMETRY_PIXEL)
    s = None if ssao is None else np.ascontiguousarray(ssao, np.float32)
    out = np.zeros(image.shape + (3,), np.uint8)
    hip.check(lib().fhip_apply_shading(hip._h, _p(image), image.shape[1], image.shape[0], depth, _p(s), _p(out), 0))
    return out


def _to_rgba(image, mode, hip=None):
    hip = hip or default_context()
    image = np.ascontiguousarray(image, np.float32)
    out = np.zeros(image.shape + (4,), np.uint8)
    hip.check(lib().fhip_to_rgba(hip._h, _p(image), image.shape[1], image.shape[0], mode, _p(out), 0))
    return out


def to_rgba_bitmap(image, transparent=False, hip=None):
    return _to_rgba(image, 1 if transparent else 0, hip)


def to_debug_bitmap(image, hip=None):
    return _to_rgba(image, 2, hip)


def to_rgba_distance(image, hip=None):
    return _to_rgba(image, 3, hip)


# ---- fidget_mesh: leaf sampling on the device -----------------------------------------------------------------------
MESH_LEAF = np.dtype([("bounds", np.float32, 6), ("path", np.uint64), ("mask", np.uint32), ("n_edges", np.uint32), ("n_verts", np.uint32),
                      ("pad", np.uint32), ("inter", np.uint16, (12, 3)), ("pad2", np.uint16, 4), ("pos", np.float32, (12, 3)),
                      ("grad", np.float32, (12, 4)), ("vert", np.float32, (4, 3)), ("qef_err", np.float32, 4)])


def debug_walk_dual(cells, root, verts, parallel):
    """Octree::walk_dual of the library's host side on a given octree (fhip_debug_walk_dual): (triangles, vertices)"""
    cells = np.ascontiguousarray(cells, np.uint32)
    root = np.ascontiguousarray(root, np.uint32)
    verts = np.ascontiguousarray(verts, np.float32)
    c = np.zeros(2, np.uint64)
    lib().fhip_debug_walk_dual(_p(cells), len(cells), _p(root), _p(verts), len(verts), int(parallel), _p(c), None, None)
    tris = np.zeros((int(c[0]), 3), np.uint64)
    out = np.zeros((int(c[1]), 3), np.float32)
    lib().fhip_debug_walk_dual(_p(cells), len(cells), _p(root), _p(verts), len(verts), int(parallel), _p(c), _p(tris), _p(out))
    return tris, out


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


class _MeshHandle(_Handle):
    """owner of an fhip_mesh whose arrays numpy views borrow"""
    def view(self, ptr, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if not n or not ptr:
            return np.zeros(shape, dtype)
        buf = (C.c_uint8 * n).from_address(ptr)
        buf._owner = self           # (numpy keeps `buf` as the view's base, `buf` keeps the handle)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)


def mesh(shape, depth, world_to_model=None, vars=None):
    """fidget_mesh::Octree::build(...).walk_dual(): (triangles [n, 3] uint64, vertices [m, 3] float32, counts)"""
    return mesh_sample(shape, depth, world_to_model, vars, _build=True)


class _DeviceArray:
    """An array of a mesh in device memory, as `__cuda_array_interface__` (version 2) describes it; keeps the mesh's handle alive.
    The interface's read-only flag is False - torch refuses a read-only one - but the array is the mesh's: a consumer reads it."""
    def __init__(self, owner, ptr, shape, typestr):
        self._owner = owner
        self.ptr, self.shape = int(ptr), tuple(shape)
        self.__cuda_array_interface__ = {"shape": self.shape, "typestr": typestr, "data": (self.ptr, False), "version": 2, "strides": None}


class Mesh:
    """A mesh of `build_mesh`: fidget_mesh::Mesh { vertices, triangles } (fidget-mesh/src/lib.rs:64-69), with what a caller does with
    one on the device.  `.triangles` [n, 3] uint64, `.vertices` [m, 3] float32, `.counts`: the views `mesh()` returns, borrowed from the handle."""
    def __init__(self, owner, hip, triangles, vertices, counts):
        self._owner, self._hip = owner, hip
        self.triangles, self.vertices, self.counts = triangles, vertices, counts

    def stl(self, out=None):
        """Mesh::write_stl's bytes (fhip_mesh_stl) as a numpy uint8 array; with `out` (a torch CUDA uint8 tensor of at least that many
        bytes) the call is asynchronous on the context's stream and returns `out`."""
        n = int(lib().fhip_mesh_stl_bytes(self._owner.h))
        if out is not None:
            assert out.is_cuda and out.is_contiguous() and out.element_size() == 1 and out.numel() >= n
            self._hip.check(lib().fhip_mesh_stl(self._hip._h, self._owner.h, _dev_ptr(out), 1))
            return out
        buf = np.zeros(n, np.uint8)
        self._hip.check(lib().fhip_mesh_stl(self._hip._h, self._owner.h, _p(buf), 0))
        return buf

    def write_stl(self, path):
        """Mesh::write_stl (fidget-mesh/src/output.rs:5-38) to a file"""
        with open(path, "wb") as f:
            f.write(self.stl().tobytes())

    def vertex_grads(self, shape, vars=None, out=None):
        """fhip_mesh_vertex_grads: [m, 4] float32 {v, dx, dy, dz} of `shape` at the mesh's vertices (model space, unnormalised); with
        `out` (a torch CUDA float32 tensor [m, 4]) the result stays on the device and `out` is returned."""
        n = len(self.vertices)
        vk, vv = _var_arrays(shape, vars)
        ax = None
        if shape._vars is not None:
            ax = np.array(shape._vars, dtype=np.int32)
            vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
        if out is not None:
            assert out.is_cuda and out.is_contiguous() and out.element_size() == 4 and out.numel() == 4 * n
            ptr, dev, res = _dev_ptr(out), 1, out
        else:
            res = np.zeros((n, 4), np.float32)
            ptr, dev = _p(res), 0
        st = lib().fhip_mesh_vertex_grads(self._hip._h, shape._h, self._owner.h, _p(ax), _p(vk), _p(vv), len(vk), ptr, dev)
        if st == 4:
            raise ValueError("MissingVar")
        self._hip.check(st)
        return res

    def voxelize(self, depth, out=None):
        """`voxelize_mesh(self, depth, out=out)`: the solid this mesh encloses as a Voxels, from the resident arrays where there are any"""
        return voxelize_mesh(self, depth, out=out)

    def topology(self, weld=None):
        """`mesh_topology(self, weld)`: what kind of mesh this is - edges, shells, volume - from the resident arrays where there are any"""
        return mesh_topology(self, weld)

    def slices(self, zs):
        """`mesh_slices(self, zs)`: the contour loops in which the planes z = zs[p] cut this mesh, from the resident arrays where there are any"""
        return mesh_slices(self, zs)

    def vertices_device(self):
        """The vertices where the dual walk left them in device memory ([m, 3] float32), as an object carrying
        `__cuda_array_interface__` that keeps the mesh alive - `torch.as_tensor(obj, device="cuda")` views it; None when the
        arrays are not resident (built with keep_device off, by the host's walk, or empty)."""
        ptr = lib().fhip_mesh_vertices_dev(self._owner.h)
        return _DeviceArray(self._owner, ptr, (len(self.vertices), 3), "<f4") if ptr else None

    def triangles_device(self):
        """... and the triangles ([n, 3] vertex indices; "<u8", which torch takes from version 2.3 on - older ones want
        `torch.as_tensor(obj, device="cuda")` of a copy of the interface with typestr "<i8": the indices are below 2^63)"""
        ptr = lib().fhip_mesh_triangles_dev(self._owner.h)
        return _DeviceArray(self._owner, ptr, (len(self.triangles), 3), "<u8") if ptr else None


def build_mesh(shape, depth, world_to_model=None, vars=None, keep_device=True):
    """fidget_mesh::Octree::build(...).walk_dual() as a `Mesh` object.  keep_device: context option mesh_keep_device for this build (the
    option is restored afterwards) - the device walk's arrays stay resident for .stl(), .vertex_grads() and the *_device() views."""
    hip = shape.hip
    with hip.options(mesh_keep_device=1 if keep_device else 0):
        owner, tris, verts, counts = mesh_sample(shape, depth, world_to_model, vars, _build=True, _owner=True)
    return Mesh(owner, hip, tris, verts, counts)


def mesh_part(shape, depth, part, n_parts, world_to_model=None, vars=None, alloc=None):
    """The device side of a mesh build for part `part` of `n_parts` (the root's octants o with o * n_parts // 8 == part;
    fhip_mesh_sample_part), as the flat uint8 buffer fhip_mesh_part_export writes: what a rank sends to the merging rank.
    `alloc(nbytes)` -> writable uint8 array to export into (shared memory, say); default: a fresh numpy array."""
    hip = shape.hip
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    vk, vv = _var_arrays(shape, vars)
    ax = None
    if shape._vars is not None:
        ax = np.array(shape._vars, dtype=np.int32)
        vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
    h = C.c_void_p()
    st = lib().fhip_mesh_sample_part(hip._h, shape._h, depth, _p(w2m), _p(ax), _p(vk), _p(vv), len(vk), part, n_parts, C.byref(h))
    if st == 4:
        raise ValueError("MissingVar")
    hip.check(st)
    try:
        n = int(lib().fhip_mesh_part_bytes(h))
        buf = np.zeros(n, np.uint8) if alloc is None else alloc(n)
        assert buf.dtype == np.uint8 and buf.size == n and buf.flags.c_contiguous
        lib().fhip_mesh_part_export(h, buf.ctypes.data_as(C.c_void_p))
    finally:
        lib().fhip_mesh_free(h)
    return buf


def mesh_merge(parts, world_to_model=None, hip=None):
    """fhip_mesh_merge: the buffers of all parts (parts[k] = mesh_part(.., k, len(parts))) -> (triangles, vertices, counts),
    the mesh of `mesh()` on one GPU.  `hip`: a context for the error text only (no device work)."""
    parts = [np.ascontiguousarray(b, np.uint8) for b in parts]
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    ptrs = (C.c_void_p * len(parts))(*[b.ctypes.data for b in parts])
    sizes = np.array([b.size for b in parts], np.uint64)
    h = C.c_void_p()
    st = lib().fhip_mesh_merge(hip._h if hip is not None else None, ptrs, _p(sizes), len(parts), _p(w2m), C.byref(h))
    if st:
        if hip is not None:
            hip.check(st)
        raise RuntimeError(f"fhip_mesh_merge: status {st}")
    try:
        c = np.zeros(8, np.uint64)
        lib().fhip_mesh_counts(h, _p(c))
        verts = np.zeros((int(c[6]), 3), np.float32)
        tris = np.zeros((int(c[7]), 3), np.uint64)
        if len(verts):
            lib().fhip_mesh_vertices(h, _p(verts))
        if len(tris):
            lib().fhip_mesh_triangles(h, _p(tris))
    finally:
        lib().fhip_mesh_free(h)
    return tris, verts, {"cells": int(c[0]), "full": int(c[1]), "empty": int(c[2]), "leaf_cells": int(c[3]), "levels": int(c[5])}


def mesh_sample(shape, depth, world_to_model=None, vars=None, _build=False, _owner=False):
    """The evaluation side of fidget_mesh::Octree::build on the device (fhip_mesh_sample): returns (leaf records as a
    MESH_LEAF array, counts dict)."""
    hip = shape.hip
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    vk, vv = _var_arrays(shape, vars)
    ax = None
    if shape._vars is not None:
        ax = np.array(shape._vars, dtype=np.int32)
        vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
    h = C.c_void_p()
    fn = lib().fhip_mesh_build if _build else lib().fhip_mesh_sample
    st = fn(hip._h, shape._h, depth, _p(w2m), _p(ax), _p(vk), _p(vv), len(vk), C.byref(h))
    if st == 4:
        raise ValueError("MissingVar")
    hip.check(st)
    try:
        c = np.zeros(8, np.uint64)
        lib().fhip_mesh_counts(h, _p(c))
        assert int(c[4]) == MESH_LEAF.itemsize, (int(c[4]), MESH_LEAF.itemsize)
        counts = {"cells": int(c[0]), "full": int(c[1]), "empty": int(c[2]), "leaf_cells": int(c[3]), "levels": int(c[5])}
        if _build:
            # the arrays where the mesh holds them, no copy: numpy views whose base keeps the handle (freed with the last of them)
            owner = _MeshHandle(h, lib().fhip_mesh_free)
            h = None
            verts = owner.view(lib().fhip_mesh_vertices_ptr(owner.h), (int(c[6]), 3), np.float32)
            tris = owner.view(lib().fhip_mesh_triangles_ptr(owner.h), (int(c[7]), 3), np.uint64)
            return (owner, tris, verts, counts) if _owner else (tris, verts, counts)
        leaves = np.zeros(int(c[3]), MESH_LEAF)
        if len(leaves):
            lib().fhip_mesh_leaves(h, _p(leaves))
    finally:
        lib().fhip_mesh_free(h)
    return leaves, {"cells": int(c[0]), "full": int(c[1]), "empty": int(c[2]), "leaf_cells": int(c[3]), "levels": int(c[5])}


# ---- shape occupancy: volume, centroid, second moments, bounds (fhip_shape_occupancy) ------------------------------------
class OccupancyStruct(C.Structure):
    """fhip_occupancy (include/fidget_hip.h)"""
    _fields_ = [("n", C.c_uint64), ("s1", C.c_uint64 * 3), ("s2", C.c_uint64 * 6), ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3),
                ("grid", C.c_uint32), ("pad", C.c_uint32), ("cells", C.c_uint64 * 4)]


class Occupancy:
    """The inside voxels of the grid of N = 4 << depth per axis over [-1, 1]^3, as the integers fhip_shape_occupancy returns (Python
    ints: n, s1 (sum of i, j, k), s2 (sum of i^2, j^2, k^2, ij, ik, jk), lo / hi (inclusive, lo = N and hi = 0 when empty), grid,
    cells = {"cells", "full", "empty", "leaf_cells"} as mesh_sample counts them) and what follows from them in float64, in the region's
    own coordinates, with h = 2 / N."""

    def __init__(self, raw):
        self.n = int(raw.n)
        self.s1 = tuple(int(v) for v in raw.s1)
        self.s2 = tuple(int(v) for v in raw.s2)
        self.lo = tuple(int(v) for v in raw.lo)
        self.hi = tuple(int(v) for v in raw.hi)
        self.grid = int(raw.grid)
        self.cells = dict(zip(("cells", "full", "empty", "leaf_cells"), (int(v) for v in raw.cells)))

    @property
    def h(self):
        return 2.0 / self.grid

    @property
    def volume(self):
        return self.n * self.h ** 3

    @property
    def centroid(self):
        """mean of the inside voxels' centres, -1 + (i + 1/2) h per axis; NaN for an empty shape"""
        if self.n == 0:
            return np.full(3, np.nan)
        # (the quotient of the integers first: exact to the last place)
        return np.array([-1.0 + (s / self.n + 0.5) * self.h for s in self.s1], np.float64)

    @property
    def covariance(self):
        """second moments of the inside voxels' centres about the centroid, [3, 3]: h^2 (sum ab / n - (sum a / n)(sum b / n)), the
        numerator n sum ab - sum a sum b taken in integers, so nothing cancels in floating point"""
        if self.n == 0:
            return np.full((3, 3), np.nan)
        pair = {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (0, 2): 4, (1, 2): 5}
        out = np.zeros((3, 3), np.float64)
        for a in range(3):
            for b in range(3):
                num = self.n * self.s2[pair[(min(a, b), max(a, b))]] - self.s1[a] * self.s1[b]
                out[a, b] = num / (self.n * self.n) * self.h * self.h
        return out

    @property
    def bounds(self):
        """the faces of the outermost inside voxels: ([x0, y0, z0], [x1, y1, z1]); NaN for an empty shape"""
        if self.n == 0:
            return np.full(3, np.nan), np.full(3, np.nan)
        return (np.array([-1.0 + l * self.h for l in self.lo], np.float64), np.array([-1.0 + (u + 1) * self.h for u in self.hi], np.float64))

    def __repr__(self):
        return f"Occupancy(grid={self.grid}, n={self.n}, s1={self.s1}, s2={self.s2}, lo={self.lo}, hi={self.hi}, cells={self.cells})"


def occupancy(shape, depth, world_to_model=None, vars=None):
    """fhip_shape_occupancy: the solid `shape < 0` on the grid of 4 << depth voxels per axis over [-1, 1]^3 (world_to_model as for
    `mesh`), counted down the mesher's octree -> Occupancy"""
    hip = shape.hip
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    vk, vv = _var_arrays(shape, vars)
    ax = None
    if shape._vars is not None:
        ax = np.array(shape._vars, dtype=np.int32)
        vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
    raw = OccupancyStruct()
    st = lib().fhip_shape_occupancy(hip._h, shape._h, depth, _p(w2m), _p(ax), _p(vk), _p(vv), len(vk), C.byref(raw))
    if st == 4:
        raise ValueError("MissingVar")
    hip.check(st)
    return Occupancy(raw)


# ---- shape voxels: the inside voxels as a packed bitmap, layer images, voxels per layer (fhip_shape_voxels) ---------------
def voxels_unpack(bricks):
    """bricks uint64 [B, B, B] (indexed [bz, by, bx]; bit lx + 4 ly + 16 lz of a word: voxel (4 bx + lx, 4 by + ly, 4 bz + lz)) ->
    bool [N, N, N], N = 4 B, indexed [i, j, k]"""
    b = np.ascontiguousarray(bricks, "<u8")
    B = b.shape[0]
    bits = np.unpackbits(b.view(np.uint8).reshape(B, B, B, 8), axis=-1, bitorder="little")       # [bz, by, bx, 16 lz + 4 ly + lx]
    return bits.reshape(B, B, B, 4, 4, 4).transpose(2, 5, 1, 4, 0, 3).reshape(4 * B, 4 * B, 4 * B).astype(bool)


def _bitmap_out(depth, out, device=None, aligned=False):
    """Where a call writes a result bitmap of this depth -> (out, pointer, on the device?).  `out`: a contiguous torch CUDA tensor of at
    least 8 B^3 bytes, B = 1 << depth, or a contiguous writeable numpy array of that size; without it a new one - a torch int64
    [B, B, B] on `device`, or with no device a numpy uint64 [B, B, B].  `aligned`: a tensor that is not 8-byte aligned fails the
    assertion here; otherwise it is left to the library's error."""
    B = 1 << depth
    words = int(lib().fhip_voxels_words(depth))       # (0 beyond depth 10: the call refuses before it touches `out`)
    if out is None and device is not None:
        import torch
        out = torch.empty((B, B, B), dtype=torch.int64, device=device)
    if out is not None and not isinstance(out, np.ndarray):
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() >= 8 * words and (not aligned or out.data_ptr() % 8 == 0)
        return out, _dev_ptr(out), 1
    if out is None:
        out = np.zeros((B, B, B) if words else 0, np.uint64)
    assert out.flags.c_contiguous and out.flags.writeable and out.nbytes >= 8 * words
    return out, _p(out), 0


def _bitmap_of(hip, out, dev, depth, cells=None):
    """the bitmap a call wrote into `out` (`_bitmap_out`) -> Voxels: the first 8 B^3 bytes as [B, B, B] bricks"""
    B = 1 << depth
    if dev:
        import torch
        bricks = out.reshape(-1).view(torch.uint8)[:8 * B ** 3].view(torch.int64).view(B, B, B)
    else:
        bricks = out.reshape(-1).view(np.uint8)[:8 * B ** 3].view(np.uint64).reshape(B, B, B)
    return Voxels(hip, bricks, depth, cells)


class Voxels:
    """The bitmap of `voxelize`: `.bricks` [B, B, B] (numpy uint64, or a view of the caller's torch CUDA tensor as int64), `.depth`,
    `.grid` = N = 4 B, `.cells` = {"cells", "full", "empty", "leaf_cells"} as Occupancy's, `.n` = the number of inside voxels.  What is
    made of it runs where the bricks are: on the host's arrays through the library's staging buffers, or on the device in place and
    asynchronous on the context's stream."""

    def __init__(self, hip, bricks, depth, cells):
        self._hip, self.bricks, self.depth, self.grid, self.cells = hip, bricks, int(depth), 4 << int(depth), cells
        self._n = None

    @property
    def on_device(self):
        return not isinstance(self.bricks, np.ndarray)

    def _ptr(self):
        return _dev_ptr(self.bricks) if self.on_device else _p(self.bricks)

    def slices(self, k0, k1, out=None):
        """fhip_voxels_slices: uint8 [k1 - k0, N, N], [k - k0, j, i] = 255 where voxel (i, j, k) is inside, 0 where not: numpy for bricks
        on the host; for bricks on the device a torch CUDA tensor (`out`, contiguous uint8 of that size, or a new one)"""
        N = self.grid
        k0, k1 = int(k0), int(k1)
        n = max(k1 - k0, 0) * N * N
        if self.on_device:
            if out is None:
                import torch
                out = torch.empty((max(k1 - k0, 0), N, N), dtype=torch.uint8, device=self.bricks.device)
            assert out.is_cuda and out.is_contiguous() and out.element_size() == 1 and out.numel() >= n
            self._hip.check(lib().fhip_voxels_slices(self._hip._h, self._ptr(), self.depth, k0, k1, _dev_ptr(out), 1))
            return out
        assert out is None, "bricks on the host: the images are returned as a numpy array"
        img = np.zeros((max(k1 - k0, 0), N, N), np.uint8)
        self._hip.check(lib().fhip_voxels_slices(self._hip._h, self._ptr(), self.depth, k0, k1, _p(img), 0))
        return img

    def layer_counts(self):
        """fhip_voxels_layer_counts: [N] inside voxels per third index k: numpy uint64, or a torch CUDA int64 tensor for bricks on the device"""
        if self.on_device:
            import torch
            out = torch.empty(self.grid, dtype=torch.int64, device=self.bricks.device)
            self._hip.check(lib().fhip_voxels_layer_counts(self._hip._h, self._ptr(), self.depth, _dev_ptr(out), 1))
            return out
        out = np.zeros(self.grid, np.uint64)
        self._hip.check(lib().fhip_voxels_layer_counts(self._hip._h, self._ptr(), self.depth, _p(out), 0))
        return out

    @property
    def n(self):
        """the number of set bits (Occupancy.n at the same depth)"""
        if self._n is None:
            self._n = int(self.layer_counts().sum())
        return self._n

    def inside(self):
        """bool [N, N, N] indexed [i, j, k], unpacked on the host (bricks on the device are copied there first)"""
        b = self.bricks.cpu().numpy().view(np.uint64) if self.on_device else self.bricks
        return voxels_unpack(b)

    def components(self, connectivity=6, complement=False):
        """fhip_voxels_components: the connected parts of the set bits - with `complement` of the clear bits, whose parts away from the
        grid's border are the enclosed voids - under connectivity 6 (faces) or 26 (faces, edges, corners) -> Components"""
        h = C.c_void_p()
        self._hip.check(lib().fhip_voxels_components(self._hip._h, self._ptr(), self.depth, int(self.on_device), int(connectivity), int(bool(complement)), C.byref(h)))
        return Components(self, _Handle(h.value, lib().fhip_components_free), int(connectivity), bool(complement))

    def distance(self, complement=False):
        """fhip_voxels_distance: the exact squared Euclidean distance, in voxels, from every voxel to the nearest set bit - with
        `complement` to the nearest clear bit -> DistanceField"""
        h = C.c_void_p()
        self._hip.check(lib().fhip_voxels_distance(self._hip._h, self._ptr(), self.depth, int(self.on_device), int(bool(complement)), C.byref(h)))
        return DistanceField(self, _Handle(h.value, lib().fhip_distance_free), bool(complement))

    def thickness(self, complement=False):
        """the local thickness of the solid's walls - `distance(complement=True).thickness()` - or with `complement` the local width of
        the empty space - `distance().thickness()` -> ThicknessField"""
        return self.distance(complement=not complement).thickness()

    def mesh(self):
        """fhip_voxels_mesh: the boundary of the set voxels -> Mesh.  Every exposed face of a voxel is two triangles, counter-clockwise
        seen from outside, in the order (brick word, direction -x +x -y +y -z +z, bit); the vertices are the lattice corners the faces
        use, one each, at float(2 a - N) / N in the cube [-1, 1]^3 the bitmap was sampled in.  The arrays are resident on the device
        (`.stl()`, `.vertex_grads()`, `.vertices_device()`, `.triangles_device()`) and copied to the host (`.triangles`, `.vertices`);
        `.counts` holds the octree's counters, all 0 here.  Overflow: 2^32 triangles or vertices and more."""
        h = C.c_void_p()
        self._hip.check(lib().fhip_voxels_mesh(self._hip._h, self._ptr(), self.depth, int(self.on_device), C.byref(h)))
        owner = _MeshHandle(h.value, lib().fhip_mesh_free)
        c = np.zeros(8, np.uint64)
        lib().fhip_mesh_counts(owner.h, _p(c))
        counts = {"cells": int(c[0]), "full": int(c[1]), "empty": int(c[2]), "leaf_cells": int(c[3]), "levels": int(c[5])}
        verts = owner.view(lib().fhip_mesh_vertices_ptr(owner.h), (int(c[6]), 3), np.float32)
        tris = owner.view(lib().fhip_mesh_triangles_ptr(owner.h), (int(c[7]), 3), np.uint64)
        return Mesh(owner, self._hip, tris, verts, counts)

    def surface(self):
        """fhip_voxels_surface: the counting pass of `mesh()` alone -> Surface: exposed faces per direction, used lattice corners and
        edges, and from them the area and the Euler number"""
        out = np.zeros(10, np.uint64)
        self._hip.check(lib().fhip_voxels_surface(self._hip._h, self._ptr(), self.depth, int(self.on_device), _p(out)))
        return Surface(self.grid, out)

    def offset(self, r, out=None):
        """the solid grown by a ball of radius r >= 0 - `distance().within(r)` - or shrunk by one of radius -r -
        `distance(complement=True).beyond(-r)`: what stays is farther than |r| from the nearest clear voxel, so offset(-1) keeps the
        voxels at distance 1 and removes nothing; to take the surface layer off, use beyond(squared=1) -> Voxels (`out` as for `within`)"""
        if r >= 0:
            return self.distance().within(r, out=out)
        return self.distance(complement=True).beyond(-r, out=out)

    def opened(self, r):
        """shrunk by r, then grown by r: drops what no ball of that radius fits into (specks, thin walls)"""
        return self.offset(-r).offset(r)

    def closed(self, r):
        """grown by r, then shrunk by r: fills what no ball of that radius fits into (pinholes, thin gaps)"""
        return self.offset(r).offset(-r)

    # ---- along a direction: d = 0 .. 5 = -x, +x, -y, +y, -z, +z, e(d) its unit vector, d ^ 1 its opposite --------------------------
    def _out_device(self):
        """where a new result bitmap goes (`_bitmap_out`): the bricks' device, or None for the host"""
        return self.bricks.device if self.on_device else None

    def flow(self, dir, blockers=None, with_seeds=False, out=None):
        """fhip_voxels_flow: these voxels as seeds S flowing towards direction `dir` past the blockers K (a Voxels of the same depth, in
        the same place as these; None: none) -> Voxels R (`.cells` None) with R(p) = (R(p - e) | S(p - e)) & ~K(p), R and S false
        outside the grid: R(p) holds iff there is t >= 1 with S(p - t e) and no blocker at p - s e for all 0 <= s < t.  A seed that is
        itself blocked still emits; a blocked voxel is never in R.  `with_seeds`: R | S.  `out` as for `DistanceField.within`, not
        the seeds' or the blockers' own array.  The space trapped along an axis - reachable from neither side, an undercut of a
        two-part mould - is the AND of the two opposite shadows: `a.shadow(4).bricks & a.shadow(5).bricks`."""
        if blockers is not None:
            if not isinstance(blockers, Voxels) or blockers.depth != self.depth:
                raise ValueError("blockers: a Voxels of the same depth")
            if blockers.on_device != self.on_device:
                raise ValueError("seeds and blockers live in the same place: both on the host or both on the device")
        out, ptr, dev = _bitmap_out(self.depth, out, self._out_device())
        self._hip.check(lib().fhip_voxels_flow(self._hip._h, self._ptr(), None if blockers is None else blockers._ptr(), self.depth, int(self.on_device),
                                               int(dir), 1 if with_seeds else 0, ptr, dev))
        return _bitmap_of(self._hip, out, dev, self.depth)

    def shadow(self, dir, out=None):
        """the clear voxels with a set voxel behind them, seen towards `dir`: `flow(dir, blockers=self)`"""
        return self.flow(dir, blockers=self, out=out)

    def swept(self, dir, out=None):
        """the solid swept towards `dir` to the grid's border - the shadow and the solid: `flow(dir, with_seeds=True)`"""
        return self.flow(dir, with_seeds=True, out=out)

    def overhangs(self, up=5, reach2=1, bed=True, out=None):
        """fhip_voxels_overhangs: the set voxels that are not supported when the part is built towards `up` -> Voxels.  p is supported iff
        there is a set q one layer below, (q - p) . e(up) = -1, whose squared perpendicular offset is at most `reach2` (0 .. 16): a
        Euclidean disc - 0 straight below only, 1 a plus of five, 2 the 3 x 3 square.  For p in the first layer every q counts as set
        iff `bed`, and as clear otherwise.  `out` as for `flow`."""
        out, ptr, dev = _bitmap_out(self.depth, out, self._out_device())
        self._hip.check(lib().fhip_voxels_overhangs(self._hip._h, self._ptr(), self.depth, int(self.on_device), int(up), int(reach2), int(bool(bed)), ptr, dev))
        return _bitmap_of(self._hip, out, dev, self.depth)

    def supports(self, up=5, reach2=1, bed=True, out=None):
        """the clear columns under every overhanging voxel, down to the next set voxel or the grid's border:
        `overhangs(up, reach2, bed).flow(up ^ 1, blockers=self)`.  On the device the calls are asynchronous on the context's stream: a
        bitmap handed to them must stay allocated until that stream has passed them - with a context on a stream other than torch's
        current one, keep the tensors (or synchronise) before dropping them."""
        over = self.overhangs(up, reach2, bed)
        res = over.flow(int(up) ^ 1, blockers=self, out=out)
        res._seeds = over          # (on the device the flow may still be reading them: they live as long as the result)
        return res

    def heights(self, axis=2, out=None):
        """fhip_voxels_heights: int32 [3, N, N] over the columns along `axis`, indexed by the two remaining coordinates, the lower axis
        fastest - axis 2 gives [j][i], 1 [k][i], 0 [k][j].  Plane 0: the smallest coordinate along the axis of a set voxel in the
        column, -1 in an empty column; plane 1: the largest, -1 likewise; plane 2: the number of set voxels.  numpy, or a torch CUDA
        int32 tensor for bricks on the device; `out`: a contiguous array of either kind with 4-byte elements and that size."""
        N = self.grid
        if out is None and self.on_device:
            import torch
            out = torch.empty((3, N, N), dtype=torch.int32, device=self.bricks.device)
        if out is not None and not isinstance(out, np.ndarray):
            assert out.is_cuda and out.is_contiguous() and out.element_size() == 4 and out.numel() >= 3 * N * N
            ptr, dev = _dev_ptr(out), 1
        else:
            if out is None:
                out = np.zeros((3, N, N), np.int32)
            assert out.flags.c_contiguous and out.flags.writeable and out.itemsize == 4 and out.size >= 3 * N * N
            ptr, dev = _p(out), 0
        self._hip.check(lib().fhip_voxels_heights(self._hip._h, self._ptr(), self.depth, int(self.on_device), int(axis), ptr, dev))
        return out

    def outlines(self, k0, k1, connectivity=4):
        """fhip_voxels_outlines: the boundary loops of every layer k0 <= k < k1 (layers along z, as for `slices`) -> Outlines.  The
        loops are closed rectilinear polygons over the corners (a, b), 0 <= a, b <= N, of the layer image P(i, j) = voxel (i, j, k),
        clear outside the grid; directed with the inside on the left, so an outer boundary runs counter-clockwise (area2 > 0) and a
        hole clockwise (area2 < 0); vertices only where the outline turns.  `connectivity` 4: pixels that touch at a corner alone
        are separate, 8: they are joined - it decides how the two vertices of a saddle corner pair up.  One blocking call, run where
        the bricks are; the vertices' arrays stay in device memory.  Integers throughout: the same bits from run to run."""
        h = C.c_void_p()
        self._hip.check(lib().fhip_voxels_outlines(self._hip._h, self._ptr(), self.depth, int(self.on_device), int(k0), int(k1), int(connectivity), C.byref(h)))
        return Outlines(_Handle(h.value, lib().fhip_outlines_free), self._hip)

    def outline(self, k, connectivity=4):
        """the loops of the one layer k: `outlines(k, k + 1)`"""
        return self.outlines(k, int(k) + 1, connectivity)

    def __repr__(self):
        return f"Voxels(depth={self.depth}, grid={self.grid}, cells={self.cells}, on_device={self.on_device})"


class Outlines:
    """The loops of `Voxels.outlines(k0, k1)`.  `.grid` = N, `.k0`, `.k1`, `.connectivity`, `.n_vertices`, `.n_loops`, `.n_layers`.
    Per layer (index k - k0): `.vertex_start` and `.loop_start` uint64 [K + 1], the ranges of the layer's vertices and loops - ids are
    global, layers ascending; `.layer_area2` int64 [K] = twice the layer's set voxels; `.layer_perimeter` uint64 [K] = its unit
    boundary edges.  Per vertex: `.xy()` uint16 [n, 2] the corner (a, b); `.next()` uint32 [n] the next vertex along the loop, a
    permutation inside each layer; `.loop_of()` uint32 [n].  Per loop (`.table()`): leader - its smallest vertex id; loops are numbered
    by ascending leader - n_vertices, area2 (int64 shoelace sum: > 0 an outer boundary, < 0 a hole), perimeter, lo and hi [., 2].
    The vertices' arrays stay in device memory (`.xy_device()` ...); host copies are made when first asked for."""

    def __init__(self, owner, hip):
        self._owner, self._hip = owner, hip
        c = np.zeros(8, np.uint64)
        lib().fhip_outlines_counts(owner.h, _p(c))
        self.n_vertices, self.n_loops, self.n_layers, self.grid, self.k0, self.connectivity = (int(v) for v in c[:6])
        self.k1 = self.k0 + self.n_layers
        K = self.n_layers
        self.vertex_start, self.loop_start = np.zeros(K + 1, np.uint64), np.zeros(K + 1, np.uint64)
        self.layer_area2, self.layer_perimeter = np.zeros(K, np.int64), np.zeros(K, np.uint64)
        hip.check(lib().fhip_outlines_layers(owner.h, _p(self.vertex_start), _p(self.loop_start), _p(self.layer_area2), _p(self.layer_perimeter)))
        self._host = None
        self._table = None

    def _layer(self, k, start):
        """the range of layer k in `start`, or everything"""
        if k is None:
            return 0, int(start[-1])
        k = int(k)
        if not self.k0 <= k < self.k1:
            raise IndexError(f"layer {k} is not among {self.k0} .. {self.k1 - 1}")
        return int(start[k - self.k0]), int(start[k - self.k0 + 1])

    def _vertices(self):
        if self._host is None:
            n = self.n_vertices
            xy, nxt, loop = np.zeros((n, 2), np.uint16), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
            self._hip.check(lib().fhip_outlines_vertices(self._owner.h, 0, n, _p(xy), _p(nxt), _p(loop)))
            self._host = (xy, nxt, loop)
        return self._host

    def xy(self, k=None):
        """uint16 [n, 2]: the corners (a, b) of all vertices, or of layer k's"""
        lo, hi = self._layer(k, self.vertex_start)
        return self._vertices()[0][lo:hi]

    def next(self, k=None):
        """uint32 [n]: every vertex's successor; for one layer the ids stay global - subtract `vertex_start[k - k0]`"""
        lo, hi = self._layer(k, self.vertex_start)
        return self._vertices()[1][lo:hi]

    def loop_of(self, k=None):
        """uint32 [n]: every vertex's loop; global ids likewise"""
        lo, hi = self._layer(k, self.vertex_start)
        return self._vertices()[2][lo:hi]

    def table(self, k=None):
        """{"leader", "n_vertices", "area2", "perimeter", "lo", "hi"}: a row per loop, of all layers or of layer k"""
        if self._table is None:
            n = self.n_loops
            t = {"leader": np.zeros(n, np.uint32), "n_vertices": np.zeros(n, np.uint32), "area2": np.zeros(n, np.int64), "perimeter": np.zeros(n, np.uint64),
                 "lo": np.zeros((n, 2), np.uint16), "hi": np.zeros((n, 2), np.uint16)}
            self._hip.check(lib().fhip_outlines_loops(self._owner.h, 0, n, *(_p(t[key]) for key in ("leader", "n_vertices", "area2", "perimeter", "lo", "hi"))))
            self._table = t
        lo, hi = self._layer(k, self.loop_start)
        return {key: a[lo:hi] for key, a in self._table.items()}

    def polygons(self, k):
        """layer k's loops as int arrays [m, 2] of corners, each from its leader on, in loop order: walked along `next` on the host"""
        xy, nxt, _ = self._vertices()
        t = self.table(k)
        out = []
        for leader, m in zip(t["leader"], t["n_vertices"]):
            ids, v = np.zeros(int(m), np.int64), int(leader)
            for q in range(int(m)):
                ids[q] = v
                v = int(nxt[v])
            out.append(xy[ids].astype(np.int64))
        return out

    def world(self, k):
        """-> (polygons as float32 [m, 2] in the cube [-1, 1]^3 - corner a at float(2 a - N) / N, as `Voxels.mesh` places it - and the
        layer's z, its centre float(2 k + 1 - N) / N)"""
        N = self.grid
        return [((2 * p - N).astype(np.float32) / np.float32(N)) for p in self.polygons(k)], float(np.float32(2 * int(k) + 1 - N) / np.float32(N))

    def svg(self, k, path=None):
        """Layer k as one <path fill-rule="evenodd"> per loop, `M x y L x y ... Z`, in `world`'s coordinates with y negated - SVG's y
        grows downward - and the cube's square as the viewBox, like `Contours.svg`.  Returns the text; written to `path` when given."""
        polys, _ = self.world(k)
        paths = "".join('<path fill-rule="evenodd" d="M ' + " L ".join(f"{float(x):.9g} {-float(y):.9g}" for x, y in p) + ' Z"/>\n' for p in polys)
        text = f'<svg xmlns="http://www.w3.org/2000/svg" viewBox="-1 -1 2 2">\n{paths}</svg>\n'
        if path is not None:
            with open(path, "w") as f:
                f.write(text)
        return text

    def _device(self, what, shape, typestr):
        ptr = getattr(lib(), f"fhip_outlines_{what}_dev")(self._owner.h)
        return _DeviceArray(self._owner, ptr, shape, typestr) if ptr else None

    def xy_device(self):
        """`.xy()` where it is in device memory ([n, 2] "<i2": the bits of the uint16 corners, which stay below 2^15) as an object
        carrying `__cuda_array_interface__` that keeps the result alive; None when there are no vertices"""
        return self._device("xy", (self.n_vertices, 2), "<i2")

    def next_device(self):
        """... `.next()` ("<i4": the bits of the uint32 ids, as `Contours.segments_device` gives its)"""
        return self._device("next", (self.n_vertices,), "<i4")

    def loop_of_device(self):
        """... and `.loop_of()` ("<i4")"""
        return self._device("loop", (self.n_vertices,), "<i4")

    def __repr__(self):
        return (f"Outlines(grid={self.grid}, layers={self.k0}..{self.k1}, connectivity={self.connectivity}, vertices={self.n_vertices}, "
                f"loops={self.n_loops})")


class Surface:
    """The surface summary of a bitmap (`Voxels.surface`): `.faces` the exposed faces per direction -x, +x, -y, +y, -z, +z; `.vertices`
    the lattice corners whose eight voxels are not all equal; `.edges` the lattice edges whose four voxels are not all equal; `.n` the
    set voxels.  `.n_faces` their sum over the directions, `.area` = n_faces h^2 with h = 2 / N, in the cube [-1, 1]^3; `.euler` =
    vertices - edges + n_faces: 2 for a solid without handles or voids, 2 more for every void, 2 fewer for every handle, 1 more where
    two parts touch along an edge or at a corner only.  Outside the grid is clear: the surface is closed."""
    def __init__(self, grid, raw):
        raw = [int(v) for v in raw]
        self.grid, self.faces, self.vertices, self.edges, self.n_faces, self.n = int(grid), tuple(raw[:6]), raw[6], raw[7], raw[8], raw[9]
        self.area = self.n_faces * (2.0 / self.grid) ** 2
        self.euler = self.vertices - self.edges + self.n_faces

    def __repr__(self):
        return f"Surface(grid={self.grid}, faces={self.faces}, vertices={self.vertices}, edges={self.edges}, area={self.area:.6g}, euler={self.euler})"


class DistanceField:
    """The exact Euclidean distance transform of a bitmap (`Voxels.distance`): per voxel the squared distance to the nearest foreground
    voxel, a uint32 - 0 on the foreground, 0xFFFFFFFF ("no distance"; -1 as int32) everywhere when there is no foreground.
    `.max_squared` the largest finite value, `.argmax` the voxel (i, j, k) of smallest index k N^2 + j N + i that has it (None without
    foreground), `.n` foreground voxels, `.depth`, `.grid`.  The field stays in device memory; results land where the bricks are - for
    bricks on the device those calls are asynchronous on the context's stream, as `Voxels.slices` is."""

    def __init__(self, voxels, owner, complement):
        self.voxels, self._owner, self.complement = voxels, owner, complement
        self._hip, self.depth, self.grid = voxels._hip, voxels.depth, voxels.grid
        c = np.zeros(4, np.uint64)
        lib().fhip_distance_info(owner.h, _p(c))
        self.max_squared, self.n = int(c[0]), int(c[2])
        N, idx = self.grid, int(c[1])
        self.argmax = None if idx == 0xFFFFFFFFFFFFFFFF else (idx % N, idx // N % N, idx // (N * N))

    def slices(self, k0, k1, out=None):
        """fhip_distance_slices: [k1 - k0, N, N], [k - k0, j, i] = the squared distance of voxel (i, j, k): numpy uint32 for bricks on the
        host; for bricks on the device a torch CUDA int32 tensor (`out`, contiguous, 4-byte elements, of that size, or a new one)"""
        v, N = self.voxels, self.grid
        k0, k1 = int(k0), int(k1)
        n = max(k1 - k0, 0) * N * N
        if v.on_device:
            if out is None:
                import torch
                out = torch.empty((max(k1 - k0, 0), N, N), dtype=torch.int32, device=v.bricks.device)
            assert out.is_cuda and out.is_contiguous() and out.element_size() == 4 and out.numel() >= n
            self._hip.check(lib().fhip_distance_slices(self._hip._h, self._owner.h, k0, k1, _dev_ptr(out), 1))
            return out
        assert out is None, "bricks on the host: the layers are returned as a numpy array"
        img = np.zeros((max(k1 - k0, 0), N, N), np.uint32)
        self._hip.check(lib().fhip_distance_slices(self._hip._h, self._owner.h, k0, k1, _p(img), 0))
        return img

    @property
    def squared_device(self):
        """the whole field where it is: uint32 [N, N, N] indexed [k, j, i], as `__cuda_array_interface__`"""
        N = self.grid
        return _DeviceArray(self._owner, lib().fhip_distance_dev(self._owner.h), (N, N, N), "<u4")

    def _threshold(self, r, squared, beyond, out):
        if (r is None) == (squared is None):
            raise ValueError("give exactly one of r and squared")
        if r is not None:
            if r < 0:
                raise ValueError("a radius is not negative")
            squared = math.floor(r * r)
        squared = int(squared)
        if squared < 0 or squared > 0xFFFFFFFF:
            raise FidgetHipError(6, "distance threshold: t at most 0xFFFFFFFE")
        out, ptr, dev = _bitmap_out(self.depth, out, self.voxels._out_device())
        if beyond == 2:          # (ThicknessField.thin)
            self._hip.check(lib().fhip_thickness_thin(self._hip._h, self._owner.h, squared, ptr, dev))
        else:
            self._hip.check(lib().fhip_distance_threshold(self._hip._h, self._owner.h, squared, int(beyond), ptr, dev))
        return _bitmap_of(self._hip, out, dev, self.depth)

    def within(self, r=None, squared=None, out=None):
        """fhip_distance_threshold: the voxels with d2 <= t as a bitmap -> Voxels (`.cells` None).  Exactly one of `r` - a radius in
        voxels, t = floor(r * r) - and `squared` - t itself.  `out` as for `Components.extract`: a contiguous torch CUDA tensor of at
        least 8 B^3 bytes, or a contiguous numpy array of that size, written completely; without it a new one where the bricks are."""
        return self._threshold(r, squared, 0, out)

    def beyond(self, r=None, squared=None, out=None):
        """... the voxels with d2 > t; "no distance" is beyond every t"""
        return self._threshold(r, squared, 1, out)

    def thickness(self):
        """fhip_distance_thickness: per voxel the squared radius of the largest ball that holds it and no foreground voxel of this field
        -> ThicknessField.  Refused for a field without foreground."""
        h = C.c_void_p()
        self._hip.check(lib().fhip_distance_thickness(self._hip._h, self._owner.h, C.byref(h)))
        return ThicknessField(self.voxels, _Handle(h.value, lib().fhip_distance_free), self.complement)

    def __repr__(self):
        return f"DistanceField(depth={self.depth}, grid={self.grid}, max_squared={self.max_squared}, argmax={self.argmax}, n={self.n}, complement={self.complement})"


class ThicknessField(DistanceField):
    """The local thickness of a distance field (`DistanceField.thickness`, `Voxels.thickness`): per voxel T = the largest F(c) over the
    centres c with F(c) > |p - c|^2, the squared radius of the largest ball that fits beside the field's foreground and holds the
    voxel; 0 on that foreground.  A uint32 in squared voxels, exact.  Of `distance(complement=True)` it is the wall thickness of the
    solid: a slab w voxels thick reads ceil(w / 2)^2 - 14 gives 49, 17 gives 81 - so 2 sqrt(T) is the wall in voxels, rounded up to even.
    Of `distance()` it is the local width of the empty space: pores, channels, clearance.
    `.max_squared`, `.argmax` the largest value and the voxel (i, j, k) of smallest index k N^2 + j N + i that has it; `.min_squared`,
    `.argmin` the smallest positive one likewise (None when nothing is covered); `.n` the voxels with T > 0; `.balls` how many balls
    were painted, of `.centres` candidates; `.complement` that of the distance field.  `slices`, `squared_device`, `within` and
    `beyond` are DistanceField's, on T."""

    def __init__(self, voxels, owner, complement):
        super().__init__(voxels, owner, complement)
        c = np.zeros(8, np.uint64)
        lib().fhip_thickness_info(owner.h, _p(c))
        N = self.grid

        def voxel(idx):
            return None if idx == 0xFFFFFFFFFFFFFFFF else (idx % N, idx // N % N, idx // (N * N))
        self.max_squared, self.argmax, self.n, self.centres, self.balls = int(c[0]), voxel(int(c[1])), int(c[4]), int(c[6]), int(c[7])
        self.min_squared, self.argmin = (int(c[2]), voxel(int(c[3]))) if self.n else (None, None)

    def thin(self, r=None, squared=None, out=None):
        """fhip_thickness_thin: the voxels with 0 < T <= t - what no ball larger than that reaches, the walls thinner than about
        2 sqrt(t) -> Voxels.  `r`, `squared` and `out` as for `within`."""
        return self._threshold(r, squared, 2, out)

    def histogram(self, edges_squared):
        """fhip_thickness_histogram: the voxels with e[b] <= T < e[b + 1] for 2 to 1024 ascending edges in squared voxels: numpy uint64
        [len(edges) - 1], or a torch CUDA int64 tensor for bricks on the device"""
        edges = np.ascontiguousarray(edges_squared, dtype=np.int64).reshape(-1)
        if len(edges) < 2 or len(edges) > 1024 or edges.min() < 0 or edges.max() > 0xFFFFFFFF or (np.diff(edges) < 0).any():
            raise ValueError("histogram: 2 to 1024 ascending edges, each a uint32")
        edges = edges.astype(np.uint32)
        if self.voxels.on_device:
            import torch
            dev = self.voxels.bricks.device
            d_edges = torch.from_numpy(edges.view(np.int32)).to(dev)
            out = torch.empty(len(edges) - 1, dtype=torch.int64, device=dev)
            self._hip.check(lib().fhip_thickness_histogram(self._hip._h, self._owner.h, _dev_ptr(d_edges), len(edges), _dev_ptr(out), 1))
            out._edges = d_edges          # (the call is asynchronous and reads them: they live as long as the result)
            return out
        out = np.zeros(len(edges) - 1, np.uint64)
        self._hip.check(lib().fhip_thickness_histogram(self._hip._h, self._owner.h, _p(edges), len(edges), _p(out), 0))
        return out

    def thickness(self):
        raise FidgetHipError(6, "thickness: of a distance field, not of a thickness")

    def __repr__(self):
        return (f"ThicknessField(depth={self.depth}, grid={self.grid}, max_squared={self.max_squared}, argmax={self.argmax}, min_squared={self.min_squared}, "
                f"argmin={self.argmin}, n={self.n}, balls={self.balls}, complement={self.complement})")


class Components:
    """The connected parts of a bitmap (`Voxels.components`), numbered by ascending seed - the voxel of smallest key word * 64 + bit:
    `.count`, `.nodes` (the bricks' own parts, what the union-find joined), `.n` (foreground voxels); per component `.sizes` uint64
    [count], `.seeds`, `.lo`, `.hi` uint32 [count, 3] (i, j, k; bounds inclusive), `.border` bool [count] (touches the grid's border:
    with complement=True the others are the enclosed voids).  It keeps its `Voxels` and hands the bricks to the calls that need them;
    for bricks on the device those calls are asynchronous on the context's stream, as `Voxels.slices` is."""

    def __init__(self, voxels, owner, connectivity, complement):
        self.voxels, self._owner, self.connectivity, self.complement = voxels, owner, connectivity, complement
        self._hip, self.depth, self.grid = voxels._hip, voxels.depth, voxels.grid
        c = np.zeros(4, np.uint64)
        lib().fhip_components_counts(owner.h, _p(c))
        self.count, self.nodes, self.n = int(c[0]), int(c[1]), int(c[2])
        n = self.count
        self.sizes, self.seeds, self.lo, self.hi = np.zeros(n, np.uint64), np.zeros((n, 3), np.uint32), np.zeros((n, 3), np.uint32), np.zeros((n, 3), np.uint32)
        border = np.zeros(n, np.uint8)
        self._hip.check(lib().fhip_components_table(owner.h, _p(self.sizes), _p(self.seeds), _p(self.lo), _p(self.hi), _p(border)))
        self.border = border.astype(bool)

    def largest(self):
        """the id of the largest component (of several, the smallest id)"""
        if not self.count:
            raise ValueError("no components")
        return int(np.argmax(self.sizes))

    def label_slices(self, k0, k1, out=None):
        """fhip_components_label_slices: int32 [k1 - k0, N, N], [k - k0, j, i] = the component of voxel (i, j, k), -1 for background:
        numpy for bricks on the host; for bricks on the device a torch CUDA tensor (`out`, contiguous int32 of that size, or a new one)"""
        v, N = self.voxels, self.grid
        k0, k1 = int(k0), int(k1)
        n = max(k1 - k0, 0) * N * N
        if v.on_device:
            if out is None:
                import torch
                out = torch.empty((max(k1 - k0, 0), N, N), dtype=torch.int32, device=v.bricks.device)
            assert out.is_cuda and out.is_contiguous() and out.element_size() == 4 and out.numel() >= n
            self._hip.check(lib().fhip_components_label_slices(self._hip._h, self._owner.h, v._ptr(), 1, k0, k1, _dev_ptr(out), 1))
            return out
        assert out is None, "bricks on the host: the images are returned as a numpy array"
        img = np.zeros((max(k1 - k0, 0), N, N), np.int32)
        self._hip.check(lib().fhip_components_label_slices(self._hip._h, self._owner.h, v._ptr(), 0, k0, k1, _p(img), 0))
        return img

    def extract(self, ids, out=None):
        """fhip_components_extract: the components `ids` as a bitmap of their own -> Voxels (`.cells` None: no octree made it).  `out`
        as for `voxelize`: a contiguous torch CUDA tensor of at least 8 B^3 bytes, or a contiguous numpy array of that size, written
        completely; without it a new one where the bricks are - a torch CUDA int64 tensor or a numpy uint64 [B, B, B]."""
        v = self.voxels
        ids = np.ascontiguousarray(np.asarray(list(ids) if not isinstance(ids, np.ndarray) else ids, np.int64).reshape(-1))
        if ((ids < 0) | (ids > 0xFFFFFFFF)).any():
            raise FidgetHipError(6, "extract: a component id beyond the number of components")
        ids = ids.astype(np.uint32)
        out, ptr, dev = _bitmap_out(self.depth, out, v._out_device(), aligned=True)
        self._hip.check(lib().fhip_components_extract(self._hip._h, self._owner.h, v._ptr(), int(v.on_device), _p(ids), len(ids), ptr, dev))
        return _bitmap_of(self._hip, out, dev, self.depth)

    def __repr__(self):
        return f"Components(count={self.count}, nodes={self.nodes}, n={self.n}, connectivity={self.connectivity}, complement={self.complement})"


def voxelize(shape, depth, world_to_model=None, vars=None, out=None):
    """fhip_shape_voxels: the solid `shape < 0` on the grid of 4 << depth voxels per axis over [-1, 1]^3 (world_to_model as for `mesh`)
    as a bitmap of 4 x 4 x 4 bricks, written down the octree `occupancy` counts -> Voxels.  `out`: a contiguous torch CUDA tensor of at
    least 8 B^3 bytes, B = 1 << depth (int64 is the natural dtype) - the bitmap stays on the device, `.bricks` views it - or a contiguous
    numpy array of that size, filled in place; without it a new numpy uint64 [B, B, B].  Either is written completely."""
    hip = shape.hip
    depth = int(depth)
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    vk, vv = _var_arrays(shape, vars)
    ax = None
    if shape._vars is not None:
        ax = np.array(shape._vars, dtype=np.int32)
        vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
    cells = np.zeros(4, np.uint64)
    out, ptr, dev = _bitmap_out(depth, out, aligned=True)
    st = lib().fhip_shape_voxels(hip._h, shape._h, depth, _p(w2m), _p(ax), _p(vk), _p(vv), len(vk), ptr, dev, _p(cells))
    if st == 4:
        raise ValueError("MissingVar")
    hip.check(st)
    return _bitmap_of(hip, out, dev, depth, dict(zip(("cells", "full", "empty", "leaf_cells"), (int(v) for v in cells))))


# ---- a triangle mesh back into the library: binary STL in, voxel bitmap out (fhip_triangles_voxels, fhip_mesh_voxels) ------------
def read_stl(path_or_bytes):
    """A binary STL file -> its triangles, float32 [T, 3, 3] (triangle, corner, xyz), read on the host; the file's normals and
    attribute words are ignored.  `path_or_bytes`: a path, or the file's bytes (bytes, bytearray, memoryview, a numpy uint8 array such
    as `Mesh.stl()` returns).  ASCII STL is refused with a ValueError."""
    if isinstance(path_or_bytes, (str, os.PathLike)):
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    elif isinstance(path_or_bytes, np.ndarray):
        data = np.ascontiguousarray(path_or_bytes).view(np.uint8).tobytes()
    else:
        data = bytes(path_or_bytes)
    n = int.from_bytes(data[80:84], "little") if len(data) >= 84 else -1
    if n < 0 or len(data) != 84 + 50 * n:
        if data.lstrip()[:5].lower() == b"solid":
            raise ValueError("read_stl: this is an ASCII STL file; only binary STL is read")
        raise ValueError(f"read_stl: not a binary STL file: {len(data)} bytes, but its header counts {n} triangles" if n >= 0 else "read_stl: not a binary STL file: shorter than its header")
    rec = np.frombuffer(data, np.uint8, 50 * n, 84).reshape(n, 50)
    return np.ascontiguousarray(rec[:, 12:48]).view("<f4").astype(np.float32).reshape(n, 3, 3)


MESH_INFO = ("triangles", "rejected", "flat", "crossings", "clipped", "open_rows", "set_voxels", "W")


def voxelize_mesh(mesh, depth, mesh_to_world=None, out=None, hip=None):
    """fhip_triangles_voxels / fhip_mesh_voxels: the solid a closed triangle mesh encloses, on the grid of 4 << depth voxels per axis
    over [-1, 1]^3, by parity counting along +x (even-odd: nested sheets make cavities) -> Voxels; the definition, exact in integers
    after the vertices are snapped to 1/256 voxel, stands in include/fidget_hip.h.  `mesh`: a `Mesh` (its resident device arrays are
    read where they are); float32 [T, 3, 3] triangles as `read_stl` returns them, a numpy array or a torch CUDA tensor; or a pair
    (vertices [V, 3] float32, triangles [T, 3] indices), both numpy or both torch CUDA (indices int64).  `mesh_to_world`: a 3 x 4
    matrix (or 4 x 4, whose first three rows are used), applied in float64 before the snap.  `out` as for `voxelize`.  `hip`: the context for
    arrays (default: `default_context()`; a `Mesh` brings its own).  A pair may be a tuple or a list of the two arrays.  The result's
    `.cells` are all zeros and `.mesh_info` = {triangles, rejected, flat, crossings, clipped, open_rows, set_voxels, W}: open_rows > 0 shows
    a mesh that is not closed.  ValueError when triangles were rejected: a vertex not finite or outside [-1.5, 1.5], or an index
    beyond the vertices."""
    depth = int(depth)
    m2w = None
    if mesh_to_world is not None:
        m2w = np.ascontiguousarray(np.asarray(mesh_to_world, np.float64).reshape(-1)[:12])
        assert m2w.size == 12, "mesh_to_world: 3 x 4 or 4 x 4"
    keep = None          # what the pointers point into, until the call returns
    if isinstance(mesh, Mesh):
        hip = mesh._hip
    else:
        hip = hip or default_context()
        # a pair is a tuple or a list of two arrays; a nested list of numbers is the [T, 3, 3] form
        pair = isinstance(mesh, (tuple, list)) and len(mesh) == 2 and all(hasattr(a, "shape") for a in mesh)
        if isinstance(mesh, (tuple, list)) and not pair and any(hasattr(a, "shape") for a in mesh):
            raise TypeError("voxelize_mesh: a mesh is a Mesh, [T, 3, 3] triangles, or a pair (vertices [V, 3], triangles [T, 3]) of two arrays")
        verts, tris = mesh if pair else (mesh, None)
        if isinstance(verts, np.ndarray) or not hasattr(verts, "is_cuda"):
            verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
            vp, dev = _p(verts), 0
            if tris is not None:
                tris = np.ascontiguousarray(tris, np.uint64).reshape(-1, 3)
            tp = _p(tris)
        else:
            assert verts.is_cuda and verts.element_size() == 4 and verts.is_floating_point(), "vertices on the device: a float32 CUDA tensor"
            verts = verts.contiguous().reshape(-1, 3)
            vp, dev = _dev_ptr(verts), 1
            if tris is not None:
                assert tris.is_cuda and tris.element_size() == 8 and not tris.is_floating_point(), "triangles on the device: an int64 CUDA tensor"
                tris = tris.contiguous().reshape(-1, 3)
            tp = _dev_ptr(tris)
        n_verts = int(verts.shape[0])
        n_tris = int(tris.shape[0]) if tris is not None else n_verts // 3
        keep = (verts, tris)
    out, ptr, out_dev = _bitmap_out(depth, out, aligned=True)
    info = np.zeros(8, np.uint64)
    if isinstance(mesh, Mesh):
        st = lib().fhip_mesh_voxels(hip._h, mesh._owner.h, _p(m2w), depth, ptr, out_dev, _p(info))
    else:
        st = lib().fhip_triangles_voxels(hip._h, vp, n_verts, tp, n_tris, dev, _p(m2w), depth, ptr, out_dev, _p(info))
    del keep
    hip.check(st)
    res = _bitmap_of(hip, out, out_dev, depth, {"cells": 0, "full": 0, "empty": 0, "leaf_cells": 0})
    res.mesh_info = dict(zip(MESH_INFO, (int(v) for v in info)))
    res._n = res.mesh_info["set_voxels"]
    if res.mesh_info["rejected"]:
        raise ValueError(f"voxelize_mesh: {res.mesh_info['rejected']} of {res.mesh_info['triangles']} triangles rejected: a vertex that is not finite or "
                         "lies outside [-1.5, 1.5] after mesh_to_world, or an index beyond the vertices")
    return res


# ---- the check of a triangle mesh: weld, edges, shells, volume (fhip_triangles_topology, fhip_mesh_topology) ----------------------
TOPOLOGY_COUNTS = ("triangles", "rejected", "degenerate", "vertices", "edges", "boundary", "flipped", "nonmanifold", "unbalanced", "shells", "vertex_slots", "edge_slots")
EDGE_KINDS = ("boundary", "flipped", "nonmanifold", "unbalanced")


class Topology:
    """What `mesh_topology` found.  `.counts`: {triangles, rejected, degenerate, vertices, edges, boundary, flipped, nonmanifold,
    unbalanced, shells, vertex_slots, edge_slots}; `.closed`: no unbalanced edge - what parity filling needs; `.manifold`: no boundary,
    flipped or nonmanifold edge; `.euler` = vertices - edges + (triangles - degenerate).  `.vertices` [V, 3] float32 and `.triangles`
    [T, 3] uint64: the indexed mesh - welded, or as given - which goes straight into `voxelize_mesh` as the pair
    `(t.vertices, t.triangles)`; `.triangle_shell` [T] uint32, 0xFFFFFFFF for a degenerate triangle; `.shells`: a dict of arrays, one
    row per shell in the order of their first triangles - triangles, first, unbalanced, lo, hi, volume6, area2; a shell with volume6 < 0
    is an inward-facing cavity.  `.volume` = sum(volume6) / 6 and `.area` = sum(area2) / 2, added on the host in shell order.  The
    host arrays are copied from the device when first asked for.  Every integer is the same from run to run; volume6 and area2 are
    float64 sums of the same terms in an order of arrival that may differ from run to run, and they alone."""
    def __init__(self, owner, hip):
        self._owner, self._hip = owner, hip
        c = np.zeros(16, np.uint64)
        lib().fhip_topology_counts(owner.h, _p(c))
        self.counts = dict(zip(TOPOLOGY_COUNTS, (int(v) for v in c)))
        n = self.counts["shells"]
        self.shells = {"triangles": np.zeros(n, np.uint64), "first": np.zeros(n, np.uint32), "unbalanced": np.zeros(n, np.uint64), "lo": np.zeros((n, 3), np.float32),
                       "hi": np.zeros((n, 3), np.float32), "volume6": np.zeros(n, np.float64), "area2": np.zeros(n, np.float64)}
        hip.check(lib().fhip_topology_shells(owner.h, *(_p(self.shells[k]) for k in ("triangles", "first", "unbalanced", "lo", "hi", "volume6", "area2"))))
        self._host = {}

    closed = property(lambda self: self.counts["unbalanced"] == 0)
    manifold = property(lambda self: self.counts["boundary"] == self.counts["flipped"] == self.counts["nonmanifold"] == 0)
    euler = property(lambda self: self.counts["vertices"] - self.counts["edges"] + self.counts["triangles"] - self.counts["degenerate"])
    volume = property(lambda self: float(sum(float(v) for v in self.shells["volume6"])) / 6.0)
    area = property(lambda self: float(sum(float(v) for v in self.shells["area2"])) / 2.0)

    def _shape(self, what):
        T = self.counts["triangles"]
        return {"vertices": ((int(lib().fhip_topology_vertex_rows(self._owner.h)), 3), np.float32, "<f4"), "triangles": ((T, 3), np.uint64, "<u8"),
                "triangle_shells": ((T,), np.uint32, "<u4")}[what]

    def _array(self, what):
        if what not in self._host:
            shape, dtype, _ = self._shape(what)
            a = np.zeros(shape, dtype)
            self._hip.check(getattr(lib(), "fhip_topology_" + what)(self._owner.h, _p(a)))
            self._host[what] = a
        return self._host[what]

    def _device(self, what):
        ptr = getattr(lib(), f"fhip_topology_{what}_dev")(self._owner.h)
        shape, _, typestr = self._shape(what)
        return _DeviceArray(self._owner, ptr, shape, typestr) if ptr else None

    vertices = property(lambda self: self._array("vertices"))
    triangles = property(lambda self: self._array("triangles"))
    triangle_shell = property(lambda self: self._array("triangle_shells"))

    def vertices_device(self):
        """`.vertices` where they are in device memory, as `Mesh.vertices_device` gives a mesh's; None for a mesh without triangles"""
        return self._device("vertices")

    def triangles_device(self):
        """... `.triangles` ("<u8": see `Mesh.triangles_device`)"""
        return self._device("triangles")

    def triangle_shell_device(self):
        """... and `.triangle_shell` ("<u4")"""
        return self._device("triangle_shells")

    def slices(self, zs, table_log2=0):
        """fhip_topology_slices: this indexed mesh cut by the planes z = zs[p] (float32, finite, strictly ascending) -> MeshSlices: per
        plane the closed polygons whose vertices lie on the mesh's edges.  `table_log2`: 0, or the size of the crossing edges' hash table
        as a power of two (tests; a table too small raises FidgetHipError Overflow)."""
        zs = np.ascontiguousarray(zs, np.float32).reshape(-1)
        h = C.c_void_p()
        self._hip.check(lib().fhip_topology_slices(self._hip._h, self._owner.h, _p(zs), len(zs), int(table_log2), C.byref(h)))
        return MeshSlices(_Handle(h.value, lib().fhip_slices_free), self._hip, self)

    def edges(self, kind, device=False):
        """fhip_topology_edges: the edges of one class - "boundary" (where the holes are), "flipped", "nonmanifold", "unbalanced" - as
        [n, 2] uint32 vertex pairs (a, b), a < b, in the order of the first corners that use them: a numpy array, or with `device` a
        torch CUDA tensor (int32: the bits of the uint32 pairs)."""
        k = EDGE_KINDS.index(kind)
        n = self.counts[kind]
        if device:
            import torch
            out = torch.empty((n, 2), dtype=torch.int32, device="cuda")
            self._hip.check(lib().fhip_topology_edges(self._hip._h, self._owner.h, k, _dev_ptr(out) if n else None, 1))
            self._hip.sync()
            return out
        out = np.zeros((n, 2), np.uint32)
        self._hip.check(lib().fhip_topology_edges(self._hip._h, self._owner.h, k, _p(out), 0))
        return out


def mesh_topology(mesh, weld=None, hip=None, table_log2=0):
    """fhip_triangles_topology / fhip_mesh_topology: what kind of triangle mesh this is -> Topology: the welded indexed mesh, the class
    of every edge (boundary, flipped, nonmanifold, unbalanced), the shells - edge-connected parts - with their triangles, bounds, volume
    and area; the definitions stand in include/fidget_hip.h.  `mesh`: as for `voxelize_mesh` - a `Mesh` (its resident device arrays are
    read where they are), float32 [T, 3, 3] triangles (numpy or a torch CUDA tensor), or a pair (vertices [V, 3] float32, triangles
    [T, 3] indices), both numpy or both torch CUDA.  `weld`: make one vertex of all corners with equal coordinates (-0 equals +0);
    default on for a soup, where it cannot be turned off, and off for a pair or a `Mesh`, whose indices then are the vertices.
    `table_log2`: 0, or the size of both hash tables as a power of two (tests; a table too small raises FidgetHipError Overflow).
    ValueError when triangles were rejected: a coordinate that is not finite, or an index beyond the vertices.  All integer results
    are the same from run to run; the shells' volume6 and area2 - float64 sums in an order of arrival - alone may differ in their last
    bits."""
    keep = None          # what the pointers point into, until the call returns
    h = C.c_void_p()
    if isinstance(mesh, Mesh):
        hip = mesh._hip
        st = lib().fhip_mesh_topology(hip._h, mesh._owner.h, int(bool(weld)), int(table_log2), C.byref(h))
    else:
        hip = hip or default_context()
        pair = isinstance(mesh, (tuple, list)) and len(mesh) == 2 and all(hasattr(a, "shape") for a in mesh)
        if isinstance(mesh, (tuple, list)) and not pair and any(hasattr(a, "shape") for a in mesh):
            raise TypeError("mesh_topology: a mesh is a Mesh, [T, 3, 3] triangles, or a pair (vertices [V, 3], triangles [T, 3]) of two arrays")
        verts, tris = mesh if pair else (mesh, None)
        if tris is None and weld is not None and not weld:
            raise ValueError("mesh_topology: a soup of triangles has no vertices until it is welded: weld=False needs a pair or a Mesh")
        if isinstance(verts, np.ndarray) or not hasattr(verts, "is_cuda"):
            verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
            vp, dev = _p(verts), 0
            if tris is not None:
                tris = np.ascontiguousarray(tris, np.uint64).reshape(-1, 3)
            tp = _p(tris)
        else:
            assert verts.is_cuda and verts.element_size() == 4 and verts.is_floating_point(), "vertices on the device: a float32 CUDA tensor"
            verts = verts.contiguous().reshape(-1, 3)
            vp, dev = _dev_ptr(verts), 1
            if tris is not None:
                assert tris.is_cuda and tris.element_size() == 8 and not tris.is_floating_point(), "triangles on the device: an int64 CUDA tensor"
                tris = tris.contiguous().reshape(-1, 3)
            tp = _dev_ptr(tris)
        n_verts = int(verts.shape[0])
        n_tris = int(tris.shape[0]) if tris is not None else n_verts // 3
        keep = (verts, tris)
        st = lib().fhip_triangles_topology(hip._h, vp, n_verts, tp, n_tris, dev, int(tris is None if weld is None else bool(weld)), int(table_log2), C.byref(h))
    del keep
    hip.check(st)
    res = Topology(_Handle(h.value, lib().fhip_topology_free), hip)
    if res.counts["rejected"]:
        raise ValueError(f"mesh_topology: {res.counts['rejected']} of {res.counts['triangles']} triangles rejected: a coordinate that is not finite, or an index beyond the vertices")
    return res


# ---- the slices of a triangle mesh: contour loops per plane (fhip_topology_slices) -------------------------------------------------
SLICES_COUNTS = ("planes", "vertices", "segments", "loops", "irregular", "edge_slots")


class MeshSlices:
    """What `mesh_slices` found: the mesh of a `Topology` cut by planes z = const; the definitions stand in include/fidget_hip.h.
    `.counts`: {planes, vertices, segments, loops, irregular, edge_slots}; `.zs` float32 [P]; `.per_plane`: {crossings, segments, loops}
    uint64 [P]; `.topology`: the mesh that was cut.  Per crossing - a vertex of the slice on a mesh edge, ids in the order of the edges'
    first corners and then by plane: `.xy` float32 [n, 2], `.plane` uint32 [n], `.edge` uint32 [n, 2] (u < v), `.next` uint32 [n]
    (0xFFFFFFFF: no segment leaves), `.loop_of` uint32 [n], `.degree` uint8 [n] (out | in << 4, each at most 15).  `.loops`: a dict of
    arrays, a row per loop in ascending order of leader - leader, plane, crossings, segments, irregular, area2 (float64: > 0 an outer
    boundary, < 0 a hole), lo, hi [., 2].  The crossings' arrays stay in device memory (`.xy_device()` ...); host copies are made when
    first asked for.  Everything is the same from run to run but area2, a float64 sum in an order of arrival."""

    def __init__(self, owner, hip, topology=None):
        self._owner, self._hip, self.topology = owner, hip, topology
        c = np.zeros(8, np.uint64)
        lib().fhip_slices_counts(owner.h, _p(c))
        self.counts = dict(zip(SLICES_COUNTS, (int(v) for v in c)))
        P, L = self.counts["planes"], self.counts["loops"]
        self.zs = np.zeros(P, np.float32)
        self.per_plane = {"crossings": np.zeros(P, np.uint64), "segments": np.zeros(P, np.uint64), "loops": np.zeros(P, np.uint64)}
        hip.check(lib().fhip_slices_planes(owner.h, _p(self.zs), *(_p(self.per_plane[k]) for k in ("crossings", "segments", "loops"))))
        self._loops = {"leader": np.zeros(L, np.uint32), "plane": np.zeros(L, np.uint32), "crossings": np.zeros(L, np.uint32), "segments": np.zeros(L, np.uint32),
                       "irregular": np.zeros(L, np.uint32), "area2": np.zeros(L, np.float64), "lo": np.zeros((L, 2), np.float32), "hi": np.zeros((L, 2), np.float32)}
        hip.check(lib().fhip_slices_loops(owner.h, *(_p(a) for a in self._loops.values())))
        self._host = None

    def _vertices(self):
        if self._host is None:
            n = self.counts["vertices"]
            a = {"xy": np.zeros((n, 2), np.float32), "plane": np.zeros(n, np.uint32), "edge": np.zeros((n, 2), np.uint32), "next": np.zeros(n, np.uint32),
                 "loop_of": np.zeros(n, np.uint32), "degree": np.zeros(n, np.uint8)}
            self._hip.check(lib().fhip_slices_vertices(self._owner.h, *(_p(v) for v in a.values())))
            self._host = a
        return self._host

    xy = property(lambda self: self._vertices()["xy"])
    plane = property(lambda self: self._vertices()["plane"])
    edge = property(lambda self: self._vertices()["edge"])
    next = property(lambda self: self._vertices()["next"])
    loop_of = property(lambda self: self._vertices()["loop_of"])
    degree = property(lambda self: self._vertices()["degree"])
    loops = property(lambda self: self._loops)

    def _plane(self, p):
        p = int(p)
        if not 0 <= p < self.counts["planes"]:
            raise IndexError(f"plane {p} is not among 0 .. {self.counts['planes'] - 1}")
        return p

    def loops_of(self, p):
        """the ids of plane p's loops, ascending"""
        return np.flatnonzero(self._loops["plane"] == self._plane(p))

    def polygons(self, p):
        """-> (the closed loops of plane p as float32 [n, 2] arrays, each from its leader on along `next`: walked on the host; the number
        of plane p's loops left out because they hold an irregular crossing)"""
        out, skipped = [], 0
        for q in self.loops_of(p):
            if self._loops["irregular"][q]:
                skipped += 1
                continue
            m = int(self._loops["crossings"][q])
            ids, v = np.zeros(m, np.int64), int(self._loops["leader"][q])
            for k in range(m):
                ids[k] = v
                v = int(self.next[v])
            out.append(self.xy[ids])
        return out, skipped

    def svg(self, p, path=None):
        """Plane p's closed loops as one <path fill-rule="evenodd"> each, `M x y L x y ... Z`, with y negated - SVG's y grows downward -
        and the bounds of the plane's loops as the viewBox.  Returns the text; written to `path` when given."""
        polys, _ = self.polygons(p)
        ids = self.loops_of(p)
        lo = self._loops["lo"][ids].min(axis=0) if len(ids) else np.array([-1.0, -1.0])
        hi = self._loops["hi"][ids].max(axis=0) if len(ids) else np.array([1.0, 1.0])
        paths = "".join('<path fill-rule="evenodd" d="M ' + " L ".join(f"{float(x):.9g} {-float(y):.9g}" for x, y in q) + ' Z"/>\n' for q in polys)
        text = (f'<svg xmlns="http://www.w3.org/2000/svg" viewBox="{float(lo[0]):.9g} {-float(hi[1]):.9g} {float(hi[0] - lo[0]):.9g} {float(hi[1] - lo[1]):.9g}">\n'
                f'{paths}</svg>\n')
        if path is not None:
            with open(path, "w") as f:
                f.write(text)
        return text

    def _device(self, what, shape, typestr):
        ptr = getattr(lib(), f"fhip_slices_{what}_dev")(self._owner.h)
        return _DeviceArray(self._owner, ptr, shape, typestr) if ptr else None

    def xy_device(self):
        """`.xy` where it is in device memory ([n, 2] "<f4") as an object carrying `__cuda_array_interface__` that keeps the result
        alive; None when nothing crosses"""
        return self._device("xy", (self.counts["vertices"], 2), "<f4")

    def next_device(self):
        """... `.next` ("<i4": the bits of the uint32 ids, as `Outlines.next_device` gives its)"""
        return self._device("next", (self.counts["vertices"],), "<i4")

    def loop_of_device(self):
        """... `.loop_of` ("<i4")"""
        return self._device("loop", (self.counts["vertices"],), "<i4")

    def plane_device(self):
        """... and `.plane` ("<i4")"""
        return self._device("plane", (self.counts["vertices"],), "<i4")

    def __repr__(self):
        return f"MeshSlices({', '.join(f'{k}={v}' for k, v in self.counts.items())})"


def mesh_slices(mesh, zs, weld=None, hip=None, table_log2=0):
    """fhip_topology_slices: the step a slicer performs on an STL - the triangles cut by the planes z = zs[p] -> MeshSlices.  `mesh`:
    anything `mesh_topology` takes - a `Mesh`, [T, 3, 3] triangles, a pair (vertices, triangles), numpy or torch CUDA - which is run
    first with `weld`, or a `Topology`, which is cut as it is.  `zs`: float32, finite and strictly ascending, else FidgetHipError
    Unsupported."""
    topo = mesh if isinstance(mesh, Topology) else mesh_topology(mesh, weld, hip)
    return topo.slices(zs, table_log2)


# ---- contours of a 2D slice: vertices on the crossing lattice edges, directed segments, loops, SVG (fhip_contour2d) -----------
def contour_loops(next):
    """fhip_contour_loops (host only): the chains of a link array as [(ids uint32 array, closed bool)] - open chains first, from the
    vertices no segment arrives at in ascending order, then the closed loops, each from its smallest id, in ascending order of that"""
    nxt = np.ascontiguousarray(next, np.uint32)
    n = len(nxt)
    order, start, closed, count = np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64), np.zeros(n, np.uint8), C.c_uint64(0)
    st = lib().fhip_contour_loops(_p(nxt), n, _p(order), _p(start), _p(closed), C.byref(count))
    if st:
        raise ValueError("not the link array of a contour")
    return [(order[int(start[k]):int(start[k + 1])].copy(), bool(closed[k])) for k in range(count.value)]


class Contours:
    """The outlines of `contour`: `.vertices` [n, 2] float32 in pixel units (the centre of pixel (i, j) is (i, j)), `.segments` [m, 2]
    uint32 {from, to} with the inside on their left, `.next` [n] uint32 (0xFFFFFFFF: no segment leaves the vertex) - host copies, made
    on first use - `.width`, `.height`, `.z`, `.n_vertices`, `.n_segments`.  The arrays themselves stay in device memory."""

    def __init__(self, owner, width, height, z, n_vertices, n_segments):
        self._owner, self.width, self.height, self.z = owner, int(width), int(height), float(z)
        self.n_vertices, self.n_segments = int(n_vertices), int(n_segments)
        self._host = {}

    def _copy(self, name, shape, dtype):
        if name not in self._host:
            a = np.zeros(shape, dtype)
            if getattr(lib(), "fhip_contours_" + name)(self._owner.h, _p(a)):
                raise FidgetHipError("fhip_contours_" + name)
            self._host[name] = a
        return self._host[name]

    @property
    def vertices(self):
        return self._copy("vertices", (self.n_vertices, 2), np.float32)

    @property
    def segments(self):
        return self._copy("segments", (self.n_segments, 2), np.uint32)

    @property
    def next(self):
        return self._copy("next", (self.n_vertices,), np.uint32)

    def vertices_device(self):
        """The vertices in device memory ([n, 2] float32) as an object carrying `__cuda_array_interface__` that keeps the result alive -
        `torch.as_tensor(obj, device="cuda")` views it; None when there are none."""
        ptr = lib().fhip_contours_vertices_dev(self._owner.h)
        return _DeviceArray(self._owner, ptr, (self.n_vertices, 2), "<f4") if ptr else None

    def segments_device(self):
        """... and the segments ([m, 2] vertex ids; "<i4" - torch has no unsigned 32-bit views before 2.3 and the ids are below 2^31
        for every image that fits device memory twice over)"""
        ptr = lib().fhip_contours_segments_dev(self._owner.h)
        return _DeviceArray(self._owner, ptr, (self.n_segments, 2), "<i4") if ptr else None

    def loops(self):
        """[(ids, closed)]: `contour_loops` of `.next`"""
        return contour_loops(self.next)

    def areas(self):
        """the signed area of every chain of `.loops()` in pixel units (shoelace sum in float64, an open chain closed by its chord):
        positive for an outer boundary, negative for a hole"""
        v = self.vertices.astype(np.float64)
        out = []
        for ids, _ in self.loops():
            x, y = v[ids, 0], v[ids, 1]
            out.append(0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)))
        return out

    def world(self):
        """the vertices through screen_to_world((W, H)) - [n, 2] float32 in the region the image spans ([-1, 1] along its shorter side, y upward: row 0
        has the largest y), before world_to_model - in the driver's f32 operation order: (m00 x + m01 y) + m02"""
        m = screen_to_world((self.width, self.height))
        v = self.vertices
        x, y = v[:, 0], v[:, 1]
        out = np.empty_like(v)
        for r in range(2):
            out[:, r] = (m[r, 0] * x + m[r, 1] * y) + m[r, 2]
        return out

    def svg(self, path=None):
        """One <path fill-rule="evenodd"> of all chains, `M x y L x y ... Z` per closed loop (no Z for an open chain).  Coordinates are
        `.world()`'s with y negated: screen_to_world puts row 0 at the largest y, SVG's y grows downward, so row 0 comes out on top
        and the drawing is the image as displayed (and the model with y up), not its mirror.  The viewBox is the image's pixel lattice
        - the corners (-0.5, -0.5) and (W - 0.5, H - 0.5) through the same transform - whatever W : H is.  Returns the text; written to
        `path` when one is given."""
        w = self.world()
        d = []
        for ids, closed in self.loops():
            pts = " L ".join(f"{float(w[k, 0]):.9g} {-float(w[k, 1]):.9g}" for k in ids)
            d.append("M " + pts + (" Z" if closed else ""))
        m = screen_to_world((self.width, self.height)).astype(np.float64)
        cx = [m[0, 0] * px + m[0, 1] * py + m[0, 2] for px in (-0.5, self.width - 0.5) for py in (-0.5, self.height - 0.5)]
        cy = [-(m[1, 0] * px + m[1, 1] * py + m[1, 2]) for px in (-0.5, self.width - 0.5) for py in (-0.5, self.height - 0.5)]
        box = f"{min(cx):.9g} {min(cy):.9g} {max(cx) - min(cx):.9g} {max(cy) - min(cy):.9g}"
        text = (f'<svg xmlns="http://www.w3.org/2000/svg" viewBox="{box}">\n'
                f'<path fill-rule="evenodd" d="{" ".join(d)}"/>\n</svg>\n')
        if path is not None:
            with open(path, "w") as f:
                f.write(text)
        return text

    def __repr__(self):
        return f"Contours({self.width}x{self.height}, z={self.z}, vertices={self.n_vertices}, segments={self.n_segments})"


def contour(shape, width, height=None, z=0.0, world_to_model=None, vars=None):
    """fhip_contour2d: the outlines of `shape < 0` in the pixel-perfect render2d image of this configuration -> Contours.  One blocking
    call; only the two totals come back from the device before the arrays are asked for."""
    height = width if height is None else height
    hip = shape.hip
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    vk, vv = _var_arrays(shape, vars)
    ax = None
    if shape._vars is not None:
        ax = np.array(shape._vars, dtype=np.int32)
        vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
    cfg = _Cfg2D(width, height, _p(w2m), z, 1, None, 0, _p(vk), _p(vv), len(vk), _p(ax))
    h = C.c_void_p()
    st = lib().fhip_contour2d(hip._h, shape._h, C.byref(cfg), C.byref(h))
    if st == 4:
        raise ValueError("MissingVar")
    hip.check(st)
    counts = np.zeros(4, np.uint64)
    owner = _Handle(h.value, lib().fhip_contours_free)
    lib().fhip_contours_counts(owner.h, _p(counts))
    return Contours(owner, width, height, z, counts[0], counts[1])


def slice_stack(shape, size, zs, world_to_model=None, vars=None):
    """One `contour` per z of `zs` (size: W, or (W, H)) -> [Contours]: what a slicer asks for, layer by layer; a layer waits for its
    two totals and nothing else"""
    w, h = (size, size) if np.isscalar(size) else size
    return [contour(shape, int(w), int(h), float(z), world_to_model, vars) for z in zs]


# ---- constraint solver (fidget::solver, fidget-solver/src/lib.rs) ---------------------------------------------------------
class Free(float):
    """Parameter::Free(start) (fidget-solver/src/lib.rs:11-17): a variable the solver moves, from this start"""


class Fixed(float):
    """Parameter::Fixed(value): a variable held at this value"""


SOLVE_EXITS = {0: "zero_residual", 1: "no_change", 2: "zero_error", 3: "zero_damping", 4: "stalled", 5: "max_iterations",
               6: "max_retries"}       # include/fidget_hip.h FHIP_SOLVE_*
SOLVE_MAX_FREE = 64


def solve_key(key):
    """'x' | 'y' | 'z' | int (a Var::V index, as Context.var) -> (axis, index) of fhip_solve"""
    if isinstance(key, str):
        return "xyz".index(key.lower()), 0
    return 3, int(key)


def solve_batch(constraints, keys, free_mask, values, max_iterations=0, hip=None):
    """fhip_solve: every row of `values` ([n_instances][n_params]: the start of a free parameter, the value of a fixed one) is one
    solve of the same constraints (a list of Shape; residual = output 0).  keys: per parameter 'x' | 'y' | 'z' | int; free_mask:
    per parameter, true = free.  Returns (out [n_instances][n_free] - the free parameters in parameter order -, err, iterations,
    exit_reason - SOLVE_EXITS)."""
    keys = list(keys)
    free = np.ascontiguousarray(np.asarray(free_mask, dtype=bool).reshape(len(keys)), dtype=np.uint8)
    vals = np.ascontiguousarray(np.asarray(values, dtype=np.float32).reshape(-1, len(keys)))
    n_inst, n_free = vals.shape[0], int(free.sum())
    ax = np.array([solve_key(k)[0] for k in keys], dtype=np.int32)
    ix = np.array([solve_key(k)[1] for k in keys], dtype=np.uint64)
    hip = hip or (constraints[0].hip if constraints else default_context())
    tapes = (C.c_void_p * max(len(constraints), 1))(*[s._h.value for s in constraints])
    out = np.zeros((n_inst, n_free), dtype=np.float32)
    err = np.zeros(n_inst, dtype=np.float32)
    its = np.zeros(n_inst, dtype=np.uint32)
    ex = np.zeros(n_inst, dtype=np.int32)
    st = lib().fhip_solve(hip._h, tapes, len(constraints), _p(ax), _p(ix), _p(free), len(keys), _p(vals), n_inst,
                          int(max_iterations), _p(out), _p(err), _p(its), _p(ex))
    if st in (1, 5, 6):
        raise ValueError(f"{STATUS[st]}: {lib().fhip_last_error(hip._h).decode()}")
    hip.check(st)
    return out, err, its, ex


def solve(constraints, params, max_iterations=0, hip=None):
    """fidget::solver::solve (fidget-solver/src/lib.rs:191): params maps 'x' | 'y' | 'z' | int to Free(start) or Fixed(value);
    returns {key: value} for the free variables"""
    keys = list(params)
    for k in keys:
        if not isinstance(params[k], (Free, Fixed)):
            raise TypeError(f"parameter {k!r}: Free(v) or Fixed(v), not {params[k]!r}")
    free = [isinstance(params[k], Free) for k in keys]
    out = solve_batch(constraints, keys, free, [[float(params[k]) for k in keys]], max_iterations, hip)[0][0]
    return {k: float(v) for k, v in zip([k for k, f in zip(keys, free) if f], out)}
