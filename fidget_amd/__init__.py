"""fidget_amd — Python binding of libfidget_hip.so (the MI355X / gfx950 backend).

Host-side mirror of the reference's user-facing surface for the evaluation hot path:

    reference (Rust)                                this package
    ---------------------------------------------   ------------------------------
    fidget_core::Context (+ from_text)              Context
    Shape<F> / F: Function + MathFunction           Shape (one device tape; simplify())
    TracingEvaluator / BulkEvaluator impls          Shape.eval_interval / eval_point /
                                                    eval_float_slice / eval_grad_slice
    fidget_raster::pixel::render / voxel::render    render2d / render3d

Everything that computes goes through the C ABI in include/fidget_hip.h (ctypes);
there is NO CPU fallback: importing works without a GPU (so the build and symbol
checks run anywhere), but creating a context without a HIP device raises.

One module per subject, each importing only the ones before it: _build (the library's path, sources and recipe), _abi (the ctypes
mirror: SIGNATURES, lib()), context, shape, render, mesher, voxels, trimesh, contours, solver (`mesh` and `solve` are functions of
the package, so their modules carry other names).  This file only re-exports their names; the modules' state (`_abi._lib`,
`context._default_ctx`) stays where it is and is read through `lib()` and `default_context()`.
"""
import ctypes as C

from ._build import _SOURCES, LIB_PATH, build
from ._abi import (BINARY, EXPORTS, FH_OPS, GEOMETRY_PIXEL, HIP_TILES_2D, HIP_TILES_3D, SIGNATURES, STATUS, UNARY, VM_TILES_2D, VM_TILES_3D,
                   FidgetHipError, _Cfg2D, _Cfg3D, _p, lib, libm_probe)
from .context import HipContext, default_context
from .shape import BAD_NODE, BadNode, Context, Node, Shape, lift_2d, mat_mul, screen_to_world, transform_point
from .render import (apply_shading, blur_ssao, compute_ssao, denoise_normals, merge_depth, pixel_fill_depth, pixel_inside, render2d, render3d,
                     to_debug_bitmap, to_rgba_bitmap, to_rgba_distance)
from .mesher import MESH_LEAF, Mesh, Occupancy, OccupancyStruct, build_mesh, debug_walk_dual, mesh, mesh_merge, mesh_part, mesh_sample, occupancy
from .voxels import Components, DistanceField, Nesting, Outlines, Surface, ThicknessField, Voxels, voxelize, voxels_unpack
from .trimesh import EDGE_KINDS, MESH_INFO, SLICES_COUNTS, SLICE_NESTING_PLANES, TOPOLOGY_COUNTS, MeshSlices, SliceNesting, Topology, mesh_slices, mesh_topology, read_stl, voxelize_mesh
from .contours import Contours, contour, contour_loops, slice_stack
from .solver import SOLVE_EXITS, SOLVE_MAX_FREE, Fixed, Free, solve, solve_batch, solve_key
