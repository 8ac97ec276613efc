"""The Python front end as a package (no GPU, and no built library but for nothing): every name callers import from `fidget_amd` is
still there and is the object its home module defines; `fidget_amd/__init__.py` only imports; the ctypes signature table agrees with
the two headers in every argument count and every void return; the source list build() watches is derived, complete and free of
duplicates; and every submodule imports on its own without loading the library."""
import ast
import ctypes
import importlib
import os
import re
import subprocess
import sys
import textwrap

import fidget_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# in import order: each module imports, at module level, only the ones before it
MODULES = ("_build", "_abi", "context", "shape", "render", "mesher", "voxels", "trimesh", "contours", "solver")

# the module-level names of the one-file front end this package replaced that do not start with "_" (its AST's assignments, functions
# and classes), and the four private ones tests use
PUBLIC = [
    "BAD_NODE", "BINARY", "BadNode", "Components", "Context", "Contours", "DistanceField", "EDGE_KINDS", "EXPORTS", "FH_OPS",
    "FidgetHipError", "Fixed", "Free", "GEOMETRY_PIXEL", "HIP_TILES_2D", "HIP_TILES_3D", "HipContext", "LIB_PATH", "MESH_INFO",
    "MESH_LEAF", "Mesh", "MeshSlices", "Node", "Occupancy", "OccupancyStruct", "Outlines", "SLICES_COUNTS", "SOLVE_EXITS",
    "SOLVE_MAX_FREE", "STATUS", "Shape", "Surface", "TOPOLOGY_COUNTS", "ThicknessField", "Topology", "UNARY", "VM_TILES_2D",
    "VM_TILES_3D", "Voxels", "apply_shading", "blur_ssao", "build", "build_mesh", "compute_ssao", "contour", "contour_loops",
    "debug_walk_dual", "default_context", "denoise_normals", "lib", "libm_probe", "lift_2d", "mat_mul", "merge_depth", "mesh",
    "mesh_merge", "mesh_part", "mesh_sample", "mesh_slices", "mesh_topology", "occupancy", "pixel_fill_depth", "pixel_inside",
    "read_stl", "render2d", "render3d", "screen_to_world", "slice_stack", "solve", "solve_batch", "solve_key", "to_debug_bitmap",
    "to_rgba_bitmap", "to_rgba_distance", "transform_point", "voxelize", "voxelize_mesh", "voxels_unpack",
    "_Cfg2D", "_Cfg3D", "_SOURCES", "_p",
]

UNINCLUDED = ("gen_asm.py", "gen_interp.py", "gen_tiles.py", "gen_tilesv.py", "gen_normals.py", "gen_prune.py", "gen_ubench.py", "gen_trans.py",
              "offsets.cpp", "trans_funcs.hip")


def _defined(module):
    """the names a module's own top-level statements bind, imports aside"""
    with open(module.__file__) as f:
        tree = ast.parse(f.read())
    names = set()
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            names.add(node.name)
        elif isinstance(node, ast.Assign):
            names |= {n.id for t in node.targets for n in ast.walk(t) if isinstance(n, ast.Name)}
    return names


def test_public_surface():
    assert PUBLIC == sorted(PUBLIC[:-4]) + sorted(PUBLIC[-4:]) and len(set(PUBLIC)) == len(PUBLIC) == 82
    modules = [importlib.import_module("fidget_amd." + m) for m in MODULES]
    for name in PUBLIC:
        assert hasattr(F, name), f"fidget_amd.{name} is gone"
        homes = [m for m in modules if name in _defined(m)]
        assert len(homes) == 1, f"{name}: defined in {[m.__name__ for m in homes]}"
        assert getattr(F, name) is getattr(homes[0], name), f"fidget_amd.{name} is not {homes[0].__name__}.{name}"
    assert F.C is ctypes
    # the modules' state is not copied into the package, where it would stay None
    assert not hasattr(F, "_lib") and not hasattr(F, "_default_ctx")


def test_init_holds_imports_only():
    with open(os.path.join(ROOT, "fidget_amd", "__init__.py")) as f:
        body = ast.parse(f.read()).body
    assert isinstance(body[0], ast.Expr) and isinstance(body[0].value, ast.Constant) and isinstance(body[0].value.value, str)
    for node in body[1:]:
        assert isinstance(node, (ast.Import, ast.ImportFrom)), f"line {node.lineno}: {type(node).__name__}"
        assert all(a.name != "*" for a in node.names), f"line {node.lineno}: import *"


def test_signatures_match_the_headers():
    hdr = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("fidget_hip.h", "fidget_hip_debug.h"))
    flat = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    decls = re.findall(r"([A-Za-z_][\w\s\*]*?)\b(fhip_\w+)\s*\(([^;{]*?)\)\s*;", flat)
    decls = {name: (ret, args) for ret, name, args in decls if name != "fhip_status"}
    assert sorted(decls) == sorted(F.SIGNATURES) and len(decls) >= 165
    assert F.EXPORTS == list(F.SIGNATURES)
    for name, (ret, args) in decls.items():
        res, argtypes = F.SIGNATURES[name]
        n = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert n == len(argtypes), f"{name}: {n} parameters declared, {len(argtypes)} in SIGNATURES"
        ret = ret.strip().splitlines()[-1].split()          # (the declaration's own line: `void`, `void *`, `fhip_status`, ...)
        assert ret, f"{name}: no return type read"
        assert (res is None) == (ret == ["void"]), f"{name}: declared to return {' '.join(ret)}, SIGNATURES has {res}"


def test_derived_source_list():
    csrc = os.path.join(ROOT, "fidget_amd", "csrc")
    assert len(F._SOURCES) > 60 and len(set(F._SOURCES)) == len(F._SOURCES)
    for s in F._SOURCES:
        assert os.path.isfile(os.path.join(csrc, s)), s
    assert "capi.hip" in F._SOURCES and set(UNINCLUDED) <= set(F._SOURCES)
    # ... in the spelling the list always had
    assert {"contour/contour.hpp", "../../include/fidget_hip.h", "../../include/fidget_hip_debug.h", "mesh_slice.hpp"} <= set(F._SOURCES)


def test_submodules_import_alone_and_load_nothing(tmp_path):
    code = textwrap.dedent(f"""
        import importlib, sys
        sys.path.insert(0, {ROOT!r})
        for name in {tuple(reversed(MODULES))!r}:
            for k in [k for k in sys.modules if k == "fidget_amd" or k.startswith("fidget_amd.")]:
                del sys.modules[k]
            importlib.import_module("fidget_amd." + name)
            loaded = [m.__file__ for k, m in sys.modules.items() if k.startswith("fidget_amd") and (getattr(m, "__file__", None) or "").endswith(".so")]
            assert not loaded, (name, loaded)
            assert sys.modules["fidget_amd._abi"]._lib is None, name
        import fidget_amd
        try:
            fidget_amd.lib()
        except ImportError:
            print("ok")
    """)
    env = dict(os.environ, FHIP_LIB=str(tmp_path / "no_such_library.so"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
