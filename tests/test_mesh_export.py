"""Mesh export without a device: the numpy restatement of Mesh::write_stl (tests/stl_ref.py) that the GPU tests compare fhip_mesh_stl
with, on meshes small enough to check by hand, and the new entry points' declarations (include/fidget_hip.h, fidget_hip_debug.h) against
the library's exports and the Python binding's tables."""
import ctypes
import os
import re

import numpy as np

from stl_ref import HEADER_TEXT, stl_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("fhip_mesh_vertices_dev", "fhip_mesh_triangles_dev", "fhip_mesh_stl_bytes", "fhip_mesh_stl", "fhip_mesh_vertex_grads")


def test_one_triangle():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    b = stl_bytes(v, np.array([[0, 1, 2]], np.uint64))
    assert b.dtype == np.uint8 and len(b) == 134
    assert len(HEADER_TEXT) == 44 and b[:44].tobytes() == HEADER_TEXT and not b[44:80].any()
    assert b[80:84].tobytes() == (1).to_bytes(4, "little")
    f = np.frombuffer(b[84:132].tobytes(), "<f4")
    assert f[:3].tolist() == [0.0, 0.0, 1.0]
    assert f[3:].tolist() == v.reshape(-1).tolist()
    assert b[132:134].tolist() == [0, 0]


def test_reversed_winding_negates_the_normal():
    rng = np.random.default_rng(11)
    v = rng.uniform(-1, 1, (6, 3)).astype(np.float32)
    fwd = stl_bytes(v, np.array([[0, 1, 2], [3, 4, 5]], np.uint64))
    rev = stl_bytes(v, np.array([[0, 2, 1], [3, 5, 4]], np.uint64))
    assert len(fwd) == len(rev) == 84 + 100 and fwd[80:84].tobytes() == (2).to_bytes(4, "little")
    for k in range(2):
        a = np.frombuffer(fwd[84 + 50 * k:84 + 50 * k + 12].tobytes(), "<f4")
        b = np.frombuffer(rev[84 + 50 * k:84 + 50 * k + 12].tobytes(), "<f4")
        assert a.any() and (a == -b).all()


def test_no_triangles_is_the_header_alone():
    b = stl_bytes(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint64))
    assert len(b) == 84 and b[:44].tobytes() == HEADER_TEXT and not b[44:].any()


def test_the_header_declares_the_new_entry_points_and_the_library_exports_them():
    import fidget_amd as F
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "fidget_hip.h")).read(), flags=re.S)
    dbg = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "fidget_hip_debug.h")).read(), flags=re.S)
    lib = ctypes.CDLL(F.LIB_PATH)
    for name in NEW_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name), name
        assert name in F.EXPORTS and getattr(F.lib(), name).argtypes is not None, name
    assert re.search(r"\bfhip_debug_stl_pack\s*\(", dbg) and hasattr(lib, "fhip_debug_stl_pack") and "fhip_debug_stl_pack" in F.EXPORTS
    assert re.search(r"fhip_status\s+fhip_mesh_stl\s*\(\s*fhip_ctx\*\s*ctx,\s*const fhip_mesh\*\s*mesh,\s*void\*\s*out,\s*int out_is_device\s*\)", hdr)
    assert re.search(r"uint64_t\s+fhip_mesh_stl_bytes\s*\(\s*const fhip_mesh\*\s*mesh\s*\)", hdr)
