"""The boundary mesh of a voxel bitmap without a GPU: the reference of voxel_mesh_ref.py on solids whose numbers are known and against
two invariants - six times the number of set voxels is the sum of det(a, b, c) over the triangles, and every directed edge is balanced
by its reverse; the bit arithmetic of fidget_amd/csrc/mesh_vmesh.hpp built for the host (tests/host_build/mesh_vmesh_host.cpp) - the
six face masks of a brick, a corner brick's used corners and edges, the numbering - against the reference; that program under ASan and
UBSan; the entry points as the header states them."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import fidget_amd as F
import voxel_mesh_ref as MR
import voxels_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "mesh_vmesh_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")
ENTRY_POINTS = ("fhip_voxels_surface", "fhip_voxels_mesh")


def box(N, lo, hi, value=True, into=None):
    """[lo, hi)^3 - or per axis where lo, hi are triples - set to `value`"""
    g = np.zeros((N, N, N), bool) if into is None else into
    lo, hi = (lo if isinstance(lo, tuple) else (lo,) * 3), (hi if isinstance(hi, tuple) else (hi,) * 3)
    g[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = value
    return g


def voxels_at(N, pts):
    g = np.zeros((N, N, N), bool)
    for p in pts:
        g[p] = True
    return g


def hollow_box16():
    return box(16, 4, 12, False, into=box(16, 2, 14))


def square_ring16():
    return box(16, (6, 6, 0), (10, 10, 16), False, into=box(16, (3, 3, 6), (13, 13, 9)))


# solid -> (F, V, E, V - E + F)
KNOWN = {
    "a full 4^3 grid": (lambda: np.ones((4, 4, 4), bool), (96, 98, 192, 2)),
    "one voxel": (lambda: voxels_at(4, [(1, 2, 1)]), (6, 8, 12, 2)),
    "two voxels sharing a face": (lambda: voxels_at(4, [(1, 2, 1), (1, 2, 2)]), (10, 12, 20, 2)),
    "two voxels sharing only an edge": (lambda: voxels_at(4, [(1, 2, 1), (2, 2, 2)]), (12, 14, 23, 3)),
    "two voxels sharing only a corner": (lambda: voxels_at(4, [(1, 1, 1), (2, 2, 2)]), (12, 15, 24, 3)),
    "16^3 hollow box": (hollow_box16, (1248, 1252, 2496, 4)),
    "square ring": (square_ring16, (336, 336, 672, 0)),
}


def check_invariants(inside, verts, tris, summary):
    N = inside.shape[0]
    corners = MR.lattice(verts, N)
    assert len(verts) == summary[6] and len(tris) == 2 * summary[8] and summary[9] == int(inside.sum())
    assert np.array_equal(((2 * corners - N).astype(np.float32) * np.float32(1.0 / N)), verts)          # the coordinates are exact
    assert MR.six_volumes(corners, tris) == 6 * summary[9]
    assert MR.edges_balanced(tris)
    assert len(tris) == 0 or (int(tris.max()) == len(verts) - 1 and len(np.unique(tris)) == len(verts))          # every vertex is used


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(name):
    make, (n_faces, n_verts, n_edges, euler) = KNOWN[name]
    inside = make()
    s = MR.summary(inside)
    assert (s[8], s[6], s[7], MR.euler(s)) == (n_faces, n_verts, n_edges, euler)
    assert sum(s[:6]) == s[8] and s[0] == s[1] and s[2] == s[3] and s[4] == s[5]          # a closed surface: as many faces -x as +x
    verts, tris = MR.mesh(inside)
    check_invariants(inside, verts, tris, s)


def test_the_order_of_faces_corners_and_vertices():
    """one voxel at (1, 2, 1) of a 4^3 grid, written out by hand"""
    verts, tris = MR.mesh(voxels_at(4, [(1, 2, 1)]))
    c = MR.lattice(verts, 4).tolist()
    # vertices ascend by local bit a + 4 b + 16 c within corner brick 0
    assert c == [[1, 2, 1], [2, 2, 1], [1, 3, 1], [2, 3, 1], [1, 2, 2], [2, 2, 2], [1, 3, 2], [2, 3, 2]]
    quads = [[c[int(v)] for v in (tris[2 * f][0], tris[2 * f][1], tris[2 * f][2], tris[2 * f + 1][2])] for f in range(6)]
    assert all(np.array_equal(tris[2 * f][[0, 2]], tris[2 * f + 1][[0, 1]]) for f in range(6))
    assert quads[0] == [[1, 2, 1], [1, 2, 2], [1, 3, 2], [1, 3, 1]]          # -x: o, o + z, o + y + z, o + y
    assert quads[1] == [[2, 2, 1], [2, 3, 1], [2, 3, 2], [2, 2, 2]]          # +x: o, o + y, o + y + z, o + z
    assert quads[2] == [[1, 2, 1], [2, 2, 1], [2, 2, 2], [1, 2, 2]]          # -y: (u, v) = (z, x): o, o + x, o + z + x, o + z
    assert quads[3] == [[1, 3, 1], [1, 3, 2], [2, 3, 2], [2, 3, 1]]          # +y: o, o + z, o + z + x, o + x
    assert quads[4] == [[1, 2, 1], [1, 3, 1], [2, 3, 1], [2, 2, 1]]          # -z: (u, v) = (x, y): o, o + y, o + x + y, o + x
    assert quads[5] == [[1, 2, 2], [2, 2, 2], [2, 3, 2], [1, 3, 2]]          # +z: o, o + x, o + x + y, o + y
    # the normal (b - a) x (c - a) of every triangle points from set to clear
    p = np.array(c)[tris.astype(np.int64)]
    normals = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    want = np.repeat(np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]]), 2, axis=0)
    assert np.array_equal(normals, want)
    # faces ascend by brick word first: at B = 2 voxel (4, 0, 0) is in word 1, (3, 7, 3) in word 2 and (0, 0, 4) in word 4
    vox, dirs = MR.faces(voxels_at(8, [(0, 0, 4), (3, 7, 3), (4, 0, 0)]))
    assert dirs.tolist() == [0, 1, 2, 3, 4, 5] * 3
    assert (vox[:6] == [4, 0, 0]).all() and (vox[6:12] == [3, 7, 3]).all() and (vox[12:] == [0, 0, 4]).all()
    # ... then by direction, then by bit: voxel (1, 0, 0) is bit 1 and (0, 1, 0) bit 4 of word 0
    vox, dirs = MR.faces(voxels_at(4, [(0, 1, 0), (1, 0, 0)]))
    assert dirs.tolist() == [d for d in range(6) for _ in range(2)] and vox.tolist() == [[1, 0, 0], [0, 1, 0]] * 6


@functools.lru_cache(maxsize=None)
def random_grids():
    rng = np.random.default_rng(77)
    return [(N, density, rng.random((N, N, N)) < density) for N in (4, 8, 16) for density in (0.05, 0.5, 0.95)]


def test_the_invariants_on_random_grids():
    for N, density, inside in random_grids():
        check_invariants(inside, *MR.mesh(inside), MR.summary(inside))


# ---- the library's bit arithmetic, built for the host --------------------------------------------------------------------------------------
def _build(name, flags):
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    deps = [SRC, os.path.join(CSRC, "mesh_vmesh.hpp"), os.path.join(CSRC, "mesh_vox.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe])      # (plain g++: the header touches no device)
    return exe


def run(exe, grids):
    """-> per grid the program's five arrays: summary, face masks [B^3, 6], corner masks [(B + 1)^3, 4], vertices f32 [V, 3], triangles [T, 3]"""
    queries = []
    for inside in grids:
        bricks = V.pack(inside)
        queries.append(f"G {bricks.shape[0].bit_length() - 1} " + " ".join(f"{int(w):x}" for w in bricks.reshape(-1)))
    res = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stdout[-300:], res.stderr[-2000:])
    lines = res.stdout.splitlines()
    assert len(lines) == 5 * len(grids) and all(line[0] == "SMCVT"[k % 5] for k, line in enumerate(lines))
    out = []
    for g in range(len(grids)):
        s, m, c, v, t = (np.array([int(x, 16) for x in line.split()[1:]], np.uint64) for line in lines[5 * g:5 * g + 5])
        out.append((s.tolist(), m.reshape(-1, 6), c.reshape(-1, 4), v.astype(np.uint32).view(np.float32).reshape(-1, 3), t.reshape(-1, 3)))
    return out


@functools.lru_cache(maxsize=None)
def sample_grids():
    """depth 0: every neighbour of the one brick absent, corner bricks 0 and B = 1 per axis.  Depth 1: every brick with three neighbours
    present and three absent.  Depth 2: bricks with all six present.  Random at several densities, empty, full, and the pinches."""
    rng = np.random.default_rng(78)
    grids = [np.zeros((4, 4, 4), bool), np.ones((4, 4, 4), bool), np.ones((8, 8, 8), bool), np.ones((16, 16, 16), bool)]
    grids += [rng.random((4, 4, 4)) < d for d in (0.05, 0.5, 0.95)]
    grids += [rng.random((8, 8, 8)) < d for d in (0.02, 0.05, 0.3, 0.5, 0.5, 0.8, 0.95, 0.99)]
    grids += [rng.random((16, 16, 16)) < d for d in (0.01, 0.5, 0.99)]
    grids += [voxels_at(8, [(3, 3, 3), (4, 4, 3)]), voxels_at(8, [(3, 3, 3), (4, 4, 4)]), voxels_at(8, [(7, 7, 7)]), voxels_at(8, [(0, 0, 0)])]
    grids += [make() for make, _ in KNOWN.values()]
    return grids


def compare(got, inside):
    s, masks, corners, verts, tris = got
    assert s == MR.summary(inside)
    assert np.array_equal(masks, MR.brick_face_masks(inside))
    assert np.array_equal(corners, MR.corner_brick_masks(inside))
    want_v, want_t = MR.mesh(inside)
    assert np.array_equal(verts.view(np.uint32), want_v.view(np.uint32)) and np.array_equal(tris, want_t)


def test_the_bit_arithmetic_is_the_references():
    grids = sample_grids()
    for got, inside in zip(run(_build("mesh_vmesh_host", ["-O1"]), grids), grids):
        compare(got, inside)
    # the sample reaches what it is meant to: corner bricks at index B that hold used corners, bricks with six neighbours
    assert any(MR.corner_brick_masks(g)[-1, 0] != 0 for g in grids) and any(g.shape[0] == 16 for g in grids)


def test_the_arithmetic_runs_clean_under_sanitizers():
    """the same program as a stand-alone executable with ASan and UBSan, on the same input: exit 0, nothing on stderr (`run` asserts
    both), the same answers"""
    grids = sample_grids()
    plain = run(_build("mesh_vmesh_host", ["-O1"]), grids)
    san = run(_build("mesh_vmesh_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), grids)
    assert len(plain) == len(san)
    for a, b in zip(plain, san):
        assert a[0] == b[0] and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a[1:], b[1:]))


# ---- the interface -----------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fidget_hip.h")).read()
    stated = " ".join(re.sub(r"^ \* ?", "", hdr, flags=re.M).split())          # (the comment's lines without their leading " * ")
    for words in ("counter-clockwise seen from outside", "o, o + u, o + u + v, o + v", "o, o + v, o + u + v, o + u", "brick word index, then d, then",
                  "((c >> 2) (B + 1) + (b >> 2)) (B + 1) + (a >> 2)", "float(2 a - N) * (1.0f / N)", "FHIP_ERR_OVERFLOW"):
        assert words in stated, words          # the definitions are in the comment
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    lib = C.CDLL(F.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in F.EXPORTS and getattr(F.lib(), name).argtypes is not None, name
    assert re.search(r"fhip_voxels_mesh\s*\([^;]*fhip_mesh\s*\*\*\s*out\s*\)", hdr)          # a real fhip_mesh
    assert re.search(r"fhip_voxels_surface\s*\([^;]*uint64_t\s+out\[10\]\s*\)", hdr)
    assert all(callable(getattr(F.Voxels, m)) for m in ("mesh", "surface"))
    ffi = open(os.path.join(ROOT, "rust", "fidget-hip", "src", "ffi.rs")).read()
    assert all(f"pub fn {name}(" in ffi for name in ENTRY_POINTS)
    mesh_only = open(os.path.join(ROOT, "tools", "src_hash.py")).read()
    assert all(f'"{name}"' in mesh_only for name in ("mesh_vmesh.hpp", "vmesh.hip", "capi_vmesh.hpp"))          # mesh-only: the render path's hash stays
    assert all(name in F._SOURCES for name in ("mesh_vmesh.hpp", "vmesh.hip", "capi_vmesh.hpp"))
    s = F.Surface(16, [1, 2, 3, 4, 5, 6, 30, 50, 21, 9])
    assert (s.faces, s.vertices, s.edges, s.n_faces, s.n, s.euler) == ((1, 2, 3, 4, 5, 6), 30, 50, 21, 9, 1) and s.area == 21 / 64
