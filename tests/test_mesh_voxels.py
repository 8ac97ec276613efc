"""A triangle mesh to a voxel bitmap without a GPU: the reference of mesh_voxels_ref.py on meshes whose solids are known - the boundary
mesh of a random bitmap voxelized back, an octahedron with everything on voxel centres, nested cubes, a box poking out of the grid -
and against invariants; the arithmetic of fidget_amd/csrc/mesh_trivox.hpp built for the host (tests/host_build/mesh_trivox_host.cpp) -
the snap, the set-up, the cover test with the crossing, the fill inside a word and along a row - against the reference, at depth 10
against Python's unbounded integers on triangles that span the whole allowed range; that program under ASan and UBSan; the entry
points as the header states them, and read_stl."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import fidget_amd as F
import mesh_voxels_ref as MV
import stl_ref
import voxel_mesh_ref as VM
import voxels_ref as V
from test_voxel_mesh import box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "mesh_trivox_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")
ENTRY_POINTS = ("fhip_triangles_voxels", "fhip_mesh_voxels")
NEW_FILES = ("mesh_trivox.hpp", "trivox.hip", "capi_trivox.hpp")
TETRA = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.uint64)


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------------
def box_mesh(lo, hi):
    """the box [lo, hi] per axis in world coordinates -> (vertices float32 [8, 3], triangles uint64 [12, 3]), outward"""
    lo, hi = (lo if isinstance(lo, tuple) else (lo,) * 3), (hi if isinstance(hi, tuple) else (hi,) * 3)
    v = np.array([[(hi if c >> a & 1 else lo)[a] for a in range(3)] for c in range(8)], np.float32)
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]          # -x +x -y +y -z +z
    t = np.array([tri for q in quads for tri in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.uint64)
    return v, t


def lattice_box(N, lo, hi):
    """... with its faces on the voxel borders lo and hi, in voxels"""
    w = lambda a: tuple((2.0 * x - N) / N for x in (a if isinstance(a, tuple) else (a,) * 3))          # noqa: E731
    return box_mesh(w(lo), w(hi))


def octahedron(N, at, reach):
    """the centre on the centre of voxel (at, at, at) of N^3, the six tips `reach` voxels away: on voxel centres too"""
    c, r = (2.0 * at + 1 - N) / N, 2.0 * reach / N
    v = np.array([[c - r, c, c], [c + r, c, c], [c, c - r, c], [c, c + r, c], [c, c, c - r], [c, c, c + r]], np.float32)
    t = []
    for sx in (0, 1):
        for sy in (0, 1):
            for sz in (0, 1):
                tri = (sx, 2 + sy, 4 + sz)
                t.append(tri if (sx + sy + sz) % 2 else tri[::-1])
    return v, np.array(t, np.uint64)


def octahedron8():
    """N = 8: the centre on the centre of voxel (4, 4, 4), the six tips two voxels away"""
    return octahedron(8, 4, 2)


def tetrahedra(n, seed, reach=1.3):
    """n random tetrahedra with vertices in [-reach, reach] -> (vertices [4 n, 3], triangles [4 n, 3])"""
    v = np.random.default_rng(seed).uniform(-reach, reach, (4 * n, 3)).astype(np.float32)
    t = np.concatenate([TETRA + np.uint64(4 * i) for i in range(n)])
    return v, t


def together(*meshes):
    vs, ts, at = [], [], 0
    for v, t in meshes:
        vs.append(v)
        ts.append(t + np.uint64(at))
        at += len(v)
    return np.concatenate(vs), np.concatenate(ts)


def sliver_and_flat():
    """a sliver a hundredth of a voxel wide at N = 16, and a triangle edge-on to x"""
    v = np.array([[-0.9, -0.7, -0.8], [0.9, 0.7, 0.8], [0.9, 0.7 + 0.00125, 0.8], [0.3, 0.2, -0.5], [0.3, 0.2, 0.5], [-0.6, 0.2, 0.1]], np.float32)
    return v, np.array([[0, 1, 2], [3, 4, 5]], np.uint64)


def spanning16():
    """16 triangles: one tetrahedron spanning the grid and a box poking out through +x and -x"""
    v = np.array([[-0.97, -0.91, -0.93], [0.95, -0.83, -0.89], [0.03, 0.96, -0.77], [0.11, 0.07, 0.98]], np.float32)
    return together((v, TETRA), box_mesh((-1.3, -0.35, -0.2), (1.4, 0.3, 0.45)))


# ---- known answers ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_grids():
    rng = np.random.default_rng(91)
    return [rng.random((N, N, N)) < d for N in (4, 8, 16) for d in (0.1, 0.4, 0.7)]


def test_the_boundary_mesh_of_a_bitmap_voxelizes_back_to_it():
    """every x-face's diagonal passes through a column centre: the tie rule decides every crossing"""
    for g in random_grids():
        N = g.shape[0]
        verts, tris = VM.mesh(g)
        s = VM.summary(g)
        inside, info = MV.voxelize(verts, tris, N)
        assert np.array_equal(inside, g)
        assert info["open_rows"] == 0 and info["rejected"] == 0 and info["set_voxels"] == int(g.sum())
        assert info["clipped"] == int(g[N - 1].sum())          # the +x faces on the grid's border: their crossing lies beyond the last centre
        assert info["flat"] == 2 * sum(s[2:6]) and info["crossings"] == s[0] + s[1] and info["triangles"] == 2 * s[8]


def test_the_octahedron_on_voxel_centres_is_read_half_open():
    v, t = octahedron8()
    inside, info = MV.voxelize(v, t, 8)
    want = np.zeros((8, 8, 8), bool)
    want[2:6, 4, 4] = True          # [-2, 2) on the middle row
    for dj, dk in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        want[3:5, 4 + dj, 4 + dk] = True          # nothing on the rows through the y and z tips, nor on the silhouette's edges
    assert int(want.sum()) == 12 and np.array_equal(inside, want)
    assert info["open_rows"] == 0 and info["flat"] == 0


def variants(v, t, seed):
    """the same surface: the triangles in another order, some turned over, their corners rotated"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(4):
        u = t[rng.permutation(len(t))].copy()
        turn = rng.random(len(u)) < 0.5
        u[turn] = u[turn][:, ::-1]
        rot = rng.integers(0, 3, len(u))
        u = np.stack([np.roll(row, r) for row, r in zip(u, rot)])
        out.append(u)
    return out


def test_the_result_does_not_depend_on_order_orientation_or_form():
    for (v, t), N in ((octahedron8(), 8), (tetrahedra(6, 5), 16), (VM.mesh(random_grids()[4]), 8)):
        inside, info = MV.voxelize(v, t, N)
        for u in variants(v, t, 17):
            again, info2 = MV.voxelize(v, u, N)
            assert np.array_equal(again, inside) and info2 == info
        soup, info3 = MV.voxelize(MV.soup(v, t).reshape(-1, 3), None, N)
        assert np.array_equal(soup, inside) and info3 == info


def test_nested_cubes_make_a_cavity():
    inside, info = MV.voxelize(*together(lattice_box(16, 2, 14), lattice_box(16, 5, 11)), 16)
    assert np.array_equal(inside, box(16, 5, 11, False, into=box(16, 2, 14))) and info["open_rows"] == 0
    assert info["crossings"] == 2 * 12 * 12 + 2 * 6 * 6 and info["flat"] == 16


def test_a_single_triangle_is_an_open_mesh():
    v = np.array([[0.1, -0.8, -0.7], [0.2, 0.9, -0.6], [-0.3, 0.1, 0.8]], np.float32)
    inside, info = MV.voxelize(v, None, 16)
    assert info["open_rows"] == info["crossings"] > 0 and info["clipped"] == 0
    assert inside[15].sum() == info["open_rows"]          # every row runs on to the border


def rejected_mesh():
    """a tetrahedron, and three triangles that must go: a NaN, a coordinate of 1.6, an index beyond the vertices"""
    v, t = tetrahedra(1, 3)
    v = np.concatenate([v, np.array([[np.nan, 0, 0], [0, 1.6, 0]], np.float32)])
    return v, np.concatenate([t, np.array([[0, 1, 4], [5, 1, 2], [0, 6, 2]], np.uint64)])


def test_what_cannot_be_snapped_is_rejected_and_not_read():
    v, t = rejected_mesh()
    inside, info = MV.voxelize(v, t, 8)
    clean, info0 = MV.voxelize(v[:4], t[:4], 8)
    assert info["rejected"] == 3 and info["triangles"] == 7 and np.array_equal(inside, clean)
    assert {k: info[k] for k in info if k not in ("rejected", "triangles")} == {k: info0[k] for k in info0 if k not in ("rejected", "triangles")}
    # an infinity, and the range is closed: 1.5 itself is taken
    w = np.array([[np.inf, 0, 0], [0, 0.5, 0], [0, 0, 0.5], [1.5, -1.5, 0], [0, 1.5, 0], [0, 0, 1.5]], np.float32)
    assert MV.voxelize(w, None, 4)[1]["rejected"] == 1
    # the matrix is applied first: half the size is inside the range again
    half = np.concatenate([0.5 * np.eye(3), np.zeros((3, 1))], axis=1)
    assert MV.voxelize(np.array([[3.0, 0, 0], [0, 3.0, 0], [0, 0, 3.0]], np.float32), None, 4, half)[1]["rejected"] == 0


def test_a_box_beyond_the_border_fills_the_grid():
    for N in (4, 16):
        inside, info = MV.voxelize(*box_mesh(-1.25, 1.25), N)
        assert inside.all() and info["open_rows"] == 0 and info["clipped"] == N * N and info["crossings"] == 2 * N * N


# ---- the library's arithmetic, built for the host --------------------------------------------------------------------------------------------
def _build(name, flags):
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("mesh_trivox.hpp", "mesh_vmesh.hpp", "mesh_vox.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        # (plain g++: the header touches no device; no contraction, as the library is built)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, SRC, "-o", exe])
    return exe


def query(depth, v, t, m=None, cols=None):
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    words = ["Q", f"{depth:x}", "1" if m is not None else "0"]
    if m is not None:
        words += [f"{int(x):x}" for x in np.ascontiguousarray(m, np.float64).reshape(-1)[:12].view(np.uint64)]
    words += [f"{len(v):x}"] + [f"{int(x):x}" for x in v.reshape(-1).view(np.uint32)]
    if t is None:
        words += ["0", f"{len(v) // 3:x}"]
    else:
        t = np.asarray(t, np.uint64).reshape(-1, 3)
        words += ["1", f"{len(t):x}"] + [f"{int(x):x}" for x in t.reshape(-1)]
    if cols is None:
        words.append("G")
    else:
        words += ["C", f"{len(cols):x}"] + [f"{int(x):x}" for jk in cols for x in jk]
    return " ".join(words)


def run(exe, queries):
    res = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stdout[-300:], res.stderr[-2000:])
    return res.stdout.splitlines()


def numbers(line, tag):
    assert line[0] == tag, line[:40]
    return [int(x, 16) for x in line.split()[1:]]


@functools.lru_cache(maxsize=None)
def grid_cases():
    """(depth, vertices, triangles or None, matrix or None): the cases above, and random tetrahedra at depths 0 to 2"""
    turn = np.array([[0.6, -0.8, 0.0, 0.05], [0.8, 0.6, 0.0, -0.1], [0.0, 0.0, 1.1, 0.02]])
    cases = [(g.shape[0].bit_length() - 3, *VM.mesh(g), None) for g in random_grids()]
    cases += [(1, *octahedron8(), None), (2, *together(lattice_box(16, 2, 14), lattice_box(16, 5, 11)), None)]
    cases += [(1, *rejected_mesh(), None), (0, *box_mesh(-1.25, 1.25), None), (2, *box_mesh(-1.25, 1.25), None)]
    cases += [(2, np.array([[0.1, -0.8, -0.7], [0.2, 0.9, -0.6], [-0.3, 0.1, 0.8]], np.float32), None, None)]
    cases += [(depth, *tetrahedra(n, 20 + depth), None) for depth, n in ((0, 5), (1, 8), (2, 20))]
    cases += [(2, *together(tetrahedra(20, 7), sliver_and_flat()), None), (2, *spanning16(), None)]
    cases += [(1, *tetrahedra(6, 9, 1.0), turn), (2, MV.soup(*tetrahedra(5, 11, 0.9)).reshape(-1, 3), None, turn)]
    cases += [(1, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint64), None)]
    return cases


def check_grids(lines):
    cases = grid_cases()
    assert len(lines) == 2 * len(cases)
    for n, (depth, v, t, m) in enumerate(cases):
        inside, info = MV.voxelize(v, t, 4 << depth, m)
        assert numbers(lines[2 * n], "I") == [info[k] for k in MV.INFO], (n, info)
        assert np.array_equal(np.array(numbers(lines[2 * n + 1], "B"), np.uint64), V.pack(inside).reshape(-1)), n


def test_the_arithmetic_is_the_references():
    cases = grid_cases()
    check_grids(run(_build("mesh_trivox_host", ["-O1"]), [query(depth, v, t, m) for depth, v, t, m in cases]))
    info = MV.voxelize(*sliver_and_flat(), 16)[1]
    assert info["flat"] == 1 and info["W"] > 100          # what the names promise: one triangle edge-on; the sliver not, with a box full of columns


@functools.lru_cache(maxsize=None)
def extremes():
    """depth 10: triangles with corners on the corners of the allowed range and on column centres, and the columns to ask about - the
    grid's corners, centres on the diagonal edge, on the other edges and on the vertices, and some anywhere"""
    N = 4096
    c = lambda j: (2.0 * j + 1 - N) / N          # noqa: E731  (the centre of column or voxel j: exact in float32)
    R = 1.5
    tris = []
    for xs in ((-R, R, -R), (R, -R, R), (R, R, R), (-R, -R, -R), (-R, R, R), (R, -R, -R)):
        tris.append([(xs[0], -R, -R), (xs[1], R, -R), (xs[2], R, R)])          # the edge a -> c is the diagonal through every centre (j, j)
        tris.append([(xs[0], -R, -R), (xs[2], R, R), (xs[1], R, -R)])          # ... turned over
        tris.append([(xs[0], c(0), c(0)), (xs[1], c(N - 1), c(0)), (xs[2], c(N - 1), c(N - 1))])          # corners on centres
        tris.append([(xs[0], R, -R), (xs[1], -R, c(1000)), (xs[2], c(3000), R)])
    tris.append([(c(100), c(0), c(0)), (c(100), c(N - 1), c(0)), (c(100), c(0), c(N - 1))])          # the crossing on a voxel's centre: at or beyond
    tris.append([(c(0), -R, -R), (c(N - 1), R, -R), (c(2047), -R, R)])
    tris.append([(-R, R, c(7)), (R, -R, c(N - 1)), (c(5), c(3), -R)])
    rng = np.random.default_rng(10)
    cols = [(0, 0), (N - 1, 0), (0, N - 1), (N - 1, N - 1), (2047, 2047), (2048, 2048), (1, 1), (N - 2, N - 2), (N - 1, 2047), (2047, 0), (2048, 0), (N - 1, 1),
            (1000, 0), (3000, N - 1), (0, 1000), (5, 3), (7, 7), (N - 1, 7), (0, 7), (100, 100), (N - 2, 1), (1, N - 2), (0, 2048), (3, 5)]
    cols += [tuple(int(x) for x in rng.integers(0, N, 2)) for _ in range(24)]
    cols += [(int(j), int(j)) for j in rng.integers(0, N, 8)]
    return np.array(tris, np.float32).reshape(-1, 3), cols


def check_extremes(lines):
    N = 4096
    v, cols = extremes()
    q, rejected = MV.corners(v, None, N)
    assert not rejected.any() and len(lines) == 2 * len(q)
    assert int(q.min()) == -64 * N and int(q.max()) == 320 * N          # the whole range
    seen = set()
    for t, tri in enumerate(q):
        a, b, c, D = MV.oriented(*[[int(x) for x in p] for p in tri])
        j0, j1, k0, k1 = MV.column_box(a, b, c, N)
        assert D > 0 and numbers(lines[2 * t], "T") == [0, j0, k0, j1 - j0 + 1, k1 - k0 + 1]
        want = [MV.crossing_scalar(tri, N, j, k) for j, k in cols]
        assert numbers(lines[2 * t + 1], "C") == [0 if w is None else (1 if w == N else w + 2) for w in want], t
        seen |= {"none" if w is None else ("exit" if w == N else ("first" if w == 0 else "between")) for w in want}
    assert seen == {"none", "exit", "first", "between"}
    # the crossing that lies exactly on the centre of voxel 100 toggles voxel 100
    assert MV.crossing_scalar(q[24], N, 5, 5) == 100


def test_the_bit_budget_holds_at_depth_10():
    v, cols = extremes()
    check_extremes(run(_build("mesh_trivox_host", ["-O1"]), [query(10, v, None, None, cols)]))


def test_the_arithmetic_runs_clean_under_sanitizers():
    """the same program as a stand-alone executable with ASan and UBSan, on the same input: exit 0, nothing on stderr (`run` asserts
    both), the same output - a signed overflow in the depth-10 products would stop it"""
    v, cols = extremes()
    queries = [query(depth, v_, t, m) for depth, v_, t, m in grid_cases()] + [query(10, v, None, None, cols)]
    plain = run(_build("mesh_trivox_host", ["-O1"]), queries)
    san = run(_build("mesh_trivox_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), queries)
    assert plain == san
    n = 2 * len(grid_cases())
    check_grids(san[:n])
    check_extremes(san[n:])


# ---- the interface -----------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fidget_hip.h")).read()
    stated = " ".join(re.sub(r"^ \* ?", "", hdr, flags=re.M).split())          # (the comment's lines without their leading " * ")
    for words in ("((m0 x + m1 y) + m2 z) + m3", "q = llrint(w (128 N) + 128 N)", "voxel i has its centre at 256 i + 128", "outside [-1.5, 1.5]",
                  "before any conversion to an integer", "D = (b.y - a.y)(c.z - a.z) - (b.z - a.z)(c.y - a.y)", "e = (r.y - p.y)(P.z - p.z) - (r.z - p.z)(P.y - p.y)",
                  "r.y - p.y > 0, or when r.y - p.y == 0 and r.z - p.z < 0", "i* = ceil((num - (128 - xmin) D) / (256 D))", "at or beyond it",
                  "XOR the exit plane's bit is 1", "n_triangles == 0 gives an all-zero bitmap", "fhip_mesh_vertices_dev"):
        assert words in stated, words          # the definition is in the comment
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    lib = C.CDLL(F.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in F.EXPORTS and getattr(F.lib(), name).argtypes is not None, name
    assert re.search(r"fhip_triangles_voxels\s*\(\s*fhip_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*vertices\s*,\s*uint64_t\s+n_vertices\s*,\s*const\s+uint64_t\s*\*\s*triangles\s*,"
                     r"\s*uint64_t\s+n_triangles\s*,\s*int\s+on_device\s*,\s*const\s+double\s*\*\s*mesh_to_world\s*,\s*uint32_t\s+depth\s*,\s*uint64_t\s*\*\s*out\s*,"
                     r"\s*int\s+out_on_device\s*,\s*uint64_t\s+info\[8\]\s*\)", hdr)
    assert re.search(r"fhip_mesh_voxels\s*\(\s*fhip_ctx\s*\*\s*ctx\s*,\s*const\s+fhip_mesh\s*\*\s*mesh\s*,\s*const\s+double\s*\*\s*mesh_to_world\s*,\s*uint32_t\s+depth\s*,"
                     r"\s*uint64_t\s*\*\s*out\s*,\s*int\s+out_on_device\s*,\s*uint64_t\s+info\[8\]\s*\)", hdr)
    assert callable(F.voxelize_mesh) and callable(F.read_stl) and callable(F.Mesh.voxelize)
    assert F.MESH_INFO == MV.INFO and "open_rows" in F.voxelize_mesh.__doc__
    ffi = open(os.path.join(ROOT, "rust", "fidget-hip", "src", "ffi.rs")).read()
    assert all(f"pub fn {name}(" in ffi for name in ENTRY_POINTS)
    assert "fhip_mesh_voxels" in open(os.path.join(ROOT, "rust", "fidget-hip", "src", "voxels.rs")).read()
    mesh_only = open(os.path.join(ROOT, "tools", "src_hash.py")).read()
    assert all(f'"{name}"' in mesh_only for name in NEW_FILES)          # mesh-only: the render path's hash stays
    assert all(name in F._SOURCES for name in NEW_FILES)


def test_read_stl_reads_what_write_stl_writes(tmp_path):
    v, t = together(tetrahedra(3, 2), octahedron8())
    data = stl_ref.stl_bytes(v, t)
    want = MV.soup(v, t)
    for given in (data, data.tobytes(), bytearray(data.tobytes()), memoryview(data.tobytes())):
        got = F.read_stl(given)
        assert got.dtype == np.float32 and got.shape == (len(t), 3, 3) and np.array_equal(got, want)
    path = tmp_path / "mesh.stl"
    path.write_bytes(data.tobytes())
    assert np.array_equal(F.read_stl(str(path)), want) and np.array_equal(F.read_stl(path), want)
    assert F.read_stl(stl_ref.stl_bytes(v, t[:0])).shape == (0, 3, 3)
    with pytest.raises(ValueError, match="ASCII"):
        F.read_stl(b"solid part\n facet normal 0 0 1\n  outer loop\n   vertex 0 0 0\n   vertex 1 0 0\n   vertex 0 1 0\n  endloop\n endfacet\nendsolid part\n")
    with pytest.raises(ValueError, match="not a binary STL"):
        F.read_stl(data.tobytes()[:-7])
