"""The check of a triangle mesh without a GPU: the reference of mesh_topology_ref.py on meshes whose answers are known by hand - a
tetrahedron, a cube with a face removed, with a triangle flipped, two cubes sharing an edge, a duplicated triangle, a repeated corner,
-0 welded to +0, a cube inside a cube, no triangles, rejected triangles, a shuffle - and on the boundary meshes of voxel bitmaps against
their Euler numbers; the pipeline of fidget_amd/csrc/mesh_topo.hpp built for the host (tests/host_build/mesh_topo_host.cpp) against the
reference, integers equal and the per-triangle float64 terms bit for bit, with tables at load factor 1 and too small; that program under
ASan and UBSan; the entry points as the header states them."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import fidget_amd as F
import mesh_topology_ref as MT
import voxel_mesh_ref as VM
from test_mesh_voxels import TETRA, box_mesh, together

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "mesh_topo_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")
ENTRY_POINTS = ("fhip_triangles_topology", "fhip_mesh_topology", "fhip_topology_counts", "fhip_topology_vertex_rows", "fhip_topology_vertices", "fhip_topology_triangles",
                "fhip_topology_triangle_shells", "fhip_topology_vertices_dev", "fhip_topology_triangles_dev", "fhip_topology_triangle_shells_dev", "fhip_topology_shells",
                "fhip_topology_edges", "fhip_topology_free")
NEW_FILES = ("mesh_topo.hpp", "topo.hip", "capi_topo.hpp")


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------------
def soup(v, t):
    return np.ascontiguousarray(np.asarray(v, np.float32)[np.asarray(t, np.int64)])


def tetrahedron():
    """the corner of the unit cube, outward: volume 1 / 6"""
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32), np.ascontiguousarray(TETRA[:, ::-1])


def open_cube():
    v, t = box_mesh(-0.5, 0.5)
    return v, t[:10]          # without the two triangles of +z


def flipped_cube():
    v, t = box_mesh(-0.5, 0.5)
    t = t.copy()
    t[3] = t[3, ::-1]
    return v, t


def two_cubes():
    """[-1, 0]^2 x [0, 1] and [0, 1]^3: they share the edge from (0, 0, 0) to (0, 0, 1)"""
    return together(box_mesh((-1.0, -1.0, 0.0), (0.0, 0.0, 1.0)), box_mesh(0.0, 1.0))


def doubled_triangle():
    v, t = tetrahedron()
    return v, np.concatenate([t, t[:1]])


def repeated_corner():
    v, t = tetrahedron()
    return v, np.concatenate([t[:2], np.array([[1, 1, 2]], np.uint64), t[2:]])


def signed_zeros():
    """two triangles that share the origin, once as +0 and once as -0"""
    return np.array([[[0.0, 0.0, 0.0], [1, 0, 0], [0, 1, 0]], [[-0.0, 0.0, -0.0], [0, 1, 0], [-1, 0, 0]]], np.float32)


def nested_cubes():
    vo, to = box_mesh(-1.0, 1.0)
    vi, ti = box_mesh(-0.5, 0.5)
    return together((vo, to), (vi, np.ascontiguousarray(ti[:, ::-1])))


def lattice_tetrahedra(n, seed=3):
    """n tetrahedra with vertices drawn from the lattice {-1, -1/2, 0, 1/2, 1}^3 -> a soup [4 n, 3, 3]: welded, they share vertices and
    edges in every way - repeated corners, edges with many uses, edges used twice in the same direction"""
    p = (np.random.default_rng(seed).integers(0, 5, (4 * n, 3)).astype(np.float32) - 2) / 2
    t = np.concatenate([TETRA + np.uint64(4 * i) for i in range(n)])
    return soup(p, t)


def thinned(tris):
    """... every 7th triangle dropped and every 11th flipped: all four classes of edges"""
    tris = tris.copy()
    tris[::11] = tris[::11, ::-1]
    return np.ascontiguousarray(tris[np.arange(len(tris)) % 7 != 0])


@functools.lru_cache(maxsize=None)
def bitmaps():
    """inside[i, j, k] of 8^3: two voxels touching along an edge; random at densities 0.1 and 0.5"""
    touching = np.zeros((8, 8, 8), bool)
    touching[1, 1, 1] = touching[2, 2, 1] = True
    rng = np.random.default_rng(1)
    return {"touching": touching, "sparse": rng.random((8, 8, 8)) < 0.1, "dense": rng.random((8, 8, 8)) < 0.5}


@functools.lru_cache(maxsize=None)
def hand_meshes():
    """name -> (vertices, triangles or None, weld or None)"""
    m = {"tetrahedron": (*tetrahedron(), None), "open cube": (*open_cube(), None), "flipped cube": (*flipped_cube(), None),
         "two cubes, indexed": (*two_cubes(), None), "two cubes, welded": (soup(*two_cubes()), None, None), "two cubes, indexed and welded": (*two_cubes(), True),
         "doubled triangle": (*doubled_triangle(), None), "repeated corner": (*repeated_corner(), None), "signed zeros": (signed_zeros(), None, None),
         "nested cubes": (*nested_cubes(), None), "nested cubes, soup": (soup(*nested_cubes()), None, None),
         "nothing": (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint64), None), "no soup": (np.zeros((0, 3, 3), np.float32), None, None)}
    return m


@functools.lru_cache(maxsize=None)
def reference(name):
    v, t, weld = hand_meshes()[name]
    return MT.topology(v, t, weld)


# ---- the reference against hand-known meshes -----------------------------------------------------------------------------------------------
def test_a_tetrahedron():
    r = reference("tetrahedron")
    c = r["counts"]
    assert (c["triangles"], c["vertices"], c["edges"], c["shells"], c["degenerate"]) == (4, 4, 6, 1, 0)
    assert MT.closed(r) and MT.manifold(r) and MT.euler(r) == 2
    assert r["shells"]["volume6"][0] == 1.0 and r["shells"]["triangles"][0] == 4 and r["shells"]["first"][0] == 0
    assert abs(r["shells"]["area2"][0] - (3.0 + np.sqrt(3.0))) < 1e-15 * 8
    assert np.array_equal(r["shells"]["lo"], [[0, 0, 0]]) and np.array_equal(r["shells"]["hi"], [[1, 1, 1]])
    v, t = tetrahedron()
    inward = MT.topology(v, t[:, ::-1])
    assert inward["shells"]["volume6"][0] == -1.0 and MT.closed(inward)


def test_a_cube_with_a_face_removed_names_its_hole():
    r = reference("open cube")
    c = r["counts"]
    assert (c["boundary"], c["unbalanced"], c["flipped"], c["nonmanifold"], c["shells"]) == (4, 4, 0, 0, 1)
    assert not MT.closed(r) and not MT.manifold(r) and r["shells"]["unbalanced"][0] == 4
    assert sorted(map(tuple, r["edges"]["boundary"].tolist())) == [(4, 5), (4, 6), (5, 7), (6, 7)]          # the rim of +z
    assert np.array_equal(r["edges"]["boundary"], r["edges"]["unbalanced"]) and c["vertices"] == 8 and c["edges"] == 17


def test_a_cube_with_a_triangle_flipped():
    r = reference("flipped cube")
    c = r["counts"]
    assert (c["flipped"], c["unbalanced"], c["boundary"], c["nonmanifold"], c["shells"]) == (3, 3, 0, 0, 1)
    t = flipped_cube()[1][3]
    assert sorted(map(tuple, r["edges"]["flipped"].tolist())) == sorted((int(min(a, b)), int(max(a, b))) for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])))
    assert not MT.closed(r) and MT.euler(r) == 2


def test_two_cubes_sharing_an_edge():
    apart, welded, both = reference("two cubes, indexed"), reference("two cubes, welded"), reference("two cubes, indexed and welded")
    assert apart["counts"]["shells"] == 2 and apart["counts"]["vertices"] == 16 and MT.manifold(apart) and MT.euler(apart) == 4
    for r in (welded, both):
        c = r["counts"]
        assert (c["triangles"], c["vertices"], c["edges"], c["nonmanifold"], c["unbalanced"], c["boundary"], c["shells"]) == (24, 14, 35, 1, 0, 0, 1)
        assert MT.closed(r) and not MT.manifold(r) and MT.euler(r) == 3
        a, b = r["edges"]["nonmanifold"][0]
        assert sorted([r["vertices"][a].tolist(), r["vertices"][b].tolist()]) == [[0, 0, 0], [0, 0, 1]]
        assert r["shells"]["volume6"][0] == 12.0 and r["shells"]["area2"][0] == 24.0


def test_a_duplicated_triangle_and_a_repeated_corner():
    r = reference("doubled triangle")
    assert (r["counts"]["nonmanifold"], r["counts"]["unbalanced"], r["counts"]["edges"], r["counts"]["shells"]) == (3, 3, 6, 1)
    r = reference("repeated corner")
    c = r["counts"]
    assert (c["triangles"], c["degenerate"], c["edges"], c["shells"]) == (5, 1, 6, 1) and MT.closed(r) and MT.manifold(r) and MT.euler(r) == 2
    assert r["triangle_shell"].tolist() == [0, 0, MT.NO_SHELL, 0, 0] and np.array_equal(r["triangles"][2], [1, 1, 2])
    assert r["shells"]["triangles"][0] == 4 and r["shells"]["volume6"][0] == 1.0


def test_minus_zero_welds_to_plus_zero():
    r = reference("signed zeros")
    assert r["counts"]["vertices"] == 4 and r["counts"]["edges"] == 5 and r["counts"]["shells"] == 1
    assert r["triangles"].tolist() == [[0, 1, 2], [0, 2, 3]]
    assert r["vertices"][0].view(np.uint32).tolist() == [0, 0, 0]          # the first corner's bits
    turned = MT.topology(signed_zeros()[::-1])
    assert turned["vertices"][0].view(np.uint32).tolist() == [0x80000000, 0, 0x80000000] and turned["shells"]["lo"][0].view(np.uint32).tolist()[1:] == [0, 0]


def test_a_cube_inside_a_cube_is_a_cavity():
    for name in ("nested cubes", "nested cubes, soup"):
        r = reference(name)
        assert r["counts"]["shells"] == 2 and MT.closed(r) and MT.manifold(r) and MT.euler(r) == 4
        assert r["shells"]["volume6"].tolist() == [48.0, -6.0] and r["shells"]["first"].tolist() == [0, 12]
        assert np.array_equal(r["triangle_shell"], np.repeat([0, 1], 12).astype(np.uint32))
        assert np.array_equal(r["shells"]["lo"], [[-1, -1, -1], [-0.5, -0.5, -0.5]]) and np.array_equal(r["shells"]["hi"], [[1, 1, 1], [0.5, 0.5, 0.5]])


def test_no_triangles_and_rejected_triangles():
    for name in ("nothing", "no soup"):
        r = reference(name)
        assert all(v == 0 for v in r["counts"].values()) and len(r["triangles"]) == 0 and len(r["shells"]["first"]) == 0
    v, t = tetrahedron()
    bad = v.copy()
    bad[3, 1] = np.nan
    r = MT.topology(bad, t)
    assert r["counts"]["rejected"] == 3 and r["counts"]["triangles"] == 4 and "triangles" not in r
    bad[3, 1] = np.inf
    assert MT.topology(soup(bad, t))["counts"]["rejected"] == 3
    far = t.copy()
    far[2, 0] = 4
    r = MT.topology(v, far)
    assert r["counts"]["rejected"] == 1 and "vertices" not in r


def test_a_shuffle_permutes_the_shells_and_nothing_else():
    tris = thinned(lattice_tetrahedra(300))
    a = MT.topology(tris)
    assert all(a["counts"][k] > 0 for k in MT.COUNTS if k != "rejected") and a["counts"]["shells"] > 10
    order = np.random.default_rng(2).permutation(len(tris))
    b = MT.topology(tris[order])
    assert a["counts"] == b["counts"]
    rows = lambda r: sorted(zip(r["shells"]["triangles"].tolist(), r["shells"]["unbalanced"].tolist(), map(tuple, r["shells"]["lo"].tolist()),          # noqa: E731
                                map(tuple, r["shells"]["hi"].tolist()), r["shells"]["volume6"].tolist(), r["shells"]["area2"].tolist()))
    assert rows(a) == rows(b)
    # the same partition: a's shell of a triangle decides b's
    pairs = set(zip(a["triangle_shell"][order].tolist(), b["triangle_shell"].tolist()))
    assert len(pairs) == a["counts"]["shells"] + 1          # (and the degenerate triangles' no shell)


def test_boundary_meshes_of_bitmaps_are_closed_with_the_surfaces_euler_number():
    facts = {"touching": dict(triangles=24, vertices=14, edges=35, nonmanifold=1, unbalanced=0, boundary=0, shells=1), "sparse": dict(shells=19),
             "dense": dict(nonmanifold=108, shells=1)}
    eulers = {"touching": 3, "dense": -37}
    for name, inside in bitmaps().items():
        v, t, s = VM.mesh_and_summary(inside)
        for r in (MT.topology(v, t), MT.topology(soup(v, t))):
            assert all(r["counts"][k] == n for k, n in facts[name].items()), (name, r["counts"])
            assert MT.closed(r) and r["counts"]["boundary"] == 0 and MT.euler(r) == VM.euler(s) == eulers.get(name, VM.euler(s))
            assert r["counts"]["vertices"] == s[6] and r["counts"]["edges"] == s[7] + s[8] and sum(r["shells"]["volume6"]) * 8 ** 3 / 48 == inside.sum()


def test_lattice_tetrahedra_meet_in_every_way():
    r = MT.topology(lattice_tetrahedra(300))
    c = r["counts"]
    assert c["vertices"] == 125 and c["degenerate"] > 0 and c["nonmanifold"] > 100 and c["shells"] > 1
    assert c["unbalanced"] == 0 and c["boundary"] == 0          # whole tetrahedra, also collapsed ones, are cycles
    c = MT.topology(thinned(lattice_tetrahedra(300)))["counts"]
    assert min(c["boundary"], c["flipped"], c["nonmanifold"], c["unbalanced"], c["degenerate"]) > 0


# ---- the library's pipeline, built for the host --------------------------------------------------------------------------------------------
def _build(name, flags):
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("mesh_topo.hpp", "mesh_vox.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        # (plain g++: the header touches no device; no contraction, as the library is built)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, SRC, "-o", exe])
    return exe


def query(v, t, weld, table_log2=0):
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    weld = (t is None) if weld is None else weld
    words = ["Q", "1" if weld else "0", f"{table_log2:x}", f"{len(v):x}"] + [f"{int(x):x}" for x in v.reshape(-1).view(np.uint32)]
    if t is None:
        words += ["0", f"{len(v) // 3:x}"]
    else:
        t = np.asarray(t, np.uint64).reshape(-1, 3)
        words += ["1", f"{len(t):x}"] + [f"{int(x):x}" for x in t.reshape(-1)]
    return " ".join(words)


def run(exe, queries):
    res = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stdout[-300:], res.stderr[-2000:])
    return res.stdout.splitlines()


def numbers(line, tag):
    assert line.split()[:len(tag.split())] == tag.split(), line[:40]
    return [int(x, 16) for x in line.split()[len(tag.split()):]]


def pow2_at_least(n):
    return max(1, int(n - 1).bit_length())


@functools.lru_cache(maxsize=None)
def host_cases():
    """(vertices, triangles or None, weld, table_log2): the hand meshes, the bitmaps' boundary meshes in both forms, the lattice
    tetrahedra whole, thinned and cut short - with the library's tables, and with tables of the least power of two that holds the
    keys: the 125 vertices in 128 slots, and the edges likewise"""
    cases = [(v, t, weld, 0) for v, t, weld in hand_meshes().values()]
    for inside in bitmaps().values():
        v, t = VM.mesh(inside)
        cases += [(v, t, None, 0), (soup(v, t), None, None, 0), (v, t, True, 0)]
    tets = lattice_tetrahedra(300)
    for tris in (tets, thinned(tets), tets[:255], tets[:256], tets[:257], tets[:1]):
        r = MT.topology(tris)
        tight = pow2_at_least(max(r["counts"]["vertices"], r["counts"]["edges"]))
        cases += [(tris, None, None, 0), (tris, None, None, tight), (r["vertices"], r["triangles"], False, pow2_at_least(r["counts"]["edges"]))]
    v, t = tetrahedron()
    bad = v.copy()
    bad[0, 0] = np.nan
    cases += [(bad, t, None, 0), (v, t + np.uint64(1), True, 0)]
    return cases


def check_host(lines):
    at = 0
    for n, (v, t, weld, log2) in enumerate(host_cases()):
        r = MT.topology(v, t, weld)
        c = numbers(lines[at], "C")
        at += 1
        assert c[:10] == [r["counts"][k] for k in MT.COUNTS], (n, c, r["counts"])
        if "triangles" not in r or r["counts"]["triangles"] == 0:
            continue
        welded = (t is None) if weld is None else weld
        assert c[10:] == ([1 << log2 if welded else 0, 1 << log2] if log2 else [(1 << pow2_at_least(max(2, 4 * c[0]))) * welded, 1 << pow2_at_least(max(2, 4 * c[0]))]), n
        assert numbers(lines[at], "V") == r["vertices"].reshape(-1).view(np.uint32).tolist(), n
        assert numbers(lines[at + 1], "T") == r["triangles"].reshape(-1).tolist(), n
        assert numbers(lines[at + 2], "S") == r["triangle_shell"].tolist(), n
        for k, kind in enumerate(MT.KINDS):
            assert numbers(lines[at + 3 + k], f"E {k:x}") == r["edges"][kind].reshape(-1).tolist(), (n, kind)
        h = np.array(numbers(lines[at + 7], "H"), np.uint64).reshape(-1, 11)
        s = r["shells"]
        assert h[:, 0].tolist() == s["triangles"].tolist() and h[:, 1].tolist() == s["first"].tolist() and h[:, 2].tolist() == s["unbalanced"].tolist(), n
        assert np.array_equal(h[:, 3:6].astype(np.uint32), s["lo"].view(np.uint32)) and np.array_equal(h[:, 6:9].astype(np.uint32), s["hi"].view(np.uint32)), n
        gamma = lambda k: k * 2.0 ** -53 / (1 - k * 2.0 ** -53)          # noqa: E731  (any order of summation of k terms)
        for col, name in ((9, "volume6"), (10, "area2")):
            got = np.ascontiguousarray(h[:, col]).view(np.float64)
            assert all(abs(g - w) <= gamma(int(k)) * a for g, w, k, a in zip(got, s[name], s["triangles"], s[name + "_abs"])), (n, name)
        assert numbers(lines[at + 8], "F") == r["volume6_terms"].view(np.uint64).tolist(), n          # the terms bit for bit
        assert numbers(lines[at + 9], "A") == r["area2_terms"].view(np.uint64).tolist(), n
        at += 10
    assert at == len(lines)


def host_queries():
    return [query(v, t, weld, log2) for v, t, weld, log2 in host_cases()]


def test_the_host_pipeline_is_the_references():
    check_host(run(_build("mesh_topo_host", ["-O1"]), host_queries()))
    assert sum(1 for case in host_cases() if case[3]) >= 12          # the tables at load factor near 1 were among them


def test_tables_too_small_report_overflow_and_end():
    tets = lattice_tetrahedra(300)
    r = MT.topology(tets)
    exe = _build("mesh_topo_host", ["-O1"])
    assert r["counts"]["vertices"] == 125 and r["counts"]["edges"] > 256
    assert run(exe, [query(tets, None, None, 6), query(*tetrahedron(), None)]) == ["O vertex"]          # 125 keys, 64 slots; the second query is not read
    assert run(exe, [query(tets, None, None, 7)]) == ["O edge"]          # 128 slots hold the vertices; not the edges
    assert run(exe, [query(r["vertices"], r["triangles"], False, pow2_at_least(r["counts"]["edges"]) - 1)]) == ["O edge"]


def test_the_host_pipeline_runs_clean_under_sanitizers():
    """the same program as a stand-alone executable with ASan and UBSan, on the same input: exit 0, nothing on stderr (`run` asserts
    both), the same output"""
    plain = run(_build("mesh_topo_host", ["-O1"]), host_queries())
    san = run(_build("mesh_topo_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), host_queries())
    assert plain == san
    check_host(san)
    assert run(_build("mesh_topo_host_san", []), [query(lattice_tetrahedra(300), None, None, 6)]) == ["O vertex"]


# ---- the interface -----------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fidget_hip.h")).read()
    stated = " ".join(re.sub(r"^ \* ?", "", hdr, flags=re.M).split())          # (the comment's lines without their leading " * ")
    for words in ("equal as floats after x + 0.0f", "in the order of their first corners", "bits unchanged", "boundary: f + r == 1", "flipped: f + r == 2 and f != r",
                  "nonmanifold: f + r >= 3", "unbalanced: f != r", "vertices - edges + (triangles - degenerate)", "its shell 0xFFFFFFFF",
                  "n = (b.y c.z - b.z c.y, b.z c.x - b.x c.z, b.x c.y - b.y c.x)", "(a.x n.x + a.y n.y) + a.z n.z", "sqrt((m.x m.x + m.y m.y) + m.z m.z)",
                  "an order of arrival that may differ from run to run", "3 n_triangles <= 2^32 - 2", "FHIP_ERR_OVERFLOW", "never from the order of the slots"):
        assert words in stated, words          # the definition is in the comment
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    lib = C.CDLL(F.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert hasattr(lib, name) and name in F.EXPORTS and getattr(F.lib(), name).argtypes is not None, name
    assert re.search(r"fhip_triangles_topology\s*\(\s*fhip_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*vertices\s*,\s*uint64_t\s+n_vertices\s*,\s*const\s+uint64_t\s*\*\s*triangles\s*,"
                     r"\s*uint64_t\s+n_triangles\s*,\s*int\s+on_device\s*,\s*int\s+weld\s*,\s*uint32_t\s+table_log2\s*,\s*void\s*\*\*\s*out\s*\)", code)
    assert re.search(r"fhip_mesh_topology\s*\(\s*fhip_ctx\s*\*\s*ctx\s*,\s*const\s+fhip_mesh\s*\*\s*mesh\s*,\s*int\s+weld\s*,\s*uint32_t\s+table_log2\s*,\s*void\s*\*\*\s*out\s*\)", code)
    assert re.search(r"fhip_topology_counts\s*\(\s*const\s+void\s*\*\s*topo\s*,\s*uint64_t\s+out\[16\]\s*\)", code)
    assert re.search(r"fhip_topology_edges\s*\(\s*fhip_ctx\s*\*\s*ctx\s*,\s*const\s+void\s*\*\s*topo\s*,\s*uint32_t\s+kind\s*,\s*uint32_t\s*\*\s*out\s*,\s*int\s+out_on_device\s*\)", code)
    assert callable(F.mesh_topology) and callable(F.Mesh.topology) and F.TOPOLOGY_COUNTS[:10] == MT.COUNTS and F.EDGE_KINDS == MT.KINDS
    for member in ("closed", "manifold", "euler", "volume", "area", "vertices", "triangles", "triangle_shell", "edges", "vertices_device", "triangles_device",
                   "triangle_shell_device"):
        assert hasattr(F.Topology, member), member
    assert "order of arrival" in F.mesh_topology.__doc__ and "order of arrival" in F.Topology.__doc__
    ffi = open(os.path.join(ROOT, "rust", "fidget-hip", "src", "ffi.rs")).read()
    assert all(f"pub fn {name}(" in ffi for name in ENTRY_POINTS)
    assert "fhip_triangles_topology" in open(os.path.join(ROOT, "rust", "fidget-hip", "src", "topology.rs")).read()
    mesh_only = open(os.path.join(ROOT, "tools", "src_hash.py")).read()
    assert all(f'"{name}"' in mesh_only for name in NEW_FILES)          # mesh-only: the render path's hash stays
    assert all(name in F._SOURCES for name in NEW_FILES)
    with pytest.raises(ValueError, match="welded"):
        F.mesh_topology(signed_zeros(), weld=False, hip=object())          # refused before the context is touched
