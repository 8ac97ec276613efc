"""The slices of a triangle mesh without a GPU: the reference of mesh_slices_ref.py against invariants - the area of every cross-section
of a voxel mesh against the bitmap's layer counts, exactly; out == in at every crossing of a closed mesh - the issue's known numbers and
hand-made cases; the arithmetic of fidget_amd/csrc/mesh_slice.hpp built for the host (tests/host_build/mesh_slice_host.cpp runs the
whole pipeline with fhtopo::Serial) against the reference, array for array and the positions by their bits; that program under ASan and
UBSan; the entry points as the header states them."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np

import fidget_amd as F
import mesh_slices_ref as SR
import voxel_mesh_ref as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "mesh_slice_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")
ENTRY_POINTS = ("fhip_topology_slices", "fhip_slices_counts", "fhip_slices_planes", "fhip_slices_loops", "fhip_slices_vertices", "fhip_slices_xy_dev", "fhip_slices_next_dev",
                "fhip_slices_loop_dev", "fhip_slices_plane_dev", "fhip_slices_free")
NEW_FILES = ("mesh_slice.hpp", "slice.hip", "capi_slice.hpp")
NONE = 0xFFFFFFFF


def centre_planes(N):
    return ((2 * np.arange(N) + 1 - N) / N).astype(np.float32)


def corner_planes(N):
    return ((2 * np.arange(N + 1) - N) / N).astype(np.float32)


@functools.lru_cache(maxsize=None)
def bitmap(name):
    if name == "random 8":
        return np.random.default_rng(0).random((8, 8, 8)) < 0.3
    if name == "random 16":
        return np.random.default_rng(0).random((16, 16, 16)) < 0.5
    if name == "ball":
        i, j, k = np.meshgrid(*[np.arange(16)] * 3, indexing="ij")
        return (i - 7.5) ** 2 + (j - 7.5) ** 2 + (k - 7.5) ** 2 < 36
    assert name == "cube"
    g = np.zeros((4, 4, 4), bool)
    g[1, 2, 1] = True          # x in [-0.5, 0], y in [0, 0.5], z in [-0.5, 0]
    return g


@functools.lru_cache(maxsize=None)
def voxel_mesh(name):
    v, t = VM.mesh(bitmap(name))
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.uint64)


@functools.lru_cache(maxsize=None)
def sliced(name, planes):
    """the reference's slices of a bitmap's mesh: planes "centre", "corner", or a tuple of floats"""
    N = bitmap(name).shape[0]
    zs = centre_planes(N) if planes == "centre" else corner_planes(N) if planes == "corner" else np.array(planes, np.float32)
    return SR.mesh_slices(*voxel_mesh(name), zs)


def cube_planes(n):
    """n planes from the cube's bottom face to its top face, both among them"""
    return tuple(np.linspace(-0.5, 0.0, n).astype(np.float32).tolist())


# ---- 1. the reference's invariants -----------------------------------------------------------------------------------------------------------
def test_cross_sections_of_a_voxel_mesh_have_the_layers_areas():
    for name in ("random 8", "random 16"):
        g = bitmap(name)
        N = g.shape[0]
        want = g.sum(axis=(0, 1)).astype(np.float64)
        at_centres = sliced(name, "centre")
        assert np.array_equal(SR.plane_area2(at_centres) / 2 * (N / 2) ** 2, want), name
        at_corners = sliced(name, "corner")          # a solid spanning [z0, z1] is cut by the planes in (z0, z1]
        area = SR.plane_area2(at_corners) / 2 * (N / 2) ** 2
        assert at_corners["per_plane"]["crossings"][0] == 0 and area[0] == 0 and np.array_equal(area[1:], want), name
        for res in (at_centres, at_corners):
            assert np.array_equal(res["out"], res["in"]), name          # a closed mesh
            L, pp = res["loops"], res["per_plane"]
            assert np.array_equal(L["leader"], np.sort(L["leader"])) and int(L["crossings"].sum()) == res["counts"]["vertices"]
            assert int(pp["crossings"].sum()) == res["counts"]["vertices"] and int(pp["segments"].sum()) == res["counts"]["segments"]
            assert int(pp["loops"].sum()) == res["counts"]["loops"] and int(L["irregular"].sum()) == res["counts"]["irregular"]
            assert np.array_equal(res["plane"][res["segments"][:, 0]], res["plane"][res["segments"][:, 1]])          # a segment stays in its plane
            assert (res["edge"][:, 0] < res["edge"][:, 1]).all()


# ---- 2. the issue's numbers ----------------------------------------------------------------------------------------------------------------
def test_the_issues_numbers():
    assert len(voxel_mesh("random 8")[1]) == 1252
    assert sliced("random 8", "centre")["counts"] == {"planes": 8, "vertices": 798, "segments": 816, "loops": 54, "irregular": 18}
    assert len(voxel_mesh("ball")[1]) == 1344
    ball = sliced("ball", "centre")
    assert ball["counts"] == {"planes": 16, "vertices": 896, "segments": 896, "loops": 12, "irregular": 0}
    assert np.array_equal(np.sort(ball["next"]), np.arange(896))


# ---- 3. hand-made cases ----------------------------------------------------------------------------------------------------------------------
def test_the_one_voxel_cube():
    res = sliced("cube", cube_planes(3))          # through the bottom face, the middle, the top face
    assert res["per_plane"]["crossings"].tolist() == [0, 8, 8] and res["per_plane"]["loops"].tolist() == [0, 1, 1]          # each face's diagonal crosses as well
    assert res["loops"]["area2"].tolist() == [0.5, 0.5] and res["loops"]["irregular"].tolist() == [0, 0]
    assert res["loops"]["lo"].tolist() == [[-0.5, 0.0]] * 2 and res["loops"]["hi"].tolist() == [[0.0, 0.5]] * 2
    (middle,), skipped = SR.polygons(res, 1)
    assert skipped == 0 and len(middle) == 8 and len(np.unique(middle, axis=0)) == 8
    (top,), _ = SR.polygons(res, 2)          # the top face's own corners: a vertex of the mesh under each crossing
    v = voxel_mesh("cube")[0]
    corners = {tuple(p[:2]) for p in v.tolist() if p[2] == 0.0}
    assert len(corners) == 4 and {tuple(p) for p in top.tolist()} == corners
    assert SR.polygons(res, 0) == ([], 0)


def test_the_cube_with_a_triangle_removed():
    v, t = voxel_mesh("cube")
    sides = [k for k in range(len(t)) if len({float(v[int(i), 2]) for i in t[k]}) == 2]          # a triangle that the middle plane cuts
    res = SR.mesh_slices(v, np.delete(t, sides[0], axis=0), np.array([-0.25], np.float32))
    assert res["counts"] == {"planes": 1, "vertices": 8, "segments": 7, "loops": 1, "irregular": 2}
    assert (res["next"] == NONE).sum() == 1 and sorted(res["degree"].tolist()) == [0x01, 0x10] + [0x11] * 6
    assert SR.polygons(res, 0) == ([], 1)


def test_a_degenerate_triangle_is_skipped():
    v, t = voxel_mesh("cube")
    zs = np.array([-0.25], np.float32)
    lower, upper = int(np.flatnonzero(v[:, 2] == -0.5)[0]), int(np.flatnonzero(v[:, 2] == 0.0)[0])
    more = np.concatenate([t, np.array([[lower, upper, upper]], np.uint64)])          # two equal ids, and an edge that would cross
    a, b = SR.mesh_slices(v, t, zs), SR.mesh_slices(v, more, zs)
    assert a["counts"] == b["counts"] and all(np.array_equal(a[k], b[k]) for k in ("xy", "edge", "next", "loop_of", "degree"))
    only = SR.mesh_slices(v, more[-1:], zs)
    assert only["counts"] == {"planes": 1, "vertices": 0, "segments": 0, "loops": 0, "irregular": 0}


def test_planes_that_are_not_ascending_are_refused():
    assert SR.planes_ok([]) and SR.planes_ok([0.0]) and SR.planes_ok([-1.0, -0.5, 3.0])
    assert not SR.planes_ok([0.0, 0.0]) and not SR.planes_ok([1.0, 0.0]) and not SR.planes_ok([0.0, np.nan]) and not SR.planes_ok([0.0, np.inf]) and not SR.planes_ok([-0.0, 0.0])


# ---- 4, 5. the library's arithmetic, built for the host ------------------------------------------------------------------------------------------
def _build(name, flags):
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("mesh_slice.hpp", "mesh_topo.hpp", "mesh_vox.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe])      # (plain g++: the header touches no device)
    return exe


def query(vertices, triangles, zs, table_log2=0):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1).view(np.uint32)
    t = np.asarray(triangles, np.uint64).reshape(-1)
    z = np.ascontiguousarray(zs, np.float32).reshape(-1).view(np.uint32)
    hexes = lambda a: " ".join(f"{int(x):x}" for x in a)          # noqa: E731
    return f"Q {table_log2:x} {len(v) // 3:x} {hexes(v)} {len(t) // 3:x} {hexes(t)} {len(z):x} {hexes(z)}".replace("  ", " ")


def run(exe, queries):
    """-> per query the program's lines as {tag: uint64 array}"""
    res = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stdout[-300:], res.stderr[-2000:])
    out = []
    for line in res.stdout.splitlines():
        tag, *words = line.split()
        if tag in "UOC":
            out.append({})
        out[-1][tag] = np.array([int(x, 16) for x in words], np.uint64)
    assert len(out) == len(queries)
    return out


@functools.lru_cache(maxsize=None)
def host_cases():
    """(name, vertices, triangles, zs): the bitmaps' meshes at the centres and at the corners, the cube under 300 planes - more
    crossings on one edge than a workgroup has lanes - open, with a degenerate triangle, under no plane, under planes that miss it"""
    cases = [(f"{name}, {planes}", *voxel_mesh(name), sliced(name, planes)["zs"]) for name in ("random 8", "ball") for planes in ("centre", "corner")]
    v, t = voxel_mesh("cube")
    cases.append(("cube, 300 planes", v, t, np.array(cube_planes(300), np.float32)))
    cases.append(("cube, open", v, t[1:], np.array(cube_planes(7), np.float32)))
    cases.append(("cube, a degenerate triangle", v, np.concatenate([t, np.array([[0, 7, 7]], np.uint64)]), np.array(cube_planes(5), np.float32)))
    cases.append(("cube, no plane", v, t, np.zeros(0, np.float32)))
    cases.append(("cube, missed", v, t, np.array([-2.0, 0.5, 1.0], np.float32)))
    cases.append(("nothing", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint64), np.array([0.0], np.float32)))
    return cases


def compare(got, want, name):
    c = want["counts"]
    assert got["C"][:5].tolist() == [c[k] for k in SR.COUNTS], name
    n, L = c["vertices"], c["loops"]
    assert np.array_equal(got["X"].astype(np.uint32), want["xy"].reshape(-1).view(np.uint32)), name          # by bits
    for tag, key in (("P", "plane"), ("E", "edge"), ("N", "next"), ("L", "loop_of"), ("D", "degree"), ("G", "segments")):
        assert np.array_equal(got[tag], want[key].reshape(-1).astype(np.uint64)), (name, key)
    H, W = got["H"].reshape(L, 10), want["loops"]
    for col, key in enumerate(("leader", "plane", "crossings", "segments", "irregular")):
        assert np.array_equal(H[:, col], W[key].astype(np.uint64)), (name, key)
    area2 = H[:, 5].copy().view(np.float64)
    assert np.all(np.abs(area2 - W["area2"]) <= W["segments"] * 2.0 ** -52 * W["area2_abs"]), name
    assert np.array_equal(H[:, 6:8].astype(np.uint32), W["lo"].view(np.uint32)) and np.array_equal(H[:, 8:10].astype(np.uint32), W["hi"].view(np.uint32)), name
    pp = want["per_plane"]
    assert np.array_equal(got["K"].reshape(-1, 3), np.stack([pp["crossings"], pp["segments"], pp["loops"]], axis=1)), name
    assert len(got["X"]) == 2 * n


def test_the_host_build_is_the_references():
    cases = host_cases()
    results = run(_build("mesh_slice_host", ["-O1"]), [query(v, t, zs) for _, v, t, zs in cases])
    for got, (name, v, t, zs) in zip(results, cases):
        compare(got, SR.mesh_slices(v, t, zs), name)
    v, t = voxel_mesh("cube")
    bad = run(_build("mesh_slice_host", ["-O1"]), [query(v, t, [0.0, 0.0]), query(v, t, [np.nan]), query(v, t, [-0.25], table_log2=1),
                                                     query(v, t, [-0.25], table_log2=5)])
    assert [sorted(r) for r in bad[:3]] == [["U"], ["U"], ["O"]] and bad[3]["C"].tolist() == [1, 8, 8, 1, 0, 32]


def test_the_host_build_runs_clean_under_sanitizers():
    """the same program as a stand-alone executable with ASan and UBSan, on the same input: exit 0, nothing on stderr (`run` asserts
    both), the same output"""
    queries = [query(v, t, zs) for _, v, t, zs in host_cases()]
    plain = run(_build("mesh_slice_host", ["-O1"]), queries)
    san = run(_build("mesh_slice_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), queries)
    for a, b in zip(plain, san):
        assert sorted(a) == sorted(b) and all(np.array_equal(a[tag], b[tag]) for tag in a)


# ---- 6. the interface --------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fidget_hip.h")).read()
    stated = " ".join(re.sub(r"^ \* ?", "", hdr, flags=re.M).split())          # (the comment's lines without their leading " * ")
    for words in ("Vertex v is above plane p iff z_v >= zs[p]", "min(a_u, a_v) <= p < max(a_u, a_v)", "cut by the planes in (z0, z1]",
                  "in the order of their first corners", "2^32 - 1 crossings or more is FHIP_ERR_OVERFLOW", "t = (zs[p] - z_u) / (z_v - z_u)",
                  "from the crossing on edge A -> B to the crossing on edge C -> A", "irregular iff out != 1 or in != 1", "in the triangle with the smallest index",
                  "A loop's leader is its smallest crossing id", "finite and strictly ascending", "n_planes == 0 is FHIP_OK", "out | in << 4"):
        assert words in stated, words          # the definitions are in the comment
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    lib = C.CDLL(F.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in F.EXPORTS and getattr(F.lib(), name).argtypes is not None, name
    assert re.search(r"fhip_topology_slices\s*\(\s*fhip_ctx\s*\*\s*ctx\s*,\s*const\s+void\s*\*\s*topology\s*,\s*const\s+float\s*\*\s*zs\s*,\s*uint32_t\s+n_planes\s*,"
                     r"\s*uint32_t\s+table_log2\s*,\s*void\s*\*\*\s*out\s*\)", hdr)
    assert callable(F.mesh_slices) and callable(F.Topology.slices) and callable(F.Mesh.slices)
    assert all(callable(getattr(F.MeshSlices, m)) for m in ("loops_of", "polygons", "svg", "xy_device", "next_device", "loop_of_device", "plane_device"))
    assert all(isinstance(getattr(F.MeshSlices, m), property) for m in ("xy", "plane", "edge", "next", "loop_of", "degree", "loops"))
    ffi = open(os.path.join(ROOT, "rust", "fidget-hip", "src", "ffi.rs")).read()
    assert all(f"pub fn {name}(" in ffi for name in ENTRY_POINTS)
    mesh_only = open(os.path.join(ROOT, "tools", "src_hash.py")).read()
    assert all(f'"{name}"' in mesh_only for name in NEW_FILES)          # mesh-only: the render path's hash stays
    assert all(name in F._SOURCES for name in NEW_FILES)
