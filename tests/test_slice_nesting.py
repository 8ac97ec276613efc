"""The nesting of a mesh's slices without a GPU: the reference of slice_nesting_ref.py on the hand-made cases of slice_nesting_cases.py -
against what the cases are built to show, and against exact rational arithmetic; the arithmetic of fidget_amd/csrc/mesh_slice_nest.hpp
built for the host (tests/host_build/slice_nest_host.cpp runs the whole pipeline serially) against the reference, array for array, for
every number of bands; that program under ASan and UBSan; the entry points as the header states them."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np

import fidget_amd as F
import mesh_slices_ref as SR
import slice_nesting_cases as K
import slice_nesting_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "slice_nest_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")
ENTRY_POINTS = ("fhip_slices_nesting", "fhip_slice_nesting_counts", "fhip_slice_nesting_planes", "fhip_slice_nesting_loops", "fhip_slice_nesting_parent_dev",
                "fhip_slice_nesting_depth_dev", "fhip_slice_nesting_free")
NEW_FILES = ("mesh_slice_nest.hpp", "slice_nest.hip", "capi_slice_nest.hpp")
NONE = 0xFFFFFFFF
HAND_MADE = ("chain", "chain, prism 1 reversed", "siblings", "comb", "long comb", "vertex on the row", "flat on the row", "shared edge", "crossing")


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    """-> (triangles float32 [T, 3, 3], planes)"""
    if name.startswith("chain"):
        return K.chain(1 if "reversed" in name else None)
    return {"siblings": K.siblings, "comb": K.comb, "long comb": K.long_comb, "vertex on the row": K.vertex_on_the_row, "flat on the row": K.flat_on_the_row, "shared edge": K.shared_edge,
            "crossing": K.crossing, "field": K.field}[name]()


@functools.lru_cache(maxsize=None)
def sliced(name):
    tri, zs = mesh_of(name)
    return SR.mesh_slices(tri.reshape(-1, 3), None, zs)


@functools.lru_cache(maxsize=None)
def nested(name):
    """the reference's nesting; on the hand-made cases from hit counts that exact arithmetic confirms"""
    res = sliced(name)
    return NR.nesting(res, NR.check_exact(res) if name in HAND_MADE else None)


# ---- 1. the reference on the hand-made cases ---------------------------------------------------------------------------------------------------------
def test_the_chain():
    res, n = sliced("chain"), nested("chain")
    pp = n["per_plane"]
    assert pp["max_depth"].tolist() == K.CHAIN_MAX_DEPTH and pp["regular"].tolist() == [d + 1 for d in K.CHAIN_MAX_DEPTH]
    assert pp["outer"].tolist() == [d // 2 + 1 for d in K.CHAIN_MAX_DEPTH] and pp["top"].tolist() == [1] * 7
    assert n["n_improper"] == 0 and n["n_misoriented"] == 0 and n["max_depth"] == 3
    for l in range(n["n_loops"]):          # a chain: each loop's parent is the one a level up on its plane
        same_plane = [m for m in range(n["n_loops"]) if res["loops"]["plane"][m] == res["loops"]["plane"][l]]
        up = [m for m in same_plane if n["depth"][m] + 1 == n["depth"][l]]
        assert (n["parent"][l] == NONE and not up) or [int(n["parent"][l])] == up
    assert sorted(n["region_area2"][n["depth"] == 0].tolist()) == [8 * (0.75 ** 2 - 0.5 ** 2)] * 5 + [8 * 0.75 ** 2] * 2
    turned = nested("chain, prism 1 reversed")
    assert turned["per_plane"]["misoriented"].tolist() == [0, 1, 1, 1, 1, 1, 0] and turned["n_misoriented"] == 5          # the planes that cut prism 1
    assert all(np.array_equal(turned[k], n[k]) for k in ("parent", "depth", "n_children"))


def test_siblings_parity_is_not_any_hit():
    n = nested("siblings")
    assert n["hit_counts"][0] == {1: 2, 2: 1, 3: 1}          # the right island's leader: the left island twice, the outer boundary and the hole once
    assert n["parent"].tolist() == [3, 3, NONE, 2] and n["depth"].tolist() == [2, 2, 0, 1] and n["n_children"].tolist() == [0, 0, 1, 2]
    assert NR.regions(sliced("siblings"), n, 0) == [(0, []), (1, []), (2, [3])]


def test_the_comb_long_hit_lists():
    for name, teeth in (("comb", K.COMB_TEETH), ("long comb", K.LONG_COMB_TEETH)):
        n = nested(name)
        assert [n["hit_counts"][l][6] for l in range(5)] == K.comb_multiplicities(teeth) == [2, 4, 2 * teeth, 1, 3]
        assert [n["hit_counts"][l][5] for l in range(5)] == [2] * 5          # the C's back, twice: the mouth is outside
        assert n["depth"].tolist()[:5] == [0, 0, 0, 1, 1] and n["parent"].tolist()[3:5] == [6, 6]
    assert 2 * K.COMB_TEETH == 80 and 2 * K.LONG_COMB_TEETH + 2 > 512          # the second: longer than the list a wave keeps in LDS


def test_a_vertex_on_the_row_counts_once():
    res, n = sliced("vertex on the row"), nested("vertex on the row")
    assert K.leader_at(res, K.ROW_Q)
    want = [w for _, _, _, w in K.ROW_DIAMONDS]
    assert [n["hit_counts"][0][m] for m in range(1, 8)] == want == [2, 0, 1, 0, 0, 2, 0]          # 0 or 2 outside, 1 inside
    assert n["parent"][0] == 3 and n["depth"][0] == 1


def test_horizontal_and_zero_length_segments_on_the_row():
    res, n = sliced("flat on the row"), nested("flat on the row")
    xy, L = res["xy"], res["loops"]
    top = np.flatnonzero(res["plane"] == 1)
    assert len(np.unique(xy[top], axis=0)) < len(top)          # several crossings share a position
    assert K.leader_at(res, (0.0, 0.0))
    on_row = [v for v in range(len(xy)) if xy[v, 1] == 0.0 and xy[int(res["next"][v]), 1] == 0.0 and res["loop_of"][v] != 0]
    assert len(on_row) >= 4          # horizontal segments of other loops on the leader's row
    for p in (0, 1):          # only the square around the leader contains it, on both planes
        first, around = [l for l in range(len(L["leader"])) if L["plane"][l] == p][0], [l for l in range(len(L["leader"])) if L["plane"][l] == p][3]
        assert n["contains"][first] == {around}


def test_irregular_loops_take_no_part():
    res, n = sliced("shared edge"), nested("shared edge")
    irregular = np.flatnonzero(res["loops"]["irregular"] > 0)
    assert len(irregular) == 2 and (n["parent"][irregular] == NONE).all() and (n["depth"][irregular] == NONE).all() and (n["n_children"][irregular] == 0).all()
    assert not any(int(i) in c for c in n["contains"].values() for i in irregular)
    assert n["per_plane"]["regular"].tolist() == [5, 5] and n["per_plane"]["max_depth"].tolist() == [3, 3]
    assert n["depth"][-2:].tolist() == [2, 2]          # the square inside the first cube: inside the hole, as if the cubes were absent


def test_crossing_loops_are_improper():
    n = nested("crossing")
    assert n["depth"].tolist() == [0, 0, 2] and n["parent"].tolist() == [NONE, NONE, 0] and n["n_improper"] == 1          # the smaller id among equals


# ---- 2. the library's arithmetic, built for the host -------------------------------------------------------------------------------------------------
def _build(name, flags):
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("mesh_slice_nest.hpp", "mesh_slice.hpp", "mesh_topo.hpp", "mesh_vox.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe])      # (plain g++: the header touches no device)
    return exe


def query(res, bands=0):
    L = res["loops"]
    hexes = lambda a: " ".join(f"{int(x):x}" for x in np.asarray(a).reshape(-1))          # noqa: E731
    f32 = lambda a: hexes(np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))          # noqa: E731
    n, nl = len(res["plane"]), len(L["leader"])
    words = [f"Q {bands:x} {n:x}", f32(res["xy"]), hexes(res["plane"]), hexes(res["next"]), hexes(res["loop_of"]), f"{nl:x}", hexes(L["leader"]), hexes(L["plane"]),
             hexes(L["crossings"]), hexes(L["irregular"]), hexes(np.ascontiguousarray(L["area2"], np.float64).view(np.uint64)), f32(L["lo"]), f32(L["hi"]),
             f"{res['counts']['planes']:x}"]
    return " ".join(w for w in words if w)


def run(exe, queries, tmp_path):
    """-> per query the program's lines as {tag: uint64 array}"""
    path = os.path.join(str(tmp_path), "cases.txt")
    with open(path, "w") as f:
        f.write("".join(q + "\n" for q in queries))
    res = subprocess.run([exe, path], capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stdout[-300:], res.stderr[-2000:])
    out = []
    for line in res.stdout.splitlines():
        tag, *words = line.split()
        if tag in "OC":
            out.append({})
        out[-1][tag] = np.array([int(x, 16) for x in words], np.uint64)
    assert len(out) == len(queries)
    return out


@functools.lru_cache(maxsize=None)
def host_cases():
    """(name, bands): every hand-made case under the host's rule and under one band; the field under every number of bands; no planes;
    planes that miss the mesh"""
    return tuple([(name, b) for name in HAND_MADE for b in (0, 1, 5)] + [("field", b) for b in K.BANDS] + [("no planes", 0), ("missed", 0)])


@functools.lru_cache(maxsize=None)
def slices_of(name):
    if name == "no planes":
        return SR.mesh_slices(K.chain()[0].reshape(-1, 3), None, np.zeros(0, np.float32))
    if name == "missed":
        return SR.mesh_slices(K.chain()[0].reshape(-1, 3), None, np.array([-2.0, 1.5], np.float32))
    return sliced(name)


def compare(got, res, want, name):
    """the host program's (or, as arrays of the same names, the device's) results against the reference's nesting `want`"""
    P, n = res["counts"]["planes"], want["n_loops"]
    totals = [n] + [want[k] for k in ("n_regular", "n_outer", "n_top", "max_depth", "n_improper", "n_misoriented")] + [P]
    assert got["C"][:8].tolist() == totals, (name, got["C"], totals)
    for tag, key in (("A", "parent"), ("D", "depth"), ("N", "n_children")):
        assert np.array_equal(got[tag], want[key].astype(np.uint64)), (name, key)
    assert np.array_equal(got["R"].copy().view(np.float64), want["region_area2"]), name          # (the same area2 in, the same order of addition: the same bits)
    K7 = got["K"].reshape(P, 7)
    for col, key in enumerate(NR.PLANE_COUNTS):
        assert np.array_equal(K7[:, col], want["per_plane"][key]), (name, key)
    return K7[:, 6]


def test_the_host_build_is_the_references(tmp_path):
    cases = host_cases()
    results = run(_build("slice_nest_host", ["-O1"]), [query(slices_of(name), b) for name, b in cases], tmp_path)
    for got, (name, b) in zip(results, cases):
        res = slices_of(name)
        bands = compare(got, res, NR.nesting(res) if name in ("no planes", "missed") else nested(name), f"{name}, bands {b}")
        if b:
            assert (bands == (b if got["C"][1] else 0)).all(), (name, b)
    by = {c: r for c, r in zip(cases, results)}
    # the host's rule: a band per 32 regular segments; nothing above 4 entries per segment; more bands than segments were asked for and used
    field = by[("field", 0)]
    regular_segments = int(sum(c for c, i in zip(sliced("field")["loops"]["crossings"], sliced("field")["loops"]["irregular"]) if i == 0))
    assert 0 < int(field["C"][9]) <= 4 * regular_segments and int(field["C"][8]) > 6
    assert int(by[("field", 4096)]["C"][8]) == 6 * 4096 > regular_segments
    assert int(by[("no planes", 0)]["C"][8]) == 0 and int(by[("missed", 0)]["C"][7]) == 2


def test_the_host_build_runs_clean_under_sanitizers(tmp_path):
    """the same program as a stand-alone executable with ASan and UBSan, on the same input: exit 0, nothing on stderr (`run` asserts
    both), the same output"""
    queries = [query(slices_of(name), b) for name, b in host_cases()]
    plain = run(_build("slice_nest_host", ["-O1"]), queries, tmp_path)
    san = run(_build("slice_nest_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), queries, tmp_path)
    for a, b in zip(plain, san):
        assert sorted(a) == sorted(b) and all(np.array_equal(a[tag], b[tag]) for tag in a)


# ---- 3. the interface ----------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fidget_hip.h")).read()
    stated = " ".join(re.sub(r"^ \* ?", "", hdr, flags=re.M).split())          # (the comment's lines without their leading " * ")
    for words in ("(s.y <= q.y) != (d.y <= q.y)", "c = (d.x - s.x) * (q.y - s.y) - (q.x - s.x) * (d.y - s.y)", "c == 0 is not a hit", "This binary64 sequence IS the definition",
                  "may fall either side, but always the same side", "m contains l iff the number of hit segments of m is odd", "the smallest id among equals",
                  "(depth even) != (area2 > 0)", "added in ascending child id", "monotone non-decreasing in y", "every plane's number is halved",
                  "2^32 - 1 bands, band entries or hits or more is FHIP_ERR_OVERFLOW", "irregular loops alone give FHIP_OK"):
        assert words in stated, words          # the definitions are in the comment
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    lib = C.CDLL(F.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in F.EXPORTS and getattr(F.lib(), name).argtypes is not None, name
    assert re.search(r"fhip_slices_nesting\s*\(\s*fhip_ctx\s*\*\s*ctx\s*,\s*const\s+void\s*\*\s*slices\s*,\s*uint32_t\s+bands\s*,\s*void\s*\*\*\s*out\s*\)", hdr)
    assert callable(F.MeshSlices.nesting) and F.SliceNesting.NONE == NONE
    assert all(callable(getattr(F.SliceNesting, m)) for m in ("children", "regions", "polygons", "svg", "parent_device", "depth_device"))
    assert all(isinstance(getattr(F.SliceNesting, m), property) for m in ("parent", "depth", "n_children", "region_area2", "regular", "outer", "top", "improper", "misoriented"))
    ffi = open(os.path.join(ROOT, "rust", "fidget-hip", "src", "ffi.rs")).read()
    assert all(f"pub fn {name}(" in ffi for name in ENTRY_POINTS)
    mesh_only = open(os.path.join(ROOT, "tools", "src_hash.py")).read()
    assert all(f'"{name}"' in mesh_only for name in NEW_FILES)          # mesh-only: the render path's hash stays
    assert all(name in F._SOURCES for name in NEW_FILES)
    mesh_hip = open(os.path.join(CSRC, "mesh.hip")).read()
    assert mesh_hip.index('#include "slice.hip"') < mesh_hip.index('#include "slice_nest.hip"')
