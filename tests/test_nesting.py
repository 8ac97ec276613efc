"""The nesting of a voxel bitmap's outlines without a GPU: the reference of nesting_ref.py - parents by the parity of the edges crossed,
no chain followed - against every fact the header states (the leader's edge and pixels, left in the same layer and before the loop,
the parent as the first loop of the other sign along the left chain, depths even exactly for outer boundaries, region sums against
flood-filled component sizes) on random images, rings, plates with holes and holes with islands; the arithmetic of
fidget_amd/csrc/mesh_nest.hpp built for the host (tests/host_build/mesh_nest_host.cpp) against the reference, loop for loop; that
program under ASan and UBSan; fhip_nesting_children, which is host code, against a stable argsort; the entry points as the header
states them."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np

import fidget_amd as F
import nesting_ref as NR
import outlines_ref as OR
import voxels_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "mesh_nest_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")
ENTRY_POINTS = ("fhip_outlines_nesting", "fhip_nesting_counts", "fhip_nesting_layers", "fhip_nesting_loops", "fhip_nesting_parent_dev", "fhip_nesting_depth_dev",
                "fhip_nesting_children", "fhip_nesting_free")
NEW_FILES = ("mesh_nest.hpp", "nest.hip", "capi_nest.hpp")


# ---- images ------------------------------------------------------------------------------------------------------------------------------
def rings(N, count, w):
    """`count` concentric square rings, each w pixels wide with w clear pixels between them: loop depths 0 .. 2 count - 1"""
    P = np.zeros((N, N), bool)
    for r in range(count):
        o = 2 * w * r
        P[o:N - o, o:N - o] = True
        P[o + w:N - o - w, o + w:N - o - w] = False
    return P


def plate_with_holes(N, holes):
    """a plate with `holes` one-pixel holes on one pixel row: the last hole's chain of left links passes all the others"""
    P = np.zeros((N, N), bool)
    P[2:N - 2, 2:N - 2] = True
    P[4:4 + 3 * holes:3, N // 2 - 2] = False
    return P


def hole_with_islands(N, islands):
    """a plate with one hole that holds `islands` one-pixel islands on one pixel row"""
    P = np.zeros((N, N), bool)
    P[1:N - 1, 1:N - 1] = True
    P[3:N - 3, N // 4:N // 2 + 4] = False
    P[5:5 + 3 * islands:3, N // 4 + 6] = True
    return P


def far_hole(N):
    """a block that starts at a = 2 with a hole at a >= 50: from the hole's leader the row scan crosses a word and a chunk"""
    P = np.zeros((N, N), bool)
    P[2:60, 5:25] = True
    P[50:53, 10:13] = False
    return P


def checkerboard(N):
    i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    return (i + j) % 2 == 0


@functools.lru_cache(maxsize=None)
def images():
    rng = np.random.default_rng(191)
    out = [(f"random {N} {d}", rng.random((N, N)) < d) for N in (8, 16, 32) for d in (0.3, 0.5, 0.7, 0.9)]
    out += [("seven rings", rings(32, 7, 1)), ("plate with 15 holes", plate_with_holes(64, 15)), ("hole with 16 islands", hole_with_islands(64, 16)),
            ("far hole", far_hole(64)), ("checkerboard", checkerboard(16)), ("full", np.ones((8, 8), bool)), ("empty", np.zeros((8, 8), bool))]
    return out


# ---- the reference against the facts -----------------------------------------------------------------------------------------------------
def facts(P, conn, name):
    """every fact of the header's block on the layer image P; -> (the outlines, the nesting) of the reference"""
    N = P.shape[0]
    L = OR.layer(P, conn)
    T = NR.layer(L)
    n = len(L["leader"])
    Q = np.zeros((N + 2, N + 2), bool)          # Q[i + 1, j + 1] = P(i, j), clear outside
    Q[1:-1, 1:-1] = P
    owner = {(a, b): e for e, es in enumerate(NR.vertical_edges(L)) for b, a in es}
    assert (L["area2"] != 0).all(), name
    for l in range(n):
        a0, b0 = (int(x) for x in L["xy"][L["leader"][l]])
        assert owner[(a0, b0)] == l, (name, conn, l)          # the edge (a0, b0)-(a0, b0 + 1) is the loop's own
        if L["area2"][l] > 0:
            assert Q[a0 + 1, b0 + 1], (name, conn, l)
        else:
            assert not Q[a0 + 1, b0 + 1] and Q[a0, b0 + 1], (name, conn, l)
        # left by the header's first definition: the largest a < a0 where the row changes
        want = -1
        for a in range(a0 - 1, -1, -1):
            if Q[a, b0 + 1] != Q[a + 1, b0 + 1]:
                want = owner[(a, b0)]
                break
        assert T["left"][l] == want and want < l, (name, conn, l)
        # the parent as the first loop of the other sign along the chain
        e = want
        while e >= 0 and (L["area2"][e] < 0) == (L["area2"][l] < 0):
            e = int(T["left"][e])
        assert T["parent"][l] == e and e < l, (name, conn, l)
        if e >= 0:
            assert (L["area2"][e] < 0) != (L["area2"][l] < 0) and T["depth"][l] == T["depth"][e] + 1, (name, conn, l)
        else:
            assert L["area2"][l] > 0 and T["depth"][l] == 0, (name, conn, l)
    assert np.array_equal(T["depth"] % 2 == 0, L["area2"] > 0), name
    assert int(T["n_children"].sum()) == n - T["top"] and int(T["region_area2"][L["area2"] > 0].sum()) == 2 * int(P.sum()), name
    fg, bg = NR.region_sizes(P, conn)
    assert np.array_equal(np.sort(T["region_area2"][L["area2"] > 0] // 2), fg), (name, conn)
    assert np.array_equal(np.sort(-T["region_area2"][L["area2"] < 0] // 2), bg), (name, conn)
    return L, T


def test_the_reference_holds_the_facts():
    loops = deepest = 0
    for name, P in images():
        for conn in (4, 8):
            L, T = facts(P, conn, name)
            loops += len(L["leader"])
            deepest = max(deepest, T["max_depth"])
    print(f"{loops} loops, nesting up to depth {deepest}")
    assert loops > 1000 and deepest == 13


def test_the_hand_made_cases():
    ring = np.zeros((8, 8), bool)
    ring[1:7, 1:7] = True
    ring[2:6, 2:6] = False
    ring[3, 3] = True          # an island in the hole
    T = NR.layer(OR.layer(ring, 4))
    assert T["left"].tolist() == [-1, 0, 1] and T["parent"].tolist() == [-1, 0, 1] and T["depth"].tolist() == [0, 1, 2]
    assert T["n_children"].tolist() == [1, 1, 0] and T["region_area2"].tolist() == [2 * 20, -2 * 15, 2] and (T["outer"], T["top"], T["max_depth"]) == (2, 1, 2)
    T = NR.layer(OR.layer(plate_with_holes(64, 15), 4))
    assert T["left"].tolist() == [-1] + list(range(15)) and T["parent"].tolist() == [-1] + [0] * 15 and T["n_children"][0] == 15          # the sibling chain
    T = NR.layer(OR.layer(hole_with_islands(64, 16), 8))
    assert T["parent"].tolist() == [-1, 0] + [1] * 16 and T["depth"].tolist() == [0, 1] + [2] * 16
    two = np.zeros((4, 4), bool)
    two[1, 1] = two[2, 2] = True          # a saddle: two loops with 4, one with 8, no nesting either way
    assert NR.layer(OR.layer(two, 4))["parent"].tolist() == [-1, -1] and NR.layer(OR.layer(two, 8))["parent"].tolist() == [-1]
    assert NR.layer(OR.layer(checkerboard(16), 4))["top"] == 128


def test_children_of_the_reference():
    start, kids = NR.children(np.array([NR.NONE, 0, 1, 0, NR.NONE, 4, 0], np.uint32))
    assert start.tolist() == [0, 3, 4, 4, 4, 5, 5, 5] and kids.tolist() == [1, 3, 6, 2, 5]


# ---- the library's arithmetic, built for the host --------------------------------------------------------------------------------------------
def _build(name, flags):
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("mesh_nest.hpp", "mesh_outline.hpp", "mesh_vox.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe])      # (plain g++: the headers touch no device)
    return exe


def run(exe, grids):
    """-> per (grid, connectivity) the program's lines as {tag: uint32 array}"""
    queries = []
    for g, conn in grids:
        w = V.pack(g)
        queries.append(f"G {w.shape[0].bit_length() - 1} {conn} " + " ".join(f"{int(x):x}" for x in w.reshape(-1)))
    res = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stdout[-300:], res.stderr[-2000:])
    lines = res.stdout.splitlines()
    assert len(lines) == 4 * len(grids), lines[-1][:200]
    out = []
    for q in range(len(grids)):
        assert [line[0] for line in lines[4 * q:4 * q + 4]] == ["S", "L", "P", "D"]
        out.append({line[0]: np.array([int(x, 16) for x in line.split()[1:]], np.uint32) for line in lines[4 * q:4 * q + 4]})
    return out


def in_layers(images, N):
    """the images [i, j] as the first layers of an otherwise empty grid"""
    g = np.zeros((N, N, N), bool)
    for k, P in enumerate(images):
        g[:P.shape[0], :P.shape[1], k] = P
    return g


@functools.lru_cache(maxsize=None)
def sample_grids():
    """depth 0 .. 2: empty, full, random at several densities; depth 3: rings; depth 4 (three chunks of 32 corners to a row, rows of
    two words): rings across corner 32, the sibling chains, the far hole, a checkerboard, random layers, the last layer"""
    rng = np.random.default_rng(192)
    grids = []
    for N in (4, 8, 16):
        grids += [np.zeros((N, N, N), bool), np.ones((N, N, N), bool)] + [rng.random((N, N, N)) < d for d in (0.3, 0.5, 0.8)]
    grids.append(in_layers([rings(32, 7, 1), rings(32, 3, 2), rng.random((32, 32)) < 0.6], 32))
    g = in_layers([rings(64, 7, 2), plate_with_holes(64, 15), hole_with_islands(64, 16), far_hole(64), checkerboard(64), rng.random((64, 64)) < 0.5,
                   np.zeros((64, 64), bool), rng.random((64, 64)) < 0.7], 64)
    g[:, :, 63] = rng.random((64, 64)) < 0.6
    grids.append(g)
    return [(g, conn) for g in grids for conn in (4, 8)]


@functools.lru_cache(maxsize=None)
def references():
    out = []
    for g, conn in sample_grids():
        S = OR.stack(g, 0, g.shape[0], conn)
        out.append((S, NR.stack(S)))
    return out


def test_the_arithmetic_is_the_references():
    grids = sample_grids()
    for got, (S, T) in zip(run(_build("mesh_nest_host", ["-O1"]), grids), references()):
        assert np.array_equal(got["S"], S["loop_start"].astype(np.uint32))
        assert np.array_equal(got["L"], T["left"]) and np.array_equal(got["P"], T["parent"]) and np.array_equal(got["D"], T["depth"])


def test_the_arithmetic_runs_clean_under_sanitizers():
    """the same program as a stand-alone executable with ASan and UBSan, on the same input: exit 0, nothing on stderr (`run` asserts
    both), the same output"""
    grids = sample_grids()
    plain = run(_build("mesh_nest_host", ["-O1"]), grids)
    san = run(_build("mesh_nest_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), grids)
    assert len(plain) == len(san)
    for a, b in zip(plain, san):
        assert all(np.array_equal(a[tag], b[tag]) for tag in "SLPD")


# ---- the host entry point and the interface ------------------------------------------------------------------------------------------------
def test_children_is_a_stable_sort_by_parent():
    lib, p = F.lib(), F._p
    rng = np.random.default_rng(193)
    cases = [np.zeros(0, np.uint32), np.array([NR.NONE], np.uint32), np.array([NR.NONE, 0, 1, 0, NR.NONE, 4, 0], np.uint32)]
    for n in (10, 1000):
        parent = rng.integers(0, n, n).astype(np.uint32)
        parent[rng.random(n) < 0.3] = NR.NONE
        cases.append(parent)
    cases.append(NR.stack(OR.stack(in_layers([rings(16, 3, 1), plate_with_holes(16, 3)], 16), 0, 2, 4))["parent"])
    for parent in cases:
        n = len(parent)
        start, kids = np.full(n + 1, 77, np.uint64), np.full(n + 1, 77, np.uint32)
        assert lib.fhip_nesting_children(p(parent), n, p(start), p(kids)) == 0
        want_start, want = NR.children(parent)
        assert np.array_equal(start, want_start) and np.array_equal(kids[:len(want)], want) and (kids[len(want):] == 77).all()
    bad = np.array([NR.NONE, 0, 3], np.uint32)          # a parent beyond the loops
    assert lib.fhip_nesting_children(p(bad), 3, p(np.zeros(4, np.uint64)), p(np.zeros(3, np.uint32))) == 6


def test_the_header_declares_and_the_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fidget_hip.h")).read()
    stated = " ".join(re.sub(r"^ \* ?", "", hdr, flags=re.M).split())          # (the comment's lines without their leading " * ")
    for words in ("The unit boundary edge (a0, b0)-(a0, b0 + 1) belongs to l", "the largest a < a0 with P(a - 1, b0) != P(a, b0)", "NONE = 0xFFFFFFFF",
                  "left[l] < l", "whose area2 has the opposite sign to l's", "parent[l] < l", "an odd number of vertical unit edges on pixel row b0 with a < a0",
                  "the enclosing loop of smallest |area2|", "even exactly for outer boundaries", "(8 for 4, 4 for 8), the outside component excluded",
                  "counts = {loops, outer, top, max depth, layers, k0, connectivity, 0}", "It MUST be the bitmap that was outlined, unchanged"):
        assert words in stated, words          # the definitions are in the comment
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    lib = C.CDLL(F.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in F.SIGNATURES and name in F.EXPORTS and getattr(F.lib(), name).argtypes is not None, name
    assert re.search(r"fhip_outlines_nesting\s*\(\s*fhip_ctx\s*\*\s*ctx\s*,\s*const\s+void\s*\*\s*outlines\s*,\s*const\s+uint64_t\s*\*\s*bricks\s*,\s*int\s+bricks_on_device\s*,"
                     r"\s*void\s*\*\*\s*out\s*\)", hdr)
    assert callable(F.Outlines.nesting) and F.Nesting.NONE == 0xFFFFFFFF and F.Nesting is F.voxels.Nesting
    assert all(callable(getattr(F.Nesting, m)) for m in ("children", "regions", "polygons", "svg", "parent_device", "depth_device"))
    assert all(isinstance(getattr(F.Nesting, m), property) for m in ("left", "parent", "depth", "n_children", "region_area2"))
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from src_hash import MESH_ONLY
    assert all(name in MESH_ONLY for name in NEW_FILES)          # mesh-only: the render path's hash stays
    assert all(name in F._SOURCES for name in NEW_FILES)
