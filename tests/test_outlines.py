"""The outlines of a voxel bitmap's layers without a GPU: the reference of outlines_ref.py against invariants - `next` a permutation,
the shoelace sums and perimeters against counts made another way, the number of loops against the connected parts of the pixels and
of their complement (components_ref.py) - on random images, a checkerboard and the trivial ones; the bit arithmetic of
fidget_amd/csrc/mesh_outline.hpp built for the host (tests/host_build/mesh_outline_host.cpp) against the reference, vertex for
vertex; that program under ASan and UBSan; the entry points as the header states them."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np

import components_ref as CR
import fidget_amd as F
import outlines_ref as OR
import voxels_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "mesh_outline_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")
ENTRY_POINTS = ("fhip_voxels_outlines", "fhip_outlines_counts", "fhip_outlines_layers", "fhip_outlines_vertices", "fhip_outlines_loops", "fhip_outlines_xy_dev",
                "fhip_outlines_next_dev", "fhip_outlines_loop_dev", "fhip_outlines_free")
NEW_FILES = ("mesh_outline.hpp", "outline.hip", "capi_outline.hpp")


def in_layer(P, k=1, N=None):
    """the image P [i, j] as layer k of an otherwise empty grid"""
    N = N or P.shape[0]
    g = np.zeros((N, N, N), bool)
    g[:P.shape[0], :P.shape[1], k] = P
    return g


def n_parts(P, connectivity):
    """the connected parts of the set pixels, and those of the clear pixels of the padded image other than the outside - under the
    dual connectivity: where diagonal pixels are separate, diagonal gaps are joined"""
    N = P.shape[0]
    M = (N + 2 + 3) // 4 * 4
    fg = CR.components(in_layer(P, 1, M), 6 if connectivity == 4 else 26).count
    bg = CR.components(in_layer(~np.pad(P, ((1, M - N - 1), (1, M - N - 1))), 1), 26 if connectivity == 4 else 6).count
    return fg, bg - 1


@functools.lru_cache(maxsize=None)
def images():
    rng = np.random.default_rng(91)
    out = [(f"random {N} {d}", rng.random((N, N)) < d) for N in (16, 64) for d in (0.1, 0.5, 0.9)]
    i, j = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    out += [("checkerboard", (i + j) % 2 == 0), ("full", np.ones((16, 16), bool)), ("empty", np.zeros((16, 16), bool))]
    one = np.zeros((16, 16), bool)
    one[5, 9] = True
    return out + [("single pixel", one)]


def test_the_reference_holds_the_invariants():
    for name, P in images():
        for conn in (4, 8):
            L = OR.layer(P, conn)
            n = len(L["next"])
            assert np.array_equal(np.sort(L["next"]), np.arange(n)), name          # a permutation
            assert int(L["area2"].sum()) == 2 * int(P.sum()), name
            assert int(L["perimeter"].sum()) == OR.boundary_edges(P), name
            assert int(L["n_vertices"].sum()) == n and np.array_equal(L["leader"], np.sort(L["leader"])), name
            fg, holes = n_parts(P, conn)
            assert len(L["leader"]) == fg + holes, (name, conn)
            assert int((L["area2"] > 0).sum()) == fg and int((L["area2"] < 0).sum()) == holes, (name, conn)
            step = L["xy"][L["next"]] - L["xy"]
            assert ((step == 0).sum(axis=1) == 1).all(), name          # every segment runs along one axis
            # no straight vertex: the segments before and after run along different axes
            axis = (step[:, 0] == 0).astype(int)
            assert (axis[L["next"]] != axis).all(), name


def test_the_hand_made_cases():
    one = np.zeros((4, 4), bool)
    one[1, 2] = True
    L = OR.layer(one, 4)
    assert L["xy"].tolist() == [[1, 2], [2, 2], [1, 3], [2, 3]] and L["next"].tolist() == [1, 3, 0, 2]          # counter-clockwise from the lower left
    assert L["area2"].tolist() == [2] and L["perimeter"].tolist() == [4] and L["lo"].tolist() == [[1, 2]] and L["hi"].tolist() == [[2, 3]]
    two = np.zeros((4, 4), bool)
    two[1, 1] = two[2, 2] = True          # a saddle at corner (2, 2)
    a, b = OR.layer(two, 4), OR.layer(two, 8)
    assert len(a["leader"]) == 2 and a["n_vertices"].tolist() == [4, 4] and len(b["leader"]) == 1 and b["n_vertices"].tolist() == [8]
    assert np.array_equal(a["xy"], b["xy"]) and a["xy"].tolist().count([2, 2]) == 2
    ring = np.ones((4, 4), bool)
    ring[1:3, 1:3] = False
    L = OR.layer(ring, 4)
    assert L["area2"].tolist() == [32, -8] and L["perimeter"].tolist() == [16, 8]          # the hole runs clockwise


def test_the_issues_numbers():
    """a random 16 x 16 image at density 0.1 (numpy's default generator, seed 0): 94 vertices; 23 loops with connectivity 4 and 22 with 8"""
    P = np.random.default_rng(0).random((16, 16)) < 0.1
    a, b = OR.layer(P, 4), OR.layer(P, 8)
    assert len(a["next"]) == 94 and len(b["next"]) == 94 and len(a["leader"]) == 23 and len(b["leader"]) == 22


# ---- the library's bit arithmetic, built for the host --------------------------------------------------------------------------------------
def _build(name, flags):
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("mesh_outline.hpp", "mesh_vox.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe])      # (plain g++: the header touches no device)
    return exe


def run(exe, grids):
    """-> per (grid, connectivity) the program's lines as {tag: uint64 array}"""
    queries = []
    for g, conn in grids:
        w = V.pack(g)
        queries.append(f"G {w.shape[0].bit_length() - 1} {conn} " + " ".join(f"{int(x):x}" for x in w.reshape(-1)))
    res = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stdout[-300:], res.stderr[-2000:])
    lines = res.stdout.splitlines()
    assert len(lines) == 3 * len(grids)
    out = []
    for q in range(len(grids)):
        assert [line[0] for line in lines[3 * q:3 * q + 3]] == ["S", "X", "N"]
        out.append({line[0]: np.array([int(x, 16) for x in line.split()[1:]], np.uint64) for line in lines[3 * q:3 * q + 3]})
    return out


@functools.lru_cache(maxsize=None)
def sample_grids():
    """depth 0 .. 2: empty, full, random at several densities; depth 3 and 4 (two and three chunks of 32 corners to a row): a few
    layers of an otherwise empty grid - random, a checkerboard, bars along x and y through every chunk, the borders"""
    rng = np.random.default_rng(92)
    grids = []
    for N in (4, 8, 16):
        grids += [np.zeros((N, N, N), bool), np.ones((N, N, N), bool)] + [rng.random((N, N, N)) < d for d in (0.1, 0.5, 0.9)]
    for N in (32, 64):
        g = np.zeros((N, N, N), bool)
        g[:, :, 0] = rng.random((N, N)) < 0.5
        i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
        g[:, :, 1] = (i + j) % 2 == 0
        g[:, 5, 2] = g[7, :, 2] = g[N - 1, :, 2] = g[:, N - 1, 2] = True
        g[:, :, N - 1] = rng.random((N, N)) < 0.9
        g[0, :, 5] = g[:, 0, 5] = True
        if N > 32:
            g[31:33, 31:33, 6] = np.array([[1, 0], [0, 1]], bool)          # a saddle at corner 32: the first of a chunk
        g[30:32, 10:12, 6] = np.array([[0, 1], [1, 0]], bool)          # ... and at corner 31, the last
        grids.append(g)
    return [(g, conn) for g in grids for conn in (4, 8)]


def compare(got, g, conn):
    N = g.shape[0]
    want = OR.stack(g, 0, N, conn)
    assert np.array_equal(got["S"], want["vertex_start"].astype(np.uint64))
    assert np.array_equal(got["X"], (want["xy"][:, 0] | (want["xy"][:, 1] << 16)).astype(np.uint64))
    assert np.array_equal(got["N"], want["next"].astype(np.uint64))


def test_the_bit_arithmetic_is_the_references():
    grids = sample_grids()
    for got, (g, conn) in zip(run(_build("mesh_outline_host", ["-O1"]), grids), grids):
        compare(got, g, conn)


def test_the_arithmetic_runs_clean_under_sanitizers():
    """the same program as a stand-alone executable with ASan and UBSan, on the same input: exit 0, nothing on stderr (`run` asserts
    both), the same output"""
    grids = sample_grids()
    plain = run(_build("mesh_outline_host", ["-O1"]), grids)
    san = run(_build("mesh_outline_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), grids)
    assert len(plain) == len(san)
    for a, b in zip(plain, san):
        assert all(np.array_equal(a[tag], b[tag]) for tag in "SXN")


# ---- the interface -----------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fidget_hip.h")).read()
    stated = " ".join(re.sub(r"^ \* ?", "", hdr, flags=re.M).split())          # (the comment's lines without their leading " * ")
    for words in ("m = P(a-1, b-1) | P(a, b-1) << 1 | P(a, b) << 2 | P(a-1, b) << 3", "0 = -x, 1 = +x, 2 = -y, 3 = +y", "m = 5: (3, 0), (2, 1); m = 10: (0, 2), (1, 3)",
                  "m = 5: (2, 0), (3, 1); m = 10: (1, 2), (0, 3)", "in the order b (N + 1) + a", "A loop's leader is its smallest vertex id",
                  "positive for an outer boundary and negative for a hole", "2^32 vertices or more is FHIP_ERR_OVERFLOW", "k0 == k1 is FHIP_OK"):
        assert words in stated, words          # the definitions are in the comment
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    lib = C.CDLL(F.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in F.EXPORTS and getattr(F.lib(), name).argtypes is not None, name
    assert re.search(r"fhip_voxels_outlines\s*\([^;]*int\s+on_device\s*,\s*uint32_t\s+k0\s*,\s*uint32_t\s+k1\s*,\s*uint32_t\s+connectivity\s*,\s*void\s*\*\*\s*out\s*\)", hdr)
    assert all(callable(getattr(F.Voxels, m)) for m in ("outlines", "outline"))
    assert all(callable(getattr(F.Outlines, m)) for m in ("xy", "next", "loop_of", "table", "polygons", "world", "svg", "xy_device", "next_device", "loop_of_device"))
    ffi = open(os.path.join(ROOT, "rust", "fidget-hip", "src", "ffi.rs")).read()
    assert all(f"pub fn {name}(" in ffi for name in ENTRY_POINTS)
    mesh_only = open(os.path.join(ROOT, "tools", "src_hash.py")).read()
    assert all(f'"{name}"' in mesh_only for name in NEW_FILES)          # mesh-only: the render path's hash stays
    assert all(name in F._SOURCES for name in NEW_FILES)
