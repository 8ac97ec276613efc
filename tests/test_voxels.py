"""The voxel bitmap without a GPU: the numpy restatement of the format (voxels_ref.py) against the library's own unpacking, the index
arithmetic of fidget_amd/csrc/mesh_vox.hpp built for the host (tests/host_build/mesh_vox_host.cpp) - a Full cell's rows cover each of
its words exactly once and nothing else -, the entry points as the header states them, and the two references of occupancy_ref.py against
each other for the inputs tests/test_voxels_gpu.py compares with brute force and tests/test_occupancy.py does not cover."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fidget_amd as F
import oracle as O
import occupancy_ref as R
import voxels_ref as V
from test_occupancy import sphere_shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "mesh_vox_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")


def half_space(M):
    c = M.Context()
    return M.Shape(c, c.sub(c.x(), 0.25))


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_pack_and_unpack_round_trip(depth):
    rng = np.random.default_rng(1000 + depth)
    N = 4 << depth
    for density in (0.5, 0.03):
        inside = rng.random((N, N, N)) < density
        bricks = V.pack(inside)
        assert bricks.dtype == np.uint64 and bricks.shape == (N // 4,) * 3
        assert np.array_equal(V.unpack(bricks), inside)
        assert np.array_equal(F.voxels_unpack(bricks), inside)          # the library's unpacking (byte order and bit order) against the shifts
        assert V.popcount(bricks) == int(inside.sum())
        assert np.array_equal(V.layer_counts(inside), [int(inside[:, :, k].sum()) for k in range(N)])
        img = V.slices(inside, 1, N - 1)
        assert img.shape == (N - 2, N, N) and img.dtype == np.uint8
        assert img[0, 2, 3] == 255 * inside[3, 2, 1] and set(np.unique(img)) <= {0, 255}


@pytest.mark.parametrize("lz", range(4))
@pytest.mark.parametrize("ly", range(4))
@pytest.mark.parametrize("lx", range(4))
def test_the_bit_of_a_single_voxel(lx, ly, lz):
    """voxel (4 bx + lx, 4 by + ly, 4 bz + lz) alone, on a grid of 8: word [bz, by, bx], bit lx + 4 ly + 16 lz, every other word 0"""
    bx, by, bz = 1, 0, 1
    inside = np.zeros((8, 8, 8), bool)
    inside[4 * bx + lx, 4 * by + ly, 4 * bz + lz] = True
    bricks = V.pack(inside)
    want = np.zeros((2, 2, 2), np.uint64)
    want[bz, by, bx] = np.uint64(1) << np.uint64(lx + 4 * ly + 16 * lz)
    assert np.array_equal(bricks, want)
    assert np.array_equal(F.voxels_unpack(want), inside)


def test_the_library_exports_the_entry_points():
    lib = C.CDLL(F.LIB_PATH)
    for name in ("fhip_voxels_words", "fhip_shape_voxels", "fhip_voxels_slices", "fhip_voxels_layer_counts"):
        assert hasattr(lib, name) and name in F.EXPORTS and getattr(F.lib(), name).argtypes is not None, name
    assert callable(F.voxelize) and callable(F.Voxels.slices) and callable(F.Voxels.layer_counts) and callable(F.Voxels.inside)
    words = F.lib().fhip_voxels_words          # (no device behind it)
    assert [int(words(d)) for d in (0, 1, 3, 10, 11, 12)] == [1, 8, 512, 1 << 30, 0, 0]


@pytest.fixture(scope="module")
def arithmetic():
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "mesh_vox_host")
    deps = [SRC, os.path.join(CSRC, "mesh_vox.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe])      # (plain g++: the header touches no device)
    res = subprocess.run([exe], capture_output=True, text=True, check=True)
    lines = {}
    for line in res.stdout.splitlines():
        name, _, rest = line.partition(":")
        lines[name] = dict(kv.split("=", 1) for kv in rest.split())
    return lines


def test_sizes_and_bit_numbers(arithmetic):
    for d in range(13):
        assert int(arithmetic[f"words_{d}"]["n"]) == (8 ** d if d <= 10 else 0)
    assert [int(b) for b in arithmetic["bits"]["b"].split(",")] == list(range(64))       # lx fastest, then ly, then lz: the lanes of a leaf cell's wave


def test_a_full_cells_rows_cover_its_words_exactly_once(arithmetic):
    cases = 0
    for depth in range(5):
        B = 1 << depth
        for level in range(depth + 1):
            r, m = B >> level, (1 << level) - 1
            origins = [(0, 0, 0)] if level == 0 else [(0, 0, 0), (m, m, m), (m // 2, 0, m), (1 & m, m, m // 2)]
            for aligned in (0, 1):
                for o in origins:
                    got = arithmetic[f"full_{depth}_{level}_{aligned}_{o[0]}_{o[1]}_{o[2]}"]
                    vec = 2 if (r >= 2 and aligned) else 1
                    assert (int(got["r"]), int(got["vec"])) == (r, vec)
                    assert int(got["rows"]) == min(r * r, 8) and int(got["slots"]) * int(got["rows"]) * vec == r ** 3
                    w = [int(x) for x in got["w"].split(",")]
                    want = sorted((bz * B + by) * B + bx for bz in range(o[2] * r, (o[2] + 1) * r) for by in range(o[1] * r, (o[1] + 1) * r)
                                  for bx in range(o[0] * r, (o[0] + 1) * r))
                    assert len(w) == r ** 3 and sorted(w) == want, (depth, level, aligned, o)         # each word once, no other word
                    if vec == 2:        # 16-byte stores: every pair starts at an even word and stays in its row
                        assert all(a % 2 == 0 and b == a + 1 for a, b in zip(w[0::2], w[1::2]))
                    # consecutive slots are consecutive pieces of a row: lanes of a wave store next to each other
                    rows = int(got["rows"])
                    firsts = w[0::vec * rows]
                    per_row = r // vec
                    assert all(firsts[i + 1] - firsts[i] == vec for i in range(len(firsts) - 1) if (i + 1) % per_row), (depth, level, aligned, o)
                    cases += 1
    assert cases == 2 * (5 + 4 * 10)


@pytest.mark.parametrize("name,make,depth", [("sphere0.9", lambda M: sphere_shape(M, 0.9), 5), ("half-space", half_space, 4)])
def test_the_recursion_gives_what_brute_force_gives(name, make, depth):
    """the inputs of test_voxels_gpu.py that are compared with brute force there and that tests/test_occupancy.py does not hold to the recursion"""
    s = make(O)
    a = R.brute_force(s, depth)
    b, counts, full_per_level = R.recursion(s, depth)
    assert np.array_equal(a, b)
    if name == "sphere0.9":
        assert full_per_level[2] > 0          # level-2 Full cells at depth 5: rows of 8 words
    else:
        assert full_per_level[:2] == [0, 4] and counts["leaf_cells"] > 0          # the four octants of x < 0 Full at level 1; cells that touch x = 0.25 stay ambiguous
        assert int(a.sum()) == 40 * 64 * 64          # c(i) < 0.25 for i <= 39 of 64
