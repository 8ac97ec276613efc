"""Shape occupancy without a GPU: the two references of occupancy_ref.py against each other - the octree recursion that defines the result
gives the count over all N^3 voxel centres wherever interval inclusion holds - the closed forms of a Full cell against plain sums over its
voxels, and the result struct and entry point as the header states them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fidget_amd as F
import oracle as O
import occupancy_ref as R
from conftest import model_path
from test_mesh import sphere

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BEAR_W2M = np.eye(4, dtype=np.float32)
BEAR_W2M[:2, 3] = 0.125          # (tests/test_mesh_export_gpu.py: the region moved to where bear.vm is)


def sphere_shape(M, r):
    c = M.Context()
    return M.Shape(c, sphere(c, (0.0, 0.0, 0.0), r))


# name -> (shape for either module, world_to_model, inside voxels / Full / Empty / leaf cells at depth 3 where the issue states them)
SHAPES = {
    "sphere0.5": (lambda M: sphere_shape(M, 0.5), None, (2176, 8, 200, 80)),
    "gyroid-sphere": (lambda M: M.Shape.from_vm(model_path("gyroid-sphere.vm")), None, (1322, 0, 152, 304)),
    "colonnade": (lambda M: M.Shape.from_vm(model_path("colonnade.vm")), None, (1986, 0, 110, 241)),
    "bear": (lambda M: M.Shape.from_vm(model_path("bear.vm")), None, (3663, 1, 178, 270)),
    "bear-moved": (lambda M: M.Shape.from_vm(model_path("bear.vm")), BEAR_W2M, None),
    "sphere0.9": (lambda M: sphere_shape(M, 0.9), None, None),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_recursion_counts_what_brute_force_counts(name):
    make, w2m, stated = SHAPES[name]
    s = make(O)
    a = R.brute_force(s, 3, w2m)
    b, counts, full_per_level = R.recursion(s, 3, w2m)
    assert a.shape == (32, 32, 32) and (a == b).all()
    assert R.sums(a) == R.sums(b)
    assert counts["cells"] == 1 + 8 * (counts["cells"] - counts["full"] - counts["empty"] - counts["leaf_cells"])      # every inner ambiguous cell has 8 children
    if stated:
        assert (int(a.sum()), counts["full"], counts["empty"], counts["leaf_cells"]) == stated
    if name == "sphere0.9":
        assert sum(1 for n in full_per_level if n) >= 2, full_per_level      # Full cells on more than one level


def test_sums_of_a_small_array():
    inside = np.zeros((4, 4, 4), bool)
    assert R.sums(inside) == {"n": 0, "s1": (0, 0, 0), "s2": (0,) * 6, "lo": (4, 4, 4), "hi": (0, 0, 0), "grid": 4}
    inside[1, 2, 3] = inside[3, 0, 3] = True
    assert R.sums(inside) == {"n": 2, "s1": (4, 2, 6), "s2": (10, 4, 18, 2, 12, 6), "lo": (1, 0, 3), "hi": (3, 2, 3), "grid": 4}


@pytest.mark.parametrize("depth,level,origin", [(0, 0, (0, 0, 0)), (2, 1, (1, 0, 1)), (3, 2, (3, 1, 2)), (3, 3, (7, 0, 5)), (3, 0, (0, 0, 0)),
                                                (10, 10, (1023, 1023, 1023)), (10, 7, (127, 0, 64)), (10, 7, (127, 127, 127))])
def test_closed_forms_of_a_full_cell(depth, level, origin):
    """a cell of level `level` at `origin` (in cells of that level): edge w = N >> level voxels; the sums over its voxels one by one"""
    N = 4 << depth
    w = N >> level
    org = tuple(o * w for o in origin)
    ax = [np.arange(o, o + w, dtype=np.uint64) for o in org]          # (uint64 as the device adds them: at depth 10 nothing may wrap)
    i, j, k = (a.ravel() for a in np.meshgrid(*ax, indexing="ij"))
    want = {"n": len(i), "s1": (int(i.sum()), int(j.sum()), int(k.sum())),
            "s2": tuple(int(v.sum()) for v in (i * i, j * j, k * k, i * j, i * k, j * k)),
            "lo": org, "hi": tuple(o + w - 1 for o in org), "grid": N}
    got = R.box_sums(org, w, N)
    assert got == want
    assert all(v < 2 ** 64 for v in got["s2"])


def test_closed_forms_of_the_whole_grid_at_depth_10_fit_64_bits():
    """the root cell Full at depth 10 (the last voxel of the grid included): the largest sums there are, against the sums of 0 .. N - 1"""
    N = 4096
    got = R.box_sums((0, 0, 0), N, N)
    t1 = sum(range(N))
    t2 = sum(v * v for v in range(N))
    assert got["n"] == N ** 3 and got["s1"] == (N * N * t1,) * 3
    assert got["s2"] == (N * N * t2,) * 3 + (N * t1 * t1,) * 3
    assert got["hi"] == (N - 1,) * 3
    assert max(got["s2"]) < 2 ** 60 < 2 ** 64
    # ... and the last voxel alone
    last = R.box_sums((N - 1,) * 3, 1, N)
    assert last["s1"] == (N - 1,) * 3 and last["s2"] == ((N - 1) ** 2,) * 6 and last["n"] == 1


def _header_struct(name):
    """[(field, C type, count)] of a one-line `typedef struct name { ... } name;` of the header"""
    src = open(os.path.join(ROOT, "include", "fidget_hip.h")).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", src, re.S).group(1)
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        ctype, rest = stmt.split(None, 1)
        for f in rest.split(","):
            m = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", f)
            out.append((m.group(1), ctype, int(m.group(2) or 1)))
    return out


def test_the_ctypes_mirror_has_the_headers_layout():
    size = {"uint64_t": 8, "uint32_t": 4}
    off, want = 0, []
    for field, ctype, count in _header_struct("fhip_occupancy"):
        off = (off + size[ctype] - 1) // size[ctype] * size[ctype]      # natural alignment
        want.append((field, off, size[ctype] * count))
        off += size[ctype] * count
    total = (off + 7) // 8 * 8
    got = [(n, getattr(F.OccupancyStruct, n).offset, getattr(F.OccupancyStruct, n).size) for n, _ in F.OccupancyStruct._fields_]
    assert got == want
    assert C.sizeof(F.OccupancyStruct) == total == 144
    assert [n for n, _, _ in want] == ["n", "s1", "s2", "lo", "hi", "grid", "pad", "cells"]


def test_the_library_exports_the_entry_point():
    lib = C.CDLL(F.LIB_PATH)
    assert hasattr(lib, "fhip_shape_occupancy")
    assert callable(F.occupancy)


def test_derived_values_from_the_integers():
    """Occupancy's float64 values for two voxels of a grid of 4 (h = 1/2): (1, 2, 3) and (3, 0, 3)"""
    raw = F.OccupancyStruct()
    raw.n, raw.grid = 2, 4
    raw.s1[:] = (4, 2, 6)
    raw.s2[:] = (10, 4, 18, 2, 12, 6)
    raw.lo[:] = (1, 0, 3)
    raw.hi[:] = (3, 2, 3)
    raw.cells[:] = (9, 0, 7, 1)
    o = F.Occupancy(raw)
    assert R.fields(o) == {"n": 2, "s1": (4, 2, 6), "s2": (10, 4, 18, 2, 12, 6), "lo": (1, 0, 3), "hi": (3, 2, 3), "grid": 4}
    assert o.cells == {"cells": 9, "full": 0, "empty": 7, "leaf_cells": 1}
    assert o.volume == 2 * 0.125
    pts = np.array([[-0.25, 0.25, 0.75], [0.75, -0.75, 0.75]])         # the two centres
    assert np.array_equal(o.centroid, pts.mean(axis=0))
    assert np.allclose(o.covariance, np.cov(pts.T, bias=True), rtol=0, atol=1e-15)
    lo, hi = o.bounds
    assert np.array_equal(lo, [-0.5, -1.0, 0.5]) and np.array_equal(hi, [1.0, 0.5, 1.0])
    raw = F.OccupancyStruct()
    raw.grid = 4
    raw.lo[:] = (4, 4, 4)
    e = F.Occupancy(raw)
    assert e.volume == 0.0 and np.isnan(e.centroid).all() and np.isnan(e.covariance).all()
