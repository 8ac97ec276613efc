"""fhip_shape_occupancy on the device against occupancy_ref.py: every integer field `==` the reference's.  (a) is the brute-force count
over all N^3 centres, (b) the octree recursion that defines the result; tests/test_occupancy.py holds the two to each other for the shapes
compared against (a) here.  The octree's counters are (b)'s where (b) is computed, and in every case what mesh_sample reports at the same
depth."""
import functools

import numpy as np
import pytest

import fidget_amd as F
import oracle as O
import occupancy_ref as R
from conftest import model_path
from test_many_inputs import spheres
from test_many_inputs_gpu import sphere_vars
from test_occupancy import BEAR_W2M, sphere_shape
from test_spills import many_live_values

pytestmark = pytest.mark.gpu

CELL_KEYS = ("cells", "full", "empty", "leaf_cells")


def vm(name):
    return lambda M: M.Shape.from_vm(model_path(name))


def var_sphere(M):
    c = M.Context()
    x, y, z = c.x(), c.y(), c.z()
    return M.Shape(c, c.sub(c.sqrt(c.add(c.add(c.square(x), c.square(y)), c.square(z))), c.var(7)))


def constant(v):
    def make(M):
        c = M.Context()
        return M.Shape(c, c.add(c.mul(c.x(), 0.0), v))       # (a tape with an axis in it, the value v everywhere)
    return make


def rotation():
    a, b = 0.4, 0.3
    rz = np.array([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    rx = np.array([[1, 0, 0, 0], [0, np.cos(b), -np.sin(b), 0], [0, np.sin(b), np.cos(b), 0], [0, 0, 0, 1]])
    m = rz @ rx
    m[:3, 3] = (0.05, -0.1, 0.02)
    return m.astype(np.float32)


def perspective():
    m = np.eye(4, dtype=np.float32)
    m[3, 2] = 0.3           # w = 1 + 0.3 z in [0.7, 1.3]: never 0 over the region
    m[0, 3] = 0.1
    return m


def mesh_counts(shape, depth, w2m=None, vars_=None):
    _, c = F.mesh_sample(shape, depth, world_to_model=w2m, vars=vars_)
    return {k: c[k] for k in CELL_KEYS}


def check(make, depth, w2m=None, vars_=None, against="b"):
    """the device's result for this case: fields == the reference's, counters == (b)'s (where computed) and == mesh_sample's"""
    s, o = make(F), make(O)
    occ = F.occupancy(s, depth, world_to_model=w2m, vars=vars_)
    got = R.fields(occ)
    if against == "a":
        want = R.sums(R.brute_force(o, depth, w2m, vars_))
    else:
        inside, counts, _ = R.recursion(o, depth, w2m, vars_)
        want = R.sums(inside)
        print("reference counters", counts, "device", occ.cells)
        assert occ.cells == counts
    print("reference", want)
    print("device   ", got)
    assert got == want
    assert occ.cells == mesh_counts(s, depth, w2m, vars_)
    return occ


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_sphere(depth):
    """depth 0: one leaf cell on a grid of 4, the smallest shape the leaf kernel sees"""
    occ = check(lambda M: sphere_shape(M, 0.5), depth)
    assert occ.grid == 4 << depth
    if depth == 0:
        assert occ.cells == {"cells": 1, "full": 0, "empty": 0, "leaf_cells": 1} and occ.n == 8
    if depth == 3:
        assert (occ.n, occ.cells["full"], occ.cells["empty"], occ.cells["leaf_cells"]) == (2176, 8, 200, 80)


def test_full_cells_on_several_levels():
    occ = check(lambda M: sphere_shape(M, 0.9), 3)
    assert occ.cells["full"] == 32          # 8 of level 2 and 24 of level 3 (tests/test_occupancy.py)


def test_constant_shapes():
    """-1: the root is Full, the closed forms of the whole grid;  +1: nothing inside, lo = N and hi = 0"""
    full = check(constant(-1.0), 2)
    assert full.n == 16 ** 3 and full.lo == (0, 0, 0) and full.hi == (15, 15, 15) and full.cells == {"cells": 1, "full": 1, "empty": 0, "leaf_cells": 0}
    assert full.s1 == (16 * 16 * 120,) * 3 and full.s2 == (16 * 16 * 1240,) * 3 + (16 * 120 * 120,) * 3
    empty = check(constant(1.0), 2)
    assert empty.n == 0 and empty.lo == (16, 16, 16) and empty.hi == (0, 0, 0) and empty.s1 == (0, 0, 0) and empty.s2 == (0,) * 6
    assert empty.cells == {"cells": 1, "full": 0, "empty": 1, "leaf_cells": 0}


@pytest.mark.parametrize("name,w2m", [("gyroid-sphere.vm", None), ("colonnade.vm", None), ("bear.vm", BEAR_W2M)])
def test_models_against_brute_force(name, w2m):
    """(test_the_recursion_counts_what_brute_force_counts: (a) == (b) for these inputs)"""
    check(vm(name), 3, w2m, against="a")
    check(vm(name), 3, w2m, against="b")      # ... and the counters


@pytest.mark.parametrize("matrix", [rotation, perspective])
@pytest.mark.parametrize("name", ["sphere", "colonnade"])
def test_transforms(name, matrix):
    check((lambda M: sphere_shape(M, 0.5)) if name == "sphere" else vm("colonnade.vm"), 3, matrix())


def test_a_variable():
    occ = check(var_sphere, 3, vars_={7: 0.625})
    assert occ.n > 2176
    with pytest.raises(ValueError, match="MissingVar"):
        F.occupancy(var_sphere(F), 3)


def test_more_than_16_inputs():
    """the bound-tape path"""
    vals = sphere_vars(80)
    make = lambda M: M.Shape(*spheres(M, 80))        # noqa: E731
    assert make(F).var_count() > 16
    check(make, 3, vars_=vals)


def test_more_leaf_cells_than_blocks():
    """gyroid-sphere at depth 6: 79 226 leaf cells for at most 4 096 blocks - every block takes some twenty cells in turn.  Against (a):
    the oracle evaluates the 256^3 centres in ~2 s"""
    occ = check(vm("gyroid-sphere.vm"), 6, against="a")
    assert occ.cells["leaf_cells"] == 79226 > 4096 and occ.n == 655036


@functools.lru_cache(maxsize=None)
def _with_and_without_simplification(name, depth):
    s = F.Shape.from_vm(model_path(name))
    hip = s.hip
    default = F.occupancy(s, depth)
    with hip.options(mesh_simplify_min_ops=0):
        plain = F.occupancy(s, depth)
        plain_counts = mesh_counts(s, depth)
    return default, plain, mesh_counts(s, depth), plain_counts


@pytest.mark.parametrize("name,depth", [("colonnade.vm", 5), ("prospero.vm", 7)])
def test_simplification_does_not_matter(name, depth):
    """the tape simplified on the way down (prospero at depth 7: twice) or not at all: the same integers, device against device"""
    default, plain, counts, plain_counts = _with_and_without_simplification(name, depth)
    print(default, plain, sep="\n")
    assert R.fields(default) == R.fields(plain) and default.n > 0
    assert default.cells == plain.cells == counts == plain_counts


def test_refusals():
    """the statuses and messages of the refused calls, and that the context works after them.  (That nothing was launched is not visible
    from here: the depth check returns before anything else; the LDS check follows the tape's upload, as in fhip_mesh_build.)"""
    s = sphere_shape(F, 0.5)
    with pytest.raises(F.FidgetHipError) as e:
        F.occupancy(s, 11)
    assert e.value.status == 6 and "depth" in str(e.value)          # FHIP_ERR_UNSUPPORTED
    big = many_live_values(F)
    assert big.slot_count() * 64 * 16 > 160 * 1024
    with pytest.raises(F.FidgetHipError) as e:
        F.occupancy(big, 2)
    assert e.value.status == 6 and "LDS" in str(e.value)
    with pytest.raises(F.FidgetHipError) as e:          # (as the mesher refuses it)
        F.mesh_sample(big, 2)
    assert e.value.status == 6
    assert F.occupancy(s, 3).n == 2176         # the context still works
    c = F.Context()
    with pytest.raises(F.FidgetHipError) as e:
        F.occupancy(F.Shape(c, roots=[c.x(), c.y()]), 2)
    assert e.value.status == 5          # FHIP_ERR_BAD_TAPE: one output


def test_derived_values_of_a_sphere():
    """r = 0.5 at depth 5: N = 128, h = 1 / 64.  A voxel counted inside has its centre inside, so what it adds beyond the ball lies within
    half a voxel diagonal e = sqrt(3) h / 2 outside the surface; what a voxel not counted leaves out lies within e inside it.  The two
    errors have opposite signs, so |volume - 4 pi r^3 / 3| <= the larger shell, the outer one: 4 pi / 3 ((r + e)^3 - r^3) = 0.0437 (f32
    rounding of the value moves a centre across the surface only where it is within ~1e-7 of it: inside the same shells)."""
    r, depth = 0.5, 5
    occ = check(lambda M: sphere_shape(M, r), depth, against="a")
    h = 2.0 / occ.grid
    assert h == 1.0 / 64
    e = np.sqrt(3.0) * h / 2
    bound = 4 * np.pi / 3 * ((r + e) ** 3 - r ** 3)
    exact = 4 * np.pi / 3 * r ** 3
    print("volume", occ.volume, "exact", exact, "bound", bound, "centroid", occ.centroid, "bounds", occ.bounds)
    assert 0.0436 < bound < 0.0437
    assert abs(occ.volume - exact) <= bound
    assert (np.abs(occ.centroid) <= h).all()
    lo, hi = occ.bounds
    assert (np.abs(lo + r) <= h).all() and (np.abs(hi - r) <= h).all()          # the outermost inside centres are within h / 2 of the poles' planes
    # the second moments about the centroid: those of the inside centres themselves, in float64
    i, j, k = np.nonzero(R.brute_force(sphere_shape(O, r), depth))
    pts = -1.0 + (np.stack([i, j, k], axis=1) + 0.5) * h
    assert np.allclose(occ.covariance, np.cov(pts.T, bias=True), rtol=1e-12, atol=1e-15)
