"""fhip_solve (fidget-solver's solve, batched; fidget_amd/csrc/solve.hip) on the device against its host build (tests/host_build/
solve_host.cpp: the same solve_lm.hpp arithmetic with the oracle's evaluators): out, err, iterations and exit reason bit for bit - for
the reference's solver tests, transcendental and min / max constraints, batches of every size and shuffle, every lane-group width,
and projections of points onto prospero.vm and bear.vm."""
import numpy as np
import pytest

import fidget_amd as F
import oracle as O
import solver_util as U
from conftest import model_path

pytestmark = pytest.mark.gpu


def same(a, b):
    """equal bits; a NaN only has to be a NaN where the other is (the sign of a NaN made by an invalid operation is the
    platform's: + on the device, - from x86's SSE)"""
    for x, y in zip(a, b):
        assert x.shape == y.shape
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype == np.float32:
            nx, ny = np.isnan(x), np.isnan(y)
            assert (nx == ny).all(), (x, y)
            x, y = np.where(nx, np.float32(0), x), np.where(ny, np.float32(0), y)
        assert x.tobytes() == y.tobytes(), (x, y)


def both(build, *args):
    fs, keys, free = build(F, *args)[:3]
    os_ = build(O, *args)[0]
    return fs, os_, keys, free


@pytest.mark.parametrize("name", sorted(U.KATS))
def test_reference_kat_bit_for_bit(name):
    fs, keys, free, vals = U.KATS[name](F)
    os_ = U.KATS[name](O)[0]
    dev = F.solve_batch(fs, keys, free, [vals])
    same(dev, U.host_solve(os_, keys, free, [vals]))
    assert U.kat_check(name, dev[0][0])


def test_public_solve_mirrors_the_reference():
    c = F.Context()
    s = F.Shape(c, c.add(c.x(), c.y()))
    sol = F.solve([s], {"x": F.Free(0.0), "y": F.Fixed(-1.0)})
    assert list(sol) == ["x"] and U.relative_eq(sol["x"], 1.0)


def test_reference_linear_bit_for_bit():
    """small_linear (1000 draws, the matrix as fixed parameters: one set of tapes) and medium_linear (constants, one call per draw:
    a row of 10 + 100 + 10 parameters exceeds the 16 inputs of a device tape).  big_linear (50 unknowns in every row) is out of
    reach of a device tape; the host build covers it (tests/test_solver_host.py)."""
    fs, os_, keys, free = both(U.linear_system, 2)
    rows, mats, sols = U.linear_draws(np.random.default_rng(102), 2, 1000)
    dev = F.solve_batch(fs, keys, free, rows)
    same(dev, U.host_solve(os_, keys, free, rows, threads=16))
    assert all(U.linear_ok(mats[i], sols[i], dev[0][i]) for i in range(1000))
    rng = np.random.default_rng(110)
    for _ in range(100):
        vals = U.rand_f32(rng, 10)
        mat = U.rand_f32(rng, 10, 10)
        sol = U.mat_vec(mat, vals)
        fs, keys, free, start = U.linear_const(F, mat, sol)
        dev = F.solve_batch(fs, keys, free, [start])
        same(dev, U.host_solve(U.linear_const(O, mat, sol)[0], keys, free, [start]))
        assert U.linear_ok(mat, sol, dev[0][0])


@pytest.mark.parametrize("n,count", [(2, 1000), (5, 100), (10, 50)])
def test_reference_quadratic_bit_for_bit(n, count):
    rng = np.random.default_rng(200 + n)
    if n == 2:      # the matrix as fixed parameters: 2 + 6 + 1 inputs per tape
        fs, os_, keys, free = both(U.quadratic_system, n)
        rows, mats, sols = U.quadratic_draws(rng, n, count)
        dev = F.solve_batch(fs, keys, free, rows)
        same(dev, U.host_solve(os_, keys, free, rows, threads=16))
        outs = dev[0]
    else:           # constants, one call per draw
        outs = []
        for _ in range(count):
            vals = U.rand_f32(rng, n)
            mat = U.rand_f32(rng, n, n * n + n)
            sol = U.mat_vec(mat, U.quadratic_col(vals))
            fs, keys, free, start = U.quadratic_const(F, mat, sol)
            dev = F.solve_batch(fs, keys, free, [start])
            same(dev, U.host_solve(U.quadratic_const(O, mat, sol)[0], keys, free, [start]))
            outs.append(dev[0][0])
        rows = None
        rng = np.random.default_rng(200 + n)
        mats, sols = [], []
        for _ in range(count):
            vals = U.rand_f32(rng, n)
            mat = U.rand_f32(rng, n, n * n + n)
            mats.append(mat)
            sols.append(U.mat_vec(mat, U.quadratic_col(vals)))
    assert sum(U.quadratic_ok(mats[i], sols[i], outs[i]) for i in range(count)) >= count * 9 // 10


trans_system = U.trans_system


def test_transcendental_and_min_max_constraints_bit_for_bit():
    fs, os_, keys, free = both(trans_system)
    rows = np.random.default_rng(5).uniform(-3, 3, (512, 2)).astype(np.float32)
    dev = F.solve_batch(fs, keys, free, rows)
    same(dev, U.host_solve(os_, keys, free, rows, threads=16))


def test_small_linear_as_one_call_equals_each_alone():
    fs, keys, free = U.linear_system(F, 2)
    rows, mats, sols = U.linear_draws(np.random.default_rng(3), 2, 1000)
    batch = F.solve_batch(fs, keys, free, rows)
    for i in range(0, 1000, 25):
        same([x[i:i + 1] for x in batch], F.solve_batch(fs, keys, free, rows[i:i + 1]))
    assert all(U.linear_ok(mats[i], sols[i], batch[0][i]) for i in range(1000))


def test_an_instance_is_the_same_bits_at_every_batch_size_and_place():
    fs, keys, free = U.quadratic_system(F, 2)
    rows = U.quadratic_draws(np.random.default_rng(9), 2, 10000)[0]
    full = F.solve_batch(fs, keys, free, rows)
    rng = np.random.default_rng(10)
    for size in (1, 63, 64, 65, 10000):
        idx = rng.permutation(10000)[:size]
        part = F.solve_batch(fs, keys, free, rows[idx])
        same(part, [x[idx] for x in full])


@pytest.mark.parametrize("n", [2, 5, 10, 20, 40, 64])
def test_every_lane_group_width(n):
    """n free -> G = 1, 2, 4, 8, 16, 32 lanes per instance (64 / G instances per wave)"""
    fs, os_, keys, free = both(U.banded_system, n)
    count = 130 if n <= 10 else 9
    rows = np.random.default_rng(300 + n).uniform(-2, 2, (count, n)).astype(np.float32)
    dev = F.solve_batch(fs, keys, free, rows)
    same(dev, U.host_solve(os_, keys, free, rows, threads=16))
    assert (dev[1] < 1e-6).all()


def test_errors_before_any_launch():
    c = F.Context()
    s = F.Shape(c, c.var(0))
    with pytest.raises(ValueError, match="Unsupported"):
        F.solve_batch([s], list(range(65)), [True] * 65, np.zeros((1, 65)))
    with pytest.raises(ValueError, match="BadVarSlice"):
        F.solve_batch([s], [0, 0], [True, True], np.zeros((1, 2)))
    with pytest.raises(ValueError, match="BadVarSlice"):
        F.solve_batch([s], ["x", "x"], [True, False], np.zeros((1, 2)))


def test_edge_cases_match_the_host_build():
    c, o = F.Context(), O.Context()
    f1, o1 = F.Shape(c, c.sub(c.add(c.x(), c.z()), c.constant(2.0))), O.Shape(o, o.sub(o.add(o.x(), o.z()), o.constant(2.0)))
    same(F.solve_batch([f1], ["x"], [True], [[0.0]]), U.host_solve([o1], ["x"], [True], [[0.0]]))       # z has no parameter: 0
    same(F.solve_batch([f1], ["x", "z"], [False, False], [[1.0, 2.0]]), U.host_solve([o1], ["x", "z"], [False, False], [[1.0, 2.0]]))
    out, err, its, ex = F.solve_batch([], ["x", "y"], [True, False], [[3.0, 4.0], [5.0, 6.0]])
    assert out.tolist() == [[3.0], [5.0]] and its.tolist() == [0, 0] and ex.tolist() == [0, 0]
    f2, o2 = F.Shape(c, c.sub(c.x(), c.constant(1.0))), O.Shape(o, o.sub(o.x(), o.constant(1.0)))
    f3 = F.Shape(c, c.sub(c.add(c.x(), c.y()), c.constant(5.0)))
    o3 = O.Shape(o, o.sub(o.add(o.x(), o.y()), o.constant(5.0)))
    same(F.solve_batch([f2, f3], ["x", "y"], [True, True], [[0.0, 0.0]]), U.host_solve([o2, o3], ["x", "y"], [True, True], [[0.0, 0.0]]))
    same(F.solve_batch(*U.banana((0.0, 0.0))(F)[:3], [[0.0, 0.0]], max_iterations=3),
         U.host_solve(*U.banana((0.0, 0.0))(O)[:3], [[0.0, 0.0]], max_iterations=3))


def projection(name, dims, count, seed):
    fs, os_ = F.Shape.from_vm(model_path(name)), O.Shape.from_vm(model_path(name))
    keys = ["x", "y", "z"][:dims]
    rows = np.random.default_rng(seed).uniform(-1, 1, (count, dims)).astype(np.float32)
    return fs, os_, keys, rows


def test_project_points_onto_prospero():
    """2D, free x and y; prospero's 126-register gradient file fits LDS next to 64 instances of 2 free variables (the LDS path)"""
    fs, os_, keys, rows = projection("prospero.vm", 2, 4096, 21)
    assert fs.slot_count() * 64 * 16 + 64 * (3 * 4 + 5 * 2 + 2) * 4 <= 160 * 1024
    dev = F.solve_batch([fs], keys, [True] * 2, rows)
    same(dev, U.host_solve([os_], keys, [True] * 2, rows, threads=16))
    # |f| at the result: most points land on the surface; the rest stall where the field's gradient vanishes or jumps (prospero is
    # a min / max of many half-planes), as the reference's loop does there - measured: 72 % at <= 1e-4, median 0, max 1.13
    f = np.sqrt(dev[1].astype(np.float64))
    assert np.isfinite(f).all() and np.median(f) <= 1e-4 and np.mean(f <= 1e-4) >= 0.65, np.percentile(f, [50, 90, 95, 99, 100])


def test_project_points_onto_bear():
    """3D with transcendentals, free x, y and z"""
    fs, os_, keys, rows = projection("bear.vm", 3, 4096, 22)
    dev = F.solve_batch([fs], keys, [True] * 3, rows)
    same(dev, U.host_solve([os_], keys, [True] * 3, rows, threads=16))
    f = np.sqrt(dev[1].astype(np.float64))
    assert np.mean(f <= 1e-4) >= 0.5, np.nanpercentile(f, [50, 90, 95, 99, 100])
    print("bear |f| percentiles 50 90 95 99 100:", np.nanpercentile(f, [50, 90, 95, 99, 100]), "share <= 1e-4:", np.mean(f <= 1e-4),
          "NaN:", int(np.isnan(f).sum()))


def test_register_file_in_the_global_slab():
    """prospero beside 40 more free variables: 4 instances of 42 free variables per wave (G = 16) leave no room in LDS for the
    126-register gradient file, which goes to the global slab"""
    n = 40
    fl, ol = F.Context(), O.Context()
    fp, op = F.Shape.from_vm(model_path("prospero.vm")), O.Shape.from_vm(model_path("prospero.vm"))
    fs, os_ = [fp], [op]
    for i in range(n):     # v_i - (x + y) * i / n
        fs.append(F.Shape(fl, fl.sub(fl.var(i), fl.mul(fl.add(fl.x(), fl.y()), fl.constant(i / n)))))
        os_.append(O.Shape(ol, ol.sub(ol.var(i), ol.mul(ol.add(ol.x(), ol.y()), ol.constant(i / n)))))
    assert fp.slot_count() * 64 * 16 + 4 * (3 * 42 * 42 + 5 * 42 + 2) * 4 > 160 * 1024
    keys = ["x", "y"] + list(range(n))
    rows = np.random.default_rng(23).uniform(-1, 1, (24, n + 2)).astype(np.float32)
    dev = F.solve_batch(fs, keys, [True] * (n + 2), rows)
    same(dev, U.host_solve(os_, keys, [True] * (n + 2), rows, threads=16))
