"""fhip_solve on the device against the independent float64 loop of tests/solver_ref.py - the case table, bounds and checks of
tests/test_solver_ref.py - and, bit for bit against the host build, what the device does alone: the ownership of an instance's work
by its lane group on both sides of every group-width boundary, parameter and slot maps with free and fixed parameters interleaved,
and waves whose instances are in different states (Jacobian / step / trial / done) at the same time."""
import functools

import numpy as np
import pytest

import fidget_amd as F
import oracle as O
import solver_ref as R
import solver_util as U
import test_solver_ref as T
from test_solver_gpu import same

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def solvers(build):
    """-> (device, host): solve(values, cap) of the system on each"""
    d, h = R.System(build, F), R.System(build, O)
    return (lambda values, cap=0: F.solve_batch(d.shapes, d.keys, d.free, values, max_iterations=cap),
            lambda values, cap=0: U.host_solve(h.shapes, h.keys, h.free, values, max_iterations=cap, threads=16))


def both(build, values, cap=0):
    """the device's result, equal to the host build's bit for bit"""
    device, host = solvers(build)
    dev = device(values, cap)
    same(dev, host(values, cap))
    return dev


@pytest.mark.parametrize("name,cap", T.CAPPED)
def test_capped_run_against_the_float64_loop(name, cap):
    """(bit-equal to the host build as well: the ratios SOLVER.md lists for the host are the device's)"""
    T.check_capped(name, cap, lambda values, cap: both(T.CASES[name].build, values, cap))


@pytest.mark.parametrize("name", T.SQUARE + T.NO_ROOT)
def test_converged_run(name):
    T.check_converged(name, lambda values, cap=0: both(T.CASES[name].build, values, cap))


@pytest.mark.parametrize("n", T.WIDTHS)
def test_lane_group_width_boundaries(n):
    """n free variables on both sides of every boundary of G, a batch that ends in a partly filled wave, to convergence (the same
    batch at cap 2 against the float64 loop: test_capped_run_against_the_float64_loop[width*])"""
    case = T.CASES[f"width{n}"]
    assert len(case.values) % T.per_wave(n) != 0
    result = both(case.build, case.values)
    assert (result[3] != R.EXIT_MAX_ITERATIONS).all() and (result[3] != R.EXIT_MAX_RETRIES).all()
    assert T.converges(T.reference(f"width{n}").system, case.values, result) == len(case.values)     # (the reference finds a root from every start)


def test_interleaved_free_and_fixed_parameters():
    """axis keys and var keys mixed, free and fixed alternating, in an order no tape's slots have, two keys nothing reads, fixed values
    that differ from instance to instance (at cap 2 against the float64 loop: test_capped_run_against_the_float64_loop[interleaved-2])"""
    case = T.CASES["interleaved"]
    fixed = ~np.asarray(case.build(R.Recording())[2])
    assert (np.ptp(case.values[:, fixed], axis=0) > 0).all()
    out, err, its, ex = both(case.build, case.values)
    assert (out[:, 4] == case.values[:, 8]).all()       # the free parameter nothing reads (key 11) is returned as it came
    device = solvers(case.build)[0]
    for i in range(0, len(case.values), 7):
        same([x[i:i + 1] for x in (out, err, its, ex)], device(case.values[i:i + 1]))


@pytest.mark.parametrize("cap", [0, 2])
@pytest.mark.parametrize("n", [7, 13, 25])
def test_waves_whose_instances_diverge(n, cap):
    build = T.banded_through(n)
    batch = T.check_divergent(n, cap, lambda values, cap: both(build, values, cap))
    device = solvers(build)[0]
    values = T.divergent_starts(n)[0]
    for i in range(len(values)):      # each instance alone: the same bits as among the others
        same([x[i:i + 1] for x in batch], device(values[i:i + 1], cap))
