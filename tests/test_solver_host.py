"""The constraint solver's host build (tests/host_build/solve_host.cpp: fidget_amd/csrc/solve_lm.hpp, the arithmetic k_solve runs,
driven by the oracle's evaluators) against the reference's own solver tests (fidget-solver/src/lib.rs:291-613), each with its
tolerance; the edge cases and exits of fhip_solve's contract (include/fidget_hip.h).  No GPU."""
import numpy as np
import pytest

import oracle as O
import solver_util as U


@pytest.mark.parametrize("name", sorted(U.KATS))
def test_reference_kat(name):
    """basic_solver, four_vars_at_once, four_vars_independent, xy_nonlinear, one_var_no_solution, solve_banana and solve_circle
    (both starts each): lib.rs:302-471"""
    shapes, keys, free, vals = U.KATS[name](O)
    out, err, its, ex = U.host_solve(shapes, keys, free, [vals])
    assert U.kat_check(name, out[0]), (name, out[0])
    assert ex[0] in (0, 1, 2, 3, 4), ex[0]          # ended by one of the reference's exits, not by a cap
    assert its[0] < 1000


@pytest.mark.parametrize("n,count", [(2, 1000), (10, 1000), (50, 50)])
def test_reference_linear(n, count):
    """small_linear / medium_linear / big_linear (lib.rs:473-539): residual norm^2 < 1e-3 and every row within 1e-2"""
    shapes, keys, free = U.linear_system(O, n)
    rows, mats, sols = U.linear_draws(np.random.default_rng(100 + n), n, count)
    out, err, its, ex = U.host_solve(shapes, keys, free, rows, threads=8)
    bad = [i for i in range(count) if not U.linear_ok(mats[i], sols[i], out[i])]
    assert not bad, bad[:10]
    assert (ex <= 4).all() and (its < 1000).all()


@pytest.mark.parametrize("n,count", [(2, 1000), (5, 100), (10, 50)])
def test_reference_quadratic(n, count):
    """small / medium / large_quadratic (lib.rs:541-630): at least 90 % succeed"""
    shapes, keys, free = U.quadratic_system(O, n)
    rows, mats, sols = U.quadratic_draws(np.random.default_rng(200 + n), n, count)
    out, err, its, ex = U.host_solve(shapes, keys, free, rows, threads=8)
    ok = sum(U.quadratic_ok(mats[i], sols[i], out[i]) for i in range(count))
    assert ok >= count * 9 // 10, (ok, count)
    assert (ex <= 4).all()


def test_no_constraints_returns_the_start():
    out, err, its, ex = U.host_solve([], ["x", "y"], [True, False], [[3.0, 4.0]])
    assert out.tolist() == [[3.0]] and its[0] == 0 and ex[0] == 0 and err[0] == 0.0


def test_all_parameters_fixed():
    shapes, keys, _, _ = U.basic_solver(O)
    out, err, its, ex = U.host_solve(shapes, keys, [False, False], [[2.0, 3.0]])
    assert out.shape == (1, 0) and its[0] == 1 and ex[0] == 1 and err[0] == 25.0


def test_a_variable_without_parameter_reads_zero():
    """x + z - 2 with only x given: z evaluates as 0 (the reference's zero-filled inputs), x -> 2"""
    c = O.Context()
    s = O.Shape(c, c.sub(c.add(c.x(), c.z()), c.constant(2.0)))
    out, err, its, ex = U.host_solve([s], ["x"], [True], [[0.0]])
    assert U.relative_eq(out[0][0], 2.0)


def test_a_free_variable_absent_from_some_constraints():
    c = O.Context()
    a = O.Shape(c, c.sub(c.x(), c.constant(1.0)))
    b = O.Shape(c, c.sub(c.add(c.x(), c.y()), c.constant(5.0)))
    out, err, its, ex = U.host_solve([a, b], ["x", "y"], [True, True], [[0.0, 0.0]])
    assert U.relative_eq(out[0][0], 1.0) and U.relative_eq(out[0][1], 4.0)


def test_more_than_64_free_variables_is_refused():
    c = O.Context()
    s = O.Shape(c, c.var(0))
    with pytest.raises(ValueError, match="Unsupported"):
        U.host_solve([s], list(range(65)), [True] * 65, [np.zeros(65)])
    U.host_solve([s], list(range(64)), [True] * 64, [np.zeros(64)])


def test_exit_reasons_are_reported():
    """zero residual at the start (0 steps), no change, zero error, and the iteration cap"""
    shapes, keys, free, _ = U.basic_solver(O)
    out, err, its, ex = U.host_solve(shapes, keys, free, [[1.0, -1.0], [0.0, -1.0]])
    assert ex.tolist()[0] == 0 and its[0] == 0
    assert ex[1] == 2 and err[1] == 0.0
    out, err, its, ex = U.host_solve(*U.banana((0.0, 0.0))(O)[:3], [[0.0, 0.0]], max_iterations=3)
    assert ex[0] == 5 and its[0] == 3
    out, err, its, ex = U.host_solve(*U.one_var_no_solution(O)[:3], [[0.0]])
    assert ex[0] in (1, 4)


def test_an_instance_does_not_depend_on_its_batch():
    shapes, keys, free = U.linear_system(O, 10)
    rows, _, _ = U.linear_draws(np.random.default_rng(7), 10, 40)
    a = U.host_solve(shapes, keys, free, rows, threads=4)
    for i in (0, 17, 39):
        b = U.host_solve(shapes, keys, free, rows[i:i + 1])
        for x, y in zip(a, b):
            assert x[i].tobytes() == y[0].tobytes()


def test_agrees_with_scipy_least_squares():
    """well-posed random linear systems (n = 5): the result agrees with scipy.optimize.least_squares(method='lm') to 1e-3"""
    opt = pytest.importorskip("scipy.optimize")
    n = 5
    shapes, keys, free = U.linear_system(O, n)
    rng = np.random.default_rng(11)
    rows, mats, sols = U.linear_draws(rng, n, 20)
    out, err, its, ex = U.host_solve(shapes, keys, free, rows)
    for i in range(20):
        m = mats[i].astype(np.float64) + 2.0 * np.eye(n)        # well conditioned
        r = rows[i].copy()
        r[n:n + n * n] = m.astype(np.float32).reshape(-1)
        o = U.host_solve(shapes, keys, free, [r])[0][0]
        ref = opt.least_squares(lambda v: m @ v - sols[i], np.zeros(n), method="lm").x
        assert np.allclose(o, ref, atol=1e-3), (o, ref)
