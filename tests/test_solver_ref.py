"""The constraint solver against an independent float64 restatement of the reference's loop (tests/solver_ref.py), step by step.

The solver's other tests compare the device with a host build of the same solve_lm.hpp, or look at where a converging loop ends -
and Levenberg-Marquardt ends in the same place under many wrong damping rules.  Here a run is CAPPED at 1, 2 and 3 accepted steps
and `out` is compared with the float64 loop at the same cap: the damped step itself, the damping after an acceptance and its growth
after rejections are all visible in those numbers, and float32 and float64 are still on the same branch (SOLVER.md, "How the solver
is tested").

The bound comes from the reference alone: with Y = the largest distance between the float32 and the float64 run of solver_ref.py
over a case's batch (distance: |a - b|_inf / max(1, |b|_inf)), the solver may be at most RATIO * Y from the float64 run.  Instances
whose closest accept / reject decision or singular value is too near its threshold for float32 and float64 to agree on the branch,
or whose Jacobian was taken at a tie of a min / max (solver_ref.Snapshot.ambiguous), are left out; at most MAX_LEFT_OUT of a batch
may be.

This file holds the case table and the checks, runs them on the host build (no GPU), and checks the reference itself against scipy
and a closed form.  tests/test_solver_ref_gpu.py runs the same table on the device.
"""
import functools

import numpy as np
import pytest

import grad_f64 as G
import oracle as O
import solver_ref as R
import solver_util as U
from conftest import model_path

RATIO = 16            # measured for the host build and the device: 0.67 to 6.59 (SOLVER.md has the table)
MAX_LEFT_OUT = 0.05
MAX_AT_A_TIE = 0.01   # of those, the share left out for a tie of a min / max (not one of the loop's own thresholds): the 1 % that
                      # tests/test_grad_f64.py allows its shapes; measured 0.78 % for bear.vm and 0 everywhere else
SEED = 2024


def banded(n, rows=None, absent=None):
    """r_i = v_i + 0.5 v_{i+1} - 0.25 v_{i+2}^2 - (i + 1) / k over the k variables that take part (all n, or all but `absent`),
    indices wrapping; `rows` constraints (default k).  All n variables are free parameters."""
    def build(be):
        c = be.Context()
        ids = [i for i in range(n) if i != absent]
        k = len(ids)
        vs = [c.var(i) for i in ids]
        shapes = []
        for i in range(rows or k):
            out = c.add(vs[i % k], c.mul(c.constant(0.5), vs[(i + 1) % k]))
            out = c.sub(out, c.mul(c.constant(0.25), c.square(vs[(i + 2) % k])))
            shapes.append(be.Shape(c, c.sub(out, c.constant((i + 1) / k))))
        return shapes, list(range(n)), [True] * n
    return build


def bear(be):
    c = be.Context()
    with open(model_path("bear.vm")) as f:
        root = G.read_vm(c, f.read())
    return [be.Shape(c, root)], ["x", "y", "z"], [True] * 3


def starts(count, n, lo=-2.0, hi=2.0, seed=SEED):
    return np.random.default_rng(seed).uniform(lo, hi, (count, n)).astype(np.float32)


BEAR_MIN_SHARE = 0.25


def bear_points(count=256):
    """Points of [-1, 1]^3 to project onto bear.vm, in the order of the seed, kept where every partial of the field is at least
    BEAR_MIN_SHARE of the largest (float64 partials: the choice does not depend on the solver).  With one constraint the step along
    axis k goes with 1 / g_k, so it carries the RELATIVE error of g_k; a float32 gradient is good to an absolute error next to its
    largest partial (what tests/test_grad_f64.py holds it to), and a partial of 0.003 beside one of 1.9 moved a correct solver's first
    step 1e-4 from the float64 one, where partials ROUNDED from float64 - the yardstick - lose 2e-7.  SOLVER.md notes the replacement."""
    system, p = R.System(bear), starts(8 * count, 3, -1.0, 1.0)
    g = np.abs(system.jacobian(p.astype(np.float64), p)[1][:, 0, :])
    with np.errstate(all="ignore"):
        ok = np.isfinite(g).all(axis=1) & (g.min(axis=1) >= BEAR_MIN_SHARE * g.max(axis=1))
    assert ok.sum() >= count
    return p[ok][:count]


class Case:
    def __init__(self, build, values, caps=(1, 2, 3), min_rejecting=0, square=False, n_unread=0):
        self.build, self._values, self.caps, self.min_rejecting, self.square = build, values, caps, min_rejecting, square
        self.n_unread = n_unread      # how many free variables no constraint reads

    @property
    def values(self):
        if callable(self._values):
            self._values = self._values()
        return self._values


WIDTHS = (3, 4, 6, 7, 12, 13, 24, 25, 48, 49)     # both sides of every lane-group boundary (chunks = ceil(n / 3): 1|2, 2|3, 4|5, 8|9, 16|17)


def per_wave(n):
    """instances per wave on the device: 64 / G, G the smallest power of two >= ceil(n / 3) (SOLVER.md)"""
    g = 1
    while g < (n + 2) // 3:
        g *= 2
    return 64 // g


INTERLEAVED_KEYS = [5, "y", 2, "x", 9, "z", 0, 7, 11, 4, 3]     # free and fixed alternate; nothing reads 7 (fixed) or 11 (free)


def interleaved(be):
    """the banded rows over x, v0, y, v2, z, v3, v4, v5, v9 - an order that is not the parameters' -, 8 constraints for the 5 free
    variables that take part; x, y, z and v4 are fixed"""
    c = be.Context()
    vs = [c.x(), c.var(0), c.y(), c.var(2), c.z(), c.var(3), c.var(4), c.var(5), c.var(9)]
    k, shapes = len(vs), []
    for i in range(8):
        out = c.add(vs[(i + 4) % k], c.mul(c.constant(0.5), vs[(i + 1) % k]))
        out = c.sub(out, c.mul(c.constant(0.25), c.square(vs[(i + 6) % k])))
        shapes.append(be.Shape(c, c.sub(out, c.constant((i + 1) / k))))
    return shapes, INTERLEAVED_KEYS, [i % 2 == 0 for i in range(len(INTERLEAVED_KEYS))]


def exact_solution(n):
    """entries in {0, +-0.5, +-1, +-2}: every term of a banded row is exact in float32 there"""
    return np.random.default_rng(n).choice(np.array([0, 0.5, -0.5, 1, -1, 2, -2], np.float32), n)


@functools.lru_cache(maxsize=None)
def banded_through(n):
    """the banded rows with the constants that make exact_solution(n) a root: r_i is exactly 0 there in float32"""
    s = exact_solution(n).astype(np.float64)

    def build(be):
        c = be.Context()
        vs = [c.var(i) for i in range(n)]
        shapes = []
        for i in range(n):
            out = c.add(vs[i], c.mul(c.constant(0.5), vs[(i + 1) % n]))
            out = c.sub(out, c.mul(c.constant(0.25), c.square(vs[(i + 2) % n])))
            shapes.append(be.Shape(c, c.sub(out, c.constant(float(s[i] + 0.5 * s[(i + 1) % n] - 0.25 * s[(i + 2) % n] ** 2)))))
        return shapes, list(range(n)), [True] * n
    return build


DIVERGENT_KINDS = ["solution"] * 8 + ["far"] * 12 + ["nan"] + ["ordinary"] * 20      # 41: no multiple of 16, 8 or 4


def divergent_starts(n):
    """-> (values [41, n], kinds): starts exactly at the root, far ones in [-8, 8], one with a NaN (it runs on
    NaN until its damping underflows to 0, some 95 steps of 32 sweeps each: the slowest instance by far), ordinary ones in [-2, 2],
    shuffled so that every wave holds instances in different states at the same time"""
    rng = np.random.default_rng(700 + n)
    kinds = np.array(DIVERGENT_KINDS)[rng.permutation(len(DIVERGENT_KINDS))]
    v = rng.uniform(-2, 2, (len(kinds), n)).astype(np.float32)
    v[kinds == "far"] = rng.uniform(-8, 8, ((kinds == "far").sum(), n)).astype(np.float32)
    v[kinds == "solution"] = exact_solution(n)
    v[kinds == "nan", rng.integers(0, n, (kinds == "nan").sum())] = np.nan
    return v, kinds


CASES = {
    **{f"banded{n}": Case(banded(n), starts(64 if n < 25 else 16, n), square=True) for n in (4, 7, 13, 25, 49)},
    **{f"width{n}": Case(banded(n), starts(2 * per_wave(n) + 1, n, seed=SEED + n), caps=(2,)) for n in WIDTHS},
    "interleaved": Case(interleaved, starts(50, len(INTERLEAVED_KEYS), seed=SEED + 1), caps=(2,), n_unread=1),
    "over_determined": Case(banded(7, rows=10), starts(64, 7)),
    "under_determined": Case(banded(7, rows=5), starts(64, 7), caps=(1,)),
    "absent_variable": Case(banded(7, absent=3), starts(64, 7), n_unread=1),
    "rosenbrock": Case(U.banana((0.0, 0.0)), starts(256, 2), min_rejecting=8, square=True),
    "transcendental": Case(U.trans_system, starts(64, 2)),
    "bear_projection": Case(bear, bear_points, caps=(1,)),
}
CAPPED = [(name, cap) for name, c in CASES.items() for cap in c.caps]
SQUARE = [name for name, c in CASES.items() if c.square]
NO_ROOT = ["over_determined"]     # the minimum is no root: the loop ends on a flat error, where err == prev_err exactly


class Reference:
    def __init__(self, case):
        self.system = R.System(case.build)
        cap = max(case.caps)
        self.f64 = R.run(self.system, case.values, cap, np.float64)
        self.f32 = R.run(self.system, case.values, cap, np.float32)


@functools.lru_cache(maxsize=None)
def reference(name):
    """a case's two reference runs, made once for all of its caps and for both test files; nobody writes to them"""
    return Reference(CASES[name])


def ratio(d, y):
    return f"{d / y:.2f}" if y else "n/a (both exactly 0)" if d == 0 else "n/a (Y is 0)"


def converges(system, values, result, steps=40):
    """Every instance that the float64 loop brings to a root within `steps` steps ends at a root in the solver too (not necessarily
    the same one: a system of quadratics has several).  At a root the float32 residuals are roundings of a few 1e-7 each, so err is
    some n x 1e-13; 1e-8 is far above that and far below the error of a start that found no root (1e-2 and more here).
    -> how many instances the reference brought to a root"""
    end = R.run(system, values, steps)[-1]
    at_root = end.err < 1e-20
    assert (result[1][at_root] < 1e-8).all(), (int(at_root.sum()), result[1][at_root].max())
    return int(at_root.sum())


def check_err(name, system, values, result, label=""):
    """`err` is the squared residual at the returned `out`: within RATIO times what the float32 evaluation of that sum loses against
    the float64 one at the same point, over the batch.  Not for an instance that took no step (err is +inf, or 0 from the
    zero-residual exit)."""
    out, err, its, ex = result
    took = (its > 0) & np.isfinite(out).all(axis=1)
    assert took.any()
    assert np.isfinite(err[took]).all()
    e64 = system.err64(out[took], values[took])
    scale = np.maximum(1.0, e64)
    y = float((np.abs(system.err32(out[took], values[took]).astype(np.float64) - e64) / scale).max())
    d = float((np.abs(err[took].astype(np.float64) - e64) / scale).max())
    print(f"{name}{label}: err at out: Y {y:.3e}, solver {d:.3e}, ratio {ratio(d, y)}")
    assert d <= RATIO * y, f"{name}{label}: err is {d:.3e} from the float64 residual at out, over {RATIO} x {y:.3e}"


def compare(label, system, values, r64, r32, result, min_rejecting=0, n_unread=0):
    """the solver's `result` for `values` against the reference's two snapshots at the same cap -> (Y, the solver's distance)"""
    cap = r64.cap
    left_out = r64.ambiguous() | r32.ambiguous()
    undecided, near_tie = r64.undecided() | r32.undecided(), r64.near_tie | r32.near_tie
    keep = ~left_out
    print(f"{label} cap {cap}: {100 * left_out.mean():.2f} % of {len(keep)} instances ambiguous ({100 * undecided.mean():.2f} % by the "
          f"decision margin or a singular value, {100 * near_tie.mean():.2f} % at a tie of a min / max), {int((r64.rejected > 0).sum())} "
          f"reject a trial (most {int(r64.rejected.max())} times), margin >= {r64.margin[keep].min():.2e}, "
          f"sigma within x{r64.sigma_gap.min():.3g}")
    assert left_out.mean() <= MAX_LEFT_OUT
    assert near_tie.mean() <= MAX_AT_A_TIE
    assert (r64.rejected > 0).sum() >= min_rejecting or cap == 1
    y = float(R.distance(r32.out, r64.out)[keep].max())
    out, err, its, ex = result
    assert np.isfinite(out[keep]).all()
    # a free variable that no constraint reads has an exactly zero Jacobian column: its step is 0, not tiny and not NaN.  (Which
    # columns these are comes from the system, not from the reference's bits: LAPACK's vectors are zero there only to rounding.)
    start, unread = values[:, system.free], system.unread_free()
    assert len(unread) == n_unread, (unread, n_unread)
    assert (out[:, unread] == start[:, unread]).all(), np.abs(out[:, unread] - start[:, unread]).max()
    assert np.abs(r64.out[:, unread] - start[:, unread]).max(initial=0.0) < 1e-13 and (r32.out[:, unread] == start[:, unread]).all()
    d = float(R.distance(out, r64.out)[keep].max())
    print(f"{label} cap {cap}: Y {y:.3e}, solver {d:.3e}, ratio {ratio(d, y)}")
    assert d <= RATIO * y, f"{label} cap {cap}: {d:.3e} from the float64 loop, over {RATIO} x {y:.3e}"
    capped = keep & (r64.exit_reason == R.EXIT_MAX_ITERATIONS) & (r32.exit_reason == R.EXIT_MAX_ITERATIONS)
    assert capped.any()
    assert (its[capped] == cap).all() and (ex[capped] == R.EXIT_MAX_ITERATIONS).all(), (its[capped], ex[capped])
    check_err(label, system, values, result, f" cap {cap}")
    return y, d


def check_capped(name, cap, solve):
    """solve(values, max_iterations) -> (out, err, iterations, exit_reason) of the solver under test"""
    case, ref = CASES[name], reference(name)
    return compare(name, ref.system, case.values, ref.f64[cap - 1], ref.f32[cap - 1], solve(case.values, cap), case.min_rejecting,
                   case.n_unread)


def check_converged(name, solve):
    """A run without a cap.  `err` is the residual at `out` whatever the trajectory was.  Where the minimum is no root the last
    trials meet an error EQUAL to the previous one: the reference accepts an equal error (lib.rs:251, err > prev_err rejects), takes
    the step and ends because nothing changed or the errors stall - as the float32 yardstick run does for every instance; a solver
    that rejects an equal error grows its damping until the retry cap instead."""
    case = CASES[name]
    result = solve(case.values)
    check_err(name, reference(name).system, case.values, result, " converged")
    if name in NO_ROOT:
        end = R.run(reference(name).system, case.values, 200, np.float32)[-1]
        own = (R.EXIT_NO_CHANGE, R.EXIT_ZERO_ERROR, R.EXIT_ZERO_DAMPING, R.EXIT_STALLED)
        assert np.isin(end.exit_reason, own).all() and (end.rejected < R.MAX_RETRIES).all()
        # ... and the case really is at the rule's boundary: the yardstick meets a trial error EQUAL to the previous one (measured:
        # in all 64 instances, 2 to 5 times each), so an input or seed that lost this would fail here, not pass for nothing
        print(f"{name} converged: {int((end.equal_trials > 0).sum())} of {len(end.equal_trials)} instances meet err == prev_err")
        assert (end.equal_trials > 0).mean() >= 0.5, end.equal_trials
        print(f"{name} converged: exits {np.bincount(result[3], minlength=7).tolist()}, yardstick {np.bincount(end.exit_reason, minlength=7).tolist()}")
        assert np.isin(result[3], own).all(), np.bincount(result[3], minlength=7)
        assert R.distance(result[0], end.out).max() < 1e-3      # the same minimum (loosely: the trajectories are long)


@functools.lru_cache(maxsize=None)
def divergent_reference(n):
    """the finite starts that are not at the root, run to cap 2"""
    values, kinds = divergent_starts(n)
    system, pick = R.System(banded_through(n)), (kinds == "far") | (kinds == "ordinary")
    return system, pick, R.run(system, values[pick], 2, np.float64)[-1], R.run(system, values[pick], 2, np.float32)[-1]


def check_divergent(n, cap, solve):
    """one batch whose instances are in different states at the same time: done at once, rejecting, running on NaN, converging"""
    values, kinds = divergent_starts(n)
    system, pick, r64, r32 = divergent_reference(n)
    result = solve(values, cap)
    out, err, its, ex = result
    at = kinds == "solution"
    assert (ex[at] == R.EXIT_ZERO_RESIDUAL).all() and (its[at] == 0).all() and (err[at] == 0).all() and (out[at] == values[at]).all()
    assert np.isnan(out[kinds == "nan"]).any(axis=1).all() and (its[kinds == "nan"] > 0).all()
    assert np.isfinite(out[pick]).all() and (its[pick] > 0).all()
    if cap == 2:
        compare(f"divergent{n}", system, values[pick], r64, r32, [x[pick] for x in result])
    else:
        check_err(f"divergent{n}", system, values[pick], [x[pick] for x in result], " cap default")
        ordinary = kinds == "ordinary"
        assert converges(system, values[ordinary], [x[ordinary] for x in result]) >= ordinary.sum() // 2     # (measured: all 20)
        # what puts the instances of a wave into different states: the far starts reject trials (back to the step while their
        # neighbours take a new Jacobian), each at its own iterations - seen by the yardstick run, so the case cannot lose it silently
        rejected = R.run(system, values[kinds == "far"], 12, np.float32)[-1].rejected
        assert (rejected > 0).sum() >= 6 and len(set(rejected.tolist())) >= 4, rejected
    return result


@functools.lru_cache(maxsize=None)
def on_backend(name, be):
    """the case's system built on `be` through a recorder of its own: the same calls in the same order as the reference's"""
    return R.System(CASES[name].build, be)


def host(name):
    s = on_backend(name, O)
    return lambda values, cap=0: U.host_solve(s.shapes, s.keys, s.free, values, max_iterations=cap, threads=8)


def host_system(build):
    s = R.System(build, O)
    return lambda values, cap=0: U.host_solve(s.shapes, s.keys, s.free, values, max_iterations=cap, threads=8)


@pytest.mark.parametrize("name,cap", CAPPED)
def test_capped_run_against_the_float64_loop(name, cap):
    check_capped(name, cap, host(name))


@pytest.mark.parametrize("name", SQUARE + NO_ROOT)
def test_converged_run(name):
    check_converged(name, host(name))


@pytest.mark.parametrize("cap", [0, 2])
@pytest.mark.parametrize("n", [7, 13, 25])
def test_starts_at_a_root_far_away_and_with_nan(n, cap):
    check_divergent(n, cap, host_system(banded_through(n)))


# ---- the reference itself -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 7, 13, 25, 49])
def test_reference_converges_where_scipy_does(n):
    """the float64 loop, run to convergence, against scipy.optimize.least_squares(method="lm") on the square banded systems: another
    implementation of the method (MINPACK) ends in the same minimum"""
    opt = pytest.importorskip("scipy.optimize")
    case = CASES[f"banded{n}"]
    system, values = reference(f"banded{n}").system, case.values[:4]
    end = R.run(system, values, 60)[-1]
    assert (end.exit_reason != R.EXIT_MAX_ITERATIONS).all() and (end.err < 1e-28).all(), (end.exit_reason, end.err)
    for i in range(len(values)):
        fun = lambda v: system.residuals(v[None, :], values[i:i + 1])[0]
        jac = lambda v: system.jacobian(v[None, :], values[i:i + 1])[1][0]
        sp = opt.least_squares(fun, values[i].astype(np.float64), jac=jac, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
        assert sp.cost < 1e-28 and np.abs(end.out[i] - sp.x).max() < 1e-12, (i, sp.cost, np.abs(end.out[i] - sp.x).max())     # measured: 3e-16


@pytest.mark.parametrize("n,rows", [(3, 3), (7, 7), (7, 10), (5, 3)])
def test_reference_first_step_of_a_linear_system_in_closed_form(n, rows):
    """r = A v + b from v = 0 with damping 1: the first step lands on -(AtA + diag(AtA))^-1 At b"""
    rng = np.random.default_rng(n * 100 + rows)
    a, b = rng.uniform(-1, 1, (rows, n)).astype(np.float32), rng.uniform(-1, 1, rows).astype(np.float32)

    def build(be):
        c = be.Context()
        vs = [c.var(i) for i in range(n)]
        shapes = []
        for i in range(rows):
            out = c.constant(float(b[i]))
            for k in range(n):
                out = c.add(out, c.mul(c.constant(float(a[i, k])), vs[k]))
            shapes.append(be.Shape(c, out))
        return shapes, list(range(n)), [True] * n

    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    ata = a64.T @ a64
    want = -np.linalg.solve(ata + np.diag(np.diag(ata)), a64.T @ b64)
    snap = R.run(R.System(build), np.zeros((1, n), np.float32), 1)[0]
    assert np.abs(snap.out[0] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert snap.iterations[0] == 1 and snap.exit_reason[0] == R.EXIT_MAX_ITERATIONS
    assert abs(snap.err[0] - ((a64 @ want + b64) ** 2).sum()) <= 1e-12


def test_reference_exits_and_diagnostics():
    """zero residual after 0 steps; a variable in no constraint does not move; a rejected trial is counted and grows the damping"""
    system = R.System(banded(7, absent=3))
    snap = R.run(system, CASES["absent_variable"].values, 3)[-1]
    assert np.abs(snap.out[:, 3] - CASES["absent_variable"].values[:, 3]).max() < 1e-13    # (LAPACK's vectors: zero to rounding)
    system = R.System(U.basic_solver)
    snap = R.run(system, np.array([[1.0, -1.0], [0.0, -1.0]], np.float32), 1)[-1]     # x + y: from x = 0, (1 + 1) delta = -1
    assert snap.exit_reason.tolist() == [R.EXIT_ZERO_RESIDUAL, R.EXIT_MAX_ITERATIONS] and snap.iterations.tolist() == [0, 1]
    assert snap.err.tolist() == [0.0, 0.25] and snap.out[:, 0].tolist() == [1.0, 0.5]
    r64 = reference("rosenbrock").f64[-1]
    assert (r64.rejected > 0).sum() >= 8 and np.isfinite(r64.margin).all()
