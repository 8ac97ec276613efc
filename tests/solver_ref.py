"""An independent reference for the constraint solver: fidget-solver's Levenberg-Marquardt loop (fidget-solver/src/lib.rs:191-289) in
plain numpy, over the expression recorder and the float64 duals of grad_f64.py.

Nothing here reads solve_lm.hpp, the host build or the oracle.  A constraint is a recorded expression; its residual and its Jacobian row
come from ONE evaluation with float64 duals that carry n_free partials.  The loop is the reference's, line by line:

    J, r at cur                                      lib.rs:227   (all r == 0: done, :230)
    JtJ = Jt J, Jtr = Jt r                           lib.rs:234-237
    A = JtJ + damping * diag(JtJ)                    lib.rs:242-243
    delta = svd(A).solve(Jtr, f32::EPSILON)          lib.rs:245-248  (numpy.linalg.svd; singular values <= EPSILON count as zero)
    err = sum f_i(cur - delta)^2                     lib.rs:250
    err > prev_err: damping *= 1.5, again            lib.rs:251-253
    otherwise: damping /= 3, cur -= delta            lib.rs:256, :265-270
    stop: nothing changed, err == 0, damping == 0, the last four errors equal      lib.rs:271-277
    prev_err = err                                   lib.rs:279

with the project's two additions (SOLVER.md): free variables are numbered in the caller's parameter order, and the loop stops after
`max_iterations` accepted steps (and after MAX_RETRIES rejected trials in a row).

Two precisions of the same function:
  float64  the reference: state, JtJ, SVD and errors in float64, from the float32 start widened exactly.
  float32  the yardstick for what honest float32 arithmetic loses: residuals and partials are the float64 ones rounded to float32, and
           everything after them (JtJ, SVD, errors, state) is numpy float32.

`run` steps a whole batch at once (the evaluations are vectorised over the instances; every instance keeps its own scalars) and keeps a
snapshot after every accepted step, so one run to the largest cap serves every smaller cap.
"""
import numpy as np

import grad_f64 as G

F32_EPS = float(np.finfo(np.float32).eps)
MAX_RETRIES = 128
EXIT_ZERO_RESIDUAL, EXIT_NO_CHANGE, EXIT_ZERO_ERROR, EXIT_ZERO_DAMPING, EXIT_STALLED, EXIT_MAX_ITERATIONS, EXIT_MAX_RETRIES = range(7)
MARGIN_MIN = 1e-3      # an instance whose closest accept / reject decision is nearer than this ...
SIGMA_BAND = 2.0       # ... or with a singular value within this factor of the EPSILON threshold is ambiguous,
TIE_TOL = 1e-4         # ... and so is one whose Jacobian was taken this near a tie of a min / max (the bound of tests/test_grad_f64.py)


def input_key(key):
    """a parameter key of solve_batch ('x' | 'y' | 'z' | int) -> the recorder's input key"""
    return "xyz".index(key) if isinstance(key, str) else ("v", int(key))


class Recording:
    """A backend (fidget_amd, oracle, or None) whose Context records: a system builder written against `be.Context()` / `be.Shape()`
    leaves its expressions on the backend and in `rec`, its residual roots in `roots`."""
    def __init__(self, be=None):
        self.be, self.rec, self.roots = be, None, []

    def Context(self):
        assert self.rec is None, "one Context per system"
        self.rec = G.Rec(self.be.Context() if self.be is not None else None)
        return self.rec

    def Shape(self, ctx, node):
        self.roots.append(node)
        return self.be.Shape(ctx.ctx, node.be) if self.be is not None else None


class System:
    """build(be) -> (shapes, keys, free_mask, ...) as the builders of solver_util.py: recorded, and built on `be` (None: recorded only)"""
    def __init__(self, build, be=None):
        r = Recording(be)
        out = build(r)
        self.shapes, self.keys, self.free = out[0], list(out[1]), np.asarray(out[2], bool)
        self.rec, self.roots = r.rec, r.roots
        self.n_free = int(self.free.sum())
        self.ins = sorted({n[1] for n in self.rec.nodes if n[0] == "in"}, key=repr)

    def unread_free(self):
        """the free variables (as columns of `out`) that no constraint reads: their Jacobian column is exactly zero"""
        free_keys = [key for key, fr in zip(self.keys, self.free) if fr]
        return [k for k, key in enumerate(free_keys) if input_key(key) not in self.ins]

    def inputs(self, cur, values, partials):
        """cur: [m, n_free] float64, values: [m, n_params] -> {input key: D}; a variable no parameter names is 0 (SOLVER.md)"""
        m, p = len(cur), self.n_free if partials else 0
        ins, gi = {k: G.D(np.zeros(m), np.zeros((m, p))) for k in self.ins}, 0
        for k, (key, fr) in enumerate(zip(self.keys, self.free)):
            d = np.zeros((m, p))
            if fr:
                if partials:
                    d[:, gi] = 1.0
                v, gi = cur[:, gi], gi + 1
            else:
                v = np.asarray(values[:, k], np.float64)
            ins[input_key(key)] = G.D(np.asarray(v, np.float64), d)
        return ins

    def jacobian(self, cur, values, tol=None):
        """-> residuals [m, n_constraints], Jacobian [m, n_constraints, n_free], float64; with `tol` also which instances have a
        constraint within tol of a tie or a step there, or beyond float32's range (grad_f64.Near)"""
        ins = self.inputs(cur, values, True)
        out = [G.evaluate(self.rec, root, ins, tol) for root in self.roots]
        r, jac = np.stack([o.v for o, _ in out], 1), np.stack([o.d for o, _ in out], 1)
        return (r, jac) if tol is None else (r, jac, np.any([near for _, near in out], axis=0))

    def residuals(self, cur, values):
        ins = self.inputs(cur, values, False)
        return np.stack([G.evaluate(self.rec, root, ins)[0].v for root in self.roots], 1)

    def err64(self, out, values):
        """the float64 squared residual at `out` ([m, n_free], widened exactly)"""
        return (self.residuals(np.asarray(out, np.float64), values) ** 2).sum(1)

    def err32(self, out, values):
        """the same sum as honest float32 arithmetic evaluates it: every operation of every constraint in float32, then squares
        added in float32 in constraint order"""
        out = np.asarray(out, np.float32)
        m = len(out)
        ins, gi = {k: np.zeros(m, np.float32) for k in self.ins}, 0
        for k, (key, fr) in enumerate(zip(self.keys, self.free)):
            if fr:
                ins[input_key(key)], gi = out[:, gi], gi + 1
            else:
                ins[input_key(key)] = np.asarray(values[:, k], np.float32)
        e = np.zeros(m, np.float32)
        for root in self.roots:
            r = eval_f32(self.rec, root, ins)
            e = e + r * r
        return e


_F32_UNARY = {"neg": np.negative, "abs": np.abs, "sqrt": np.sqrt, "square": np.square, "sin": np.sin, "cos": np.cos, "tan": np.tan,
              "asin": np.arcsin, "acos": np.arccos, "atan": np.arctan, "exp": np.exp, "ln": np.log, "floor": np.floor, "ceil": np.ceil,
              "recip": lambda a: np.float32(1) / a, "not": lambda a: (a == 0).astype(np.float32),
              "round": lambda a: np.copysign(np.floor(np.abs(a) + np.float32(0.5)), a)}
_F32_BINARY = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide, "atan2": np.arctan2,
               "min": lambda a, b: np.where(np.isnan(a) | np.isnan(b), np.float32(np.nan), np.where(a < b, a, b)),
               "max": lambda a, b: np.where(np.isnan(a) | np.isnan(b), np.float32(np.nan), np.where(a > b, a, b)),
               "compare": lambda a, b: np.where(a < b, -1, np.where(a > b, 1, np.where(a == b, 0, np.nan))).astype(np.float32),
               "mod": lambda a, b: np.where(np.fmod(a, b) < 0, np.fmod(a, b) + np.abs(b), np.fmod(a, b)),
               "and": lambda a, b: np.where(a == 0, a, b), "or": lambda a, b: np.where(a != 0, a, b)}


def eval_f32(rec, root, ins):
    """the value of a recorded node with every operation in numpy float32"""
    val, m = {}, len(next(iter(ins.values())))
    order, stack = set(), [root.i]
    while stack:
        i = stack.pop()
        if i not in order:
            order.add(i)
            stack.extend(G._operands(rec.nodes[i]))
    with np.errstate(all="ignore"):
        for i in sorted(order):
            r = rec.nodes[i]
            if r[0] == "in":
                val[i] = ins[r[1]]
            elif r[0] == "const":
                val[i] = np.full(m, r[1], np.float32)
            elif len(r) == 2:
                val[i] = np.asarray(_F32_UNARY[r[0]](val[r[1]]), np.float32)
            else:
                val[i] = np.asarray(_F32_BINARY[r[0]](val[r[1]], val[r[2]]), np.float32)
    return val[root.i]


class Snapshot:
    """the batch after `cap` accepted steps (or an earlier exit): what a solve with max_iterations = cap returns, and the diagnostics
    of the trials up to there"""
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def ambiguous(self):
        """by the loop's own two thresholds (the decision margin, a singular value near EPSILON), or by a tie of a constraint"""
        return self.undecided() | self.near_tie

    def undecided(self):
        return (self.margin < MARGIN_MIN) | (self.sigma_gap < SIGMA_BAND)


def step(jtj, jtr, damping, T):
    """delta = A+ Jtr for A = JtJ + damping * diag(JtJ), batched: the pseudo-inverse from the SVD with singular values <= f32::EPSILON
    treated as zero (nalgebra's SVD::solve(b, eps)).  -> delta, the singular values"""
    n = jtj.shape[-1]
    a = jtj + damping[:, None, None] * (jtj * np.eye(n, dtype=T))
    delta, sig = np.full(jtr.shape, np.nan, T), np.full(jtr.shape, np.nan, T)
    ok = np.isfinite(a).all(axis=(1, 2))
    if ok.any():
        u, s, vt = np.linalg.svd(a[ok])
        assert s.dtype == T
        w = np.einsum("mji,mj->mi", u, jtr[ok])     # Ut b
        with np.errstate(all="ignore"):
            w = np.where(s > T(F32_EPS), w / s, T(0))
        delta[ok], sig[ok] = np.einsum("mji,mj->mi", vt, w), s
    return delta, sig


def run(system, values, max_iterations, dtype=np.float64):
    """The loop for every row of `values` ([m, n_params] float32), to `max_iterations` accepted steps.  -> [Snapshot] for the caps
    1 .. max_iterations, each with: out [m, n_free], err, iterations, exit_reason, and per instance the number of rejected trials,
    the decision margin (the smallest |err - prev_err| / prev_err over its trials), sigma_gap (the smallest factor between a
    singular value and the EPSILON threshold, either way round) and near_tie (a Jacobian was taken within TIE_TOL of a tie or a step
    of one of its constraints, or where an intermediate value leaves float32's range: there a float32 gradient is another branch's,
    or infinite, whatever the solver does with it), and equal_trials (the number of trials whose error EQUALLED the previous one: the
    accept / reject rule's boundary, lib.rs:251)."""
    T = np.dtype(dtype).type
    values = np.asarray(values, np.float32).reshape(-1, len(system.keys))
    m, f32 = len(values), T is np.float32
    cur = values[:, system.free].astype(T)
    damping, prev_err, err_out = np.ones(m, T), np.full(m, np.inf, T), np.full(m, np.inf, T)
    err_buf = np.zeros((m, 4), T)
    iters, exit_ = np.zeros(m, np.int64), np.full(m, -1, np.int64)
    rejected, margin, sigma_gap, near_tie = np.zeros(m, np.int64), np.full(m, np.inf), np.full(m, np.inf), np.zeros(m, bool)
    equal_trials = np.zeros(m, np.int64)
    snaps = []

    def rnd(a):
        return a.astype(np.float32).astype(T) if f32 else a

    for i in range(max_iterations):
        act = np.nonzero(exit_ < 0)[0]
        if len(act):
            r, jac, near = system.jacobian(cur[act].astype(np.float64), values[act], TIE_TOL)
            near_tie[act] |= near
            r, jac = rnd(r).astype(T), rnd(jac).astype(T)
            zero = (r == 0).all(axis=1)                                  # lib.rs:230
            exit_[act[zero]] = EXIT_ZERO_RESIDUAL
            err_out[act[zero]] = 0
            act, r, jac = act[~zero], r[~zero], jac[~zero]
        if len(act):
            jtj = np.einsum("mci,mcj->mij", jac, jac)                     # lib.rs:234-237
            jtr = np.einsum("mci,mc->mi", jac, r)
            assert jtj.dtype == T and jtr.dtype == T
            delta, err = np.zeros((len(act), system.n_free), T), np.zeros(len(act), T)
            pending, retries = np.arange(len(act)), np.zeros(len(act), np.int64)
            while len(pending):                                          # lib.rs:241-259
                g = act[pending]
                d, sig = step(jtj[pending], jtr[pending], damping[g], T)
                with np.errstate(all="ignore"):
                    e = rnd(system.residuals((cur[g] - d).astype(np.float64), values[g])).astype(T)
                    e = np.cumsum(e * e, axis=1, dtype=T)[:, -1]
                    gap = np.where(np.isfinite(prev_err[g]), np.abs(e - prev_err[g]) / prev_err[g], np.inf)
                    sg = np.where(sig > 0, np.maximum(sig / F32_EPS, F32_EPS / sig), np.inf).min(axis=1)
                margin[g] = np.fmin(margin[g], gap.astype(np.float64))
                sigma_gap[g] = np.fmin(sigma_gap[g], sg.astype(np.float64))
                delta[pending], err[pending] = d, e
                rej = e > prev_err[g]
                equal_trials[g] += e == prev_err[g]
                damping[g[rej]] *= T(1.5)
                rejected[g[rej]] += 1
                retries[pending[rej]] += 1
                damping[g[~rej]] /= T(3)
                out_of_retries = rej & (retries[pending] >= MAX_RETRIES)
                exit_[g[out_of_retries]] = EXIT_MAX_RETRIES
                pending = pending[rej & ~out_of_retries]
            took = exit_[act] < 0
            act, delta, err = act[took], delta[took], err[took]
            nxt = cur[act] - delta                                       # lib.rs:265-270
            changed = (nxt != cur[act]).any(axis=1)
            cur[act] = nxt
            err_buf[act, i % 4] = err
            iters[act] += 1
            err_out[act] = err
            stalled = (err_buf[act] == err_buf[act, :1]).all(axis=1)
            reason = np.where(~changed, EXIT_NO_CHANGE, np.where(err == 0, EXIT_ZERO_ERROR, np.where(
                damping[act] == 0, EXIT_ZERO_DAMPING, np.where(stalled, EXIT_STALLED, -1))))
            exit_[act] = reason
            go = reason < 0
            prev_err[act[go]] = err[go]
        snaps.append(Snapshot(cap=i + 1, out=cur.copy(), err=err_out.copy(), iterations=iters.copy(),
                              exit_reason=np.where(exit_ < 0, EXIT_MAX_ITERATIONS, exit_), rejected=rejected.copy(),
                              margin=margin.copy(), sigma_gap=sigma_gap.copy(), near_tie=near_tie.copy(), equal_trials=equal_trials.copy()))
    return snaps


def distance(out, ref):
    """per instance: |out - ref|_inf / max(1, |ref|_inf)"""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    if ref.shape[1] == 0:
        return np.zeros(len(ref))
    return np.abs(out - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))
