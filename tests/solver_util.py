"""Shared by the solver tests and tools/solve_times.py: the host build of the constraint solver (tests/host_build/solve_host.cpp:
fidget_amd/csrc/solve_lm.hpp driven by the oracle's evaluators) and the reference's solver test systems
(fidget-solver/src/lib.rs:291-613) as builders over either backend's Context (fidget_amd or oracle)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "solve_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")
F32_EPS = float(np.finfo(np.float32).eps)

_lib = None


def host_lib():
    global _lib
    if _lib is None:
        out = os.path.join(ROOT, "tests", "host_build", "_build")
        os.makedirs(out, exist_ok=True)
        so = os.path.join(out, "libsolve_host.so")
        deps = [SRC, os.path.join(CSRC, "solve_lm.hpp")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I", CSRC, SRC,
                                   "-o", so])
        L = C.CDLL(so)
        L.fs_host_solve.restype = C.c_int
        L.fs_host_solve.argtypes = [C.c_void_p] * 6 + [C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                                       C.c_uint32] + [C.c_void_p] * 4
        _lib = L
    return _lib


def _key(k):
    if isinstance(k, str):
        return "xyz".index(k), 0
    return 3, int(k)


def host_solve(shapes, keys, free_mask, values, max_iterations=0, threads=1):
    """fhip_solve's contract on the host, with oracle shapes: (out, err, iterations, exit_reason)"""
    import oracle as O
    keys = [_key(k) for k in keys]
    if len(set((a, i if a == 3 else 0) for a, i in keys)) != len(keys):
        raise ValueError("BadVarSlice: a variable is given twice")
    free = np.ascontiguousarray(np.asarray(free_mask, bool).reshape(len(keys)), dtype=np.uint8)
    vals = np.ascontiguousarray(np.asarray(values, np.float32).reshape(-1, len(keys)))
    n_inst, n_free = vals.shape[0], int(free.sum())
    n_slots, n_out, slot_param = [], [], []
    for s in shapes:
        ns = s.var_count()
        m = [-1] * ns
        for p, (a, i) in enumerate(keys):
            slot = s.axis_index(a) if a < 3 else s.var_index(i)
            if slot >= 0:
                m[slot] = p
        n_slots.append(ns)
        n_out.append(max(s.output_count(), 1))
        slot_param += m
    ol = O.lib()
    hs = (C.c_void_p * max(len(shapes), 1))(*[s._h for s in shapes])
    a_slots, a_out = np.array(n_slots + [0], np.uint32), np.array(n_out + [0], np.uint32)
    a_sp = np.array(slot_param + [0], np.int32)
    out = np.zeros((n_inst, n_free), np.float32)
    err = np.zeros(n_inst, np.float32)
    its = np.zeros(n_inst, np.uint32)
    ex = np.zeros(n_inst, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    r = host_lib().fs_host_solve(C.cast(ol.orc_eval_grad_slice, C.c_void_p), C.cast(ol.orc_eval_point, C.c_void_p), hs, p(a_slots),
                                 p(a_out), p(a_sp), len(shapes), p(free), len(keys), p(vals), n_inst, int(max_iterations), int(threads),
                                 p(out), p(err), p(its), p(ex))
    if r == 6:
        raise ValueError("Unsupported: more than 64 free parameters")
    return out, err, its, ex


def relative_eq(a, b, epsilon=F32_EPS, max_relative=F32_EPS):
    """approx::relative_eq! for f32 (the reference's assert_relative_eq!)"""
    a, b = np.float32(a), np.float32(b)
    if a == b:
        return True
    d = abs(float(a) - float(b))
    return d <= epsilon or d <= max(abs(float(a)), abs(float(b))) * max_relative


def rand_f32(rng, *shape):
    """rand::random::<f32>(): uniform in [0, 1), 24 random bits"""
    return (rng.integers(0, 1 << 24, size=shape) / float(1 << 24)).astype(np.float32)


# ---- the reference's systems: build(be) -> (shapes, keys, free, values[n_params]) ----------------------------------------------
def _shape(be, c, node):
    return be.Shape(c, node)


def basic_solver(be):           # lib.rs:302-316
    c = be.Context()
    return [_shape(be, c, c.add(c.x(), c.y()))], ["x", "y"], [True, False], [0.0, -1.0]


def four_vars_at_once(be):      # lib.rs:318-338
    c = be.Context()
    vs = [c.var(i) for i in range(4)]
    r = vs[0]
    for v in vs[1:]:
        r = c.add(r, v)
    return [_shape(be, c, r)], [0, 1, 2, 3], [True] * 4, [0.0, 1.0, 2.0, 3.0]


def four_vars_independent(be):  # lib.rs:340-362
    c = be.Context()
    shapes = [_shape(be, c, c.sub(c.var(i), c.constant(float(i)))) for i in range(4)]
    return shapes, [0, 1, 2, 3], [True] * 4, [0.0, 2.0, 4.0, 6.0]


def xy_nonlinear(be):           # lib.rs:364-390
    c = be.Context()
    x, y = c.x(), c.y()
    a = c.sub(c.mul(c.add(c.mul(x, c.constant(2.0)), c.mul(y, c.constant(3.0))), c.sub(x, y)), c.constant(2.0))
    b = c.sub(c.add(c.mul(x, c.constant(3.0)), y), c.constant(5.0))
    return [_shape(be, c, a), _shape(be, c, b)], ["x", "y"], [True, True], [0.0, 0.0]


def one_var_no_solution(be):    # lib.rs:392-413
    c = be.Context()
    x = c.x()
    return [_shape(be, c, c.sub(x, c.constant(1.0))), _shape(be, c, c.sub(x, c.constant(2.0)))], ["x"], [True], [0.0]


def banana(start):              # lib.rs:415-446 (Rosenbrock)
    def build(be):
        c = be.Context()
        x, y = c.x(), c.y()
        a = c.sub(c.constant(1.0), x)
        b = c.mul(c.constant(100.0), c.sub(y, c.square(x)))
        return [_shape(be, c, a), _shape(be, c, b)], ["x", "y"], [True, True], list(start)
    return build


def circle(start):              # lib.rs:448-471
    def build(be):
        c = be.Context()
        x, y = c.x(), c.y()
        return [_shape(be, c, c.sqrt(c.add(c.square(x), c.square(y))))], ["x", "y"], [True, True], list(start)
    return build


def linear_system(be, n):
    """one_linear (lib.rs:473-518) with the matrix and right-hand side as FIXED parameters, so that one set of tapes serves every
    draw: params 0..n-1 are the free unknowns (start 0), then the n x n matrix row major, then the n right-hand sides (Var::V
    indices in the same order).  Constraint row: -sol[row] + sum_col mat[row, col] * v_col, in the reference's order."""
    c = be.Context()
    vs = [c.var(i) for i in range(n)]
    shapes = []
    for row in range(n):
        out = c.neg(c.var(n + n * n + row))
        for col in range(n):
            out = c.add(out, c.mul(c.var(n + row * n + col), vs[col]))
        shapes.append(_shape(be, c, out))
    keys = list(range(n + n * n + n))
    return shapes, keys, [True] * n + [False] * (n * n + n)


def linear_draws(rng, n, count):
    """count draws of (values, matrix, sol = matrix @ values) as rows of fhip_solve values (free starts 0)"""
    rows, mats, sols = [], [], []
    for _ in range(count):
        vals = rand_f32(rng, n)
        mat = rand_f32(rng, n, n)
        sol = mat_vec(mat, vals)
        rows.append(np.concatenate([np.zeros(n, np.float32), mat.reshape(-1), sol]))
        mats.append(mat)
        sols.append(sol)
    return np.array(rows, np.float32), mats, sols


def mat_vec(mat, v):
    """f32 matrix * vector, accumulated column by column in f32"""
    out = np.zeros(mat.shape[0], np.float32)
    for k in range(mat.shape[1]):
        out = (out + mat[:, k] * np.float32(v[k])).astype(np.float32)
    return out


def linear_ok(mat, sol, x):     # lib.rs:507-517
    sol2 = mat_vec(mat, np.asarray(x, np.float32))
    err = float(np.sum((sol.astype(np.float64) - sol2) ** 2))
    return err < 1e-3 and all(relative_eq(a, b, epsilon=1e-2) for a, b in zip(sol, sol2))


def quadratic_system(be, n):
    """one_quadratic (lib.rs:541-613) with the n x (n*n + n) matrix and the right-hand side as FIXED parameters: params 0..n-1 free
    (start 0.5), then the matrix row major, then the n right-hand sides"""
    m = n * n + n
    c = be.Context()
    vs = [c.var(i) for i in range(n)]
    shapes = []
    for row in range(n):
        out = c.neg(c.var(n + n * m + row))
        for col in range(n):
            out = c.add(out, c.mul(c.var(n + row * m + col), vs[col]))
        for i in range(n):
            for j in range(n):
                out = c.add(out, c.mul(c.mul(c.var(n + row * m + i * n + j + n), vs[i]), vs[j]))
        shapes.append(_shape(be, c, out))
    return shapes, list(range(n + n * m + n)), [True] * n + [False] * (n * m + n)


def quadratic_col(x):
    n = len(x)
    col = np.zeros(n * n + n, np.float32)
    col[:n] = x
    for i in range(n):
        for j in range(n):
            col[i * n + j + n] = np.float32(x[i]) * np.float32(x[j])
    return col


def quadratic_draws(rng, n, count):
    rows, mats, sols = [], [], []
    for _ in range(count):
        vals = rand_f32(rng, n)
        mat = rand_f32(rng, n, n * n + n)
        sol = mat_vec(mat, quadratic_col(vals))
        rows.append(np.concatenate([np.full(n, 0.5, np.float32), mat.reshape(-1), sol]))
        mats.append(mat)
        sols.append(sol)
    return np.array(rows, np.float32), mats, sols


def quadratic_ok(mat, sol, x):  # lib.rs:595-612
    return linear_ok(mat, sol, quadratic_col(np.asarray(x, np.float32)))


def trans_system(be):
    """sin, cos, exp, ln (the device's restated libm routines) and min / max (the gradient picked by value)"""
    c = be.Context()
    x, y = c.x(), c.y()
    a = c.sub(c.add(c.sin(x), c.cos(c.mul(y, c.constant(0.7)))), c.constant(0.5))
    b = c.sub(c.add(c.exp(c.mul(x, c.constant(0.3))), c.ln(c.add(c.square(y), c.constant(1.5)))), c.constant(2.0))
    m = c.sub(c.max(c.min(x, c.mul(y, c.constant(0.5))), c.sub(y, c.constant(3.0))), c.constant(0.25))
    return [_shape(be, c, a), _shape(be, c, b), _shape(be, c, m)], ["x", "y"], [True, True]


KATS = {"basic_solver": basic_solver, "four_vars_at_once": four_vars_at_once, "four_vars_independent": four_vars_independent,
        "xy_nonlinear": xy_nonlinear, "one_var_no_solution": one_var_no_solution, "banana_0": banana((0.0, 0.0)),
        "banana_1": banana((1.0, 1.0)), "circle_0": circle((0.0, 0.0)), "circle_1": circle((1.0, 1.5))}


def kat_check(name, out):
    """the reference's assertions on a KAT's free values (parameter order)"""
    if name == "basic_solver":
        return relative_eq(out[0], 1.0)
    if name == "four_vars_at_once":
        s = np.float32(0.0)
        for v in out:
            s = np.float32(s + np.float32(v))
        return relative_eq(s, 0.0)
    if name == "four_vars_independent":
        return all(relative_eq(float(i), out[i]) for i in range(4))
    if name == "xy_nonlinear":
        x, y = np.float32(out[0]), np.float32(out[1])
        return relative_eq((x * np.float32(2) + y * np.float32(3)) * (x - y), 2.0) and relative_eq(x * np.float32(3) + y, 5.0)
    if name == "one_var_no_solution":
        return relative_eq(out[0], 1.5)
    if name.startswith("banana"):
        return relative_eq(out[0], 1.0) and relative_eq(out[1], 1.0)
    if name.startswith("circle"):
        return relative_eq(out[0], 0.0) and relative_eq(out[1], 0.0)
    raise KeyError(name)


# ---- forms for device tapes, which read at most 16 input variables each (FH_MAX_INPUTS) ------------------------------------------
def linear_const(be, mat, sol):
    """one_linear's constraints with the matrix and right-hand side as constants (lib.rs:495-503): params 0..n-1, start 0"""
    n = len(sol)
    c = be.Context()
    vs = [c.var(i) for i in range(n)]
    shapes = []
    for row in range(n):
        out = c.constant(float(-sol[row]))
        for col in range(n):
            out = c.add(out, c.mul(c.constant(float(mat[row, col])), vs[col]))
        shapes.append(_shape(be, c, out))
    return shapes, list(range(n)), [True] * n, [0.0] * n


def quadratic_const(be, mat, sol):
    """one_quadratic's constraints with constants (lib.rs:571-588): params 0..n-1, start 0.5"""
    n = len(sol)
    c = be.Context()
    vs = [c.var(i) for i in range(n)]
    shapes = []
    for row in range(n):
        out = c.constant(float(-sol[row]))
        for col in range(n):
            out = c.add(out, c.mul(c.constant(float(mat[row, col])), vs[col]))
        for i in range(n):
            for j in range(n):
                out = c.add(out, c.mul(c.mul(c.constant(float(mat[row, i * n + j + n])), vs[i]), vs[j]))
        shapes.append(_shape(be, c, out))
    return shapes, list(range(n)), [True] * n, [0.5] * n


def banded_system(be, n):
    """n free variables, n constraints of at most three each: v_i + 0.5 v_{i+1} - 0.25 v_{i+2} - (i + 1) / n, as FIXED coefficients
    would exceed a device tape's inputs; starts are the instance's values"""
    c = be.Context()
    shapes = []
    for i in range(n):
        out = c.var(i)
        if i + 1 < n:
            out = c.add(out, c.mul(c.constant(0.5), c.var(i + 1)))
        if i + 2 < n:
            out = c.sub(out, c.mul(c.constant(0.25), c.var(i + 2)))
        shapes.append(_shape(be, c, c.sub(out, c.constant((i + 1) / n))))
    return shapes, list(range(n)), [True] * n
