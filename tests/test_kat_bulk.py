"""Point / bulk-f32 / bulk-gradient known-answer tests, ported from the
reference's conformance suite:
  /root/reference/fidget-core/src/eval/test/point.rs
  /root/reference/fidget-core/src/eval/test/float_slice.rs
  /root/reference/fidget-core/src/eval/test/grad_slice.rs
Each test names the lines it restates.  Oracle on CPU; HIP backend with -m gpu.

The gradient sweeps (test_g_unary, test_g_binary) hold every opcode to two independent criteria: the reference's own finite-difference
check, unchanged, and value and partials within K ulp of the float64 duals of grad_f64.py (K derived below from the roundings of each rule).
"""
import math

import numpy as np
import pytest

import grad_f64 as G64
from kat_util import (BINARY_DEFS, NAN, UNARY_DEFS, build_stress_fn, f32, f_mix, f_rand, libm, same, spicy_args)

L, R, B = 1, 2, 3
TRANSCENDENTAL = {"sin", "cos", "tan", "asin", "acos", "atan", "exp", "ln", "atan2"}


def ulp_close(a, b, ulps):
    if same(a, b):
        return True
    if math.isnan(a) or math.isnan(b) or math.isinf(a) or math.isinf(b):
        return False
    return abs(a - b) <= ulps * float(np.spacing(np.float32(abs(b))))


def value_ok(be, name, got, want):
    """Exact for every opcode on every backend: the transcendental opcodes are the host libm's routines restated
    (trans_libm.hpp), the reference's own bar (`o == v`, eval/test/float_slice.rs:404-412)."""
    return same(got, want)


def pt(shape, x=0.0, y=0.0, z=0.0):
    return shape.eval_point(x, y, z)


# ---- point.rs ---------------------------------------------------------------
def test_constant(be):  # point.rs:26-33
    ctx = be.Context()
    s = be.Shape(ctx, ctx.constant(1.5))
    assert s.eval_point_raw([])[0][0] == 1.5


def test_constant_push(be):  # point.rs:35-57
    ctx = be.Context()
    s = be.Shape(ctx, ctx.min(1.5, ctx.x()))
    r, trace = pt(s, 2.0)
    assert r == 1.5 and trace is not None
    nxt = s.simplify(trace)
    assert nxt.size() == 2  # constant, output
    assert nxt.eval_point_raw([2.0])[0][0] == 1.5
    assert nxt.eval_point_raw([1.0])[0][0] == 1.5
    with pytest.raises(ValueError):
        nxt.eval_point_raw([])  # vars are inherited from the parent (BadVarSlice)


def test_circle(be):  # point.rs:59-73
    ctx = be.Context()
    x, y = ctx.x(), ctx.y()
    c = ctx.sub(ctx.add(ctx.mul(x, x), ctx.mul(y, y)), 1.0)
    s = be.Shape(ctx, c)
    assert pt(s, 0.0, 0.0)[0] == -1.0
    assert pt(s, 1.0, 0.0)[0] == 0.0


def test_p_min_max(be):  # point.rs:75-137
    ctx = be.Context()
    x, y = ctx.x(), ctx.y()
    s = be.Shape(ctx, ctx.min(x, y))
    r, t = pt(s, 0.0, 0.0)
    assert r == 0.0 and t is None
    r, t = pt(s, 0.0, 1.0)
    assert r == 0.0 and list(t) == [L]
    r, t = pt(s, 2.0, 0.0)
    assert r == 0.0 and list(t) == [R]
    r, t = pt(s, NAN, 0.0)
    assert math.isnan(r) and t is None
    r, t = pt(s, 0.0, NAN)
    assert math.isnan(r) and t is None
    s = be.Shape(ctx, ctx.max(x, y))
    r, t = pt(s, 0.0, 0.0)
    assert r == 0.0 and t is None
    r, t = pt(s, 0.0, 1.0)
    assert r == 1.0 and list(t) == [R]
    r, t = pt(s, 2.0, 0.0)
    assert r == 2.0 and list(t) == [L]
    r, t = pt(s, NAN, 0.0)
    assert math.isnan(r) and t is None
    r, t = pt(s, 0.0, NAN)
    assert math.isnan(r) and t is None


def test_p_and_or(be):  # point.rs:139-209
    ctx = be.Context()
    x, y = ctx.x(), ctx.y()
    s = be.Shape(ctx, ctx.and_(x, y))
    for (a, b), (want, ch) in [((0.0, 0.0), (0.0, L)), ((0.0, 1.0), (0.0, L)), ((0.0, NAN), (0.0, L)),
                               ((f32(0.1), 1.0), (1.0, R)), ((f32(0.1), 0.0), (0.0, R)),
                               ((NAN, f32(1.2)), (f32(1.2), R))]:
        r, t = pt(s, a, b)
        assert r == want and list(t) == [ch]
    s = be.Shape(ctx, ctx.or_(x, y))
    for (a, b), (want, ch) in [((0.0, 0.0), (0.0, R)), ((0.0, 1.0), (1.0, R)), ((0.0, NAN), (NAN, R)),
                               ((f32(0.1), 1.0), (f32(0.1), L)), ((f32(0.1), 0.0), (f32(0.1), L)),
                               ((NAN, f32(1.2)), (NAN, L))]:
        r, t = pt(s, a, b)
        assert same(r, want) and list(t) == [ch]


def test_p_sin(be):  # point.rs:211-245
    ctx = be.Context()
    x = ctx.x()
    sn = ctx.sin(x)
    s = be.Shape(ctx, sn)
    for v in [0.0, 1.0, 2.0]:
        r, t = pt(s, v)
        assert value_ok(be, "sin", r, libm("sinf", v)) and t is None
    s = be.Shape(ctx, ctx.add(sn, ctx.y()))
    for a, b in [(0.0, 1.0), (1.0, 3.0), (2.0, 8.0)]:
        r, t = pt(s, a, b)
        assert ulp_close(r, f32(np.float32(libm("sinf", a)) + np.float32(b)), 0)
        assert t is None


def test_basic_interpreter(be):  # point.rs:247-260
    ctx = be.Context()
    x, y = ctx.x(), ctx.y()
    s = be.Shape(ctx, ctx.min(ctx.add(x, 1.0), y))
    assert pt(s, 1.0, 2.0)[0] == 2.0
    assert pt(s, 1.0, 3.0)[0] == 2.0
    assert pt(s, 3.0, 3.5)[0] == 3.5


def test_push(be):  # point.rs:262-327
    ctx = be.Context()
    x, y = ctx.x(), ctx.y()
    s = be.Shape(ctx, ctx.min(x, y))
    assert pt(s, 1.0, 2.0)[0] == 1.0
    assert pt(s, 3.0, 2.0)[0] == 2.0
    n = s.simplify([L])
    assert pt(n, 1.0, 2.0)[0] == 1.0
    assert pt(n, 3.0, 2.0)[0] == 3.0
    n = s.simplify([R])
    assert pt(n, 1.0, 2.0)[0] == 2.0
    assert pt(n, 3.0, 2.0)[0] == 2.0
    s = be.Shape(ctx, ctx.min(x, 1.0))
    assert pt(s, 0.5)[0] == 0.5
    assert pt(s, 3.0)[0] == 1.0
    n = s.simplify([L])
    assert pt(n, 0.5)[0] == 0.5
    assert pt(n, 3.0)[0] == 3.0
    n = s.simplify([R])
    assert pt(n, 0.5)[0] == 1.0
    assert pt(n, 3.0)[0] == 1.0
    with pytest.raises(ValueError):
        s.simplify([L, R])  # BadChoiceSlice (vm/data.rs:129-134)


def test_basic(be):  # point.rs:329-354
    ctx = be.Context()
    x, y = ctx.x(), ctx.y()
    assert pt(be.Shape(ctx, x), 1.0)[0] == 1.0
    assert pt(be.Shape(ctx, y), y=4.0)[0] == 4.0
    s = be.Shape(ctx, ctx.add(x, ctx.mul(y, 2.5)))
    assert pt(s, 1.0, 2.0)[0] == 6.0


def test_p_rand_mix(be):  # point.rs:445-548
    ctx = be.Context()
    a, b = ctx.x(), ctx.y()
    s = be.Shape(ctx, ctx.rand(a))
    for v in [0.0, 1.0, 2.0, f32(math.pi / 2)]:
        assert pt(s, v)[0] == f_rand(v)
    s = be.Shape(ctx, ctx.mix(a, b))
    assert pt(s, 0.0, 2.0)[0] == f_mix(0.0, 2.0)
    s = be.Shape(ctx, ctx.mix(a, 5.0))
    assert pt(s, 1.0)[0] == f_mix(1.0, 5.0)
    s = be.Shape(ctx, ctx.mix(5.0, a))
    assert pt(s, 1.0)[0] == f_mix(5.0, 1.0)


@pytest.mark.parametrize("n", [4, 8, 12, 16, 32, 256, 512])
def test_p_f_stress(be, oracle_mod, n):  # point.rs:389-443, float_slice.rs:265-316
    args = [f32(np.float32(i) / np.float32(32)) for i in range(32)]
    x, y, z = args, args[1:] + args[:1], args[2:] + args[:2]
    ctx, node = build_stress_fn(be, n)
    s = be.Shape(ctx, node)
    out = s.eval_float_slice(x, y, z)
    octx, onode = build_stress_fn(oracle_mod, n)
    ref = oracle_mod.Shape(octx, onode).eval_float_slice(x, y, z)
    for i in range(32):
        q = octx.eval_xyz(onode, x[i], y[i], z[i])
        assert abs(out[i] - q) < 1e-2
        assert out[i] == ref[i]  # `a == b` vs VmShape, on every backend
    if n <= 32:
        for i in range(0, 32, 5):
            assert ulp_close(pt(s, x[i], y[i], z[i])[0], float(out[i]), 0)


# ---- float_slice.rs ---------------------------------------------------------
def test_vectorized(be):  # float_slice.rs:48-93
    ctx = be.Context()
    x, y = ctx.x(), ctx.y()
    s = be.Shape(ctx, x)
    for n in (4, 8, 9):
        a = np.arange(n, dtype=np.float32)
        assert list(s.eval_float_slice(a, a * 0, a * 0)) == list(a)
    s = be.Shape(ctx, ctx.mul(y, 2.0))
    assert list(s.eval_float_slice([0] * 4, [3, 2, 1, 0], [0] * 4)) == [6, 4, 2, 0]
    assert list(s.eval_float_slice([0] * 3, [1, 4, 8], [0] * 3)) == [2, 8, 16]
    assert list(s.eval_float_slice([0] * 7, [1, 4, 4, -1, -2, -3, 0], [0] * 7)) == [2, 8, 8, -2, -4, -6, 0]


def test_f_sin_rand_mix(be):  # float_slice.rs:95-187
    ctx = be.Context()
    a, b = ctx.x(), ctx.y()
    args = [0.0, 1.0, 2.0, f32(math.pi / 2)]
    zeros = [0.0] * 4
    out = be.Shape(ctx, ctx.sin(a)).eval_float_slice(args, zeros, zeros)
    assert all(value_ok(be, "sin", float(o), libm("sinf", v)) for o, v in zip(out, args))
    out = be.Shape(ctx, ctx.rand(a)).eval_float_slice(args, zeros, zeros)
    assert [float(o) for o in out] == [f_rand(v) for v in args]
    out = be.Shape(ctx, ctx.mix(a, b)).eval_float_slice([2.0, 3.0], [0.0, 1.0], [0, 0])
    assert [float(o) for o in out] == [f_mix(2.0, 0.0), f_mix(3.0, 1.0)]
    out = be.Shape(ctx, ctx.mix(a, 5.0)).eval_float_slice([0.0, 1.0], [0, 0], [0, 0])
    assert [float(o) for o in out] == [f_mix(0.0, 5.0), f_mix(1.0, 5.0)]
    out = be.Shape(ctx, ctx.mix(5.0, a)).eval_float_slice([0.0, 1.0], [0, 0], [0, 0])
    assert [float(o) for o in out] == [f_mix(5.0, 0.0), f_mix(5.0, 1.0)]
    out = be.Shape(ctx, ctx.mix(a, NAN)).eval_float_slice([0.0, 1.0], [0, 0], [0, 0])
    assert all(same(float(o), f_mix(v, NAN)) for o, v in zip(out, [0.0, 1.0]))


def test_f_shape_var(be):  # float_slice.rs:189-263 (argument-shape errors)
    ctx = be.Context()
    v = 0xABCDEF
    a = ctx.add(ctx.add(ctx.x(), ctx.y()), ctx.var(v))
    s = be.Shape(ctx, a)
    out = s.eval_float_slice([1.0, 2.0], [2.0, 3.0], [0.0, 0.0], extra={v: np.array([4.0, 5.0], np.float32)})
    assert list(out) == [7.0, 10.0]
    with pytest.raises(ValueError):  # too few variable slices -> BadVarSlice (var/mod.rs:167-197)
        s.eval_float_slice_raw([np.zeros(2, np.float32)])
    with pytest.raises(ValueError):  # MismatchedSlices
        s.eval_float_slice_raw([np.zeros(2, np.float32), np.zeros(3, np.float32), np.zeros(2, np.float32)])
    # extra variables are fine
    vs = [np.zeros(2, np.float32)] * 5
    s.eval_float_slice_raw(vs)


def test_f_multiple_outputs(be):  # float_slice.rs:318-383
    ctx = be.Context()
    s = be.Shape(ctx, roots=[ctx.x(), ctx.y(), ctx.z()])
    vs = [None] * 3
    for axis, val in enumerate([0.0, 1.0, 2.0]):
        vs[s.axis_index(axis)] = np.full(8, val, np.float32)
    out = s.eval_float_slice_raw(vs)
    assert (out[0] == 0).all() and (out[1] == 1).all() and (out[2] == 2).all()
    s = be.Shape(ctx, roots=[ctx.x(), ctx.constant(4.0), ctx.constant(5.0)])
    out = s.eval_float_slice_raw([np.zeros(8, np.float32)])
    assert (out[0] == 0).all() and (out[1] == 4).all() and (out[2] == 5).all()


@pytest.mark.parametrize("name", list(UNARY_DEFS))
def test_f_unary(be, name):  # float_slice.rs:391-413
    args = spicy_args()
    ctx = be.Context()
    v = ctx.var(9)
    s = be.Shape(ctx, getattr(ctx, name)(v))
    out = s.eval_float_slice_raw([np.array(args, np.float32)])[0]
    for a, o in zip(args, out):
        assert value_ok(be, name, float(o), UNARY_DEFS[name](a)), f"{name} at {a}: {UNARY_DEFS[name](a)} != {o}"
    # the tracing point evaluator shares the definition (point.rs:550-592)
    for a in args[::7]:
        r, t = s.eval_point_raw([a])
        assert value_ok(be, name, float(r[0]), UNARY_DEFS[name](a)) and t is None


@pytest.mark.parametrize("name", list(BINARY_DEFS))
def test_f_binary(be, name):  # float_slice.rs:415-533
    args = spicy_args()
    fn = BINARY_DEFS[name]
    ctx = be.Context()
    va, vb = ctx.var(1), ctx.var(2)
    s = be.Shape(ctx, getattr(ctx, name)(va, vb))
    ia, ib = s.var_index(1), s.var_index(2)
    for rot in range(0, len(args), 3):
        rgsa = args[rot:] + args[:rot]
        vs = [None, None]
        vs[ia], vs[ib] = np.array(args, np.float32), np.array(rgsa, np.float32)
        out = s.eval_float_slice_raw(vs)[0]
        for a, b, o in zip(args, rgsa, out):
            assert value_ok(be, name, float(o), fn(a, b)), f"{name}(reg,reg) at {a} {b}: {fn(a, b)} != {o}"
    for imm in args[::5]:
        for imm_first in (False, True):
            ctx = be.Context()
            v = ctx.var(1)
            node = getattr(ctx, name)(imm, v) if imm_first else getattr(ctx, name)(v, imm)
            s = be.Shape(ctx, node)
            if s.var_count() == 0:
                continue  # constant-folded
            out = s.eval_float_slice_raw([np.array(args, np.float32)])[0]
            for a, o in zip(args, out):
                want = fn(imm, a) if imm_first else fn(a, imm)
                assert value_ok(be, name, float(o), want) or (math.isnan(want) and s.ssa_len() <= 2), \
                    f"{name}({'imm,reg' if imm_first else 'reg,imm'}) at {a} imm {imm}: {want} != {o}"


# ---- grad_slice.rs ----------------------------------------------------------
def g(shape, x, y=None, z=None):
    n = len(x)
    y = [0.0] * n if y is None else y
    z = [0.0] * n if z is None else z
    return [tuple(float(v) for v in row) for row in shape.eval_grad_slice(x, y, z)]


def test_g_xyz(be):  # grad_slice.rs:54-88
    ctx = be.Context()
    assert g(be.Shape(ctx, ctx.x()), [2.0], [3.0], [4.0])[0] == (2.0, 1.0, 0.0, 0.0)
    assert g(be.Shape(ctx, ctx.y()), [2.0], [3.0], [4.0])[0] == (3.0, 0.0, 1.0, 0.0)
    assert g(be.Shape(ctx, ctx.z()), [2.0], [3.0], [4.0])[0] == (4.0, 0.0, 0.0, 1.0)


def test_g_square_abs_sqrt(be):  # grad_slice.rs:90-147
    ctx = be.Context()
    x = ctx.x()
    s = be.Shape(ctx, ctx.square(x))
    assert g(s, [0.0])[0] == (0, 0, 0, 0)
    assert g(s, [1.0])[0] == (1, 2, 0, 0)
    assert g(s, [2.0])[0] == (4, 4, 0, 0)
    assert g(s, [3.0])[0] == (9, 6, 0, 0)
    s = be.Shape(ctx, ctx.abs(x))
    assert g(s, [2.0])[0] == (2, 1, 0, 0)
    assert g(s, [-2.0])[0] == (2, -1, 0, 0)
    s = be.Shape(ctx, ctx.sqrt(x))
    assert g(s, [1.0])[0] == (1, 0.5, 0, 0)
    assert g(s, [4.0])[0] == (2, 0.25, 0, 0)


def test_g_sin(be):  # grad_slice.rs:149-170 (compare_eq: 1e-6)
    ctx = be.Context()
    x = ctx.x()
    v = g(be.Shape(ctx, ctx.sin(x)), [1.0, 2.0, 3.0])
    for got, a in zip(v, [1.0, 2.0, 3.0]):
        want = (math.sin(a), math.cos(a), 0, 0)
        assert max(abs(p - q) for p, q in zip(got, want)) < 1e-6
    y = ctx.mul(ctx.y(), 2.0)
    v = g(be.Shape(ctx, ctx.sin(y)), [0.0] * 3, [1.0, 2.0, 3.0])
    for got, a in zip(v, [2.0, 4.0, 6.0]):
        want = (math.sin(a), 0, 2 * math.cos(a), 0)
        assert max(abs(p - q) for p, q in zip(got, want)) < 1e-6


def test_g_mul_div_recip(be):  # grad_slice.rs:172-226
    ctx = be.Context()
    x, y = ctx.x(), ctx.y()
    s = be.Shape(ctx, ctx.mul(x, y))
    assert g(s, [1.0], [0.0])[0] == (0, 0, 1, 0)
    assert g(s, [0.0], [1.0])[0] == (0, 1, 0, 0)
    assert g(s, [4.0], [1.0])[0] == (4, 1, 4, 0)
    assert g(s, [4.0], [2.0])[0] == (8, 2, 4, 0)
    assert g(be.Shape(ctx, ctx.div(x, 2.0)), [1.0])[0] == (0.5, 0.5, 0, 0)
    s = be.Shape(ctx, ctx.recip(x))
    assert g(s, [1.0])[0] == (1, -1, 0, 0)
    assert g(s, [2.0])[0] == (0.5, -0.25, 0, 0)


def test_g_min_max(be):  # grad_slice.rs:228-286
    ctx = be.Context()
    x, y, z = ctx.x(), ctx.y(), ctx.z()
    mn = ctx.min(x, y)
    s = be.Shape(ctx, mn)
    assert g(s, [2.0], [3.0])[0] == (2, 1, 0, 0)
    assert g(s, [4.0], [3.0])[0] == (3, 0, 1, 0)
    s = be.Shape(ctx, ctx.max(mn, z))
    assert g(s, [2.0], [3.0], [0.0])[0] == (2, 1, 0, 0)
    assert g(s, [4.0], [3.0], [0.0])[0] == (3, 0, 1, 0)
    assert g(s, [4.0], [3.0], [5.0])[0] == (5, 0, 0, 1)
    s = be.Shape(ctx, ctx.max(x, y))
    assert g(s, [2.0], [3.0])[0] == (3, 0, 1, 0)
    assert g(s, [4.0], [3.0])[0] == (4, 1, 0, 0)


def test_g_add_not_rand_mix(be):  # grad_slice.rs:288-390
    ctx = be.Context()
    a, b = ctx.x(), ctx.y()
    s = be.Shape(ctx, ctx.add(a, b))
    vs = [None, None]
    vs[s.axis_index(0)] = np.array([[0, 0, 0, 0], [1, 0, 0, 0]], np.float32)
    vs[s.axis_index(1)] = np.array([[2, 0, 0, 0], [3, 0, 0, 0]], np.float32)
    out = s.eval_grad_slice_raw(vs)[0]
    assert [tuple(r) for r in out] == [(2, 0, 0, 0), (4, 0, 0, 0)]
    assert g(be.Shape(ctx, ctx.not_(a)), [0.0])[0] == (1, 0, 0, 0)
    args = [0.0, 1.0, 2.0, f32(math.pi / 2)]
    out = g(be.Shape(ctx, ctx.rand(a)), args)
    assert out == [(f_rand(v), 0, 0, 0) for v in args]
    out = g(be.Shape(ctx, ctx.mix(a, b)), [2.0, 3.0], [0.0, 1.0])
    assert out == [(f_mix(2.0, 0.0), 0, 0, 0), (f_mix(3.0, 1.0), 0, 0, 0)]
    out = g(be.Shape(ctx, ctx.mix(a, 5.0)), [0.0, 1.0])
    assert out == [(f_mix(0.0, 5.0), 0, 0, 0), (f_mix(1.0, 5.0), 0, 0, 0)]
    out = g(be.Shape(ctx, ctx.mix(5.0, a)), [0.0, 1.0])
    assert out == [(f_mix(5.0, 0.0), 0, 0, 0), (f_mix(5.0, 1.0), 0, 0, 0)]


def test_g_circle_modulo(be):  # grad_slice.rs:392-445
    ctx = be.Context()
    x, y = ctx.x(), ctx.y()
    c = ctx.sub(ctx.sqrt(ctx.add(ctx.square(x), ctx.square(y))), 0.5)
    s = be.Shape(ctx, c)
    assert g(s, [1.0], [0.0])[0] == (0.5, 1, 0, 0)
    assert g(s, [0.0], [1.0])[0] == (0.5, 0, 1, 0)
    assert g(s, [2.0], [0.0])[0] == (1.5, 1, 0, 0)
    assert g(s, [0.0], [2.0])[0] == (1.5, 0, 1, 0)
    s = be.Shape(ctx, ctx.sub(y, ctx.modulo(x, 1.0)))
    assert g(s, [0.0], [0.5])[0] == (0.5, -1, 1, 0)
    assert g(s, [f32(-0.01)], [0.5])[0] == (f32(np.float32(0.5) - np.float32(rem(f32(-0.01)))), -1, 1, 0)
    assert g(s, [f32(0.01)], [0.5])[0] == (f32(np.float32(0.5) - np.float32(f32(0.01))), -1, 1, 0)


def rem(a):
    from kat_util import rem_euclid
    return rem_euclid(a, 1.0)


@pytest.mark.parametrize("n", [4, 8, 12, 16, 32])
def test_g_stress(be, oracle_mod, n):  # grad_slice.rs:447-493
    args = [f32(np.float32(i) / np.float32(32)) for i in range(32)]
    x, y, z = args, args[1:] + args[:1], args[2:] + args[:2]
    ctx, node = build_stress_fn(be, n)
    out = be.Shape(ctx, node).eval_grad_slice(x, y, z)
    octx, onode = build_stress_fn(oracle_mod, n)
    ref = oracle_mod.Shape(octx, onode).eval_grad_slice(x, y, z)
    assert np.abs(out - ref).max() < 1e-6 * max(1.0, float(n))  # compare_eq, scaled by the gradient magnitude


# ---- g_unary / g_binary: grad_slice.rs:495-778 -------------------------------
# K: how many float32 ulp the value and a partial may lie from the float64 reference, per opcode and operand form.
#
# Each float32 operation rounds once: a relative error of at most 2^-24, which is less than one ulp of whatever the result later becomes.
# A libm routine counts one more (glibc's float routines are within 1 ulp).  So K = the number of float32 roundings on the way to the
# number, + 1 per libm call - counting every operation of the rule as the reference writes it, also those that happen to be exact here.
# With unit seeds at most one term of a rule's numerator is non-zero (or, when both operands are the same axis, the two cancel or add
# exactly), so no cancellation slack is part of any K.  Two rules square or difference an already-rounded number and are conditioned:
#   tan        d / cos(v)^2: cosf (1), squared (its error twice) + the product (1) + the quotient (1)            -> 4
#   asin, acos d / sqrt(1 - v*v): the product's rounding (1) is magnified by c = v^2 / (1 - v^2) in the difference, which rounds (1);
#              the root halves both and rounds (1); the quotient (1)                                             -> 2.5 + c/2, rounded up
K_UNARY = {  # name: (value, partial)
    "neg": (0, 0), "abs": (0, 0),              # sign changes and selection: exact
    "recip": (1, 5),                           # 1/v; (v*0 - 1*1) / (v*v): two products, a difference, a product, a quotient (vm/mod.rs:1127-1132)
    "sqrt": (1, 3),                            # sqrtf; d / (2 * s): the root, a product, a quotient
    "square": (1, 3),                          # v*v; v*d + v*d: two products and a sum (vm/mod.rs:1138-1143)
    "sin": (1, 2), "cos": (1, 2),              # libm; d * cosf(v), d * -sinf(v): libm and a product
    "tan": (1, 4),
    "asin": (1, None), "acos": (1, None),      # None: k_asin(v) below
    "atan": (1, 3),                            # libm; d / (v*v + 1): a product, a sum, a quotient
    "exp": (1, 2),                             # libm; expf(v) * d
    "ln": (1, 1),                              # libm; d / v
    "floor": (0, 0), "ceil": (0, 0), "round": (0, 0), "not_": (0, 0), "rand": (0, 0),   # exact values, partials 0
}
K_BINARY = {  # name: {form: (value, partial)}; forms "rr", "ri" (reg, imm), "ir" (imm, reg)
    "add": (1, 1), "sub": (1, 1),              # one sum / difference each
    "mul": {"rr": (1, 3), "ri": (1, 1), "ir": (1, 1)},   # a*b' + b*a': two products and a sum; by an immediate: d * imm (vm/mod.rs:1219-1223)
    "div": (1, 5),                             # (b*a' - a*b') / (b*b): two products, a difference, a product, a quotient
    "atan2": (1, 7),                           # libm; (x*y' - y*x') / (x*x + y*y): 2 + 1 in the numerator, 2 + 1 in the denominator, a quotient
    "modulo": (1, 2),                          # fmodf is exact, + |b| rounds; a' - b' * e: a product and a difference
    "min": (0, 0), "max": (0, 0), "and_": (0, 0), "or_": (0, 0),   # selection: exact
    "compare": (0, 0), "mix": (0, 0),          # exact values, partials 0
}
G64_NAME = {"not_": "not", "and_": "and", "or_": "or", "modulo": "mod"}


def k_asin(v):
    c = v * v / (1.0 - v * v) if abs(v) < 1 else 0.0
    return math.ceil(2.5 + 0.5 * c)


def k_binary(name, form):
    k = K_BINARY[name]
    return k[form] if isinstance(k, dict) else k


def ulps(got, want64):
    """|got - want| in float32 ulp of want (float64 arithmetic)"""
    return abs(float(got) - want64) / float(np.spacing(np.float32(abs(want64))))


def tight(label, out, ref, kv, kd_of):
    """value and the three partials of every point within K ulp of the float64 duals `ref`.  A point where the reference's value is NaN
    (outside the domain) asks for a NaN value and nothing else; where a component of the reference is infinite or NaN (a pole), the same
    component of the result must not be finite either, and the point's other components - 0 * inf on the axes not seeded - are left alone.
    Returns the largest (value, partial) distance seen, in ulp."""
    worst_v = worst_d = 0.0
    for p in range(len(out)):
        o, rv, rd = out[p], float(ref.v[p]), ref.d[p]
        if math.isnan(rv):
            assert math.isnan(o[0]), f"{label} point {p}: value {o[0]}, the reference is NaN"
            continue
        want32 = np.array([rv, *rd], np.float64).astype(np.float32)   # (a finite float64 beyond float32's range counts as infinite)
        pole = ~np.isfinite(want32)
        if pole.any():
            for c in np.nonzero(pole)[0]:
                assert not math.isfinite(o[c]), f"{label} point {p}: component {c} is {o[c]}, the reference {want32[c]}"
            continue
        u = ulps(o[0], rv)
        assert u <= kv, f"{label} point {p}: value {o[0]} is {u:.2f} ulp from {rv!r} (K = {kv})"
        worst_v = max(worst_v, u)
        kd = kd_of(p)
        for c in range(3):
            u = ulps(o[1 + c], float(rd[c]))
            assert u <= kd, f"{label} point {p}: d/d{'xyz'[c]} {o[1 + c]} is {u:.2f} ulp from {float(rd[c])!r} (K = {kd})"
            worst_d = max(worst_d, u)
    return worst_v, worst_d


def est_ok(err, grad):
    """`err.min(err / grad.abs()) < 1e-2` (f32::min / f64::min ignore a NaN operand)"""
    rel = err / abs(grad) if grad != 0 else (math.inf if err != 0 else math.nan)
    m = err if math.isnan(rel) else min(err, rel)
    return m < 1e-2


def xyz(i, v, zero, j=None, w=None):
    """three argument lists with `v` on axis i (and `w` on axis j)"""
    a = [zero, zero, zero]
    a[i] = v
    if j is not None and j != i:
        a[j] = w
    return a


@pytest.mark.parametrize("name", [n for n in UNARY_DEFS if n not in ("rand",)])
def test_g_unary(be, name):  # grad_slice.rs:495-553, as the reference runs it: EPSILON 1e-4, every argument, every seed axis
    EPS = np.float32(1e-4)
    args = spicy_args()
    zero = [0.0] * len(args)
    fn = UNARY_DEFS[name]
    kv, kd = K_UNARY[name]
    for i in range(3):
        ctx = be.Context()
        s = be.Shape(ctx, getattr(ctx, name)((ctx.x, ctx.y, ctx.z)[i]()))
        out = g(s, *xyz(i, args, zero))
        for a, o in zip(args, out):
            v = fn(a)
            assert value_ok(be, name, o[0], v), f"{name} value at {a}"
            rest = [o[1 + k] for k in range(3) if k != i]
            assert all(r == 0 or math.isnan(r) for r in rest)  # 0/NaN outside a function's domain
            if name in ("floor", "ceil", "round", "not_"):
                assert o[1:] == (0, 0, 0)
            if name == "not_" and a == 0.0:   # discontinuous_at (eval/test/mod.rs:207)
                continue
            grad = float(o[1 + i])
            if not math.isnan(v) and grad < 1e9 and not math.isinf(grad):
                d = fn(f32(np.float32(a) + EPS))
                err = abs((float(d) - float(v)) / float(EPS) - grad)
                d = fn(f32(np.float32(a) - EPS))
                err = min(err, abs((float(v) - float(d)) / float(EPS) - grad))
                assert est_ok(err, grad), f"{name} d/d{'xyz'[i]} at {a}: {grad}, estimated within {err}"
        # ... and the tight criterion, against the float64 duals
        ref = G64._unary(G64_NAME.get(name, name), G64.D.seed(args, i), None)
        kd_of = (lambda p: kd) if kd is not None else (lambda p: k_asin(args[p]))
        wv, wd = tight(f"{name} seeded on {'xyz'[i]}", out, ref, kv, kd_of)
        print(f"{name} axis {i}: value within {wv:.2f} ulp (K {kv}), partials within {wd:.2f} ulp (K {kd if kd is not None else 'k_asin'})")


def discontinuous_at(name, a, b):
    """eval/test/mod.rs:220-245"""
    if name == "compare":
        return a == b
    if name == "modulo":
        v = np.float32(a) / np.float32(b)
        return abs(np.float32(libm("roundf", float(v))) - v) < 1e-9
    if name in ("and_", "or_"):
        return a == 0.0
    return name == "mix"


def compare_grad_results(name, i, j, lhs, rhs, out, constant_folded, label):
    """grad_slice.rs:555-644, arithmetic widths included: the estimate of d/d(lhs) is taken in f64, those of d/d(rhs) and of the
    shared axis in f32.  i, j: the seeded axis of each operand, 3 for an immediate."""
    EPS = np.float32(1e-3)
    fn = BINARY_DEFS[name]
    F = np.float32

    def ev(a, b):
        return fn(f32(a), f32(b))

    for a, b, o in zip(lhs, rhs, out):
        v = fn(a, b)
        assert same(o[0], v) or (math.isnan(v) and constant_folded), f"value mismatch in {label} at ({a}, {b}): {v} != {o[0]}"
        if math.isnan(v) or discontinuous_at(name, a, b):
            continue
        if i == j:
            grad = F(o[1 + i])
            if grad < 1e9 and not np.isinf(grad):
                err = abs((F(ev(F(a) + EPS, F(b) + EPS)) - F(v)) / EPS - grad)
                err = min(err, abs((F(v) - F(ev(F(a) - EPS, b))) / EPS - grad))
                assert est_ok(float(err), float(grad)), f"gradient estimate mismatch in {label} at ({a} + epsilon, {b}): {grad} ({err})"
            continue
        if i < 3:
            grad = float(o[1 + i])
            if grad < 1e9 and not math.isinf(grad):
                err = abs((float(ev(F(a) + EPS, b)) - float(v)) / float(EPS) - grad)
                err = min(err, abs((float(v) - float(ev(F(a) - EPS, b))) / float(EPS) - grad))
                assert est_ok(err, grad), f"gradient estimate mismatch in {label} at ({a} + epsilon, {b}): {grad} ({err})"
        if j < 3:
            grad = float(o[1 + j])
            if grad < 1e9 and not math.isinf(grad):
                err = abs(float((F(ev(a, F(b) + EPS)) - F(v)) / EPS) - grad)
                err = min(err, abs(float((F(v) - F(ev(a, F(b) - EPS))) / EPS) - grad))
                assert est_ok(err, grad), f"gradient estimate mismatch in {label} at ({a}, {b} + epsilon): {grad} ({err})"


def tight_binary(name, form, i, j, lhs, rhs, out, label):
    """the K-ulp criterion at the points the reference does not call discontinuous (and at those alone)"""
    keep = [p for p, (a, b) in enumerate(zip(lhs, rhs)) if not discontinuous_at(name, a, b)]
    if not keep:
        return 0.0, 0.0
    a = G64.D.seed([lhs[p] for p in keep], i if i < 3 else None)
    b = G64.D.seed([rhs[p] for p in keep], j if j < 3 else None)
    if name in ("min", "max") and i > j:
        # the Context orders the operands of a commutative node by handle (context/mod.rs:215-224; x, y, z, then constants, as they are made
        # here), and a tie takes the right-hand one (grad.rs:173-195): the expression that was built is min(b, a)
        a, b = b, a
    ref = G64._binary(G64_NAME.get(name, name), a, b, None)
    kv, kd = k_binary(name, form)
    return tight(label, [out[p] for p in keep], ref, kv, lambda p: kd)


# Strides of the sweep (the reference takes every rotation and every immediate; test_f_binary above subsamples the same way):
#   reg,reg   every fifth rotation of the argument list against itself, all nine axis pairs
#   immediate every fifth argument as the immediate, three axes, against the whole argument list.  (The reference also rotates the list
#             here, which only reorders the same (argument, immediate) pairs.)
ROT_STRIDE, IMM_STRIDE = 5, 5


@pytest.mark.parametrize("name", list(BINARY_DEFS))
def test_g_binary(be, name):  # grad_slice.rs:646-778
    args = spicy_args()
    zero = [0.0] * len(args)
    worst = {}

    def note(form, w):
        worst[form] = tuple(max(p, q) for p, q in zip(worst.get(form, (0.0, 0.0)), w))

    for rot in range(0, len(args), ROT_STRIDE):
        rgsa = args[rot:] + args[:rot]
        for i in range(3):
            for j in range(3):
                ctx = be.Context()
                ax = (ctx.x(), ctx.y(), ctx.z())
                s = be.Shape(ctx, getattr(ctx, name)(ax[i], ax[j]))
                folded = s.var_count() == 0
                out = g(s, *xyz(i, args, zero, j, rgsa))
                rhs = args if i == j else rgsa
                label = f"{name}(reg {'xyz'[i]}, reg {'xyz'[j]}) rotation {rot}"
                compare_grad_results(name, i, j, args, rhs, out, folded, label)
                if not folded:
                    note("rr", tight_binary(name, "rr", i, j, args, rhs, out, label))
    for imm in args[::IMM_STRIDE]:
        for imm_first in (False, True):
            for i in range(3):
                ctx = be.Context()
                v = (ctx.x, ctx.y, ctx.z)[i]()
                s = be.Shape(ctx, getattr(ctx, name)(imm, v) if imm_first else getattr(ctx, name)(v, imm))
                folded = s.var_count() == 0 or s.ssa_len() <= 2
                out = g(s, *xyz(i, args, zero))
                imms = [imm] * len(args)
                form = "ir" if imm_first else "ri"
                label = f"{name}({'imm, reg' if imm_first else 'reg, imm'}) on {'xyz'[i]}, imm {imm}"
                if imm_first:
                    compare_grad_results(name, 3, i, imms, args, out, folded, label)
                    if not (folded and math.isnan(imm)):
                        note(form, tight_binary(name, form, 3, i, imms, args, out, label))
                else:
                    compare_grad_results(name, i, 3, args, imms, out, folded, label)
                    if not (folded and math.isnan(imm)):
                        note(form, tight_binary(name, form, i, 3, args, imms, out, label))
    for form, (wv, wd) in sorted(worst.items()):
        print(f"{name} {form}: value within {wv:.2f} ulp, partials within {wd:.2f} ulp (K {k_binary(name, form)})")
