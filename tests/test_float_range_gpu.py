"""The arithmetic opcodes over the whole float range on the device (float_range.py holds the inputs and the float64 references,
test_float_range.py the legs that need no GPU):
  - the bulk f32 evaluator on each of its five paths (float_range.PATHS, pinned by what the tape holds and asserted on the tape), every
    opcode, operand form and immediate, the in-place and the out-of-place handler: bit for bit the float64 reference rounded once;
    short and odd lengths equal the prefix of the full result;
  - the value component of the gradient evaluator (k_eval_grad, dev_ops.hpp GR) and the tracing point evaluator (k_eval_f32 with
    choices): the same values, and the point evaluator's choices the oracle's;
  - the interval evaluator (k_eval_interval) on 20 000 intervals per opcode and form: bit for bit the oracle's, choices and the
    simplify flag too, and sound against the float64 reference at sample points of the operands.
Bits equal, a NaN equals any NaN, +0 != -0.  The forms the front end folds away (float_range.FOLDED, with the reasons) are the only
ones not run; test_float_range.py asserts that the list is exact."""
import numpy as np
import pytest

import float_range as R
from float_range import F32, U32

pytestmark = pytest.mark.gpu

N_RR, N_IMM, N_IV = 1 << 20, 1 << 18, 20000
LENGTHS = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257]          # the kernels take 256 or 128 samples a wave (k_eval_f32: 64)

_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
        _cache[key].setflags(write=False)
    return _cache[key]


def inputs(form):
    """(x, y, z): z feeds only the roots that pin a path"""
    if form == "rr":
        x, y = cached(("pairs", N_RR), lambda: np.stack(R.pairs(N_RR, 12)))
    else:
        n = N_RR if form == "u" else N_IMM
        x = cached(("patterns", n), lambda: R.patterns(n, 11 if form == "u" else 13).copy())
        y = x
    z = cached(("z", len(x)), lambda: np.random.default_rng(14).uniform(-1, 1, len(x)).astype(F32))
    return x, y, z


def reference(shape, name, form, imm, x, y):
    """the float64 reference for the operands in the order the tape's opcode takes them; computed once per (opcode, form, immediate,
    order) and shared by every path and evaluator"""
    order = R.operand_axes(shape, name, form)
    arr = (x, y)

    def compute():
        if form == "u":
            return R.ref_unary(name, arr[order[0]])
        if form == "rr":
            return R.ref_binary(name, arr[order[0]], arr[order[1]])
        i = np.full(len(x), imm, F32)
        return R.ref_binary(name, x, i) if form == "ri" else R.ref_binary(name, i, x)
    return cached(("ref", name, form, imm, len(x), order), compute)


def immediates(name, form):
    return [None] if form in ("u", "rr") else [i for i in R.IMMEDIATES if not R.folded(name, form, i)]


CASES = [(name, form) for name in R.UNARY + R.BINARY for form in R.forms(name)]


# ---- the bulk f32 evaluator, five paths ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", CASES)
@pytest.mark.parametrize("path", R.PATHS)
def test_bulk_float_evaluator(path, name, form):
    import fidget_amd as F
    hip = F.default_context()
    x, y, z = inputs(form)
    with hip.options(no_asm=1 if path == "k_eval_f32" else 0):
        assert hip.option("no_asm") == (1 if path == "k_eval_f32" else 0)
        for imm in immediates(name, form):
            for keep in (False, True):
                s = R.path_shape(F, path, name, form, imm, keep)
                label = f"{path} {name} {form} {imm} {'out of place' if keep else 'in place'}"
                lo, hi = R.PATH_SLOTS[path]
                assert lo <= s.slot_count() <= hi, f"{label}: {s.slot_count()} registers"
                assert R.in_place(s, name, form) == (not keep), label
                assert R.takes_compiled_routines(s) == (path.endswith("_t") or name in ("modulo", "rand", "mix")), label
                want = reference(s, name, form, imm, x, y)
                got = np.asarray(s.eval_float_slice(x, y, z), F32)
                assert R.same_bits(got, want).all(), f"{label}: {R.first_diff(got, want, x, y)}"
                if imm is None or imm == immediates(name, form)[0]:
                    for n in LENGTHS:
                        part = np.asarray(s.eval_float_slice(x[:n], y[:n], z[:n]), F32)
                        assert R.same_bits(part, got[:n]).all(), f"{label}, {n} samples: {R.first_diff(part, got[:n], x[:n], y[:n])}"
                    # ... and a last, partial wave behind full ones
                    n = R.N_SPECIAL ** 2 + 4 * 256 + 77
                    part = np.asarray(s.eval_float_slice(x[:n], y[:n], z[:n]), F32)
                    assert R.same_bits(part, got[:n]).all(), f"{label}, {n} samples: {R.first_diff(part, got[:n], x[:n], y[:n])}"


# ---- the other evaluators of the same values ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", CASES)
def test_gradient_evaluator_value_component(name, form):
    """k_eval_grad (dev_ops.hpp GR): the value of every opcode, seeds as eval_grad_slice sets them.  It is the f32 evaluator's for every
    opcode but abs at -0 (float_range.ref_grad_value)."""
    import fidget_amd as F
    x, y, z = inputs(form)
    n = N_IMM
    x, y, z = x[:n], y[:n], z[:n]
    for imm in immediates(name, form):
        s = R.single_op(F, name, form, imm)
        want = reference(s, name, form, imm, *inputs(form)[:2])[:n]
        if name == "abs":           # (the one opcode whose value the reference's gradient type computes another way: -0 stays -0)
            want = R.ref_grad_value(name, x)
        got = np.ascontiguousarray(s.eval_grad_slice(x, y, z)[:, 0])
        assert R.same_bits(got, want).all(), f"{name} {form} {imm}: {R.first_diff(got, want, x, y)}"


@pytest.mark.parametrize("name,form", CASES)
def test_point_evaluator_values_and_choices(name, form):
    """fhip_point_eval (k_eval_f32 with choices) on the specials' cross product: the value, and for min / max / and_ / or_ the choice and
    the simplify flag of the oracle's tracing evaluator - equal operands, +-0 and NaN decide them"""
    import fidget_amd as F
    import oracle as O
    x, y = R.special_cross()
    for imm in immediates(name, form):
        s, o = R.single_op(F, name, form, imm), R.single_op(O, name, form, imm)
        assert [s.axis_index(a) for a in range(3)] == [o.axis_index(a) for a in range(3)] and s.choice_count() == o.choice_count()
        v = np.zeros((len(x), max(s.var_count(), 1)), F32)
        by_slot = {}
        for axis, arr in enumerate((x, y)):
            if s.axis_index(axis) >= 0:
                v[:, s.axis_index(axis)] = arr
                by_slot[s.axis_index(axis)] = arr
        a, b = R.operands(s, name, form, imm, by_slot)
        want = R.ref_unary(name, a) if form == "u" else R.ref_binary(name, a, b)
        out, ch, simp = s._tracing(F.lib().fhip_point_eval, v, 1)
        label = f"{name} {form} {imm}"
        assert R.same_bits(out[:, 0], want).all(), f"{label}: {R.first_diff(out[:, 0], want, x, y)}"
        o_out, o_ch, o_simp = R.oracle_points(o, v)
        assert R.same_bits(o_out, want).all(), f"{label}: the oracle, {R.first_diff(o_out, want, x, y)}"
        assert (simp == o_simp).all(), f"{label}: simplify flags differ at points {np.nonzero(simp != o_simp)[0][:8]}"
        assert (ch == o_ch).all(), f"{label}: choices differ at points {np.nonzero((ch != o_ch).any(axis=1))[0][:8]}"
        if name in ("min", "max", "and_", "or_"):
            assert s.choice_count() == 1 and set(np.unique(ch)) <= {1, 2, 3} and len(np.unique(ch)) >= 2


# ---- the interval evaluator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", CASES)
def test_interval_evaluator(name, form):
    """k_eval_interval through Shape._tracing on an array [n, n_vars, 2]"""
    import fidget_amd as F
    import oracle as O
    for f, imm, n in R.interval_cases(name, N_IV):
        if f != form:
            continue
        s, o = R.single_op(F, name, form, imm), R.single_op(O, name, form, imm)
        assert [s.axis_index(a) for a in range(3)] == [o.axis_index(a) for a in range(3)] and s.choice_count() == o.choice_count()
        by_axis = [R.intervals(n, 21), tuple(np.roll(b, 97) for b in R.intervals(n, 22))]
        v, by_slot = R.interval_vars(s, by_axis)
        out, ch, simp = s._tracing(F.lib().fhip_interval_eval, v, 2)
        out = out[:, 0, :]
        want, want_ch, want_simp = R.oracle_intervals(o, v)
        label = f"{name} {form} {imm}"
        flat = [b for p in by_axis for b in p]
        assert R.same_bits(out[:, 0], want[:, 0]).all(), f"{label}: lower bounds, {R.first_diff(out[:, 0], want[:, 0], *flat)}"
        assert R.same_bits(out[:, 1], want[:, 1]).all(), f"{label}: upper bounds, {R.first_diff(out[:, 1], want[:, 1], *flat)}"
        assert (ch == want_ch).all(), f"{label}: choices differ at intervals {np.nonzero((ch != want_ch).any(axis=1))[0][:8]}"
        assert (simp == want_simp).all(), f"{label}: simplify flags differ at intervals {np.nonzero(simp != want_simp)[0][:8]}"
        R.check_sound(label, np.ascontiguousarray(out[:, 0]), np.ascontiguousarray(out[:, 1]),
                      R.sample_values(s, name, form, imm, by_axis, by_slot, 31))


# ---- named cases: what the sweeps found --------------------------------------------------------------------------------------------
def test_interval_bounds_of_signed_zeros_take_minus_zero_for_the_smaller():
    """k_eval_interval on test_float_range.SIGNED_ZERO_CASES: an interval bound that is f32::min / f32::max of +0 and -0 (the reference
    leaves the choice open) is -0 for min and +0 for max, whichever operand comes first - as in the oracle"""
    import fidget_amd as F
    from test_float_range import SIGNED_ZERO_CASES
    for name, x, y, want in SIGNED_ZERO_CASES:
        s = R.single_op(F, name, "rr")
        for a, b in ((x, y), (y, x)) if name in ("min", "max", "mul") else ((x, y),):
            v, _ = R.interval_vars(s, [(np.full(3, a[0], F32), np.full(3, a[1], F32)), (np.full(3, b[0], F32), np.full(3, b[1], F32))])
            out, _, _ = s._tracing(F.lib().fhip_interval_eval, v, 2)
            assert (out[:, 0, :].view(U32) == np.array(want, F32).view(U32)).all(), (name, a, b, out[0, 0])


def test_gradient_abs_keeps_a_minus_zero(be):
    """The value of abs in the gradient evaluator is `if v < 0 { -v } else { v }` (types/grad.rs:44-55): -0 stays -0, where the f32
    evaluator's f32::abs gives +0.  Found when the gradient evaluator's values were held to the f32 reference."""
    c = be.Context()
    s = be.Shape(c, c.abs(c.x()))
    x = np.array([-0.0, 0.0, -1.5, np.inf, -np.inf], F32)
    zero = np.zeros(len(x), F32)
    g = np.ascontiguousarray(s.eval_grad_slice(x, zero, zero)[:, 0])
    f = np.asarray(s.eval_float_slice(x, zero, zero), F32)
    assert g.view(U32).tolist() == np.array([-0.0, 0.0, 1.5, np.inf, np.inf], F32).view(U32).tolist()
    assert f.view(U32).tolist() == np.array([0.0, 0.0, 1.5, np.inf, np.inf], F32).view(U32).tolist()
