"""The arithmetic opcodes over the whole float range, the legs that need no GPU (float_range.py holds the inputs and the float64
references; test_float_range_gpu.py the device's legs):
  - the generator really holds the inputs that decide each opcode;
  - the oracle's f32 evaluator equals the float64 references bit for bit (2^20 inputs reg/reg, 2^18 per immediate);
  - the oracle's interval evaluator never excludes a finite value of a point of its operands (20 000 intervals per opcode and form);
  - the assembly tile kernels' interval handlers (fh_tiles, fh_tiles_v32, fh_tiles_v64 and their _t kernels) on the emulator equal
    emu_util.ref_interval bit for bit, their pruned child tapes ref_prune, and ref_interval equals the oracle on the same intervals;
  - the assembly bulk kernels' handlers (fh_float_eval_16x4, _32x2 and their _t kernels) on the emulator equal the float64
    references on the specials' cross product, in place and out of place, for every immediate.
A stricter rule, "a non-finite value of a sample point makes the interval NaN", does not hold on this range (an overflow gives an
infinite bound) and is not asserted."""
import numpy as np
import pytest

import float_range as R
from float_range import F32, U32

N_RR, N_IMM, N_IV = 1 << 20, 1 << 18, 20000

# ---- the generator ---------------------------------------------------------------------------------------------------------------
def _has(a, bits):
    return (np.ascontiguousarray(a, F32).view(U32) == U32(bits)).any()


def _has_pair(a, b, abits, bbits):
    a, b = np.ascontiguousarray(a, F32).view(U32), np.ascontiguousarray(b, F32).view(U32)
    return ((a == U32(abits)) & (b == U32(bbits))).any()


def test_the_generator_holds_the_inputs_that_decide_each_opcode():
    x = R.patterns(N_IMM, 1)
    xb = x.view(U32)
    # every sign / exponent / top-mantissa combination
    assert len(np.unique(xb[:R.N_SWEEP] >> U32(16))) == 1 << 16
    for bits in R.SPECIAL_BITS:
        assert _has(x, bits), hex(int(bits))
    # round: the x.5 ties, 0.5 less an ulp, the largest x.5 and the first float without a fraction bit, both signs
    for bits in (0x3F000000, 0xBF000000, 0x3FC00000, 0xBFC00000, 0x40200000, 0xC0200000, 0x3EFFFFFF, 0xBEFFFFFF, 0x4AFFFFFF, 0xCAFFFFFF,
                 0x4B000000, 0xCB000000):
        assert _has(x, bits)
    # denormals, infinities, NaN: what a flush-to-zero mode or a reciprocal approximation would show on
    assert _has(x, 1) and _has(x, 0x807FFFFF) and _has(x, 0x7F800000) and _has(x, 0xFF800000) and np.isnan(x).any()
    a, b = R.pairs(N_IMM, 2)
    assert len(a) == len(b) == N_IMM
    cls = R.pair_class(N_IMM)
    ab, bb = a.view(U32), b.view(U32)
    ea, eb = ((ab >> U32(23)) & U32(0xFF)).astype(int), ((bb >> U32(23)) & U32(0xFF)).astype(int)
    # add: equal magnitude, opposite sign; sub: equal operands - in every wave of 256 samples (and of 128)
    assert (bb[cls == 3] == (ab[cls == 3] ^ U32(0x80000000))).all() and (bb[cls == 2] == ab[cls == 2]).all()
    assert (ea[cls == 4] == eb[cls == 4]).all() and (ab[cls == 4] != bb[cls == 4]).any()
    assert (np.abs(ea[cls == 5] - eb[cls == 5]) <= 30).all()
    assert (ea[cls == 6] - eb[cls == 6] >= 146).all() and (ea[cls == 6] - eb[cls == 6] >= 200).mean() > 0.7     # (b's exponent ends at 0: the denormals)
    assert (eb[cls == 7] - ea[cls == 7] >= 146).all() and (eb[cls == 7] - ea[cls == 7] >= 200).mean() > 0.7
    head = R.N_SPECIAL ** 2
    for w in range(head, N_IMM - 128, 128):
        assert set(cls[w:w + 128]) >= ({0, 2, 3, 4, 5} | ({6, 7} if w >= head + R.N_SWEEP + R.N_SPECIAL else set()))
    # div, modulo: (largest finite, smallest denormal) and the reverse; an overflowing and an underflowing product
    assert _has_pair(a, b, 0x7F7FFFFF, 0x00000001) and _has_pair(a, b, 0x00000001, 0x7F7FFFFF)
    assert _has_pair(a, b, 0x7F7FFFFF, 0x7F7FFFFF) and _has_pair(a, b, 0x00000001, 0x00000001)
    # min, max, compare: the four +-0 pairs; a NaN on either side; inf - inf, 0 * inf, 0 / 0, inf / inf
    for p, q in ((0, 0), (0, 0x80000000), (0x80000000, 0), (0x80000000, 0x80000000), (0x7FC00000, 0x3F800000), (0x3F800000, 0x7FC00000),
                 (0x7F800000, 0x7F800000), (0x7F800000, 0xFF800000), (0, 0x7F800000), (0x7F800000, 0)):
        assert _has_pair(a, b, p, q), (hex(p), hex(q))
    # the x.5 ties reach round as an interval's bounds too, and the intervals hold every kind
    lo, hi = R.intervals(N_IV, 3)
    assert len(lo) == N_IV and not (lo > hi).any() and (np.isnan(lo) == np.isnan(hi)).all() and np.isnan(lo).any()
    assert _has_pair(lo, hi, 0x3EFFFFFF, 0x3F000000) and _has_pair(lo, hi, 0x80000000, 0) and _has_pair(lo, hi, 0, 0)
    assert _has_pair(lo, hi, 0xFF800000, 0x7F800000) and _has_pair(lo, hi, 0x7F800000, 0x7F800000)
    tail = slice(len(R.special_intervals()[0]), None)
    l, h = R._ord(np.nan_to_num(lo[tail], nan=0.0)), R._ord(np.nan_to_num(hi[tail], nan=0.0))
    kind = np.arange(len(l)) % 8
    assert ((h - l)[kind < 2] <= 1 << 20).all() and ((h - l)[kind == 7] == 0).all() and ((h - l)[kind == 4] > 1 << 24).any()
    assert (np.isinf(lo[tail]) & ~np.isinf(hi[tail])).any() and (np.isinf(hi[tail]) & ~np.isinf(lo[tail])).any()
    pts = R.samples(lo, hi, 8, 4)
    assert not R.violations(lo, hi, pts).any() and (pts[:, 0].view(U32) == lo.view(U32)).all() and (pts[:, -1].view(U32) == hi.view(U32)).all()


def test_folded_forms_are_the_listed_ones_and_the_path_pins_hold():
    """What the front end folds away is exactly FOLDED (so no form is skipped silently), and the five bulk paths of the GPU leg are pinned
    by construction: register counts and in-place / out-of-place handlers as the tape holds them (host side only)."""
    import fidget_amd as F
    import oracle as O
    for name in R.BINARY:
        for form in ("ri", "ir"):
            if form == "ir" and name in R.COMMUTATIVE:
                continue
            for imm in R.IMMEDIATES:
                for be in (F, O):
                    rec, _ = R.the_op(R.single_op(be, name, form, imm), name, form)
                    assert (rec is None) == R.folded(name, form, imm), (be.__name__, name, form, imm)
    for name in R.UNARY + R.BINARY:
        for form in R.forms(name):
            if R.folded(name, form, 3.0):
                continue
            for path in R.PATHS:
                for keep in (False, True):
                    s = R.path_shape(F, path, name, form, 3.0, keep)
                    lo, hi = R.PATH_SLOTS[path]
                    assert lo <= s.slot_count() <= hi, (name, form, path, keep, s.slot_count())
                    assert R.in_place(s, name, form) == (not keep), (name, form, path, keep)
                    # (modulo, rand and mix are handlers of the _t texts alone: for them the plain kernels' cases run the _t kernels again)
                    assert R.takes_compiled_routines(s) == (path.endswith("_t") or name in T_ONLY)


# ---- the oracle's f32 evaluator against the float64 references -------------------------------------------------------------------
def oracle_values(name, form, imm, by_axis):
    import oracle as O
    s = R.single_op(O, name, form, imm)
    vs = [None] * s.var_count()
    by_slot = {}
    for axis, arr in enumerate(by_axis):
        i = s.axis_index(axis)
        if i >= 0:
            vs[i] = arr
            by_slot[i] = arr
    return s.eval_float_slice_raw(vs)[0], R.operands(s, name, form, imm, by_slot)


@pytest.mark.parametrize("name", R.UNARY)
def test_oracle_unary_equals_float64_reference(name):
    x = R.patterns(N_RR, 11)
    got, (a, _) = oracle_values(name, "u", None, [x])
    want = R.ref_unary(name, a)
    assert R.same_bits(got, want).all(), f"{name}: {R.first_diff(got, want, a)}"


@pytest.mark.parametrize("name", R.BINARY)
def test_oracle_binary_equals_float64_reference(name):
    x, y = R.pairs(N_RR, 12)
    got, (a, b) = oracle_values(name, "rr", None, [x, y])
    want = R.ref_binary(name, a, b)
    assert R.same_bits(got, want).all(), f"{name} reg/reg: {R.first_diff(got, want, a, b)}"
    x = R.patterns(N_IMM, 13)
    for form, imm in R.imm_cases(name):
        got, (a, b) = oracle_values(name, form, imm, [x])
        want = R.ref_binary(name, a, b)
        assert R.same_bits(got, want).all(), f"{name} {form} {imm}: {R.first_diff(got, want, a, b)}"


# ---- the oracle's interval evaluator: sound on the whole range -------------------------------------------------------------------
@pytest.mark.parametrize("name", R.UNARY + R.BINARY)
def test_oracle_intervals_are_sound(name):
    import oracle as O
    for form, imm, n in R.interval_cases(name, N_IV):
        s = R.single_op(O, name, form, imm)
        by_axis = [R.intervals(n, 21), R.intervals(n, 22)]
        by_axis[1] = tuple(np.roll(b, 97) for b in by_axis[1])          # (the specials' intervals against others than themselves)
        v, by_slot = R.interval_vars(s, by_axis)
        out, _, _ = R.oracle_intervals(s, v)
        R.check_sound(f"{name} {form} {imm}", out[:, 0], out[:, 1], R.sample_values(s, name, form, imm, by_axis, by_slot, 31))


# ---- the assembly tile kernels' interval handlers on the emulator ----------------------------------------------------------------
TILE_WAVES = 6            # 384 lanes: the specials' 379 intervals and a few of every other kind
TILE_IMMEDIATES = [3.0, -7.77]
T_ONLY = {"modulo", "rand", "mix"}          # handlers of the _t kernels only


def tile_kernels(name):
    return ["fh_tiles_t", "fh_tiles_v32_t", "fh_tiles_v64_t"] if name in T_ONLY else ["fh_tiles", "fh_tiles_v32", "fh_tiles_v64"]


def tile_inputs(form):
    n = 64 * TILE_WAVES
    a = R.intervals(n, 41)
    b = R.intervals(n, 42)
    perm = np.random.default_rng(43).permutation(n)
    return [a, (b[0][perm], b[1][perm])] if form == "rr" else [a]


@pytest.mark.parametrize("name", R.UNARY + R.BINARY)
def test_tile_kernels_interval_handlers_on_the_emulator(name):
    import emu_util as U
    import fidget_amd as F
    import oracle as O
    import test_emu_tiles as T
    for form in R.forms(name):
        for imm in ([None] if form in ("u", "rr") else [i for i in TILE_IMMEDIATES if not R.folded(name, form, i)]):
            s, o = R.single_op(F, name, form, imm), R.single_op(O, name, form, imm)
            tape = U.shape_tape(s)
            ik = [3] * 16
            for axis in range(3):
                if s.axis_index(axis) >= 0:
                    ik[s.axis_index(axis)] = axis
            by_axis = tile_inputs(form)
            zero = np.zeros(64, F32)
            # the oracle and the numpy restatement on all the lanes at once
            v, _ = R.interval_vars(o, by_axis)
            want, want_ch, _ = R.oracle_intervals(o, v)
            assert [o.axis_index(a) for a in range(3)] == [s.axis_index(a) for a in range(3)]
            inputs = {slot: by_axis[axis] for slot, axis in enumerate(ik) if axis < len(by_axis)}
            el, eh, ch, _ = U.ref_interval(tape, inputs, 64 * TILE_WAVES)
            label = f"{name} {form} {imm}"
            assert R.same_bits(el, want[:, 0]).all(), f"{label}: emu_util.ref_interval lower bounds, {R.first_diff(el, want[:, 0], *[b for p in by_axis for b in p])}"
            assert R.same_bits(eh, want[:, 1]).all(), f"{label}: emu_util.ref_interval upper bounds, {R.first_diff(eh, want[:, 1], *[b for p in by_axis for b in p])}"
            if len(ch):
                assert (ch[0] == want_ch[:, 0]).all(), f"{label}: choices differ at lanes {np.nonzero(ch[0] != want_ch[:, 0])[0][:8]}"
            for kernel in tile_kernels(name):
                for w in range(TILE_WAVES):
                    lanes = slice(64 * w, 64 * w + 64)
                    xyz = []
                    for axis in range(3):
                        xyz += [by_axis[axis][0][lanes], by_axis[axis][1][lanes]] if axis < len(by_axis) else [zero, zero]
                    try:
                        T.check_slot(kernel, tape, xyz, ik, s.slot_count(), s.choice_count())
                    except AssertionError as e:
                        raise AssertionError(f"{kernel} {label} wave {w}: {e}") from e


# ---- the assembly bulk kernels' handlers on the emulator --------------------------------------------------------------------------
def bulk_tape(name, form, inplace):
    """One tape with the opcode once per immediate (reg/reg and unary: once), each with an output of its own: register 0 and 1 hold the
    inputs; in place the opcode works on a copy of its operand (out == a), out of place it writes a third register."""
    import emu_util as U
    P, OP = U.pack, U.OPN
    tape = [P(OP["INPUT"], 0, 0, 0), P(OP["INPUT"], 1, 0, 1)]
    code = OP[R.OPCODE[name].upper() + ("_" + R.FORM_SUFFIX[form] if form != "u" else "")]
    imms = [None] if form in ("u", "rr") else R.IMMEDIATES
    for k, imm in enumerate(imms):
        w1 = 1 if form == "rr" else (0 if form == "u" else int(U.f2u(imm)))
        if inplace:
            tape += [P(OP["COPY_REG"], 2, 0, 0), P(code, 2, 2, w1)]
        else:
            tape += [P(code, 2, 0, w1)]
        tape += [P(OP["OUTPUT"], 0, 2, k)]
    return tape, imms


@pytest.mark.parametrize("kernel,zb", [("fh_float_eval_16x4", 4), ("fh_float_eval_32x2", 2)])
@pytest.mark.parametrize("name", R.UNARY + R.BINARY)
def test_bulk_kernels_handlers_on_the_emulator(kernel, zb, name):
    """(every immediate here, folded or not: the tape is packed by hand, and the handlers take what they are given)"""
    import emu_util as U
    from test_emu_bulk import run_bulk
    trans = name in T_ONLY
    x, y = R.special_cross()
    n = len(x)
    for form in R.forms(name):
        for inplace in (True, False):
            tape, imms = bulk_tape(name, form, inplace)
            got = run_bulk(kernel + ("_t" if trans else ""), zb, tape, {0: x, 1: y}, n, len(imms), trans=trans)
            also = U.ref_f32(np.asarray(tape, np.uint64), {0: x, 1: y}, n)
            for k, imm in enumerate(imms):
                i = None if imm is None else np.full(n, imm, F32)
                want = R.ref_unary(name, x) if form == "u" else R.ref_binary(name, *{"rr": (x, y), "ri": (x, i), "ir": (i, x)}[form])
                label = f"{kernel} {name} {form} {imm} {'in place' if inplace else 'out of place'}"
                assert R.same_bits(got[k], want).all(), f"{label}: {R.first_diff(got[k], want, x, y)}"
                assert R.same_bits(also[k], want).all(), f"{label}: emu_util.ref_f32, {R.first_diff(also[k], want, x, y)}"


# ---- named cases: what the sweeps above found ------------------------------------------------------------------------------------
SIGNED_ZERO_CASES = [    # (opcode, x, y, result): interval bounds whose f32::min / f32::max has +0 and -0 to choose from; -0 is the smaller
    ("min", (-0.0, -0.0), (0.0, 2.5), (-0.0, -0.0)),
    ("min", (0.0, 2.5), (-0.0, -0.0), (-0.0, -0.0)),
    ("max", (-np.inf, 0.0), (-1.0, -0.0), (-1.0, 0.0)),
    ("max", (-1.0, -0.0), (-np.inf, 0.0), (-1.0, 0.0)),
    ("mul", (0.0, 0.0), (-2.5, 8388608.0), (-0.0, 0.0)),
    ("and_", (-1.0, 0.0), (-0.0, 1.5), (-0.0, 1.5)),
    ("or_", (-0.0, 0.5), (0.0, 2.0), (-0.0, 2.0)),
]


def test_interval_bounds_of_signed_zeros_take_minus_zero_for_the_smaller():
    """Found by test_tile_kernels_interval_handlers_on_the_emulator: where an interval bound is f32::min / f32::max of +0 and -0 the
    reference leaves the result open ("either input may be returned") and libm's fminf gave the oracle the second operand, while the
    device's v_min_f32 / v_max_f32 order the zeros.  The oracle and emu_util.ref_interval now take -0 < +0 as well (oracle/src/types.hpp
    rmin / rmax): the same bound whichever operand comes first."""
    import emu_util as U
    import fidget_amd as F
    import oracle as O
    for name, x, y, want in SIGNED_ZERO_CASES:
        for swap in (False, True):        # (the Context orders the operands of a commutative opcode itself: give the pair both ways)
            s, o = R.single_op(F, name, "rr"), R.single_op(O, name, "rr")
            a, b = (y, x) if swap and name in ("min", "max", "mul") else (x, y)
            by_axis = [(np.full(64, a[0], F32), np.full(64, a[1], F32)), (np.full(64, b[0], F32), np.full(64, b[1], F32))]
            v, _ = R.interval_vars(o, by_axis)
            out, _, _ = R.oracle_intervals(o, v)
            w = np.array(want, F32)
            assert (out.view(U32) == w.view(U32)).all(), (name, x, y, out[0])
            tape = U.shape_tape(s)
            ik = [3] * 16
            ik[s.axis_index(0)], ik[s.axis_index(1)] = 0, 1
            el, eh, _, _ = U.ref_interval(tape, {s.axis_index(0): by_axis[0], s.axis_index(1): by_axis[1]}, 64)
            assert (el.view(U32) == w.view(U32)[0]).all() and (eh.view(U32) == w.view(U32)[1]).all(), (name, x, y, el[0], eh[0])
