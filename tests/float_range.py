"""Inputs and references for holding the arithmetic opcodes to IEEE over the whole float range (test_float_range.py,
test_float_range_gpu.py).  No tests here.

Inputs: bit patterns, not numbers - every sign / exponent / top-mantissa combination, the values that decide each opcode
(SPECIAL_BITS), pairs of operands of every relative magnitude, and intervals with bounds anywhere in the range.
References: the operation in float64 numpy, rounded once to f32 (for + - * / sqrt of f32 operands the double rounding is
innocuous: 53 >= 2 * 24 + 2), the selecting opcodes by their definitions in kat_util (eval/test/mod.rs:190-243).
Comparison: bits equal, any NaN equals any NaN, +0 != -0 (a NaN's sign and payload are not part of
the contract)."""
import numpy as np

F32, F64, U32, I64 = np.float32, np.float64, np.uint32, np.int64

# the values that decide each opcode
SPECIAL_BITS = np.array([
    0x00000000, 0x80000000,             # +-0
    0x00000001, 0x80000001,             # +- smallest denormal
    0x007FFFFF, 0x807FFFFF,             # +- largest denormal
    0x00800000, 0x80800000,             # +- smallest normal (2^-126)
    0x3F800000, 0xBF800000,             # +-1
    0x7F7FFFFF, 0xFF7FFFFF,             # +- largest finite
    0x7F800000, 0xFF800000, 0x7FC00000,  # +-inf, NaN
    0x3F000000, 0xBF000000,             # +-0.5
    0x3FC00000, 0xBFC00000,             # +-1.5
    0x40200000, 0xC0200000,             # +-2.5
    0x3EFFFFFF, 0xBEFFFFFF,             # +-0.49999997: 0.5 less one ulp (x + 0.5 rounds up to 1 in f32)
    0x4AFFFFFF, 0xCAFFFFFF,             # +-8388607.5: the largest x.5
    0x4B000000, 0xCB000000,             # +-8388608 = 2^23: the first float without a fraction bit
    0x4F000000,                         # 2^31
], U32)
N_SPECIAL = len(SPECIAL_BITS)
N_SWEEP = 1 << 16                       # the (i << 16) | 0x8001 block

# immediates of the reg/imm and imm/reg forms
IMMEDIATES = [3.0, -7.77, 0.3, -0.0, 2.0 ** -40, 1e30, 1e-30, 1e-40, float(F32(3.4028234663852886e38)), float("inf"), 1.0, -0.5]

UNARY = ["neg", "abs", "recip", "sqrt", "square", "floor", "ceil", "round", "not_", "rand"]
BINARY = ["add", "sub", "mul", "div", "min", "max", "compare", "modulo", "and_", "or_", "mix"]
COMMUTATIVE = {"add", "mul", "min", "max"}          # the Context orders their operands: an immediate comes second (context/mod.rs:215-224)
OPCODE = {"neg": "Neg", "abs": "Abs", "recip": "Recip", "sqrt": "Sqrt", "square": "Square", "floor": "Floor", "ceil": "Ceil",
          "round": "Round", "not_": "Not", "rand": "Rand", "add": "Add", "sub": "Sub", "mul": "Mul", "div": "Div", "min": "Min",
          "max": "Max", "compare": "Compare", "modulo": "Mod", "and_": "And", "or_": "Or", "mix": "Mix"}
FORM_SUFFIX = {"u": "", "rr": "RR", "ri": "RI", "ir": "IR"}


def specials():
    return SPECIAL_BITS.view(F32).copy()


def special_cross():
    """(a, b): the full cross product of the specials"""
    s = specials()
    return np.repeat(s, N_SPECIAL), np.tile(s, N_SPECIAL)


def _random_bits(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)


def patterns(n, seed):
    """n f32 values as bit patterns: every sign / exponent / top-mantissa combination ((i << 16) | 0x8001), then the specials, then
    random 32-bit patterns."""
    assert n >= N_SWEEP + N_SPECIAL
    xs = _random_bits(np.random.default_rng(seed), n)
    xs[:N_SWEEP] = (np.arange(N_SWEEP, dtype=U32) << 16) | 0x8001
    xs[N_SWEEP:N_SWEEP + N_SPECIAL] = SPECIAL_BITS
    return xs.view(F32)


# pairs(): what b is, by (index - N_SPECIAL^2) % 8
PAIR_CLASSES = ["independent", "independent", "equal", "negated", "same exponent", "exponents within 30", "a 200+ exponents above b",
                "a 200+ exponents below b"]


def pairs(n, seed):
    """(a, b): the cross product of the specials in the first lanes, then a = patterns() and b by PAIR_CLASSES on the residue of the
    index, so that every class is in every wave.  The two far-apart classes set a's exponent as well (behind the fixed blocks of a only)."""
    head = N_SPECIAL * N_SPECIAL
    m = n - head
    rng = np.random.default_rng(seed)
    a = patterns(m, seed).view(U32).copy()
    b = _random_bits(rng, m)
    idx = np.arange(m)
    k = idx % 8
    frac = _random_bits(rng, m) & U32(0x007FFFFF)
    b = np.where(k == 2, a, b)
    b = np.where(k == 3, a ^ U32(0x80000000), b)
    b = np.where(k == 4, (a & U32(0xFF800000)) | frac, b)
    ea = ((a >> U32(23)) & U32(0xFF)).astype(I64)
    eb = np.clip(ea + rng.integers(-30, 31, m), 0, 255)
    b = np.where(k == 5, (b & U32(0x807FFFFF)) | (eb.astype(U32) << U32(23)), b)
    free = idx >= N_SWEEP + N_SPECIAL
    hi_e = rng.integers(200, 255, m)                 # 200 .. 254
    lo_e = hi_e - rng.integers(200, 255, m)          # at least 200 below, clipped to the denormals' exponent
    lo_e = np.clip(lo_e, 0, 54)
    for cls, (e_a, e_b) in ((6, (hi_e, lo_e)), (7, (lo_e, hi_e))):
        sel = free & (k == cls)
        a = np.where(sel, (a & U32(0x807FFFFF)) | (e_a.astype(U32) << U32(23)), a)
        b = np.where(sel, (b & U32(0x807FFFFF)) | (e_b.astype(U32) << U32(23)), b)
    ca, cb = special_cross()
    return (np.concatenate([ca, a.astype(U32).view(F32)]).astype(F32), np.concatenate([cb, b.astype(U32).view(F32)]).astype(F32))


def pair_class(n):
    """the class index of each lane of pairs(n, .), -1 for the specials' cross product; the far-apart classes only where they apply"""
    head = N_SPECIAL * N_SPECIAL
    idx = np.arange(n - head)
    k = idx % 8
    k = np.where((k >= 6) & (idx < N_SWEEP + N_SPECIAL), 0, k)
    return np.concatenate([np.full(head, -1), k])


# ---- intervals -------------------------------------------------------------------------------------
def _ord(f):
    """f32 -> integers in the floats' order (+-0 -> 0)"""
    b = np.ascontiguousarray(f, F32).view(U32).astype(I64)
    return np.where(b & 0x80000000, -(b & 0x7FFFFFFF), b)


def _unord(o):
    o = np.asarray(o, I64)
    return np.where(o < 0, (-o) | 0x80000000, o).astype(U32).view(F32)


_ORD_INF = 0x7F800000


def special_intervals():
    """every (lo, hi) of the specials with lo <= hi, and (NaN, NaN)"""
    a, b = special_cross()
    keep = a <= b
    return np.concatenate([a[keep], [F32(np.nan)]]).astype(F32), np.concatenate([b[keep], [F32(np.nan)]]).astype(F32)


INTERVAL_KINDS = ["narrow", "narrow", "same scale", "same scale", "arbitrary", "arbitrary", "arbitrary", "point"]


def intervals(n, seed, head=True):
    """(lo, hi): the specials' intervals first (head), then by INTERVAL_KINDS on the residue of the index - narrow (1 .. 2^20 ulp wide),
    both bounds of one exponent, any two values, one value - with bounds from the whole range, infinities included; a NaN bound makes
    (NaN, NaN), the only invalid interval the evaluators are given (types/interval.rs)."""
    rng = np.random.default_rng(seed)
    hl, hh = special_intervals() if head else (np.zeros(0, F32), np.zeros(0, F32))
    m = n - len(hl)
    assert m >= 0
    p, q = _random_bits(rng, m), _random_bits(rng, m)
    k = np.arange(m) % 8
    # narrow
    width = np.floor(2.0 ** rng.uniform(0, 20, m)).astype(I64)
    op = _ord(p.view(F32))
    op = np.where(np.abs(op) > _ORD_INF, np.sign(op) * (_ORD_INF - 1 - (np.abs(op) & 0xFFFF)), op)      # (a NaN pattern: a large finite value instead)
    narrow_lo, narrow_hi = _unord(op), _unord(np.minimum(op + width, _ORD_INF))
    # same scale: q takes p's exponent
    q_same = (q & U32(0x807FFFFF)) | (p & U32(0x7F800000))
    lo = np.where(k < 2, narrow_lo, p.view(F32))
    other = np.where(k < 2, narrow_hi, np.where(k < 4, q_same.view(F32), np.where(k < 7, q.view(F32), p.view(F32))))
    inf_lo = (k == 4) & (np.arange(m) % 24 == 4)
    inf_hi = (k == 5) & (np.arange(m) % 24 == 5)
    lo = np.where(inf_lo, F32(-np.inf), lo)
    other = np.where(inf_hi, F32(np.inf), other)
    with np.errstate(all="ignore"):
        bad = np.isnan(lo) | np.isnan(other)
        l2, h2 = np.where(other < lo, other, lo), np.where(other < lo, lo, other)
    l2 = np.where(bad, F32(np.nan), l2).astype(F32)
    h2 = np.where(bad, F32(np.nan), h2).astype(F32)
    return np.concatenate([hl, l2]).astype(F32), np.concatenate([hh, h2]).astype(F32)


def samples(lo, hi, k, seed):
    """[n, k] f32 points of each interval: both bounds and k - 2 points between, uniform in the floats' order (so every magnitude
    between the bounds is as likely as another); NaN for (NaN, NaN).  A zero between the bounds takes the sign of a bound that is zero:
    rand and mix go by bit pattern, and take an interval for a point when its bounds' bits are equal (types/interval.rs:600-627)."""
    rng = np.random.default_rng(seed)
    n = len(lo)
    with np.errstate(all="ignore"):
        bad = np.isnan(lo) | np.isnan(hi)
    ol, oh = _ord(np.where(bad, F32(0), lo)), _ord(np.where(bad, F32(0), hi))
    u = rng.random((n, k - 2))
    mid = ol[:, None] + np.floor(u * (oh - ol + 1)[:, None]).astype(I64)
    mid = _unord(np.minimum(mid, oh[:, None]))
    zero = np.where(hi == 0, hi, np.where(lo == 0, lo, F32(0)))[:, None]
    mid = np.where(mid == 0, zero, mid)
    pts = np.concatenate([lo[:, None], mid, hi[:, None]], axis=1).astype(F32)
    pts[bad] = np.nan
    return pts


def violations(lo, hi, v):
    """where a finite value v (shape [n, ...]) of an interval's sample points lies outside [lo, hi] (shape [n]), unless the interval is NaN"""
    shape = (len(lo),) + (1,) * (v.ndim - 1)
    lo, hi = lo.reshape(shape), hi.reshape(shape)
    with np.errstate(all="ignore"):
        is_nan = np.isnan(lo) | np.isnan(hi)
        return np.isfinite(v) & ~is_nan & ~((lo <= v) & (v <= hi))


# ---- references ------------------------------------------------------------------------------------
def pcg(v):
    """rng::hash (rng/mod.rs:8-13, kat_util.rng_hash) on uint32 arrays"""
    v = np.asarray(v, np.uint64)
    s = (v * np.uint64(747796405) + np.uint64(2891336453)) & np.uint64(0xFFFFFFFF)
    w = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(277803737)) & np.uint64(0xFFFFFFFF)
    return (((w >> np.uint64(22)) ^ w) & np.uint64(0xFFFFFFFF)).astype(U32)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def _once(x):
    return np.asarray(x, F64).astype(F32)


def ref_unary(name, a):
    a = np.asarray(a, F32)
    with np.errstate(all="ignore"):
        d = a.astype(F64)
        if name == "neg":
            return _once(-d)
        if name == "abs":
            return _once(np.abs(d))
        if name == "recip":
            return _once(1.0 / d)
        if name == "sqrt":
            return _once(np.sqrt(d))
        if name == "square":
            return _once(d * d)
        if name == "floor":
            return _once(np.floor(d))
        if name == "ceil":
            return _once(np.ceil(d))
        if name == "round":                       # half away from zero; |x| + 0.5 is exact in float64 wherever x has a fraction
            return _once(np.copysign(np.floor(np.abs(d) + 0.5), d))
        if name == "not_":
            return (a == 0).astype(F32)
        if name == "rand":
            return _once(((pcg(_bits(a)) >> U32(9)) | U32(0x3F800000)).view(F32).astype(F64) - 1.0)
    raise KeyError(name)


def ref_binary(name, a, b):
    a, b = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32))
    nan = F32(np.nan)
    with np.errstate(all="ignore"):
        x, y = a.astype(F64), b.astype(F64)
        un = np.isnan(a) | np.isnan(b)
        if name == "add":
            return _once(x + y)
        if name == "sub":
            return _once(x - y)
        if name == "mul":
            return _once(x * y)
        if name == "div":
            return _once(x / y)
        if name == "min":                         # kat_util.f_min: NaN if either is, the second operand when equal
            return np.where(a < b, a, np.where(b < a, b, np.where(un, nan, b))).astype(F32)
        if name == "max":
            return np.where(a > b, a, np.where(b > a, b, np.where(un, nan, b))).astype(F32)
        if name == "compare":
            return np.where(a < b, F32(-1), np.where(a == b, F32(0), np.where(a > b, F32(1), nan))).astype(F32)
        if name == "modulo":                      # fmod is exact; the sum rounds once
            r = np.fmod(x, y)
            return _once(np.where(r < 0, r + np.abs(y), r))
        if name == "and_":
            return np.where(a == 0, a, b).astype(F32)
        if name == "or_":
            return np.where(a != 0, a, b).astype(F32)
        if name == "mix":
            s = (_bits(a).astype(np.uint64) + pcg(_bits(b)).astype(np.uint64)) & np.uint64(0xFFFFFFFF)
            return pcg(s).view(F32).reshape(a.shape)
    raise KeyError(name)


def ref_grad_value(name, a):
    """the value a unary opcode gives in the gradient evaluator where it is not the f32 evaluator's: abs is `if v < 0 { -v } else { v }`
    there (types/grad.rs:44-55), which keeps a -0, while f32::abs clears the sign"""
    a = np.asarray(a, F32)
    if name == "abs":
        with np.errstate(all="ignore"):
            return np.where(a < 0, -a, a).astype(F32)
    return ref_unary(name, a)


def same_bits(got, want):
    """per element: bits equal, or both NaN"""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    return (got.view(U32) == want.view(U32)) | (np.isnan(got) & np.isnan(want))


def first_diff(got, want, *inputs):
    bad = np.nonzero(~same_bits(got, want))[0]
    if not len(bad):
        return "no difference"
    i = int(bad[0])
    ins = ", ".join(hex(int(_bits(x)[i])) for x in inputs)
    return f"{len(bad)} of {len(got)} differ, first at lane {i}: inputs {ins}, got {hex(int(_bits(got)[i]))}, want {hex(int(_bits(want)[i]))}"


# ---- single-op shapes ------------------------------------------------------------------------------
def forms(name):
    """the operand forms an opcode has on a tape"""
    if name in UNARY:
        return ["u"]
    if name in COMMUTATIVE or name in ("and_", "or_"):       # (and_ / or_ of an immediate and x: the branch is known, there is no such opcode)
        return ["rr", "ri"]
    return ["rr", "ri", "ir"]


def op_name(name, form):
    return OPCODE[name] + FORM_SUFFIX[form]


def live_values(c, v, n):
    """n values of v that are all live at once (test_spills.many_live_values, small): each is used by a min chain, then by a sum"""
    ts = [c.sub(c.square(c.sub(v, 0.1 * i - 0.7)), 0.01 + 0.001 * i) for i in range(n)]
    a = ts[0]
    for t in ts[1:]:
        a = c.min(a, t)
    b = ts[0]
    for t in ts[1:]:
        b = c.add(b, c.mul(t, 1e-6))
    return c.add(a, c.mul(b, 1e-9))


WIDE_N = 20


def single_op(be, name, form, imm=None, keep=False, trans=False, wide=False):
    """A shape whose first root is one opcode of x (and y, or an immediate).  Further roots pin the tape to a kernel or a handler:
    keep - x itself (the opcode cannot work in place); trans - rand(z), or z mod 3 beside a rand under test (the tape takes the kernels with the compiled routines);
    wide - WIDE_N values of z live at once (more than 16 registers)."""
    c = be.Context()
    x, y, z = c.x(), c.y(), c.z()
    fn = getattr(c, name)
    node = {"u": lambda: fn(x), "rr": lambda: fn(x, y), "ri": lambda: fn(x, float(imm)), "ir": lambda: fn(float(imm), x)}[form]()
    roots = [node]
    if keep:
        roots.append(x)
    if trans:
        roots.append(c.modulo(z, 3.0) if name == "rand" else c.rand(z))
    if wide:
        roots.append(live_values(c, z, WIDE_N))
    s = be.Shape(c, roots=roots) if len(roots) > 1 else be.Shape(c, node)
    s._ctx = c          # (the nodes live in the context)
    return s


# The five ways the bulk f32 evaluator runs a tape (capi_eval.hpp bulk_eval), pinned by what the tape holds: the assembly kernels take
# up to 16 registers four samples a lane, up to 32 two samples a lane, each in a text of its own (_t) once the tape holds an opcode that
# calls a compiled routine; the HIP kernel k_eval_f32 runs under the context option no_asm.
PATHS = ["fh_float_eval_16x4", "fh_float_eval_16x4_t", "fh_float_eval_32x2", "fh_float_eval_32x2_t", "k_eval_f32"]
PATH_SLOTS = {"fh_float_eval_16x4": (1, 16), "fh_float_eval_16x4_t": (1, 16), "fh_float_eval_32x2": (17, 32), "fh_float_eval_32x2_t": (17, 32),
              "k_eval_f32": (1, 16)}
COMPILED = ("Sin", "Cos", "Tan", "Asin", "Acos", "Atan", "Exp", "Ln", "Rand", "Atan2", "Mix", "Mod")


def path_shape(be, path, name, form, imm=None, keep=False):
    return single_op(be, name, form, imm, keep=keep, trans=path.endswith("_t"), wide="32x2" in path)


def takes_compiled_routines(shape):
    return any(op.startswith(COMPILED) for op, _, _, _ in _records(shape))


def _records(shape):
    """(opcode name with its form suffix, out, a, b or input slot) per op, evaluation order: the device tape's ops() of the product, the
    register tape of the oracle"""
    if hasattr(shape, "ops"):
        return [(r[0], r[1], r[2], r[3]) for r in shape.ops()]
    suffix = {"": "", "Reg": "", "RegReg": "RR", "RegImm": "RI", "ImmReg": "IR"}
    return [(r[0] + suffix[r[1]], r[2], r[3], r[5] if r[0] == "Input" else r[4]) for r in shape.asm_ops()]


def the_op(shape, name, form):
    """((out, a, b) registers of the opcode under test, {register: input slot} as it runs), or (None, ..) when the front end folded
    the form away"""
    src, hit = {}, None
    for op, out, a, b in _records(shape):
        if op == "Input":
            src[out] = b
        elif op == op_name(name, form) and hit is None:
            hit = ((out, a, b), dict(src))
        elif op != "Output":
            src.pop(out, None)          # the register was overwritten
    return hit if hit is not None else (None, src)


def in_place(shape, name, form):
    (out, a, _), _ = the_op(shape, name, form)
    return out == a


def operand_axes(shape, name, form):
    """(axis of a, axis of b or None): which of x, y, z the tape's opcode takes first"""
    rec, src = the_op(shape, name, form)
    ax = {shape.axis_index(k): k for k in range(3) if shape.axis_index(k) >= 0}
    return ax[src[rec[1]]], (ax[src[rec[2]]] if form == "rr" else None)


def operands(shape, name, form, imm, by_slot):
    """(a, b) as the tape's opcode takes them: by_slot maps an input slot to its array.  A commutative opcode's operands are in the
    order the Context gave them, which min / max show on a tie (the second operand when equal)."""
    rec, src = the_op(shape, name, form)
    assert rec is not None, f"{name} {form} {imm}: folded away"
    a = by_slot[src[rec[1]]]
    if form == "u":
        return a, None
    if form == "rr":
        return a, by_slot[src[rec[2]]]
    i = np.full(len(a), imm, F32)
    return (a, i) if form == "ri" else (i, a)


# ---- immediate forms -------------------------------------------------------------------------------
# The immediate forms the front end folds away (context/mod.rs: identities and absorbing constants), by (opcode, form): the immediates
# that leave no such opcode on the tape.  and_ / or_ with the immediate FIRST fold for every immediate (the branch is known).
FOLDED = {
    ("add", "ri"): {-0.0},              # x + -0 = x  (the check is `== 0`: +0 folds as well)
    ("sub", "ri"): {-0.0},              # x - 0 = x
    ("sub", "ir"): {-0.0},              # 0 - x = neg(x)
    ("mul", "ri"): {-0.0, 1.0},         # x * 0 = 0, x * 1 = x
    ("div", "ri"): {1.0},               # x / 1 = x
    ("div", "ir"): {-0.0},              # 0 / x = 0
    ("or_", "ri"): {-0.0},              # or(x, 0) = x
    ("and_", "ir"): set(IMMEDIATES),
    ("or_", "ir"): set(IMMEDIATES),
}


def folded(name, form, imm):
    return any(imm == v and np.signbit(imm) == np.signbit(v) for v in FOLDED.get((name, form), ()))


def imm_cases(name):
    return [(form, imm) for form in forms(name) if form != "rr" for imm in IMMEDIATES if not folded(name, form, imm)]


# ---- interval evaluators -----------------------------------------------------------------------------
def oracle_intervals(shape, v):
    """v [n, n_vars, 2] -> (out [n, 2], choices [n, n_choices], simplify [n]) by the oracle's interval evaluator, one call per interval"""
    import oracle as O
    v = np.ascontiguousarray(v, F32)
    n, nv = v.shape[0], v.shape[1]
    nc = shape.choice_count()
    out = np.zeros((n, max(shape.output_count(), 1), 2), F32)
    ch = np.zeros((n, max(nc, 1)), np.uint8)
    simp = np.zeros(n, np.uint8)
    fn = O.lib().orc_eval_interval
    pv, po, pc = v.ctypes.data, out.ctypes.data, ch.ctypes.data
    sv, so, sc = v.strides[0], out.strides[0], ch.strides[0]
    h = shape._h
    for i in range(n):
        simp[i] = fn(h, pv + i * sv, nv, po + i * so, pc + i * sc) == 1
    return out[:, 0, :], ch[:, :nc], simp


def oracle_points(shape, v):
    """v [n, n_vars] -> (out [n], choices [n, n_choices], simplify [n]) by the oracle's tracing point evaluator"""
    import oracle as O
    v = np.ascontiguousarray(v, F32)
    n, nv = v.shape[0], v.shape[1]
    nc = shape.choice_count()
    out = np.zeros((n, max(shape.output_count(), 1)), F32)
    ch = np.zeros((n, max(nc, 1)), np.uint8)
    simp = np.zeros(n, np.uint8)
    fn = O.lib().orc_eval_point
    pv, po, pc = v.ctypes.data, out.ctypes.data, ch.ctypes.data
    sv, so, sc = v.strides[0], out.strides[0], ch.strides[0]
    h = shape._h
    for i in range(n):
        simp[i] = fn(h, pv + i * sv, nv, po + i * so, pc + i * sc) == 1
    return out[:, 0], ch[:, :nc], simp


def interval_vars(shape, by_axis):
    """[n, n_vars, 2] from per-axis (lo, hi)"""
    n = len(by_axis[0][0])
    v = np.zeros((n, max(shape.var_count(), 1), 2), F32)
    by_slot = {}
    for axis, (lo, hi) in enumerate(by_axis):
        i = shape.axis_index(axis)
        if i >= 0:
            v[:, i, 0], v[:, i, 1] = lo, hi
            by_slot[i] = axis
    return v, by_slot


def sample_values(shape, name, form, imm, by_axis, by_slot, seed):
    """the float64 reference at 8 points of each operand interval (8 x 8 for two): [n, 8] or [n, 8, 8]"""
    pts = {slot: samples(*by_axis[axis], 8, seed + axis) for slot, axis in by_slot.items()}
    rec, src = the_op(shape, name, form)
    a = pts[src[rec[1]]]
    if form == "u":
        return ref_unary(name, a)
    if form == "rr":
        return ref_binary(name, a[:, :, None], pts[src[rec[2]]][:, None, :])
    i = np.full(a.shape, imm, F32)
    return ref_binary(name, a, i) if form == "ri" else ref_binary(name, i, a)


IV_IMMEDIATES = [3.0, -7.77]                                   # every interval; the immediates below on a tenth of them
IV_IMMEDIATES_FEW = [-0.0, 1e-40, 1e30, float("inf")]


def interval_cases(name, n):
    """(form, immediate, number of intervals)"""
    out = []
    for form in forms(name):
        if form in ("u", "rr"):
            out.append((form, None, n))
            continue
        out += [(form, imm, n) for imm in IV_IMMEDIATES if not folded(name, form, imm)]
        out += [(form, imm, n // 10) for imm in IV_IMMEDIATES_FEW if not folded(name, form, imm)]
    return out


def check_sound(label, lo, hi, v):
    bad = violations(lo, hi, v)
    if bad.any():
        i = int(np.nonzero(bad.reshape(len(lo), -1).any(axis=1))[0][0])
        raise AssertionError(f"{label}: {int(bad.reshape(len(lo), -1).any(axis=1).sum())} intervals exclude a value of their operands, first "
                             f"interval {i}: [{lo[i]!r}, {hi[i]!r}] excludes {v[i][bad[i]].ravel()[0]!r}")
