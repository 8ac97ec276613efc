"""An independent float64 reference for gradients: forward-mode duals in plain numpy, over an expression recorder.

Nothing here reads the product's tapes, the oracle, or their models of the reference's grad.rs.  The derivative rules are the calculus ones
(d sin = cos, quotient rule, ...), evaluated in float64 on the float32 arguments widened exactly.  Only what calculus leaves open - the value
taken AT a non-differentiable point - follows the reference, and each such convention names the line it restates (fidget-core/src/types/grad.rs).

  Rec      wraps any backend's Context (oracle, fidget_amd, or None), forwards each call and keeps its own tree, so that one expression
           exists on the backend and here.  Inputs are x, y, z (keys 0, 1, 2 of `evaluate`'s inputs) and var(i) (key ("v", i)).
  read_vm  the .vm text format of models/ into a Rec.
  D        a value and P partials per point, float64.
  evaluate a Rec node at seeded inputs; also reports which points lie within `tol` of a tie or a step.
  xf       a 4 x 4 matrix applied to seeded coordinates and the division by w, numerically (D) or folded into a Rec.
"""
import numpy as np

from kat_util import f_mix, f_rand

F64 = np.float64
F32_MAX = float(np.finfo(np.float32).max)


class D:
    """v: [n] float64; d: [n, P] float64.  Arithmetic by the sum, product and quotient rules."""
    __slots__ = ("v", "d")

    def __init__(self, v, d):
        self.v, self.d = np.asarray(v, F64), np.asarray(d, F64)

    @staticmethod
    def const(c, n, p=3):
        return D(np.full(n, c, F64), np.zeros((n, p), F64))

    @staticmethod
    def seed(v, axis, p=3):
        """an input: the f32 values widened exactly, unit partial along `axis` (None: no partial)"""
        v = np.asarray(np.asarray(v, np.float32), F64)
        d = np.zeros((len(v), p), F64)
        if axis is not None:
            d[:, axis] = 1.0
        return D(v, d)

    def _lift(self, o):
        return o if isinstance(o, D) else D.const(o, len(self.v), self.d.shape[1])

    def __neg__(self): return D(-self.v, -self.d)
    def __add__(self, o): o = self._lift(o); return D(self.v + o.v, self.d + o.d)
    def __sub__(self, o): o = self._lift(o); return D(self.v - o.v, self.d - o.d)
    def __mul__(self, o): o = self._lift(o); return D(self.v * o.v, self.d * o.v[:, None] + o.d * self.v[:, None])

    def __truediv__(self, o):
        # d(a/b) = a'/b - a b'/b^2; a term whose partial is exactly zero contributes nothing (0 * inf is not formed)
        o = self._lift(o)
        v = self.v / o.v
        t1 = np.where(self.d != 0, self.d / o.v[:, None], 0.0)
        t2 = np.where(o.d != 0, o.d * (self.v / (o.v * o.v))[:, None], 0.0)
        return D(v, t1 - t2)

    __radd__ = __add__
    def __rsub__(self, o): return self._lift(o) - self
    __rmul__ = __mul__
    def __rtruediv__(self, o): return self._lift(o) / self


def _chain(a, v, dv):
    """f(a) with f' = dv.  A zero partial stays zero whatever f' is (the partials of an axis the expression does not depend on)."""
    return D(v, np.where(a.d != 0, a.d * dv[:, None], 0.0))


def _select(m, a, b):
    return D(np.where(m, a.v, b.v), np.where(m[:, None], a.d, b.d))


def _flat(v, n, p):
    return D(v, np.zeros((n, p), F64))


def _frac_dist(q):
    """distance of q to the nearest integer"""
    return np.abs(q - np.round(q))


class Near:
    """Finds, per point, whether the result hangs on a node that is within `tol` of a tie or a step - from the f64 values alone.

    Every such node has a quantity that decides it: a - b for min, max and compare, a for abs, floor, ceil, round, and, or, a / b for modulo.
    A node is near its tie at a point when
      - that quantity is within tol of the tie or step, and
      - it moves there (has a non-zero partial).  A decider without partials is locally constant: two clamped terms that are both exactly
        0, a 0 / 1 flag, the hash of a grid cell.  Nothing near the point changes the choice, and where both operands of a min carry the same
        partials either choice gives the same gradient.  (prospero.vm is at a min or max of two clamped zeros at every point of space.)
    and the point counts as near when such a node is one the result depends on there: `evaluate` walks back from the root and follows,
    through min, max, and, or, only the operand that was chosen (both, at a node that is itself near its tie).  A tie between two terms that
    a later min or max discards cannot reach the result.  (A few thousand min / max nodes of prospero.vm put a third of all points within
    1e-4 of a tie somewhere in the tree; on the path to the result it is the fraction of a percent the test allows.)"""
    def __init__(self, n, tol):
        self.n, self.tol = n, tol
        self.at, self.chose_a, self.beyond, self.cur = {}, {}, {}, None

    def add(self, close, decider_d):
        self.at[self.cur] = close & (decider_d != 0).any(axis=1)

    def choice(self, chose_a):
        self.chose_a[self.cur] = chose_a

    def range(self, r):
        """... and a point is left out as well where a node the result depends on has a finite value or partial that float32 cannot hold
        (beyond 3.4e38): exp(85) with a partial of 6e38 inside a smooth minimum of bear.vm is
        infinite in any float32 evaluation, whatever its derivative rules."""
        m = np.abs(np.c_[r.v, r.d])
        bad = (np.isfinite(m) & (m > F32_MAX)).any(axis=1)
        if bad.any():
            self.beyond[self.cur] = bad


def _unary(op, a, near):
    v, n, p = a.v, len(a.v), a.d.shape[1]
    with np.errstate(all="ignore"):
        if op == "neg": return -a
        if op == "abs":
            # grad.rs:44-55: the negated branch only for v < 0, so |.| at 0 takes the + side (and -0.0 stays -0.0)
            if near: near.add(np.abs(v) < near.tol, a.d)
            return _select(v < 0, -a, a)
        if op == "recip": return _chain(a, 1.0 / v, -1.0 / (v * v))
        if op == "sqrt":
            s = np.sqrt(v)
            return _chain(a, s, 0.5 / s)
        if op == "square": return _chain(a, v * v, 2.0 * v)
        if op == "sin": return _chain(a, np.sin(v), np.cos(v))
        if op == "cos": return _chain(a, np.cos(v), -np.sin(v))
        if op == "tan":
            c = np.cos(v)
            return _chain(a, np.tan(v), 1.0 / (c * c))
        if op == "asin": return _chain(a, np.arcsin(v), 1.0 / np.sqrt((1.0 - v) * (1.0 + v)))
        if op == "acos": return _chain(a, np.arccos(v), -1.0 / np.sqrt((1.0 - v) * (1.0 + v)))
        if op == "atan": return _chain(a, np.arctan(v), 1.0 / (1.0 + v * v))
        if op == "exp":
            e = np.exp(v)
            return _chain(a, e, e)
        if op == "ln": return _chain(a, np.log(v), 1.0 / v)
        # piecewise constant functions: partials 0 everywhere, steps included (grad.rs:227-256 floor / ceil / round, :283-285 not)
        if op == "floor":
            if near: near.add(_frac_dist(v) < near.tol, a.d)
            return _flat(np.floor(v), n, p)
        if op == "ceil":
            if near: near.add(_frac_dist(v) < near.tol, a.d)
            return _flat(np.ceil(v), n, p)
        if op == "round":
            # f32::round is half away from zero; its steps are at the half-integers
            if near: near.add(_frac_dist(v - 0.5) < near.tol, a.d)
            return _flat(np.copysign(np.floor(np.abs(v) + 0.5), v), n, p)
        if op == "not": return _flat((v == 0).astype(F64), n, p)
        if op == "rand":
            # a hash of the f32 bit pattern (grad.rs:288-291): no derivative; defined on f32 values only
            return _flat(np.array([f_rand(float(np.float32(x))) for x in v], F64), n, p)
    raise NotImplementedError(op)


def _binary(op, a, b, near):
    n, p = len(a.v), a.d.shape[1]
    with np.errstate(all="ignore"):
        if op == "add": return a + b
        if op == "sub": return a - b
        if op == "mul": return a * b
        if op == "div": return a / b
        if op == "atan2":
            # atan2(y, x): d/dy = x / (x^2 + y^2), d/dx = -y / (x^2 + y^2)
            y, x = a, b
            r2 = x.v * x.v + y.v * y.v
            t1 = np.where(y.d != 0, y.d * (x.v / r2)[:, None], 0.0)
            t2 = np.where(x.d != 0, x.d * (y.v / r2)[:, None], 0.0)
            return D(np.arctan2(y.v, x.v), t1 - t2)
        if op in ("min", "max"):
            # grad.rs:173-195: NaN (no partials) if either is NaN; a tie takes the right-hand side
            if near: near.add(np.abs(a.v - b.v) < near.tol, a.d - b.d)
            first = a.v < b.v if op == "min" else a.v > b.v
            if near: near.choice(first)
            r = _select(first, a, b)
            un = np.isnan(a.v) | np.isnan(b.v)
            return _select(un, D.const(np.nan, n, p), r)
        if op == "compare":
            # grad.rs:273-279: -1 / 0 / 1 (NaN if unordered), no partials
            if near: near.add(np.abs(a.v - b.v) < near.tol, a.d - b.d)
            v = np.where(a.v < b.v, -1.0, np.where(a.v > b.v, 1.0, np.where(a.v == b.v, 0.0, np.nan)))
            return _flat(v, n, p)
        if op == "mod":
            # grad.rs:199-207: a' - b' * floor(a / b) (div_euclid), the derivative of a - b * floor(a / b) away from the steps of the floor;
            # the value is the least non-negative remainder
            q = a.v / b.v
            if near: near.add(_frac_dist(q) < near.tol, a.d * b.v[:, None] - b.d * a.v[:, None])
            r = np.fmod(a.v, b.v)
            r = np.where(r < 0, r + np.abs(b.v), r)
            e = np.where(b.v > 0, np.floor(q), np.ceil(q))     # div_euclid: the quotient that leaves a remainder >= 0
            return D(r, a.d - np.where(b.d != 0, b.d * e[:, None], 0.0))
        if op in ("and", "or"):
            # grad.rs:213-223: and -> a if a == 0 else b; or -> a if a != 0 else b, value and partials together.
            # The selector steps where a crosses 0; a 0 / 1 flag sits at 0 without partials (its own steps are found at the compare that made it)
            if near: near.add(np.abs(a.v) < near.tol, a.d)
            first = a.v == 0 if op == "and" else a.v != 0
            if near: near.choice(first)
            return _select(first, a, b)
        if op == "mix":
            # a hash of two f32 bit patterns (grad.rs:294-298): no derivative
            v = np.array([f_mix(float(np.float32(x)), float(np.float32(y))) for x, y in zip(a.v, b.v)], F64)
            return _flat(v, n, p)
    raise NotImplementedError(op)


UNARY = ["neg", "abs", "recip", "sqrt", "square", "floor", "ceil", "round", "sin", "cos", "tan", "asin", "acos", "atan", "exp", "ln",
         "not", "rand"]
BINARY = ["add", "sub", "mul", "div", "atan2", "min", "max", "compare", "mod", "and", "or", "mix"]
_PY = {"not": "not_", "and": "and_", "or": "or_", "mod": "modulo"}


class N:
    """a recorded node: `i` in the recorder's own tree, `be` the backend's node (None without a backend)"""
    __slots__ = ("i", "be")

    def __init__(self, i, be):
        self.i, self.be = i, be


class Rec:
    """Records an expression while building it on a backend.  Numbers passed as operands reach the backend as numbers (so that it forms
    its immediate operand forms) and are kept here as the float32 they become there."""
    def __init__(self, ctx=None):
        self.ctx, self.nodes = ctx, []

    def _new(self, rec, be):
        self.nodes.append(rec)
        return N(len(self.nodes) - 1, be)

    def _arg(self, a):
        """-> (index in the tree, what to hand to the backend)"""
        if isinstance(a, N):
            return a.i, a.be
        self.nodes.append(("const", float(np.float32(a))))
        return len(self.nodes) - 1, float(a)

    def _fwd(self, name, *args):
        return None if self.ctx is None else getattr(self.ctx, name)(*args)

    def x(self): return self._new(("in", 0), self._fwd("x"))
    def y(self): return self._new(("in", 1), self._fwd("y"))
    def z(self): return self._new(("in", 2), self._fwd("z"))
    def var(self, index): return self._new(("in", ("v", int(index))), self._fwd("var", int(index)))   # Var::V(index); input key ("v", index)
    def constant(self, f): return self._new(("const", float(np.float32(f))), self._fwd("constant", f))

    def unary(self, op, a):
        i, be = self._arg(a)
        return self._new((op, i), self._fwd(_PY.get(op, op), be))

    def binary(self, op, a, b):
        (i, bea), (j, beb) = self._arg(a), self._arg(b)
        return self._new((op, i, j), self._fwd(_PY.get(op, op), bea, beb))


def _mk(kind, op):
    return (lambda self, a: self.unary(op, a)) if kind == 1 else (lambda self, a, b: self.binary(op, a, b))


for _o in UNARY:
    setattr(Rec, _PY.get(_o, _o), _mk(1, _o))
for _o in BINARY:
    setattr(Rec, _PY.get(_o, _o), _mk(2, _o))


def read_vm(rec, text, axes=None):
    """The text format of models/ (`name op args...`, `#` comments) into `rec`; the last line is the root.  axes: three recorded nodes that
    stand for var-x, var-y, var-z (default: the recorder's own x, y, z)."""
    names, last = {}, None
    ax = {}
    for line in text.splitlines():
        t = line.split()
        if not t or t[0].startswith("#"):
            continue
        name, op, args = t[0], t[1], t[2:]
        if op == "const":
            node = rec.constant(float(args[0]))
        elif op in ("var-x", "var-y", "var-z"):
            k = "xyz".index(op[-1])
            if k not in ax:
                ax[k] = axes[k] if axes is not None else (rec.x, rec.y, rec.z)[k]()
            node = ax[k]
        elif op in UNARY and len(args) == 1:
            node = rec.unary(op, names[args[0]])
        elif op in BINARY and len(args) == 2:
            node = rec.binary(op, names[args[0]], names[args[1]])
        else:
            raise ValueError(f"unknown line: {line!r}")
        names[name] = last = node
    return last


def evaluate(rec, root, inputs, tol=None):
    """inputs: {axis: D}; returns (D of `root`, mask of the points near a tie or a step as `Near` defines it; None without tol)."""
    any_in = next(iter(inputs.values()))
    n, p = len(any_in.v), any_in.d.shape[1]
    near = Near(n, tol) if tol is not None else None
    # the nodes `root` depends on, in recording order (operands precede their users), and each one's last user
    last, stack = {}, [root.i]
    while stack:
        i = stack.pop()
        if i not in last:
            last[i] = i
            stack.extend(_operands(rec.nodes[i]))
    order = sorted(last)
    for i in order:
        for j in _operands(rec.nodes[i]):
            last[j] = max(last[j], i)
    val = {}
    for i in order:
        r = rec.nodes[i]
        if near: near.cur = i
        if r[0] == "in":
            val[i] = inputs[r[1]]
        elif r[0] == "const":
            val[i] = D.const(r[1], n, p)
        elif len(r) == 2:
            val[i] = _unary(r[0], val[r[1]], near)
        else:
            val[i] = _binary(r[0], val[r[1]], val[r[2]], near)
        if near and r[0] not in ("in", "const"):
            near.range(val[i])
        for j in set(_operands(r)):
            if last[j] == i:
                del val[j]
    if near is None:
        return val[root.i], None
    # which nodes the result depends on, point by point, from the root down
    live = {root.i: np.ones(n, bool)}
    out = np.zeros(n, bool)
    for i in reversed(order):
        m = live.pop(i, None)
        if m is None or not m.any():
            continue
        here = near.at.get(i)
        if here is not None:
            out |= m & here
        if i in near.beyond:
            out |= m & near.beyond[i]
        r = rec.nodes[i]
        ops = _operands(r)
        if i in near.chose_a:
            first = near.chose_a[i]
            both = here if here is not None else False
            masks = [m, m & (~first | both)] if r[0] in ("and", "or") else [m & (first | both), m & (~first | both)]
        else:
            masks = [m] * len(ops)
        for j, mj in zip(ops, masks):
            live[j] = live[j] | mj if j in live else mj
    return val[root.i], out


def _operands(r):
    return () if r[0] in ("in", "const") else r[1:]


def seeds(x, y, z):
    """x, y, z with the identity as partials (what eval_grad_slice seeds)"""
    return {0: D.seed(x, 0), 1: D.seed(y, 1), 2: D.seed(z, 2)}


def xf(m, x, y, z):
    """rows 0..2 of the 4 x 4 matrix `m` (16 float32, row major) applied to (x, y, z, 1), each divided by row 3's: three D.
    x, y, z: D, or arrays (then seeded with the identity)."""
    m = np.asarray(np.asarray(m, np.float32), F64).reshape(4, 4)
    if not isinstance(x, D):
        s = seeds(x, y, z)
        x, y, z = s[0], s[1], s[2]
    r = [x * m[i, 0] + y * m[i, 1] + z * m[i, 2] + m[i, 3] for i in range(4)]
    return [r[i] / r[3] for i in range(3)]


def xf_fold(rec, m):
    """the same transform as recorded nodes over rec's x, y, z: the axes of a shape seen through `m`"""
    m = np.asarray(m, np.float32).reshape(4, 4)
    x, y, z = rec.x(), rec.y(), rec.z()
    r = [rec.add(rec.add(rec.add(rec.mul(x, float(m[i, 0])), rec.mul(y, float(m[i, 1]))), rec.mul(z, float(m[i, 2]))), float(m[i, 3]))
         for i in range(4)]
    return [rec.div(r[i], r[3]) for i in range(3)]


def measure(g32, g64):
    """|g32 - g64|_inf / max(|g64|_inf, 1) per point, over the partials ([n, P] each)"""
    g64 = np.asarray(g64, F64)
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(g32, F64) - g64).max(axis=1) / np.maximum(np.abs(g64).max(axis=1), 1.0)


class View:
    """`rec` with other axes: x(), y(), z() give the three nodes `axes` (a shape seen through a transform); every other call is rec's"""
    def __init__(self, rec, axes):
        self._rec, self._axes = rec, axes

    def x(self): return self._axes[0]
    def y(self): return self._axes[1]
    def z(self): return self._axes[2]

    def __getattr__(self, name):
        return getattr(self._rec, name)
