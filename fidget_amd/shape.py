"""The expression front end: `Context` (host mirror of fidget_core::Context), `Shape` (one function compiled to a device tape, with the
evaluators) and the f32 matrix helpers that keep the C++ driver's operation order."""
import ctypes as C
import os

import numpy as np

from ._abi import BINARY, FH_OPS, STATUS, UNARY, FidgetHipError, _p, lib
from .context import default_context

BAD_NODE = 0xFFFFFFFF


class BadNode(Exception):
    pass


class Node(int):
    pass


class Context:
    """Host mirror of fidget_core::Context (constructor identities, dedup, .vm text)."""

    def __init__(self):
        self._h = C.c_void_p(lib().fhip_graph_new())

    def __del__(self):
        try:
            lib().fhip_graph_free(self._h)
        except Exception:
            pass

    def __len__(self):
        return lib().fhip_graph_len(self._h)

    def _node(self, v):
        if isinstance(v, (float, int)) and not isinstance(v, Node):
            return self.constant(float(v))
        return v

    def x(self): return Node(lib().fhip_graph_var(self._h, 0, 0))
    def y(self): return Node(lib().fhip_graph_var(self._h, 1, 0))
    def z(self): return Node(lib().fhip_graph_var(self._h, 2, 0))
    def var(self, index): return Node(lib().fhip_graph_var(self._h, 3, int(index)))
    def constant(self, f): return Node(lib().fhip_graph_constant(self._h, float(f)))

    def _un(self, name, a):
        r = lib().fhip_graph_unary(self._h, UNARY.index(name), int(self._node(a)))
        if r == BAD_NODE:
            raise BadNode()
        return Node(r)

    def _bin(self, name, a, b):
        r = lib().fhip_graph_binary(self._h, BINARY.index(name), int(self._node(a)), int(self._node(b)))
        if r == BAD_NODE:
            raise BadNode()
        return Node(r)

    # derived constructors (context/mod.rs:701-780)
    def less_than(self, lhs, rhs):
        return self.max(self._bin("compare", rhs, lhs), 0.0)

    def less_than_or_equal(self, lhs, rhs):
        return self.min(self.add(self._bin("compare", rhs, lhs), 1.0), 1.0)

    def if_nonzero_else(self, cond, a, b):
        cond, a, b = self._node(cond), self._node(a), self._node(b)
        lhs = self.and_(cond, a)
        rhs = self.and_(self.not_(cond), b)
        return self.or_(lhs, rhs)

    @staticmethod
    def from_text(text):
        ctx = Context()
        if isinstance(text, str):
            text = text.encode()
        r = lib().fhip_graph_from_text(ctx._h, text)
        if r == BAD_NODE:
            raise ValueError("parse error")
        return ctx, Node(r)


def _mk_un(name):
    def f(self, a):
        return self._un(name, a)
    return f


def _mk_bin(name):
    def f(self, a, b):
        return self._bin(name, a, b)
    return f


for _n in UNARY:
    setattr(Context, {"not": "not_"}.get(_n, _n), _mk_un(_n))
for _n in BINARY:
    setattr(Context, {"and": "and_", "or": "or_", "mod": "modulo"}.get(_n, _n), _mk_bin(_n))


class Shape:
    """One function compiled to a device tape (the role of `Shape<HipFunction>`)."""

    def __init__(self, ctx=None, node=None, n_regs=255, _h=None, roots=None, hip=None, _vars=None):
        # n_regs is accepted for signature parity with GenericVmFunction<N>; device tapes
        # always use dense renumbering over up to 256 registers (no spills).
        self._hip = hip  # created lazily: tape construction and simplify are host-only
        self.n_regs = n_regs
        if _h is not None:
            self._h = _h
            self._vars = _vars
            return
        if roots is None:
            roots = [node]
        r = np.array([int(n) for n in roots], dtype=np.uint32)
        h = C.c_void_p()
        st = lib().fhip_tape_from_graph(None, ctx._h, _p(r), len(r), C.byref(h))
        if st != 0:
            raise FidgetHipError(st, "tape construction failed")
        self._h = h
        self._vars = None

    @property
    def hip(self):
        if self._hip is None:
            self._hip = default_context()
        return self._hip

    def __del__(self):
        try:
            lib().fhip_tape_free(self._h)
        except Exception:
            pass

    def groups(self):
        """Tape parallelism: (combining op name, [Shape of each independent sub-tape]); ('', []) if the
        root of the function is not a min / max of many parts."""
        n = lib().fhip_tape_group_count(self._h)
        out = []
        for g in range(n):
            h = C.c_void_p()
            st = lib().fhip_tape_group(None, self._h, g, C.byref(h))
            if st != 0:
                raise FidgetHipError(st, "tape group")
            out.append(Shape(_h=h, hip=self._hip, _vars=self._vars))
        op = lib().fhip_tape_group_op(self._h)
        return ({30: "min", 31: "max"}.get(op, ""), out)

    def term_parts(self):
        """(group Shapes, tree ops as an (n, 3) u32 array, choice sources as a u32 array) of term_plan()."""
        n = self.term_plan()
        gs = []
        for g in range(n["groups"]):
            h = C.c_void_p()
            st = lib().fhip_tape_term_group(None, self._h, g, C.byref(h))
            if st != 0:
                raise FidgetHipError(st, "term group")
            gs.append(Shape(_h=h, hip=self._hip, _vars=self._vars))
        tree = np.zeros((max(n["tree_ops"], 1), 3), np.uint32)
        lib().fhip_tape_term_tree(self._h, _p(tree), n["tree_ops"])
        src = np.zeros(max(n["choices"], 1), np.uint32)
        lib().fhip_tape_term_choice_src(self._h, _p(src), n["choices"])
        return gs, tree[:n["tree_ops"]], src[:n["choices"]]

    def term_plan(self):
        """The renderer's root-level split: dict(groups, terms, tree_ops, tree_regs, choices); groups = 0 if none."""
        info = (C.c_uint32 * 4)()
        n = lib().fhip_tape_term_plan(self._h, info)
        return dict(groups=n, terms=info[0], tree_ops=info[1], tree_regs=info[2], choices=info[3])

    @staticmethod
    def from_vm(path_or_text, n_regs=255, hip=None):
        text = open(path_or_text).read() if os.path.exists(path_or_text) else path_or_text
        ctx, root = Context.from_text(text)
        return Shape(ctx, root, n_regs, hip=hip)

    @staticmethod
    def from_bytecode(words, axis_slots=(0, 1, 2), hip=None):
        """The reference wire format (fidget_bytecode::Bytecode::data()); axis_slots = VarMap slots of X, Y, Z."""
        w = np.ascontiguousarray(words, dtype=np.uint32)
        h = C.c_void_p()
        st = lib().fhip_tape_from_bytecode(None, _p(w), len(w), C.byref(h))
        if st != 0:
            raise FidgetHipError(st, "bad bytecode")
        return Shape(_h=h, hip=hip, _vars=tuple(axis_slots))

    # sizes ---------------------------------------------------------------
    def device_len(self): return lib().fhip_tape_len(self._h)

    def size(self):
        """Function::size (eval/mod.rs:171) = VmData<N>::len(): the device tape's length - one op per SSA op - or, for a Shape made with
        fewer than 255 registers, the reference's RegTape under that limit with its loads and stores (fhip_tape_reg_tape)."""
        if self.n_regs == 255 and lib().fhip_tape_reg_count(self._h) <= 255:
            return self.device_len()
        return int(self.reg_tape()[1][0])     # (also for a tape that needs more than 255 registers: VmData<255>::len() counts its loads / stores)
    __len__ = size
    def ssa_len(self): return self.device_len()  # device tapes carry no load/store: one op per SSA op

    def reg_tape(self, n_regs=None, want_words=False):
        """RegTape::new::<N> + Bytecode::new of this tape (host side): ([(op, form, out, a, b, idx, imm bits)] in evaluation order - the
        oracle's asm_ops() records -, (len, slot_count, reg_count, mem_count)[, bytecode words])."""
        n_regs = self.n_regs if n_regs is None else n_regs
        info = np.zeros(4, np.uint32)
        st = lib().fhip_tape_reg_tape(self._h, n_regs, None, 0, None, 0, _p(info))
        if st not in (0, 6):
            raise FidgetHipError(st, "register allocation")
        n = int(info[0])
        rec = np.zeros((n, 4), np.uint32)
        words = np.zeros(2 * n + 4, np.uint32)
        st = lib().fhip_tape_reg_tape(self._h, n_regs, _p(rec), n, _p(words), len(words), _p(info))
        if want_words and st == 6:
            raise ValueError("ReservedRegister")
        NAMES = ["Output", "Input", "CopyReg", "CopyImm", "Neg", "Abs", "Recip", "Sqrt", "Square", "Floor", "Ceil", "Round", "Sin", "Cos", "Tan",
                 "Asin", "Acos", "Atan", "Exp", "Ln", "Not", "Rand"]
        BIN = ["Add", "Sub", "Mul", "Div", "Atan2", "Compare", "Mix", "Mod", "Min", "Max", "And", "Or"]
        ops = []
        for op, o, a, w in rec.tolist():
            if op == 52: ops.append(("Load", "", o, 0, 0, w, 0))
            elif op == 53: ops.append(("Store", "", 0, a, 0, w, 0))
            elif op == 0: ops.append(("Output", "", 0, a, 0, w, 0))
            elif op == 1: ops.append(("Input", "", o, 0, 0, w, 0))
            elif op == 3: ops.append(("CopyImm", "", o, 0, 0, 0, w))
            elif op < 22: ops.append((NAMES[op], "Reg", o, a, 0, 0, 0))
            elif op < 34: ops.append((BIN[op - 22], "RegReg", o, a, w, 0, 0))
            elif op < 46: ops.append((BIN[op - 34], "RegImm", o, a, 0, 0, w))
            else: ops.append((["Sub", "Div", "Atan2", "Compare", "Mix", "Mod"][op - 46], "ImmReg", o, a, 0, 0, w))
        out = (ops, tuple(int(v) for v in info))
        return out + (words,) if want_words else out

    def asm_ops(self): return self.reg_tape()[0]

    def bytecode(self):
        """fidget_bytecode::Bytecode::new of the tape as VmData<n_regs>: (words, reg_count, mem_count)"""
        _, info, words = self.reg_tape(want_words=True)
        return words, info[2], info[3]
    def choice_count(self): return lib().fhip_tape_choice_count(self._h)
    def output_count(self): return lib().fhip_tape_output_count(self._h)
    def slot_count(self): return lib().fhip_tape_reg_count(self._h)
    def var_count(self): return lib().fhip_tape_var_count(self._h)

    def axis_index(self, axis):
        if self._vars is not None:
            return self._vars[axis]
        return lib().fhip_tape_axis_slot(self._h, axis)

    def var_index(self, index): return lib().fhip_tape_var_slot(self._h, int(index))

    def words(self):
        """Device tape as raw 8-byte ops (tape_format.h), evaluation order."""
        n = self.device_len()
        w = np.zeros(max(n, 1), dtype=np.uint64)
        lib().fhip_tape_ops(self._h, _p(w), n)
        return w[:n]

    def links(self):
        """Per-op links for the linked prune (fhip_debug_tape_links; host_graph.hpp compute_links): [n, 5] = (opcode, class, choice ordinal,
        producer of a, producer of b) - a producer is an op index, 0x8000 | ordinal for a choice op, 0xFFFF for none; None when the tape
        does not qualify."""
        n = self.device_len()
        w = np.zeros(max(n, 1), dtype=np.uint64)
        if lib().fhip_debug_tape_links(self._h, _p(w), n) != n:
            return None
        w = w[:n]
        return np.stack([w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFFFF, (w >> 32) & 0xFFFF, (w >> 48) & 0xFFFF], axis=1).astype(np.int64)

    def chain(self):
        """The root chain for the linked prune's liveness pass (fhip_debug_tape_chain): [n, 2] = (choice ordinal, op index) per chain op in
        evaluation order; empty when the root tree is no chain"""
        w = np.zeros(65536, dtype=np.uint32)
        n = lib().fhip_debug_tape_chain(self._h, _p(w), len(w))
        return np.stack([w[:n] & 0xFFFF, w[:n] >> 16], axis=1).astype(np.int64)

    def ops(self):
        """Device tape as (name, out, a, b, imm_bits) tuples in evaluation order."""
        n = self.device_len()
        w = np.zeros(max(n, 1), dtype=np.uint64)
        lib().fhip_tape_ops(self._h, _p(w), n)
        out = []
        for v in w[:n]:
            v = int(v)
            out.append((FH_OPS[v & 0xFF], (v >> 8) & 0xFFF, (v >> 20) & 0xFFF, v >> 32, v >> 32))  # (name, out, a, b|imm, imm)
        return out

    def simplify(self, choices, n_regs=None):
        c = np.ascontiguousarray(choices, dtype=np.uint8)
        h = C.c_void_p()
        st = lib().fhip_simplify(None, self._h, _p(c), len(c), C.byref(h))
        if st != 0:
            raise ValueError(STATUS.get(st, str(st)))
        return Shape(_h=h, hip=self._hip, _vars=self._vars if self._vars is not None else tuple(self.axis_index(a) for a in range(3)),
                     n_regs=self.n_regs if n_regs is None else n_regs)._with_named(self)

    def _with_named(self, parent):
        self._named_parent = parent  # children keep the parent's Var::V slots
        return self

    def _named_slot(self, index):
        p = self
        while getattr(p, "_named_parent", None) is not None:
            p = p._named_parent
        return lib().fhip_tape_var_slot(p._h, int(index))

    # evaluators ------------------------------------------------------------
    def _xyz_vars(self, x, y, z, extra=None):
        n = max(self.var_count(), 1)
        vs = [None] * n
        for axis, v in enumerate((x, y, z)):
            i = self.axis_index(axis)
            if 0 <= i < n:
                vs[i] = v
        for k, v in (extra or {}).items():
            i = self._named_slot(k)
            if 0 <= i < n:
                vs[i] = v
        return vs

    def _tracing(self, fn, v, comp):
        n, nv = v.shape[0], v.shape[1]
        no, nc = self.output_count(), self.choice_count()
        out = np.zeros((n, max(no, 1)) + ((2,) if comp == 2 else ()), dtype=np.float32)
        ch = np.zeros((n, max(nc, 1)), dtype=np.uint8)
        simp = np.zeros(n, dtype=np.uint8)
        st = fn(self.hip._h, self._h, _p(v), nv, n, _p(out), _p(ch), _p(simp))
        if st in (1, 2, 3):
            raise ValueError(STATUS[st])
        self.hip.check(st)
        return out[:, :no], ch[:, :nc], simp

    def eval_interval_batch(self, batch):
        """batch: list of per-variable (lo, hi) lists (None = [0,0]).  Returns [((lo,hi), trace|None)]."""
        v = np.array([[(0.0, 0.0) if a is None else a for a in vs] for vs in batch], dtype=np.float32)
        if v.ndim != 3:
            v = v.reshape(len(batch), -1, 2)
        out, ch, simp = self._tracing(lib().fhip_interval_eval, np.ascontiguousarray(v), 2)
        return [((float(out[i, 0, 0]), float(out[i, 0, 1])), (ch[i].copy() if simp[i] else None)) for i in range(len(batch))]

    def eval_interval_raw(self, vars_):
        v = np.array(vars_, dtype=np.float32).reshape(1, -1, 2)
        out, ch, simp = self._tracing(lib().fhip_interval_eval, v, 2)
        return out[0], (ch[0].copy() if simp[0] else None)

    def eval_interval(self, x, y, z, extra=None):
        vs = self._xyz_vars(x, y, z, extra)
        vs = [(0.0, 0.0) if v is None else ((v, v) if np.isscalar(v) else tuple(v)) for v in vs]
        out, tr = self.eval_interval_raw(vs)
        return (float(out[0][0]), float(out[0][1])), tr

    def eval_point_raw(self, vars_):
        v = np.array(vars_, dtype=np.float32).reshape(1, -1)
        out, ch, simp = self._tracing(lib().fhip_point_eval, v, 1)
        return out[0], (ch[0].copy() if simp[0] else None)

    def eval_point(self, x, y, z, extra=None):
        vs = [0.0 if v is None else v for v in self._xyz_vars(x, y, z, extra)]
        out, tr = self.eval_point_raw(vs)
        return float(out[0]), tr

    def _bulk(self, fn, arrs, comp):
        n = len(arrs[0]) // comp if arrs else 0
        lens = np.array([len(a) // comp for a in arrs], dtype=np.uint32)
        ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
        no = self.output_count()
        outs = [np.zeros(n * comp, dtype=np.float32) for _ in range(no)]
        optrs = (C.c_void_p * max(no, 1))(*[o.ctypes.data for o in outs])
        st = fn(self.hip._h, self._h, ptrs, _p(lens), len(arrs), optrs)
        if st in (1, 2, 3):
            raise ValueError(STATUS[st])
        self.hip.check(st)
        return outs

    def eval_float_slice_raw(self, arrays):
        arrs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in arrays]
        outs = self._bulk(lib().fhip_float_eval, arrs, 1)
        n = len(arrs[0]) if arrs else 0
        return np.array(outs, dtype=np.float32).reshape(self.output_count(), n)

    def eval_float_slice(self, x, y, z, extra=None):
        x, y, z = (np.asarray(a, dtype=np.float32) for a in (x, y, z))
        n = len(x)
        vs = self._xyz_vars(x, y, z, extra)
        vs = [np.zeros(n, np.float32) if v is None else (np.full(n, v, np.float32) if np.isscalar(v) else v) for v in vs]
        return self.eval_float_slice_raw(vs)[0]

    def eval_grad_slice_raw(self, arrays):
        arrs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in arrays]
        outs = self._bulk(lib().fhip_grad_eval, arrs, 4)
        n = len(arrs[0]) // 4 if arrs else 0
        return np.array(outs, dtype=np.float32).reshape(self.output_count(), n, 4)

    def eval_grad_slice(self, x, y, z, extra=None):
        x, y, z = (np.asarray(a, dtype=np.float32) for a in (x, y, z))
        n = len(x)

        def seed(v, k):
            g = np.zeros((n, 4), np.float32)
            g[:, 0] = v
            g[:, 1 + k] = 1.0
            return g
        vs = self._xyz_vars(seed(x, 0), seed(y, 1), seed(z, 2), extra)
        out = []
        for v in vs:
            if v is None:
                out.append(np.zeros((n, 4), np.float32))
            elif np.isscalar(v):
                g = np.zeros((n, 4), np.float32)
                g[:, 0] = v
                out.append(g)
            else:
                out.append(v)
        return self.eval_grad_slice_raw(out)[0]


# ---- geometry helpers (host f32, same operation order as the C++ driver) --------------
def screen_to_world(size):
    n = len(size)
    s = np.array(size, dtype=np.uint32)
    out = np.zeros((n + 1, n + 1), dtype=np.float32)
    lib().fhip_screen_to_world(_p(s), n, _p(out))
    return out


def mat_mul(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    d = a.shape[0]
    out = np.zeros((d, d), np.float32)
    for col in range(d):
        for row in range(d):
            acc = np.float32(a[row, 0] * b[0, col])
            for k in range(1, d):
                acc = np.float32(np.float32(a[row, k] * b[k, col]) + acc)
            out[row, col] = acc
    return out


def lift_2d(m3):
    m3 = np.asarray(m3, np.float32)
    m = np.zeros((4, 4), np.float32)
    m[0, :2] = m3[0, :2]; m[0, 3] = m3[0, 2]
    m[1, :2] = m3[1, :2]; m[1, 3] = m3[1, 2]
    m[2, 2] = 1.0
    m[3, :2] = m3[2, :2]; m[3, 3] = m3[2, 2]
    return m


def transform_point(mat4, x, y, z):
    m = np.asarray(mat4, np.float32)
    x, y, z = np.float32(x), np.float32(y), np.float32(z)
    r = [np.float32(np.float32(np.float32(m[i, 0] * x) + np.float32(m[i, 1] * y)) + np.float32(m[i, 2] * z)) + m[i, 3]
         for i in range(4)]
    r = [np.float32(v) for v in r]
    if r[3] != 0:
        return np.array([r[0] / r[3], r[1] / r[3], r[2] / r[3]], np.float32)
    return np.array(r[:3], np.float32)
