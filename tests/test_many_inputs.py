"""Tapes of more than 16 variables on the host: graph-built and reference-bytecode tapes keep their whole VarMap, compile, register-allocate
and simplify as the oracle does; the bound tape a render takes of them (capi_bound.hpp, fidget_hip_debug.h fhip_debug_bound_tape) changes
exactly its bound inputs; the assembly bulk interpreter reads input slots far beyond 16 (gfx950 emulator)."""
import ctypes as C
import time

import numpy as np
import pytest

import emu_util as U
import fidget_amd as F
import oracle as O
from conftest import model_path
from test_emu_bulk import run_bulk, same
from test_host_frontend import canon_oracle, canon_product

OP = {n: i for i, n in enumerate(U.OPS)}
BYTECODE_SLOTS = [16, 31, 32, 63, 64, 255, 256, 299]


def spheres(M, n_vars, axes_last=False, consts=None):
    """A union of spheres over `n_vars` variables: sphere k has centre var(4k .. 4k + 2) and radius var(4k + 3) (a partial last
    sphere keeps constants).  axes_last: the variables come first in the tape's VarMap and the axes after them (slots >= 16).
    consts: {var index: value} - the same function with constants in place of the variables."""
    c = M.Context()
    x, y, z = c.x(), c.y(), c.z()
    used, terms, k = 0, [], 0
    while used < n_vars:
        p = []
        for j in range(4):
            if used < n_vars:
                p.append(c.var(4 * k + j) if consts is None else c.constant(consts[4 * k + j])); used += 1
            else:
                p.append(c.constant(0.25 * (j + 1)))
        d = c.add(c.add(c.square(c.sub(x, p[0])), c.square(c.sub(y, p[1]))), c.square(c.sub(z, p[2])))
        terms.append(c.sub(c.sqrt(d), p[3]))
        k += 1
    r = terms[0]
    for t in terms[1:]:
        r = c.min(r, t)
    if axes_last:       # (a later node is the second operand of the add, which the tape order visits first: its variables get the first slots)
        v = c.var(0)
        for i in range(1, n_vars):
            v = c.add(v, c.var(i))
        r = c.add(r, c.mul(v, c.constant(1.0 / 1024)))
    return c, r


def var_indices(n_vars):
    return list(range(n_vars))


@pytest.mark.parametrize("n_vars", [17, 33, 65, 300])
@pytest.mark.parametrize("axes_last", [False, True])
def test_graph_tape_with_many_variables_matches_oracle(n_vars, axes_last):
    pc, pr = spheres(F, n_vars, axes_last)
    oc, orr = spheres(O, n_vars, axes_last)
    p, o = F.Shape(pc, pr), O.Shape(oc, orr)
    assert p.var_count() == o.var_count() == n_vars + 3
    assert [p.axis_index(a) for a in range(3)] == [o.axis_index(a) for a in range(3)]
    assert [p.var_index(i) for i in var_indices(n_vars)] == [o.var_index(i) for i in var_indices(n_vars)]
    assert p.var_index(n_vars + 7) == -1
    assert canon_product(p) == canon_oracle(o)
    rng = np.random.default_rng(n_vars)
    for _ in range(4):
        ch = rng.integers(1, 4, o.choice_count()).tolist()
        assert canon_product(p.simplify(ch)) == canon_oracle(o.simplify(ch))


def test_axes_can_sit_at_slots_beyond_16():
    o = O.Shape(*spheres(O, 65, axes_last=True))
    assert min(o.axis_index(a) for a in range(3)) >= 16


@pytest.mark.parametrize("axes_last", [False, True])
def test_reference_bytecode_with_high_input_slots(axes_last):
    oc, orr = spheres(O, 300, axes_last)
    o = O.Shape(oc, orr)
    words, _, _ = o.bytecode()
    w = np.asarray(words, np.uint32)
    ins = {int(w[i + 1]) for i in range(2, len(w) - 1, 2) if (w[i] & 0xFF) == 1 and w[i] != 0xFFFFFFFF}
    assert set(BYTECODE_SLOTS) <= ins
    p = F.Shape.from_bytecode(words, axis_slots=[o.axis_index(a) for a in range(3)])
    ref = F.Shape(*spheres(F, 300, axes_last))
    assert p.var_count() == o.var_count() == 303
    assert canon_product(p) == canon_product(ref) == canon_oracle(o)
    rng = np.random.default_rng(3)
    ch = rng.integers(1, 4, o.choice_count()).tolist()
    assert canon_product(p.simplify(ch)) == canon_oracle(o.simplify(ch))


def test_bytecode_input_slot_bound():
    def tape(slot):
        return [0xFFFFFFFF, 0, 0x01 | (0 << 8), slot, 0x00 | (0 << 8), 0, 0xFFFFFFFF, 0xFFFFFFFF]
    assert F.Shape.from_bytecode(tape(65535)).var_count() == 65536
    with pytest.raises(F.FidgetHipError):
        F.Shape.from_bytecode(tape(0xFFFFFFFF))


def test_thousands_of_variables_build_quickly():
    c = F.Context()
    r = c.x()
    for i in range(4000):
        r = c.add(r, c.mul(c.var(i), c.constant(1.0 + i)))
    t0 = time.perf_counter()
    s = F.Shape(c, r)
    dt = time.perf_counter() - t0
    assert s.var_count() == 4001 and s.var_index(3999) >= 0
    assert dt < 1.0, dt


# ---- the bound tape ---------------------------------------------------------------------------------------------------------------
def bound(shape, axis_slots, vars_):
    k = np.array(list(vars_.keys()), np.uint64)
    v = np.array(list(vars_.values()), np.float32)
    ax = None if axis_slots is None else np.ascontiguousarray(axis_slots, np.int32)
    h = C.c_void_p()
    st = F.lib().fhip_debug_bound_tape(None, shape._h, None if ax is None else ax.ctypes.data, k.ctypes.data, v.ctypes.data, len(k), C.byref(h))
    if st:
        return st
    return F.Shape(_h=h, _vars=None)


def check_bound(parent, child, slot_kind, slot_value):
    a, b = parent.words(), child.words()
    assert len(a) == len(b)
    assert child.slot_count() == parent.slot_count() and child.choice_count() == parent.choice_count()
    assert child.var_count() == 3
    changed = 0
    for wa, wb in zip(a.tolist(), b.tolist()):
        if wa & 0xFF != OP["INPUT"]:
            assert wa == wb
            continue
        slot = wa >> 32
        kind = slot_kind[slot]
        assert (wb & 0xFFF00) == (wa & 0xFFF00)     # the same out register
        if kind < 3:
            assert wb == (wa & 0xFFFFFFFF) | (kind << 32)
        else:
            assert wb & 0xFF == OP["COPY_IMM"] and (wb >> 20) & 0xFFF == 0
            assert wb >> 32 == int(np.float32(slot_value[slot]).view(np.uint32))
            changed += 1
    return changed


def test_bound_tape_rewrites_only_bound_inputs():
    s = F.Shape(*spheres(F, 80))
    rng = np.random.default_rng(1)
    vals = {i: float(rng.uniform(-1, 1)) for i in range(80)}
    vals[999] = 5.0           # not read by the tape: ignored
    b = bound(s, None, vals)
    assert isinstance(b, F.Shape)
    kind, val = {}, {}
    for a in range(3):
        kind[s.axis_index(a)] = a
    for i in range(80):
        kind[s.var_index(i)] = 3; val[s.var_index(i)] = vals[i]
    assert check_bound(s, b, kind, val) == 80
    assert [b.axis_index(a) for a in range(3)] == [0, 1, 2]


def test_bound_tape_keeps_groups_and_term_plan():
    """prospero.vm rebuilt with 60 of its constants as variables: the tape is long enough for groups and a term plan, and its bound
    tape keeps both as they are, with the same rewrite in every group"""
    c, root, consts = prospero_with_vars(F, 60)
    s = F.Shape(c, root)
    assert s.var_count() > 16 and len(s.groups()[1]) > 0 and s.term_plan()["groups"] > 0
    b = bound(s, None, consts)
    kind, val = {s.axis_index(a): a for a in range(3)}, {s.var_index(i): v for i, v in consts.items()}
    kind.update({s.var_index(i): 3 for i in consts})
    check_bound(s, b, kind, val)
    assert b.term_plan() == s.term_plan()
    gp, gb = s.groups(), b.groups()
    assert gp[0] == gb[0] and len(gp[1]) == len(gb[1])
    for x, y in zip(gp[1], gb[1]):
        check_bound(x, y, kind, val)
    tp, tb = s.term_parts(), b.term_parts()
    assert (tp[1] == tb[1]).all() and (tp[2] == tb[2]).all()
    for x, y in zip(tp[0], tb[0]):
        check_bound(x, y, kind, val)


def test_bound_tape_of_bytecode_and_missing_variable():
    o = O.Shape(*spheres(O, 40, axes_last=True))
    words, _, _ = o.bytecode()
    ax = [o.axis_index(a) for a in range(3)]
    p = F.Shape.from_bytecode(words, axis_slots=ax)
    slots = [sl for sl in range(p.var_count()) if sl not in ax]
    vals = {sl: 0.5 + sl for sl in slots}
    b = bound(p, ax, vals)
    kind = {ax[a]: a for a in range(3)}
    kind.update({sl: 3 for sl in slots})
    assert check_bound(p, b, kind, vals) == 40
    del vals[slots[7]]
    assert bound(p, ax, vals) == 4           # FHIP_ERR_MISSING_VAR
    s = F.Shape(*spheres(F, 80))
    assert bound(s, None, {i: 1.0 for i in range(80) if i != 33}) == 4


def test_bound_tape_host_time_for_a_prospero_sized_parent():
    c, root, consts = prospero_with_vars(F, 60)
    s = F.Shape(c, root)
    bound(s, None, consts)
    t0 = time.perf_counter()
    for _ in range(10):
        bound(s, None, consts)
    dt = (time.perf_counter() - t0) / 10
    print(f"bound tape of a {s.device_len()}-op parent: {dt * 1e6:.0f} us")
    assert dt < 0.05


def prospero_with_vars(M, n):
    """prospero.vm through the Context API with its first `n` distinct constants (other than 0, 1 and 2) turned into variables;
    returns (context, root, {var index: the constant's value})"""
    text = open(model_path("prospero.vm")).read()
    c = M.Context()
    names, consts, seen = {}, {}, {}
    un = {"neg", "square", "sqrt", "abs", "exp", "ln", "sin", "cos"}
    last = None
    for line in text.splitlines():
        if not line or line.startswith("#"):
            continue
        t = line.split()
        if t[1] == "const":
            v = float(np.float32(float(t[2])))
            if v not in (0.0, 1.0, 2.0) and len(seen) < n and v not in seen:
                seen[v] = len(seen)
            node = c.var(seen[v]) if v in seen else c.constant(v)
            if v in seen:
                consts[seen[v]] = v
        elif t[1] == "var-x":
            node = c.x()
        elif t[1] == "var-y":
            node = c.y()
        elif t[1] == "var-z":
            node = c.z()
        elif t[1] in un:
            node = getattr(c, t[1])(names[t[2]])
        else:
            node = getattr(c, t[1])(names[t[2]], names[t[3]])
        names[t[0]] = node
        last = node
    assert len(consts) == n
    return c, last, consts


# ---- the assembly bulk interpreter with high input slots (gfx950 emulator) ---------------------------------------------------------
@pytest.mark.parametrize("kernel,zb", [("fh_float_eval_16x4", 4), ("fh_float_eval_32x2", 2)])
def test_bulk_kernel_reads_high_input_slots(kernel, zb):
    rng = np.random.default_rng(9)
    n = 64 * zb + 21
    slots = [0, 15, 16, 31, 32, 63, 64, 255, 256, 299]
    inputs = {s: rng.uniform(-10, 10, n).astype(np.float32) for s in slots}
    P = U.pack
    tape = [P(OP["INPUT"], r, 0, s) for r, s in enumerate(slots)]        # r0 .. r9 (16 registers at most: the 16x4 shape)
    tape.append(P(OP["MUL_RR"], 10, 0, 1))
    for r in range(2, len(slots)):
        tape.append(P(OP["SUB_RR"] if r % 2 else OP["ADD_RR"], 10, 10, r))
    tape += [P(OP["OUTPUT"], 0, 10, 0), P(OP["OUTPUT"], 0, 9, 1)]
    got = run_bulk(kernel, zb, tape, inputs, n, 2)
    want = U.ref_f32(np.asarray(tape, np.uint64), inputs, n)
    assert same(got[0], want[0]) and same(got[1], want[1])
    assert same(got[1], inputs[299])
