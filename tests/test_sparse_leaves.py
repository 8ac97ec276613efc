"""The leaf stage driven by the slab's list of leaves (capi_render.hpp by_list; render_state.h leaf_list) on the CPU emulator: the list
entry mode of fh_columns (kernarg flags bit 21) and of fh_normals (kernarg mode bit 0) on small synthetic slabs, against the words
the table-driven modes of the same kernels give for the same leaves - and, for the normals, against the numpy restatement too.

Cases: a few leaves, an empty and a full z-buffer, a leaf in the list's last slot, counts that are no multiple of 64 (more and
fewer leaves than waves), count 0, and records behind the count that must not be looked at."""
import numpy as np
import pytest

import emu_util as U
from emu_util import E, F32, U32
from test_emu_columns import AFFINE32, col_kernarg, column_shape, run_columns
from test_emu_normals import AFFINE, PERSPECTIVE, expect, leaf_at, leaves_of, run_normals, same
from test_emu_tiles import shape_of

SIZE = 32       # columns: 4 x 4 footprints, 4 layers


def run_columns_list(tape, n_regs, in_kind, mat, leaves_xyz, waves, cap=None, zbuf_init=None, size=SIZE, n_leaves=None, junk=True):
    """fh_columns by the list: `leaves_xyz` are the slab's FhLeaf records 0 .., the array holds `cap` of them (the ones behind the count
    filled with junk that would fault or draw if a wave took them), the launch has `waves` waves."""
    off = U.offsets()
    mem = E.Memory()
    arena = np.zeros(4096, np.uint64)
    arena[16:16 + len(tape)] = tape
    n = len(leaves_xyz) if n_leaves is None else n_leaves
    cap = max(len(leaves_xyz), 1) if cap is None else cap
    leaves = np.zeros((cap, 6), U32)
    if junk:
        leaves[:] = [0x7FFFFF00, 40, 8, 8, 8, 0]
    for k, (lx, ly, lz) in enumerate(leaves_xyz):
        leaves[k] = [16, len(tape), n_regs, lx, ly, lz]
    zbuf = np.zeros(size * size, np.uint64) if zbuf_init is None else zbuf_init.copy()
    a_arena, a_leaves, a_z = mem.map(arena), mem.map(leaves), mem.map(zbuf)
    st = U.Blob(off["sizeof_state"])
    st.arr(off["P.mat"], np.asarray(mat, F32))
    st.u32(off["P.width"], size); st.u32(off["P.height"], size); st.u32(off["P.tiles"], size); st.u32(off["P.slab"], size)
    for s in range(16):
        st.u32(off["P.in_kind"] + 4 * s, in_kind[s] if s < len(in_kind) else 3)
    st.u64(off["arena"], a_arena); st.u64(off["leaves"], a_leaves); st.u64(off["zbuf"], a_z)
    st.u32(off["n_leaves"], n); st.u32(off["leaf_cap"], cap)
    st.u32(off["slab_z"], 0)
    a_st = mem.map(st.b)
    ka = col_kernarg(a_st, in_kind, mat, size, True, 6, a_tab=a_leaves, layers=size // 8)
    ka[5] |= 1 << 21            # by the list: the table pointer is the FhLeaf array, footprints per layer its capacity, the reciprocal the waves
    ka[6] = waves
    ka[10] = cap
    ws = E.launch(U.program(), mem, "fh_columns", ka.tobytes(), waves, grid_y=1, lds_bytes=16, n_vgpr=128)
    return zbuf, ws


def by_table(tape, n_regs, ik, mat, leaves_xyz, zbuf_init=None):
    got, _ = run_columns(tape, n_regs, ik, mat, leaves_xyz[0], size=SIZE, zbuf_init=zbuf_init, column_mode=True, more_leaves=leaves_xyz[1:])
    return got


LEAVES = [(8, 0, 8), (24, 16, 24), (0, 24, 0)]      # one leaf per footprint column, as the frames that take this path guarantee


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("waves", [64, 2, 1])
def test_columns_by_list_equal_columns_by_table(kind, waves):
    """three leaves, 64 waves (61 of them without a leaf), 2 and 1 (waves that take several leaves one after the other)"""
    sh, tape, ik = column_shape(kind)
    z = np.zeros(SIZE * SIZE, np.uint64)
    z[5::7] = np.uint64((3 << 32) | 9)
    want = by_table(tape, sh.slot_count(), ik, AFFINE32, LEAVES, z)
    got, _ = run_columns_list(tape, sh.slot_count(), ik, AFFINE32, LEAVES, waves, cap=16, zbuf_init=z)
    assert (got == want).all(), f"{(got != want).sum()} z-buffer words differ"
    assert (got != z).any()


def test_columns_by_list_random_shape():
    sh, tape, ik = shape_of(2)
    want = by_table(tape, sh.slot_count(), ik, AFFINE32, LEAVES)
    got, _ = run_columns_list(tape, sh.slot_count(), ik, AFFINE32, LEAVES, 64, cap=7)
    assert (got == want).all()


def test_columns_by_list_full_z_buffer():
    """every pixel already hit in front of every leaf: nothing pending, nothing written"""
    sh, tape, ik = column_shape(1)
    z = np.full(SIZE * SIZE, np.uint64((SIZE << 32) | 5))
    want = by_table(tape, sh.slot_count(), ik, AFFINE32, LEAVES, z)
    got, _ = run_columns_list(tape, sh.slot_count(), ik, AFFINE32, LEAVES, 64, cap=16, zbuf_init=z)
    assert (got == want).all() and (got == z).all()


def test_columns_by_list_last_slot_and_odd_counts():
    """the list full to its capacity - the last leaf sits in the last record - with 70 leaves over 64 waves (six waves take two)"""
    sh, tape, ik = column_shape(1)
    size = 128                   # 16 x 16 footprints
    cols = [(8 * (k % 16), 8 * (k // 16), 8 * (k % 5)) for k in range(70)]
    cols[49], cols[69] = cols[69], cols[49]         # (a leaf that has hits, in the last record)
    got, ws = run_columns_list(tape, sh.slot_count(), ik, [1 / 64, 0, 0, -1, 0, -1 / 64, 0, 1 - 1 / 64, 0, 0, 1 / 64, -1, 0, 0, 0, 1], cols, 64, cap=70, size=size)
    one, _ = run_columns_list(tape, sh.slot_count(), ik, [1 / 64, 0, 0, -1, 0, -1 / 64, 0, 1 - 1 / 64, 0, 0, 1 / 64, -1, 0, 0, 0, 1], cols, 70, cap=70, size=size)
    assert (got == one).all()
    ids = set((got & np.uint64(0xFFFFFFFF)).tolist())
    assert 70 in ids and max(ids) == 70 and len(ids) > 5, "the leaf in the last slot drew its pixels, and nothing behind it was taken"


def test_columns_by_list_count_zero():
    """no leaves: every wave leaves before any pixel set-up (no vector memory instruction at all), the junk records untouched"""
    sh, tape, ik = column_shape(0)
    z = np.zeros(SIZE * SIZE, np.uint64)
    z[3::5] = np.uint64((2 << 32) | 1)
    got, ws = run_columns_list(tape, sh.slot_count(), ik, AFFINE32, [], 64, cap=16, zbuf_init=z)
    assert (got == z).all()
    assert all(w.counts.get("vmem", 0) == 0 for w in ws)
    # ... and a count beyond the capacity (the push counts the leaves it could not store) is clamped to it
    got, _ = run_columns_list(tape, sh.slot_count(), ik, AFFINE32, LEAVES, 64, cap=3, n_leaves=1000)
    assert (got == by_table(tape, sh.slot_count(), ik, AFFINE32, LEAVES)).all()


def run_normals_by_leaves(tapes, in_kind, mat, hits, corners, n_waves, n_leaves=None, cap=None, size=16, z_lo=0, z_hi=1 << 20):
    """fh_normals with mode bit 0: no hit lists (the pointer is null - a wave that read one would fault), leaf i by wave pass i"""
    off = U.offsets()
    mem = E.Memory()
    arena = np.zeros(8192, np.uint64)
    cap = max(len(tapes), 1) if cap is None else cap
    leaves = np.zeros((cap, 6), U32)
    leaves[:] = [0x7FFFFF00, 40, 8, 0, 0, 0]
    at = 16
    for k, (ops, regs) in enumerate(tapes):
        arena[at:at + len(ops)] = ops
        leaves[k] = [at, len(ops), regs, corners[k][0], corners[k][1], 0]
        at += len(ops) + 24
    zbuf = np.zeros(size * size, np.uint64)
    for (px, py), (leaf, depth) in hits.items():
        zbuf[py * size + px] = (depth << 32) | (leaf + 1)
    normals = np.full(size * size * 3, 7.5, F32)
    a_arena, a_leaves, a_z, a_n = mem.map(arena), mem.map(leaves), mem.map(zbuf), mem.map(normals)
    st = U.Blob(off["sizeof_state"])
    st.arr(off["P.mat"], np.asarray(mat, F32))
    st.u32(off["P.width"], size); st.u32(off["P.height"], size)
    for s in range(16):
        st.u32(off["P.in_kind"] + 4 * s, in_kind[s] if s < len(in_kind) else 3)
        st.f32(off["P.in_value"] + 4 * s, 0.25 + s)
    st.u64(off["arena"], a_arena); st.u64(off["leaves"], a_leaves); st.u64(off["zbuf"], a_z); st.u64(off["normals"], a_n)
    st.u32(off["n_leaves"], len(tapes) if n_leaves is None else n_leaves); st.u32(off["leaf_cap"], cap)
    a_st = mem.map(st.b)
    slot = [-1, -1, -1]
    for s_, k in enumerate(list(in_kind) + [3] * (16 - len(in_kind))):
        if k < 3:
            slot[k] = s_
    slots = sum((0xFF if slot[ax] < 0 else slot[ax]) << (8 * ax) for ax in range(3))
    ka = np.array([a_st & 0xFFFFFFFF, a_st >> 32, n_waves, slots, z_lo, z_hi, 0, 1], U32)
    ws = E.launch(U.program(), mem, "fh_normals", ka.tobytes(), n_waves, lds_bytes=16, n_vgpr=224, wg_y_sgpr=None)
    return zbuf, normals.reshape(size * size, 3), ws


def normals_case(seed=0):
    sh, tape, ik = shape_of(seed)
    assert sh.slot_count() <= 40
    return leaves_of([(tape, sh.slot_count())]) + (ik,)       # one leaf per footprint: four leaves


@pytest.mark.parametrize("mat", [AFFINE, PERSPECTIVE], ids=["affine", "perspective"])
@pytest.mark.parametrize("n_waves", [64, 3])
def test_normals_by_leaves_equal_normals_by_hit_lists(mat, n_waves):
    tapes, corners, ik = normals_case()
    rng = np.random.default_rng(4)
    hits = {}
    for _ in range(60):
        px, py = int(rng.integers(0, 16)), int(rng.integers(0, 16))
        hits[(px, py)] = (leaf_at(px, py, 0, 1), int(rng.integers(1, 17)))
    ref_z, ref_n = run_normals(tapes, ik, mat, hits, z_lo=2, z_hi=14, corners=corners)
    got_z, got_n, _ = run_normals_by_leaves(tapes, ik, mat, hits, corners, n_waves, cap=9, z_lo=2, z_hi=14)
    want_z, want_n = expect(tapes, ik, mat, hits, 16, z_lo=2, z_hi=14)
    assert (got_z == ref_z).all() and same(got_n, ref_n)
    assert (got_z == want_z).all() and same(got_n, want_n)


def test_normals_by_leaves_empty_and_full_z_buffer():
    tapes, corners, ik = normals_case(2)
    got_z, got_n, ws = run_normals_by_leaves(tapes, ik, AFFINE, {}, corners, 64)
    assert (got_z == 0).all() and (got_n == 7.5).all(), "no hit anywhere: every leaf leaves after its z-buffer words"
    hits = {(x, y): (leaf_at(x, y, 0, 1), 1 + (3 * x + y) % 15) for x in range(16) for y in range(16)}
    got_z, got_n, _ = run_normals_by_leaves(tapes, ik, AFFINE, hits, corners, 64)
    ref_z, ref_n = run_normals(tapes, ik, AFFINE, hits, corners=corners)
    assert (got_z == ref_z).all() and same(got_n, ref_n)
    assert ((got_z & np.uint64(0xFFFFFFFF)) == 0).all(), "every pixel's normal done"


def test_normals_by_leaves_last_slot_count_zero_and_large_leaves():
    tapes, corners, ik = normals_case()
    hits = {(x, y): (leaf_at(x, y, 0, 1), 5) for x in (1, 9, 14) for y in (2, 8, 15)}
    # the list full to its capacity, fewer waves than leaves: leaf 3 (the last record) is the second pass of wave 0
    got_z, got_n, _ = run_normals_by_leaves(tapes, ik, AFFINE, hits, corners, 3, cap=4)
    want_z, want_n = expect(tapes, ik, AFFINE, hits, 16)
    assert (got_z == want_z).all() and same(got_n, want_n)
    # count 0: nothing is looked at, although the z-buffer names leaves
    got_z, got_n, ws = run_normals_by_leaves(tapes, ik, AFFINE, hits, corners, 64, n_leaves=0)
    assert ((got_z & np.uint64(0xFFFFFFFF)) != 0).sum() == len(hits) and (got_n == 7.5).all()
    assert all(w.counts.get("vmem", 0) == 0 for w in ws)
    # a leaf of more registers than the kernel's file (the C++ kernel's, through list 2): skipped, its pixels left pending
    big = [(t, 41 if k == 1 else r) for k, (t, r) in enumerate(tapes)]
    got_z, got_n, _ = run_normals_by_leaves(big, ik, AFFINE, hits, corners, 64)
    mine = np.array([(got_z[i] & np.uint64(0xFFFFFFFF)) == 2 for i in range(256)])
    assert mine.sum() == sum(1 for v in hits.values() if v[0] == 1) > 0
    keep = ~np.array([((want_z[i] >> np.uint64(32)) == 5) and leaf_at(i % 16, i // 16, 0, 1) == 1 for i in range(256)])
    assert (got_z[keep] == want_z[keep]).all() and same(got_n[keep], want_n[keep]) and (got_n[~keep] == 7.5).all()
