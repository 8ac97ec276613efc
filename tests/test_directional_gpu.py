"""fhip_voxels_flow, fhip_voxels_overhangs and fhip_voxels_heights on the device against directional_ref.py: bitmaps made in numpy
(voxels_ref.pack) and handed to the library as host bricks and as a torch CUDA tensor; every result is compared with np.array_equal -
bitmaps and integers.  Then supports end to end, a shape end to end, two runs, the refused calls."""
import ctypes as C
import functools

import numpy as np
import pytest

import directional_ref as DR
import fidget_amd as F
import voxels_ref as V
from test_directional import table16
from test_mesh import sphere
from test_voxel_mesh import box, hollow_box16, voxels_at

pytestmark = pytest.mark.gpu
COMBOS = [(False, False), (True, False), (False, True), (True, True)]          # (with blockers, with seeds)
REACHES = (0, 1, 2, 4, 5, 8, 9, 16)


@functools.lru_cache(maxsize=None)
def _torch():
    import torch
    return torch


def pack(inside):
    """voxels_ref.pack by bytes - the inverse of fidget_amd.voxels_unpack - for the grids of 256^3 and 512^3; checked against it below"""
    B = inside.shape[0] // 4
    if B < 2:
        bits = inside.reshape(B, 4, B, 4, B, 4).transpose(4, 2, 0, 5, 3, 1)          # [bz, by, bx, lz, ly, lx]
        return np.packbits(np.ascontiguousarray(bits).reshape(B, B, B, 64), axis=-1, bitorder="little").view("<u8").reshape(B, B, B)
    # rows along i to bytes first - a byte holds the rows lx = 0 .. 3 of two bricks - then the 16 rows (ly, lz) of a brick into its word
    rows = np.packbits(np.ascontiguousarray(inside.transpose(2, 1, 0)), axis=-1, bitorder="little").reshape(B, 4, B, 4, B // 2)          # [bz, lz, by, ly, bx / 2]
    words = np.zeros((B, B, B), np.uint64)
    for lz in range(4):
        for ly in range(4):
            r = rows[:, lz, :, ly, :]
            shift = np.uint64(4 * ly + 16 * lz)
            words[:, :, 0::2] |= (r & 15).astype(np.uint64) << shift
            words[:, :, 1::2] |= (r >> 4).astype(np.uint64) << shift
    return words


def rand(depth, density, seed):
    N = 4 << depth
    return np.random.default_rng(seed).random((N, N, N)) < density


def at(N, axis, along, p, q):
    """the voxel whose coordinate along `axis` is `along`, its two others p and q in ascending order of axis"""
    c = [p, q]
    c.insert(axis, along)
    return tuple(c)


def across(N, lo_block=None):
    """depth 1: along every axis a seed at local 3 of the first brick, and a blocker in the next brick at the given local coordinate"""
    seeds = voxels_at(N, [at(N, axis, 3, 1 + axis, 6 - axis) for axis in range(3)] + [at(N, axis, 4, 2, 2) for axis in range(3)])
    blockers = voxels_at(N, [] if lo_block is None else [at(N, axis, 4 + lo_block, 1 + axis, 6 - axis) for axis in range(3)])
    return seeds, blockers


def sparse_columns(N, axis):
    """(p, q) of three columns along `axis` of each of three kinds: "free", "stopped", "far".  No two columns of the grid meet."""
    return {"free": [(5 + axis + 16 * rep, 9 + 2 * axis + 24 * rep) for rep in range(3)],
            "stopped": [(N // 2 + axis + 12 * rep, N - 3 - axis - 20 * rep) for rep in range(3)],
            "far": [(N - 1 - axis - 28 * rep, N // 3 + 5 * axis + 8 * rep) for rep in range(3)]}


def sparse(depth):
    """per axis three columns of each kind: a seed at one end and nothing in its way - it must fill all B bricks; the same with one
    blocker at coordinate 300 (of 512; in proportion on a smaller grid); a seed at the far end, which flows the other way"""
    N = 4 << depth
    seeds, blockers = np.zeros((N, N, N), bool), np.zeros((N, N, N), bool)
    for axis in range(3):
        for kind, cols in sparse_columns(N, axis).items():
            for p, q in cols:
                seeds[at(N, axis, N - 1 if kind == "far" else 0, p, q)] = True
                if kind == "stopped":
                    blockers[at(N, axis, 300 * N // 512, p, q)] = True
    return seeds, blockers


def dense(depth):
    """many voxels in every column: a random 64^3 of density 0.03 tiled up.  A third of the layers k is cleared below i = 0.53 N and a third
    from 0.49 N on, so that at depth 7 the lowest voxel along x of those columns lies in the second chunk of 64 bricks or the highest
    in the first"""
    N = 4 << depth
    g = np.tile(rand(4, 0.03, 16), (N // 64,) * 3)
    g[:N * 270 // 512, :, 0::3] = False
    g[N * 250 // 512:, :, 1::3] = False
    return g, np.zeros((N, N, N), bool)


# name -> (seeds, blockers)
GRIDS = {
    "d0-empty": lambda: (np.zeros((4, 4, 4), bool), np.zeros((4, 4, 4), bool)),
    "d0-full": lambda: (np.ones((4, 4, 4), bool), np.zeros((4, 4, 4), bool)),
    "d0-ends-lo": lambda: (voxels_at(4, [(0, 1, 2), (2, 0, 1), (1, 2, 0)]), voxels_at(4, [(2, 1, 2)])),
    "d0-ends-hi": lambda: (voxels_at(4, [(3, 1, 2), (2, 3, 1), (1, 2, 3)]), voxels_at(4, [(1, 2, 1)])),
    "d0-blocked-seed": lambda: (voxels_at(4, [(1, 1, 1)]), voxels_at(4, [(1, 1, 1), (3, 1, 1)])),
    "d0-random0.5": lambda: (rand(0, 0.5, 1), rand(0, 0.3, 2)),
    "d1-across": lambda: across(8),
    "d1-across-blocked-at-0": lambda: across(8, 0),
    "d1-across-blocked-at-3": lambda: across(8, 3),
    "d1-random0.05": lambda: (rand(1, 0.05, 3), rand(1, 0.1, 4)),
    "d1-random0.5": lambda: (rand(1, 0.5, 5), rand(1, 0.5, 6)),
    "d2-random0.1": lambda: (rand(2, 0.1, 7), rand(2, 0.1, 8)),
    "d2-table": lambda: (table16(), box(16, (0, 0, 5), (16, 16, 6))),
    # depth 4: B = 16, four rows of bricks in a wave - the scan along x must restart at every row
    "d4-random0.001": lambda: (rand(4, 0.001, 9), rand(4, 0.01, 10)),
    "d4-random0.2": lambda: (rand(4, 0.2, 11), rand(4, 0.3, 12)),
    # depth 6: B = 64, a row is exactly one wave
    "d6-sparse": lambda: sparse(6),
    "d6-dense": lambda: dense(6),
}
SMALL = [n for n in GRIDS if not n.startswith("d6")]
# ... that only some tests use: B = 128, the smallest grid whose rows span two chunks of 64 bricks; solids for the overhangs
EXTRA = {
    "d7-sparse": lambda: sparse(7),
    "d7-dense": lambda: dense(7),
    "d4-solid0.02": lambda: (rand(4, 0.02, 13), np.zeros((64, 64, 64), bool)),
    "d4-solid0.3": lambda: (rand(4, 0.3, 14), np.zeros((64, 64, 64), bool)),
    "d4-solid0.9": lambda: (rand(4, 0.9, 15), np.zeros((64, 64, 64), bool)),
}


@functools.lru_cache(maxsize=None)
def grid(name):
    s, k = (GRIDS.get(name) or EXTRA[name])()
    s.setflags(write=False)
    k.setflags(write=False)
    return s, k


@functools.lru_cache(maxsize=None)
def bricks_of(name):
    s, k = (pack(g) for g in grid(name))
    s.setflags(write=False)
    k.setflags(write=False)
    return s, k


@functools.lru_cache(maxsize=None)
def flow_ref(name, d, blocked, with_seeds):
    s, k = grid(name)
    r = pack(DR.flow(s, k if blocked else None, d, with_seeds))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def overhangs_ref(name, up, reach2, bed):
    r = pack(DR.overhangs(grid(name)[0], up, reach2, bed))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def heights_ref(name, axis):
    r = DR.heights(grid(name)[0], axis)
    r.setflags(write=False)
    return r


def voxels(bricks, where):
    """a Voxels over these bricks: on the host, or in a torch CUDA tensor"""
    depth = bricks.shape[0].bit_length() - 1
    hip = F.default_context()
    if where == "host":
        return F.Voxels(hip, np.array(bricks), depth, None)
    torch = _torch()
    t = torch.from_numpy(np.array(bricks).view(np.int64)).cuda()
    torch.cuda.synchronize()
    return F.Voxels(hip, t, depth, None)


def words(vox):
    """a result's bricks on the host, after the context's stream"""
    if not vox.on_device:
        return vox.bricks
    vox._hip.sync()
    return vox.bricks.cpu().numpy().view(np.uint64)


def array(a, hip):
    if isinstance(a, np.ndarray):
        return a
    hip.sync()
    return a.cpu().numpy()


def test_the_quick_pack_is_voxels_refs():
    for depth, density in ((0, 0.5), (1, 0.3), (2, 0.7), (3, 0.4), (4, 0.1)):
        g = rand(depth, density, 40 + depth)
        assert np.array_equal(pack(g), V.pack(g))
        assert np.array_equal(F.voxels_unpack(pack(g)), g)


# ---- flow ------------------------------------------------------------------------------------------------------------------------------------
def check_flow(name, where, dirs, combos):
    s, k = (voxels(b, where) for b in bricks_of(name))
    for d in dirs:
        for blocked, with_seeds in combos:
            got = s.flow(d, blockers=k if blocked else None, with_seeds=with_seeds)
            assert got.on_device == (where == "torch") and got.depth == s.depth and got.cells is None
            want = flow_ref(name, d, blocked, with_seeds)
            same = np.array_equal(words(got), want)
            print(f"{name} {where} dir {d} blockers {blocked} with_seeds {with_seeds}: {V.popcount(want)} voxels, {'equal' if same else 'DIFFERENT'}")
            assert same


@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("name", SMALL)
def test_flow(name, where):
    check_flow(name, where, range(6), COMBOS)
    if name == "d1-across":          # the flow crosses the one brick boundary of each axis
        assert all(F.voxels_unpack(flow_ref(name, 2 * axis + 1, False, False))[at(8, axis, 7, 1 + axis, 6 - axis)] for axis in range(3))
    if name == "d0-blocked-seed":          # a blocked seed emits, up to the next blocker
        assert F.voxels_unpack(flow_ref(name, 1, True, False)).nonzero()[0].tolist() == [2]


@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("d", range(6))
def test_flow_when_a_row_is_one_wave(d, where):
    check_flow("d6-sparse", where, [d], COMBOS)


@pytest.mark.parametrize("blocked", [True, False])
@pytest.mark.parametrize("d", range(6))
def test_flow_when_a_row_spans_two_chunks(d, blocked):
    """depth 7, B = 128: the whole grid of 512^3, plain and with the seeds"""
    name, N, axis = "d7-sparse", 512, d >> 1
    check_flow(name, "torch", [d], [(blocked, False), (blocked, True)])
    r = F.voxels_unpack(flow_ref(name, d, blocked, False))
    cols = sparse_columns(N, axis)
    line = lambda pq: r[at(N, axis, slice(None), *pq)]          # noqa: E731
    for free, stopped, far in zip(cols["free"], cols["stopped"], cols["far"]):
        if d & 1:          # all 128 bricks of the free column; up to the blocker at 300, or past it; nothing from the far end
            assert line(free)[1:].all() and int(line(stopped).sum()) == (299 if blocked else 511) and not line(far).any()
        else:
            assert line(far)[:-1].all() and not line(free).any() and not line(stopped).any()


# ---- overhangs ---------------------------------------------------------------------------------------------------------------------------------
def check_overhangs(name, where, ups, reaches, beds=(True, False)):
    a = voxels(bricks_of(name)[0], where)
    for up in ups:
        for bed in beds:
            for reach2 in reaches:
                got = a.overhangs(up, reach2, bed)
                want = overhangs_ref(name, up, reach2, bed)
                same = np.array_equal(words(got), want)
                print(f"{name} {where} up {up} bed {bed} reach2 {reach2}: {V.popcount(want)} overhangs, {'equal' if same else 'DIFFERENT'}")
                assert same


@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("name", ["d0-empty", "d0-full", "d0-random0.5", "d1-random0.05", "d1-random0.5", "d2-random0.1", "d2-table"])
def test_overhangs(name, where):
    check_overhangs(name, where, range(6), (0, 1, 2, 4, 16))
    if name == "d2-table":
        for reach2, n in ((0, 128), (1, 112), (2, 108), (4, 92)):
            assert V.popcount(overhangs_ref(name, 5, reach2, True)) == n and V.popcount(overhangs_ref(name, 5, reach2, False)) == n + 16


def pair_grids(up, case):
    """depth 1: grids of two voxels, one in layer `top` along the axis of `up` and one a layer below it.  The upper one lies at local 0 or
    at local 3 of a brick in the perpendicular plane.  Case "near": the lower one is its neighbour across a face of the brick (offset 1
    along one axis) or across an edge or a corner (diagonal).  Case "far": 4 voxels away to the lower or to the upper side, the farthest
    a disc of reach2 = 16 reaches.  -> [(grid, the upper voxel, the squared offset)]"""
    axis, top = up >> 1, (5 if up & 1 else 2)
    low = top - 1 if up & 1 else top + 1
    if case == "near":          # (p, q) of the voxel, (p, q) of the one below
        pairs = [((4, 1), (3, 1)), ((1, 4), (1, 3)), ((3, 6), (4, 6)), ((4, 4), (3, 3)), ((3, 6), (4, 7)), ((4, 3), (3, 4))]
    else:
        pairs = [((4, 1), (0, 1)), ((3, 6), (7, 6)), ((1, 4), (1, 0)), ((6, 3), (6, 7))]
    return [(voxels_at(8, [at(8, axis, top, *p), at(8, axis, low, *q)]), at(8, axis, top, *p), (p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2) for p, q in pairs]


@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("up", range(6))
def test_overhangs_across_bricks_and_at_the_farthest_reach(up, where):
    for case, reaches in (("near", (0, 1, 2)), ("far", (15, 16))):
        for g, top, offset2 in pair_grids(up, case):
            assert offset2 in ((1, 2) if case == "near" else (16,))
            a = voxels(V.pack(g), where)
            for reach2 in reaches:
                for bed in (True, False):
                    got = F.voxels_unpack(words(a.overhangs(up, reach2, bed)))
                    assert np.array_equal(got, DR.overhangs(g, up, reach2, bed)), (case, reach2, bed)
                    assert bool(got[top]) == (reach2 < offset2)          # a diagonal neighbour supports from 2 on; 4 away from 16 on


@pytest.mark.parametrize("density", [0.02, 0.3, 0.9])
def test_overhangs_on_random_grids_of_depth_4(density):
    check_overhangs(f"d4-solid{density}", "torch", range(6), REACHES)


@pytest.mark.parametrize("up", range(6))
def test_overhangs_on_a_sparse_grid_of_depth_6(up):
    check_overhangs("d6-sparse", "torch", [up], (1, 16))


# ---- supports ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "torch"])
def test_supports(where):
    for name, cases in (("d2-table", [(5, 0, True), (5, 0, False), (5, 1, True), (0, 2, True), (2, 1, False)]), ("d4-random0.2", [(5, 1, True), (4, 0, False), (1, 4, True), (2, 16, True)])):
        solid = grid(name)[0]
        a = voxels(bricks_of(name)[0], where)
        for up, reach2, bed in cases:
            got = a.supports(up, reach2, bed)
            want = DR.flow(DR.overhangs(solid, up, reach2, bed), solid, up ^ 1)
            assert np.array_equal(words(got), pack(want)), (name, up, reach2, bed)
            if name == "d2-table" and (up, reach2) == (5, 0):
                assert got.n == 1280
    a = voxels(bricks_of("d2-table")[0], where)
    assert np.array_equal(words(a.supports()), words(a.supports(5, 1, True))) and a.supports().n == 1120


# ---- heights -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_heights(name, where):
    torch = _torch()
    a = voxels(bricks_of(name)[0], where)
    N = a.grid
    for axis in range(3):
        want = heights_ref(name, axis)
        got = a.heights(axis)
        assert (isinstance(got, np.ndarray) and got.dtype == np.int32) if where == "host" else (got.is_cuda and got.dtype == torch.int32)
        assert tuple(got.shape) == (3, N, N) and np.array_equal(array(got, a._hip), want), axis
        # into a caller's array, which is written completely; one of the other kind lands there, too
        out = np.full((3, N, N), 77, np.int32) if where == "host" else torch.full((3, N, N), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert a.heights(axis, out=out) is out and np.array_equal(array(out, a._hip), want)
    other = torch.full((3 * N * N + 5,), 77, dtype=torch.int32, device="cuda") if where == "host" else np.full(3 * N * N + 5, 77, np.int32)
    torch.cuda.synchronize()
    flat = array(a.heights(2, out=other), a._hip)
    assert np.array_equal(flat[:3 * N * N], heights_ref(name, 2).reshape(-1)) and (flat[3 * N * N:] == 77).all()
    if name == "d2-table":
        h = heights_ref(name, 2)
        assert sorted(set(h[2].reshape(-1).tolist())) == [0, 2, 12] and int(h[0].min()) == -1 and int((h[2] == 12).sum()) == 16


@pytest.mark.parametrize("name", ["d7-sparse", "d7-dense"])
def test_heights_along_x_when_a_row_spans_two_chunks(name):
    a = voxels(bricks_of(name)[0], "torch")
    want = heights_ref(name, 0)
    assert np.array_equal(array(a.heights(0), a._hip), want)
    if name == "d7-dense":          # columns of many voxels: whose lowest lies in the second chunk, whose highest in the first, that span both
        lo, hi, n = want
        assert int(n.max()) > 10 and (lo >= 256).any() and ((hi >= 0) & (hi < 256)).any() and ((lo >= 0) & (lo < 256) & (hi >= 256)).any()


def test_the_dense_grid_of_depth_6_has_columns_of_many_voxels():
    lo, hi, n = heights_ref("d6-dense", 0)
    assert int(n.max()) > 5 and ((n > 1) & (hi // 4 == lo // 4)).any() and ((n > 1) & (hi // 4 > lo // 4)).any()          # within one brick; across lanes


# ---- a shape end to end ------------------------------------------------------------------------------------------------------------------------
def test_a_shape_end_to_end():
    torch = _torch()
    depth = 4
    c = F.Context()
    shape = F.Shape(c, sphere(c, (0.0, 0.0, 0.0), 0.6))
    vox = F.voxelize(shape, depth, out=torch.zeros(8 * 8 ** depth, dtype=torch.uint8, device="cuda"))
    assert vox.on_device and vox.n > 0
    inside = vox.inside()
    N = vox.grid
    over = vox.overhangs()          # up = +z, reach2 = 1, on a bed
    assert over.on_device and np.array_equal(over.inside(), DR.overhangs(inside, 5, 1, True))
    assert over.n > 0 and not over.inside()[:, :, N // 2:].any()          # every overhang lies in the lower half
    sup = vox.supports()
    assert sup.n == int(DR.supports(inside, 5, 1, True).sum()) and sup.n > 0
    assert np.array_equal(vox.swept(4).inside(), vox.shadow(4).inside() | inside)
    h = array(vox.heights(2), vox._hip)
    assert vox.shadow(4).n == int((h[1] + 1 - h[2])[h[2] > 0].sum())
    # the two opposite shadows of a hollow box AND to exactly its cavity, along every axis
    hollow = voxels(V.pack(hollow_box16()), "torch")
    for axis in range(3):
        lo, hi = hollow.shadow(2 * axis), hollow.shadow(2 * axis + 1)
        hollow._hip.sync()
        trapped = lo.bricks & hi.bricks
        assert np.array_equal(F.voxels_unpack(trapped.cpu().numpy().view(np.uint64)), box(16, 4, 12))


# ---- determinism and refusals --------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_arrays():
    s, k = (voxels(b, "torch") for b in bricks_of("d4-random0.2"))
    for d in (0, 3, 5):
        assert np.array_equal(words(s.flow(d, blockers=k)), words(s.flow(d, blockers=k)))
    assert np.array_equal(words(s.overhangs(5, 5)), words(s.overhangs(5, 5)))
    assert np.array_equal(words(s.supports(1, 2)), words(s.supports(1, 2)))
    assert np.array_equal(array(s.heights(0), s._hip), array(s.heights(0), s._hip))


def test_refusals():
    """the refused calls - before any launch, `out` untouched - and that the context works after them"""
    torch = _torch()
    name = "d1-random0.05"
    s, k = (voxels(b, "host") for b in bricks_of(name))
    hip, lib, p = s._hip, F.lib(), F._p
    out = np.full(8, 0x5A5A5A5A5A5A5A5A, np.uint64)
    hts = np.full(3 * 8 * 8, 77, np.int32)
    flow = lambda **kw: lib.fhip_voxels_flow(*[kw.get(a, v) for a, v in (("ctx", hip._h), ("seeds", p(s.bricks)), ("blockers", p(k.bricks)), ("depth", 1), ("dev", 0),          # noqa: E731
                                                                        ("dir", 1), ("flags", 0), ("out", p(out)), ("out_dev", 0))])
    over = lambda **kw: lib.fhip_voxels_overhangs(*[kw.get(a, v) for a, v in (("ctx", hip._h), ("bricks", p(s.bricks)), ("depth", 1), ("dev", 0), ("up", 5),          # noqa: E731
                                                                             ("reach2", 1), ("bed", 1), ("out", p(out)), ("out_dev", 0))])
    high = lambda **kw: lib.fhip_voxels_heights(*[kw.get(a, v) for a, v in (("ctx", hip._h), ("bricks", p(s.bricks)), ("depth", 1), ("dev", 0), ("axis", 2),          # noqa: E731
                                                                           ("out", p(hts)), ("out_dev", 0))])
    BAD_TAPE, UNSUPPORTED = 5, 6
    assert flow(ctx=None) == BAD_TAPE and over(ctx=None) == BAD_TAPE and high(ctx=None) == BAD_TAPE
    assert flow(out=None) == BAD_TAPE and over(out=None) == BAD_TAPE and high(out=None) == BAD_TAPE
    assert flow(seeds=None) == UNSUPPORTED and over(bricks=None) == UNSUPPORTED and high(bricks=None) == UNSUPPORTED
    assert flow(seeds=None, dev=1) == UNSUPPORTED
    assert flow(depth=11) == UNSUPPORTED and over(depth=11) == UNSUPPORTED and high(depth=11) == UNSUPPORTED
    assert flow(dir=6) == UNSUPPORTED and over(up=6) == UNSUPPORTED and high(axis=3) == UNSUPPORTED
    assert over(reach2=17) == UNSUPPORTED and flow(flags=2) == UNSUPPORTED and flow(flags=3) == UNSUPPORTED
    assert flow(out=p(s.bricks)) == UNSUPPORTED and flow(out=p(k.bricks)) == UNSUPPORTED and over(out=p(s.bricks)) == UNSUPPORTED
    assert high(out=p(s.bricks)) == UNSUPPORTED
    assert (out == 0x5A5A5A5A5A5A5A5A).all() and (hts == 77).all()
    assert np.array_equal(s.bricks, bricks_of(name)[0]) and np.array_equal(k.bricks, bricks_of(name)[1])
    for call in (lambda: s.flow(6), lambda: s.overhangs(6), lambda: s.overhangs(5, 17), lambda: s.heights(3)):
        with pytest.raises(F.FidgetHipError) as e:
            call()
        assert e.value.status == UNSUPPORTED
    raw = torch.zeros(8 * 8 + 8, dtype=torch.uint8, device="cuda")          # a bitmap on the device that is not 8-byte aligned
    torch.cuda.synchronize()
    odd = F.Voxels(hip, raw[4:4 + 64], 1, None)
    for call in (lambda: odd.flow(1), lambda: odd.overhangs(), lambda: odd.heights(), lambda: voxels(bricks_of(name)[0], "torch").flow(1, out=raw[4:4 + 64])):
        with pytest.raises(F.FidgetHipError) as e:
            call()
        assert e.value.status == UNSUPPORTED and "aligned" in str(e.value)
    # seeds and blockers in different places, or of different depths
    with pytest.raises(ValueError):
        s.flow(1, blockers=voxels(bricks_of(name)[1], "torch"))
    with pytest.raises(ValueError):
        voxels(bricks_of(name)[0], "torch").flow(1, blockers=k)
    with pytest.raises(ValueError):
        s.flow(1, blockers=voxels(bricks_of("d0-full")[0], "host"))
    assert flow() == 0 and np.array_equal(out.reshape(2, 2, 2), flow_ref(name, 1, True, False))          # the context still works
