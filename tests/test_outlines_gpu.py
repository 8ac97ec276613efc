"""fhip_voxels_outlines on the device against outlines_ref.py: bitmaps made in numpy (voxels_ref.pack) and handed to the library as host
bricks and as a torch CUDA tensor, with connectivity 4 and 8; every result - the layers' ranges and sums, xy, next, loop_of, the loops'
table - is compared with np.array_equal on integers.  Then the cross-checks against what the library computes elsewhere (layer counts,
the surface's faces, the 4-connected parts), two runs, the device views, the polygons, the refused calls."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import components_ref as CR
import fidget_amd as F
import outlines_ref as OR
import voxels_ref as V
from test_mesh import sphere
from test_outlines import in_layer

pytestmark = pytest.mark.gpu
WHERE = ("host", "torch")
CONN = (4, 8)
TABLE = ("leader", "n_vertices", "area2", "perimeter", "lo", "hi")


@functools.lru_cache(maxsize=None)
def _torch():
    import torch
    return torch


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


def same(o, want, k0, k1):
    N = o.grid
    print(f"outlines N={N} layers {k0}..{k1} conn {o.connectivity}: {o.n_vertices} vertices (reference {len(want['next'])}), {o.n_loops} loops "
          f"(reference {len(want['leader'])}), perimeter {int(o.layer_perimeter.sum())} (reference {int(want['layer_perimeter'].sum())})")
    assert (o.k0, o.k1, o.n_layers) == (k0, k1, k1 - k0) and o.n_vertices == len(want["next"]) and o.n_loops == len(want["leader"])
    assert np.array_equal(o.vertex_start, want["vertex_start"].astype(np.uint64)) and np.array_equal(o.loop_start, want["loop_start"].astype(np.uint64))
    assert np.array_equal(o.layer_area2, want["layer_area2"]) and np.array_equal(o.layer_perimeter, want["layer_perimeter"].astype(np.uint64))
    assert o.xy().dtype == np.uint16 and o.next().dtype == np.uint32 and o.loop_of().dtype == np.uint32
    assert np.array_equal(o.xy(), want["xy"].astype(np.uint16)) and int(o.xy().max(initial=0)) <= N
    assert np.array_equal(o.next(), want["next"].astype(np.uint32))
    assert np.array_equal(o.loop_of(), want["loop_of"].astype(np.uint32))
    t = o.table()
    for key in TABLE:
        assert np.array_equal(t[key], want[key].astype(t[key].dtype)), key


def check(g, k0, k1, wheres=WHERE):
    """layers k0 .. k1 - 1 of the grid g [i, j, k], in both places and with both connectivities, against the reference"""
    bricks = V.pack(g)
    for conn in CONN:
        want = OR.stack(g, k0, k1, conn)
        for where in wheres:
            same(voxels(bricks, where).outlines(k0, k1, conn), want, k0, k1)


# ---- depth 0: every 2 x 2 pattern everywhere ----------------------------------------------------------------------------------------------
def test_depth_0_every_2x2_pattern_at_every_position():
    """the 16 patterns of a 2 x 2 block at each of the 9 positions - 144 layers, four to a grid - and the full and the empty layer"""
    layers = []
    for bits, (x, y) in itertools.product(range(16), itertools.product(range(3), range(3))):
        P = np.zeros((4, 4), bool)
        P[x:x + 2, y:y + 2] = np.array([[bits & 1, bits >> 3 & 1], [bits >> 1 & 1, bits >> 2 & 1]], bool)
        layers.append(P)
    layers += [np.ones((4, 4), bool), np.zeros((4, 4), bool)]
    hip = F.default_context()
    torch = _torch()
    for q in range(0, len(layers), 4):
        g = np.stack((layers[q:q + 4] + [np.zeros((4, 4), bool)] * 3)[:4], axis=2)
        bricks = V.pack(g)
        dev = torch.from_numpy(bricks.view(np.int64)).cuda()
        for conn in CONN:
            want = OR.stack(g, 0, 4, conn)
            same(F.Voxels(hip, bricks, 0, None).outlines(0, 4, conn), want, 0, 4)
            same(F.Voxels(hip, dev, 0, None).outlines(0, 4, conn), want, 0, 4)


# ---- depth 1: the brick boundary and the grid's borders ------------------------------------------------------------------------------------
def test_depth_1_across_the_brick_boundary_and_on_the_borders():
    g = np.zeros((8, 8, 8), bool)
    g[1:7, 3, 0] = g[2, 1:7, 0] = True                                  # runs across 3|4 in x and in y
    g[3:5, 3:5, 1] = np.array([[1, 0], [0, 1]], bool)                   # a saddle on the corner (4, 4) where four bricks meet
    g[3:5, 0:2, 2] = np.array([[0, 1], [1, 0]], bool)                   # saddles that straddle 3|4 in x ...
    g[0:2, 3:5, 2] = np.array([[0, 1], [1, 0]], bool)                   # ... and in y
    g[0, :, 3] = g[7, :, 3] = g[:, 0, 3] = g[:, 7, 3] = True            # a frame on all four borders
    g[0, 0, 4] = g[7, 0, 4] = g[0, 7, 4] = g[7, 7, 4] = True            # the four corners
    g[0, 2:6, 5] = g[7, 3:5, 5] = g[2:6, 0, 5] = g[3:5, 7, 5] = True    # pieces of each border
    g[:, :, 7] = np.random.default_rng(101).random((8, 8)) < 0.5
    check(g, 0, 8)


# ---- depth 4: 65 corners, one wave and one ----------------------------------------------------------------------------------------------------
def spiral(N):
    """a path one pixel wide that winds inward with a clear pixel between its turns: one long loop"""
    P = np.zeros((N, N), bool)
    l, r, b, t = 0, N - 1, 0, N - 1
    while r - l >= 2 and t - b >= 2:
        P[l:r + 1, b] = P[r, b:t + 1] = True
        P[l + 2:r + 1, t] = P[l + 2, b + 2:t + 1] = True
        l, r, b, t = l + 2, r - 2, b + 2, t - 2
    return P


@functools.lru_cache(maxsize=None)
def depth4():
    N = 64
    i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    g = np.zeros((N, N, N), bool)
    g[:, :, 0] = np.random.default_rng(102).random((N, N)) < 0.5
    g[:, :, 1] = (i + j) % 2 == 0
    g[:, 0, 2] = True
    g[:, 63, 3] = True
    g[:, :, 5] = spiral(N)
    g[:, :, 63] = np.random.default_rng(103).random((N, N)) < 0.5
    g.setflags(write=False)
    return g


def test_depth_4_random_checkerboard_rows_spiral():
    g = depth4()
    assert len(OR.layer(g[:, :, 5], 4)["leader"]) == 1 and len(OR.layer(g[:, :, 5], 4)["next"]) > 100          # the spiral: one loop
    check(g, 0, 7)


def test_layer_ranges():
    g = depth4()
    check(g, 0, 64, wheres=("torch",))          # all layers
    check(g, 5, 6)                              # a single layer
    check(g, 63, 64, wheres=("host",))
    for where in WHERE:
        v = voxels(V.pack(g), where)
        o = v.outlines(9, 9)                    # k0 == k1: an empty result
        assert (o.n_vertices, o.n_loops, o.n_layers, o.k0, o.k1, o.grid) == (0, 0, 0, 9, 9, 64) and o.vertex_start.tolist() == [0] and o.loop_start.tolist() == [0]
        assert o.xy().shape == (0, 2) and o.xy_device() is None and "vertices=0" in repr(o)
        o = v.outlines(4, 7)                    # layer 5 between two empty ones: their ranges are empty
        assert o.vertex_start[0] == o.vertex_start[1] == 0 and o.vertex_start[2] == o.vertex_start[3] == o.n_vertices > 0
        assert o.loop_start.tolist() == [0, 0, 1, 1] and o.xy(4).shape == (0, 2) and o.polygons(6) == []
        one = v.outline(5)
        assert np.array_equal(one.xy(), o.xy(5)) and np.array_equal(one.next(), o.next(5)) and one.n_loops == 1
        o = v.outlines(20, 30)                  # nothing but empty layers: no arrays
        assert o.n_vertices == 0 and o.vertex_start.tolist() == [0] * 11 and o.layer_area2.tolist() == [0] * 10 and o.next_device() is None


# ---- depth 6 and 7: rows longer than a wave ---------------------------------------------------------------------------------------------------
def test_depth_6_random_layers_and_bars_through_every_chunk():
    g = np.tile(np.random.default_rng(104).random((64, 64, 64)) < 0.3, (4, 4, 4))
    g[:, :, 5] = False
    g[:, 100, 5] = g[77, :, 5] = True          # a bar of 256 pixels along x and one along y, crossing
    g[:, :, 6] = False
    g[:, 0, 6] = g[255, :, 6] = g[3:250, 255, 6] = True
    check(g, 3, 9)


def test_depth_7_bars_in_the_first_and_the_last_layer():
    N = 512
    g = np.zeros((N, N, N), bool)
    for k in (0, N - 1):
        g[:, 300, k] = g[129, :, k] = True
    bricks = V.pack(g)
    want = OR.stack(g, 0, N, 4)
    assert len(want["next"]) == 24 and np.array_equal(OR.stack(g, 0, N, 8)["next"], want["next"])          # no saddles: the connectivities agree
    for where in WHERE:
        for conn in CONN:
            same(voxels(bricks, where).outlines(0, N, conn), want, 0, N)


# ---- against what the library computes elsewhere ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sphere_with_hole():
    c = F.Context()
    return F.voxelize(F.Shape(c, c.max(sphere(c, (0.0, 0.0, 0.0), 0.8), c.neg(sphere(c, (0.2, 0.1, 0.0), 0.35)))), 5)


@pytest.mark.parametrize("shrunk", [False, True])
def test_cross_checks_on_a_sphere_with_a_hole(shrunk):
    v = sphere_with_hole().offset(-2) if shrunk else sphere_with_hole()
    N = v.grid
    inside = v.inside()
    for conn in CONN:
        o = v.outlines(0, N, conn)
        print(f"sphere with a hole, shrunk {shrunk}, conn {conn}: {v.n} voxels, {o.n_vertices} vertices, {o.n_loops} loops, {int((o.table()['area2'] < 0).sum())} holes, "
              f"perimeter {int(o.layer_perimeter.sum())}, faces {v.surface().faces}")
        assert np.array_equal(o.layer_area2, 2 * v.layer_counts().astype(np.int64))
        assert int(o.layer_perimeter.sum()) == int(sum(v.surface().faces[0:4]))
        assert (o.table()["area2"] < 0).any()          # the cavity shows as holes
    o = v.outlines(0, N, 4)
    for k in (N // 2, N // 2 + 9, 8):
        parts = CR.components(in_layer(inside[:, :, k], 1), 6).count
        assert int((o.table(k)["area2"] > 0).sum()) == parts and (parts > 0 or k == 8)
    same(v.outlines(60, 66, 8), OR.stack(inside, 60, 66, 8), 60, 66)


def test_two_runs_device_views_and_polygons():
    torch = _torch()
    g = depth4()
    v = voxels(V.pack(g), "torch")
    a, b = v.outlines(0, 7, 8), v.outlines(0, 7, 8)
    assert np.array_equal(a.xy(), b.xy()) and np.array_equal(a.next(), b.next()) and np.array_equal(a.loop_of(), b.loop_of())
    assert all(np.array_equal(a.table()[key], b.table()[key]) for key in TABLE)
    xy, nxt, loop = (torch.as_tensor(d, device="cuda").cpu().numpy() for d in (a.xy_device(), a.next_device(), a.loop_of_device()))
    assert np.array_equal(xy.view(np.uint16), a.xy()) and np.array_equal(nxt.view(np.uint32), a.next()) and np.array_equal(loop.view(np.uint32), a.loop_of())
    for k in (0, 1, 5):
        polys, t = a.polygons(k), a.table(k)
        assert len(polys) == len(t["leader"])
        nx, allxy = a.next(), a.xy()
        for p, leader, m, area2 in zip(polys, t["leader"], t["n_vertices"], t["area2"]):
            assert p.shape == (m, 2) and np.array_equal(p[0], allxy[leader])
            w = int(leader)
            for _ in range(int(m)):
                w = int(nx[w])
            assert w == int(leader)          # back at the leader after n_vertices steps
            assert int((p[:, 0] * np.roll(p[:, 1], -1) - np.roll(p[:, 0], -1) * p[:, 1]).sum()) == int(area2)
        world, z = a.world(k)
        assert z == float(np.float32(2 * k + 1 - 64) / np.float32(64)) and all(np.array_equal(w, ((2 * p - 64) / 64).astype(np.float32)) for w, p in zip(world, polys))
    svg = a.svg(5)
    assert svg.count("<path") == 1 and 'fill-rule="evenodd"' in svg and svg.count(" L ") == int(a.table(5)["n_vertices"][0]) - 1 and " Z" in svg


def test_refusals():
    g = depth4()
    v = voxels(V.pack(g), "host")
    hip, lib, p = v._hip, F.lib(), F._p
    h = C.c_void_p()
    call = lambda **kw: lib.fhip_voxels_outlines(*[kw.get(a, d) for a, d in (("ctx", hip._h), ("bricks", p(v.bricks)), ("depth", 4), ("dev", 0), ("k0", 0), ("k1", 2),          # noqa: E731
                                                                            ("conn", 4), ("out", C.byref(h)))])
    BAD_TAPE, UNSUPPORTED = 5, 6
    assert call(ctx=None) == BAD_TAPE and call(out=None) == BAD_TAPE
    for kw in ({"k0": 3, "k1": 2}, {"k1": 65}, {"depth": 11}, {"conn": 6}, {"conn": 0}, {"bricks": None}):
        assert call(**kw) == UNSUPPORTED and h.value is None, kw
    for bad in (lambda: v.outlines(3, 2), lambda: v.outlines(0, 65), lambda: v.outlines(0, 1, 6)):
        with pytest.raises(F.FidgetHipError) as e:
            bad()
        assert e.value.status == UNSUPPORTED
    o = v.outlines(0, 2)
    n, m = o.n_vertices, o.n_loops
    buf = np.zeros(2 * n + 2, np.uint32)
    assert lib.fhip_outlines_vertices(o._owner.h, 1, n, None, p(buf), None) == UNSUPPORTED and lib.fhip_outlines_vertices(o._owner.h, n + 1, 0, None, None, None) == UNSUPPORTED
    assert lib.fhip_outlines_loops(o._owner.h, m, 1, p(buf), None, None, None, None, None) == UNSUPPORTED and not buf.any()
    assert lib.fhip_outlines_vertices(o._owner.h, n - 1, 1, None, p(buf), None) == 0 and buf[0] == o.next()[-1]          # any pointer may be NULL
    assert lib.fhip_outlines_loops(o._owner.h, 0, m, None, None, None, None, None, None) == 0
    with pytest.raises(IndexError):
        o.xy(2)
    same(v.outlines(0, 2), OR.stack(g, 0, 2, 4), 0, 2)          # the context still works
