"""fhip_outlines_nesting on the device against nesting_ref.py: bitmaps made in numpy (voxels_ref.pack) and handed to the library as host
bricks and as a torch CUDA tensor, with connectivity 4 and 8; every result - left, parent, depth, n_children, region_area2 per loop,
outer, top, max_depth per layer, the totals - is compared with np.array_equal on integers.  Then the region sums against the
library's own connected components on layers of a voxelized shape, two runs, the device views, sub-ranges, the regions, the SVG and
the refused calls."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
from conftest import model_path

import fidget_amd as F
import nesting_ref as NR
import outlines_ref as OR
import voxels_ref as V
from test_nesting import checkerboard, far_hole, hole_with_islands, in_layers, plate_with_holes, rings
from test_outlines_gpu import _torch, spiral, voxels

pytestmark = pytest.mark.gpu
WHERE = ("host", "torch")
CONN = (4, 8)
PER_LOOP = ("left", "parent", "depth", "n_children", "region_area2")


def same(t, S, want, k0, k1):
    """the Nesting t against the reference `want` of the reference outlines S"""
    print(f"nesting layers {k0}..{k1} conn {t.connectivity}: {t.n_loops} loops (reference {len(want['parent'])}), {t.n_outer} outer, {t.n_top} top, max depth "
          f"{t.max_depth} (reference {int(want['max_depth'].max(initial=0))})")
    assert (t.k0, t.k1, t.n_layers, t.n_loops) == (k0, k1, k1 - k0, len(want["parent"])) and t.n_loops == t.outlines.n_loops
    assert np.array_equal(t.outlines.loop_start, S["loop_start"].astype(np.uint64))
    for key in PER_LOOP:
        got = getattr(t, key)
        assert got.dtype == want[key].dtype and np.array_equal(got, want[key]), key
    assert np.array_equal(t.outer, want["outer"]) and np.array_equal(t.top, want["top"]) and np.array_equal(t.layer_max_depth, want["max_depth"])
    assert (t.n_outer, t.n_top, t.max_depth) == (int(want["outer"].sum()), int(want["top"].sum()), int(want["max_depth"].max(initial=0)))


def check(g, k0, k1, wheres=WHERE):
    """layers k0 .. k1 - 1 of the grid g [i, j, k], in both places and with both connectivities, against the reference"""
    bricks = V.pack(g)
    for conn in CONN:
        S = OR.stack(g, k0, k1, conn)
        want = NR.stack(S)
        for where in wheres:
            same(voxels(bricks, where).outlines(k0, k1, conn).nesting(), S, want, k0, k1)


# ---- depth 0: every 2 x 2 pattern everywhere: saddles, and the comparison with the outside at a = 0 ------------------------------------------
def test_depth_0_every_2x2_pattern_at_every_position():
    layers = []
    for bits, (x, y) in itertools.product(range(16), itertools.product(range(3), range(3))):
        P = np.zeros((4, 4), bool)
        P[x:x + 2, y:y + 2] = np.array([[bits & 1, bits >> 3 & 1], [bits >> 1 & 1, bits >> 2 & 1]], bool)
        layers.append(P)
    layers += [np.ones((4, 4), bool), np.zeros((4, 4), bool)]
    for q in range(0, len(layers), 4):
        check(np.stack((layers[q:q + 4] + [np.zeros((4, 4), bool)] * 3)[:4], axis=2), 0, 4)


# ---- depth 1: the brick boundary and the grid's borders ------------------------------------------------------------------------------------
def test_depth_1_across_the_brick_boundary_and_on_the_borders():
    g = np.zeros((8, 8, 8), bool)
    g[1:7, 1:7, 0] = True
    g[2:6, 2:6, 0] = False
    g[3, 4, 0] = True                                                   # a ring across 3|4 that holds a one-pixel island
    g[:, :, 1] = rings(8, 2, 1)                                         # a frame on all four borders with a ring inside it
    g[:, :, 3] = np.random.default_rng(201).random((8, 8)) < 0.5       # (layer 2 stays empty)
    check(g, 0, 4)
    S = OR.stack(g, 0, 4, 4)
    assert NR.stack(S)["depth"][:7].tolist() == [0, 1, 2, 0, 1, 2, 3] and S["loop_start"].tolist()[:4] == [0, 3, 7, 7]


# ---- depth 4: 65 corners, three chunks, rows wider than a word ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def depth4():
    N = 64
    rng = np.random.default_rng(202)
    g = in_layers([rings(N, 7, 2), plate_with_holes(N, 15), hole_with_islands(N, 16), spiral(N), far_hole(N), checkerboard(N), rng.random((N, N)) < 0.3,
                   np.zeros((N, N), bool), rng.random((N, N)) < 0.5, rng.random((N, N)) < 0.7], N)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def depth4_reference(conn):
    S = OR.stack(depth4(), 0, 10, conn)
    return S, NR.stack(S)


def test_depth_4_rings_chains_spiral_far_hole_checkerboard_random():
    g = depth4()
    S, want = depth4_reference(4)
    ls = S["loop_start"]
    assert want["max_depth"].tolist()[:6] == [13, 1, 2, 0, 1, 0] and int(ls[4] - ls[3]) == 1                 # the rings; the spiral is one loop
    assert want["left"][ls[1]:ls[2]].tolist() == [NR.NONE] + list(range(ls[1], ls[1] + 15))                # the sibling chain: 15 links
    assert int(ls[6] - ls[5]) == 2048 and int(want["top"][5]) == 2048                                       # the checkerboard with 4: all at the top
    bricks = V.pack(g)
    for conn in CONN:
        S, want = depth4_reference(conn)
        for where in WHERE:
            same(voxels(bricks, where).outlines(0, 10, conn).nesting(), S, want, 0, 10)


# ---- depth 5: the regions against the library's connected components -------------------------------------------------------------------------------
def test_depth_5_regions_are_the_connected_parts_of_a_layer():
    torch = _torch()
    dev = torch.empty(32 ** 3, dtype=torch.int64, device="cuda")
    v = F.voxelize(F.Shape.from_vm(model_path("gyroid-sphere.vm")), 5, out=dev)
    layers = (37, 64, 90, 126)
    for conn, conn3 in ((4, 6), (8, 26)):
        for k in layers:
            t = v.outline(k, conn).nesting()
            mask = 0xFFFF << (16 * (k & 3))
            alone = torch.zeros_like(v.bricks)
            alone[k >> 2] = v.bricks[k >> 2] & (mask - (1 << 64) if mask >= 1 << 63 else mask)          # the layer's bits alone
            parts = F.Voxels(v._hip, alone, 5, None).components(conn3)
            outer = t.outlines.table()["area2"] > 0
            print(f"gyroid-sphere depth 5 layer {k} conn {conn}: {t.n_loops} loops, {t.n_outer} outer, max depth {t.max_depth}; {parts.count} parts of {parts.n} voxels")
            assert int(t.outer[0]) == t.n_outer == parts.count == int(outer.sum()) and (parts.count > 0 or k == 126)
            assert np.array_equal(np.sort(t.region_area2[outer] // 2), np.sort(parts.sizes.astype(np.int64)))


# ---- consistency -------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_device_views_sub_ranges_regions_and_svg():
    torch = _torch()
    g = depth4()
    v = voxels(V.pack(g), "torch")
    o = v.outlines(0, 64, 8)
    a, b = o.nesting(), o.nesting()
    assert all(np.array_equal(getattr(a, key), getattr(b, key)) for key in PER_LOOP)
    assert np.array_equal(a.outer, b.outer) and np.array_equal(a.top, b.top) and np.array_equal(a.layer_max_depth, b.layer_max_depth)
    parent, depth = (torch.as_tensor(d, device="cuda").cpu().numpy().view(np.uint32) for d in (a.parent_device(), a.depth_device()))
    assert np.array_equal(parent, a.parent) and np.array_equal(depth, a.depth)
    # a sub-range is the slice of all layers, ids shifted
    sub = v.outlines(2, 9, 8).nesting()
    l0, l1 = int(o.loop_start[2]), int(o.loop_start[9])
    assert sub.n_loops == l1 - l0
    for key in ("left", "parent"):
        want = getattr(a, key)[l0:l1].astype(np.int64)
        assert np.array_equal(getattr(sub, key), np.where(want == NR.NONE, NR.NONE, want - l0).astype(np.uint32)), key
    for key in ("depth", "n_children", "region_area2"):
        assert np.array_equal(getattr(sub, key), getattr(a, key)[l0:l1]), key
    assert np.array_equal(sub.outer, a.outer[2:9]) and np.array_equal(sub.top, a.top[2:9]) and np.array_equal(sub.layer_max_depth, a.layer_max_depth[2:9])
    # the sums: every loop's area2 is counted once in the region sums, and the outer boundaries' regions are the layer's set pixels
    area2 = o.table()["area2"]
    counts = v.layer_counts().cpu().numpy()
    for k in range(10):
        l0, l1 = int(o.loop_start[k]), int(o.loop_start[k + 1])
        top = a.parent[l0:l1] == NR.NONE
        assert int(a.region_area2[l0:l1].sum()) - int(area2[l0:l1][~top].sum()) == int(o.layer_area2[k])
        assert int(a.region_area2[l0:l1][area2[l0:l1] > 0].sum()) == int(o.layer_area2[k]) == 2 * int(counts[k])
        regions = a.regions(k)
        assert sorted([l for l, _ in regions] + [h for _, holes in regions for h in holes]) == list(range(l0, l1))
        assert all(area2[l] > 0 and all(area2[h] < 0 and a.parent[h] == l for h in holes) for l, holes in regions)
        polys, flat = a.polygons(k), o.polygons(k)
        assert len(polys) == len(regions) and all(np.array_equal(p, flat[l - l0]) and all(np.array_equal(q, flat[h - l0]) for q, h in zip(hs, holes))
                                                   for (p, hs), (l, holes) in zip(polys, regions))
        svg = a.svg(k)
        assert svg.count("<path") == int(a.outer[k]) == len(regions) and svg.count(" Z") == l1 - l0 and svg.count('fill-rule="evenodd"') == len(regions)
    start, kids = a.children()
    want_start, want = NR.children(a.parent)
    assert np.array_equal(start, want_start) and np.array_equal(kids, want)
    with pytest.raises(IndexError):
        a.regions(64)


def test_the_region_sums_count_every_loop_once():
    """summing region_area2 over a layer's loops counts a loop with a parent twice - in its own row and in its parent's - and the others
    once: without the second count the sum is the layer's area2.  (The plain sum is not: a 6 x 6 ring whose 4 x 4 hole holds one pixel
    has area2 72, -32, 2 and region sums 40, -30, 2 - these add up to 12, the layer's area2 is 42.  The outer boundaries' region sums
    alone, 40 + 2, are the layer's area2, which test_two_runs_device_views_sub_ranges_regions_and_svg asserts.)"""
    v = voxels(V.pack(depth4()), "host")
    o = v.outlines(0, 10, 4)
    t = o.nesting()
    area2 = o.table()["area2"]
    own = np.zeros(t.n_loops, np.int64)
    has = t.parent != NR.NONE
    np.add.at(own, t.parent[has].astype(np.int64), area2[has])
    assert np.array_equal(t.region_area2 - own, area2)
    for k in range(10):
        l0, l1 = int(o.loop_start[k]), int(o.loop_start[k + 1])
        assert int((t.region_area2 - own)[l0:l1].sum()) == int(o.layer_area2[k])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    v = voxels(V.pack(depth4()), "host")
    hip, lib, p = v._hip, F.lib(), F._p
    o = v.outlines(0, 3, 4)
    h = C.c_void_p()
    BAD_TAPE, UNSUPPORTED = 5, 6
    assert lib.fhip_outlines_nesting(hip._h, None, p(v.bricks), 0, C.byref(h)) == BAD_TAPE and h.value is None
    assert lib.fhip_outlines_nesting(hip._h, o._owner.h, None, 0, C.byref(h)) == UNSUPPORTED and h.value is None
    assert lib.fhip_outlines_nesting(None, o._owner.h, p(v.bricks), 0, C.byref(h)) == BAD_TAPE and lib.fhip_outlines_nesting(hip._h, o._owner.h, p(v.bricks), 0, None) == BAD_TAPE
    t = o.nesting()
    n = t.n_loops
    buf = np.zeros(n + 2, np.uint32)
    assert lib.fhip_nesting_loops(t._owner.h, 1, n, p(buf), None, None, None, None) == UNSUPPORTED and lib.fhip_nesting_loops(t._owner.h, n + 1, 0, None, None, None, None, None) == UNSUPPORTED
    assert not buf.any()
    assert lib.fhip_nesting_loops(t._owner.h, n - 1, 1, None, None, p(buf), None, None) == 0 and buf[0] == t.depth[-1]          # any pointer may be NULL
    assert lib.fhip_nesting_loops(None, 0, 0, None, None, None, None, None) == BAD_TAPE and lib.fhip_nesting_layers(None, None, None, None) == BAD_TAPE
    assert lib.fhip_nesting_layers(t._owner.h, None, None, None) == 0
    for where in WHERE:
        w = voxels(V.pack(depth4()), where)
        e = w.outlines(9, 9).nesting()          # k0 == k1: an empty nesting
        assert (e.n_loops, e.n_outer, e.n_top, e.max_depth, e.n_layers, e.k0, e.k1) == (0, 0, 0, 0, 0, 9, 9)
        assert all(getattr(e, key).shape == (0,) for key in PER_LOOP) and e.outer.shape == (0,) and e.parent_device() is None and e.depth_device() is None
        assert e.children()[0].tolist() == [0] and e.children()[1].shape == (0,) and "loops=0" in repr(e)
        e = w.outlines(20, 23).nesting()          # nothing but empty layers
        assert e.n_loops == 0 and e.outer.tolist() == [0, 0, 0] and e.top.tolist() == [0, 0, 0] and e.layer_max_depth.tolist() == [0, 0, 0] and e.regions(21) == []
        assert e.svg(21).count("<path") == 0
    same(v.outlines(0, 3, 4).nesting(), OR.stack(depth4(), 0, 3, 4), NR.stack(OR.stack(depth4(), 0, 3, 4)), 0, 3)          # the context still works
