"""fhip_contour2d on the device against the numpy model contours_ref.py run on the ORACLE's pixel-perfect render2d image of the same
configuration: vertices bit for bit, segments and next equal, the loops the model's.  Shapes: disc, annulus, both saddles, the NaN and
-inf shapes, bear.vm with its region moved, a shape with a bound variable, each at every size of the list; sizes with blocks straddling row ends (40 x 24, 200 x 136 -
no multiple of the render's tiles, scans of more than one block's worth of cells -, 257 x 3), and the sizes without cells."""
import numpy as np
import pytest

import fidget_amd as F
import contours_cases as K
import contours_ref as R

pytestmark = pytest.mark.gpu

NONE = R.NONE
_made = {}


def shape(make):
    if make not in _made:
        _made[make] = make(F)
    return _made[make]


def check(make, w, h, z=0.0, w2m=None, vars_=None):
    m = R.contours(K.image(make, w, h, z, w2m, vars_))
    c = F.contour(shape(make), w, h, z=z, world_to_model=w2m, vars=vars_)
    print(f"{w} x {h} z {z}: device vertices {c.n_vertices} segments {c.n_segments}; model {len(m['vertices'])} {len(m['segments'])}; "
          f"cases {sorted(m['hist'].items(), key=str)}; t = 0.5 by rule {m['t_half']}")
    assert (c.n_vertices, c.n_segments, c.width, c.height) == (len(m["vertices"]), len(m["segments"]), w, h)
    assert c.vertices.dtype == np.float32 and c.vertices.shape == (c.n_vertices, 2)
    assert c.segments.dtype == np.uint32 and c.segments.shape == (c.n_segments, 2)
    assert np.array_equal(c.vertices.view(np.uint32), m["vertices"].view(np.uint32))          # bit for bit
    assert np.array_equal(c.segments, m["segments"])
    assert np.array_equal(c.next, m["next"])
    assert [([int(v) for v in ids], closed) for ids, closed in c.loops()] == R.loops(m["next"])
    return c, m


SIZES = [(16, 16), (40, 24), (200, 136), (257, 3), (2, 2), (1, 8)]
K15 = (2.0 / 15) ** 2 / 8
# name -> (shape, world_to_model, vars)
SHAPES = {"disc": (K.disc, None, None), "annulus": (K.annulus, None, None), "saddle": (K.saddle(1, K15), None, None),
          "saddle-other": (K.saddle(-1, -K15), None, None), "sqrt-x": (K.sqrt_x, None, None), "inv-square": (K.inv_square, None, None),
          "bear-moved": (K.bear, K.BEAR_W2M_2D, None), "var-disc": (K.var_disc, None, {7: 0.55})}


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_and_sizes(name, w, h):
    make, w2m, vars_ = SHAPES[name]
    check(make, w, h, w2m=w2m, vars_=vars_)


def test_prefix_sums_of_more_than_one_block():
    """513 x 512: 524 287 lattice edges are 2048 blocks of 256 - the first size at which the counts' prefix sums take a second block of
    k_scan_block (one element in it) and k_scan_add"""
    c, _ = check(K.annulus, 513, 512)
    assert c.n_vertices > 2000


def test_saddles_both_ways():
    """an odd size: the origin in the middle of a cell (tests/test_contours.py test_both_saddles_both_ways)"""
    hist = {}
    for sign in (1, -1):
        for k in (K15, -K15):
            _, m = check(K.saddle(sign, k), 15, 15)
            for key, v in m["hist"].items():
                hist[key] = hist.get(key, 0) + v
    for key in ((5, True), (5, False), (10, True), (10, False)):
        assert hist.get(key, 0) >= 1, key


def test_the_middle_rule_on_the_device():
    for make, w, h in ((K.sqrt_x, 16, 16), (K.inv_square, 16, 8)):
        _, m = check(make, w, h)
        assert m["t_half"] >= 1


@pytest.mark.parametrize("z", [0.0, 0.3])
def test_z(z):
    check(K.bear, 40, 24, z=z)


@pytest.mark.parametrize("w,h,z", [(200, 136, 0.0), (64, 48, 0.125)])
def test_bear_moved(w, h, z):
    c, _ = check(K.bear, w, h, z=z, w2m=K.BEAR_W2M_2D)
    assert c.n_vertices > 0


def test_world_to_model():
    a, s = 0.5, 1.25
    m = np.array([[s * np.cos(a), -s * np.sin(a), 0.1], [s * np.sin(a), s * np.cos(a), -0.05], [0, 0, 1]], np.float32)
    check(K.annulus, 40, 24, w2m=m)
    check(K.two_discs, 40, 24, w2m=m)


def test_bound_variable_and_missing_variable():
    c, _ = check(K.var_disc, 40, 24, vars_={7: 0.55})
    assert c.n_vertices > 0
    with pytest.raises(ValueError):
        F.contour(shape(K.var_disc), 40, 24)


def test_loops_areas_world_and_svg():
    c, m = check(K.annulus, 40, 40)
    areas = c.areas()
    assert [a > 0 for a in areas] == [True, False] and all(closed for _, closed in c.loops())
    assert np.allclose(areas, [R.area(m["vertices"], ids) for ids, _ in R.loops(m["next"])], rtol=1e-12, atol=0)
    s2w = F.screen_to_world((40, 40))
    want = np.array([[np.float32(np.float32(s2w[r, 0] * x) + np.float32(s2w[r, 1] * y)) + s2w[r, 2] for r in range(2)] for x, y in c.vertices], np.float32)
    assert np.array_equal(c.world().view(np.uint32), want.view(np.uint32))
    text = c.svg()
    assert text.count("<path") == 1 and 'fill-rule="evenodd"' in text and text.count("M ") == 2 and text.count(" Z") == 2
    first = int(c.loops()[0][0][0])          # the path starts at the first loop's first vertex: world x, world y negated (SVG's y grows downward)
    assert f'd="M {float(want[first, 0]):.9g} {-float(want[first, 1]):.9g} L ' in text


def test_device_views_are_the_host_copies():
    import torch
    c, _ = check(K.disc, 200, 136)
    v = torch.as_tensor(c.vertices_device(), device="cuda")
    s = torch.as_tensor(c.segments_device(), device="cuda")
    assert tuple(v.shape) == (c.n_vertices, 2) and tuple(s.shape) == (c.n_segments, 2)
    assert np.array_equal(v.cpu().numpy().view(np.uint32), c.vertices.view(np.uint32))
    assert np.array_equal(s.cpu().numpy().view(np.uint32), c.segments)
    empty = F.contour(shape(K.sqrt_x), 1, 8)          # (x = -1 in its one column: NaN, outside)
    assert empty.n_vertices == 0 and empty.vertices_device() is None and empty.segments_device() is None and empty.loops() == []


def test_a_stack_of_slices_is_the_single_calls():
    zs = [-0.1, 0.0, 0.125]
    stack = F.slice_stack(shape(K.bear), (64, 48), zs, world_to_model=K.BEAR_W2M_2D)
    assert len(stack) == 3
    for z, c in zip(zs, stack):
        one = F.contour(shape(K.bear), 64, 48, z=z, world_to_model=K.BEAR_W2M_2D)
        assert c.z == z and (c.n_vertices, c.n_segments) == (one.n_vertices, one.n_segments)
        assert np.array_equal(c.vertices.view(np.uint32), one.vertices.view(np.uint32))
        assert np.array_equal(c.segments, one.segments) and np.array_equal(c.next, one.next)
    assert len({c.n_vertices for c in stack}) > 1          # (the layers differ)


def test_a_context_is_reused_after_free():
    first, _ = check(K.disc, 40, 24)
    n = first.n_vertices
    del first          # fhip_contours_free
    again, _ = check(K.disc, 40, 24)
    assert again.n_vertices == n
    check(K.annulus, 16, 16)         # another shape, another size, the same context's buffers
    img = F.render2d(shape(K.disc), 40, 24, pixel_perfect=True)[0]         # and render2d still gives the image the contours came from
    assert np.array_equal(img.view(np.uint32), K.image(K.disc, 40, 24).view(np.uint32))
