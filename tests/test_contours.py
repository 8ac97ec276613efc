"""2D contouring without a GPU: the arithmetic of fidget_amd/csrc/contour/contour.hpp built for the host
(tests/host_build/contour_host.cpp: the kernels' passes as plain loops over the header) against the numpy model contours_ref.py -
vertices by bits, segments and next equal - on the oracle's pixel-perfect images and on hand-made arrays; and properties that hold the
model and the header without using the case table: every vertex used at most once each way, the inside on every segment's left, the
number and the signs of the loops, areas against pixel counts, both resolutions of both saddles, the t = 0.5 rule, the empty sizes.
The same program built with the address and undefined-behaviour sanitizers runs once."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import fidget_amd as F
import contours_cases as K
import contours_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "contour_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "host_build", "_build")
NONE = R.NONE


def build(name, flags):
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, name)
    deps = [SRC, os.path.join(CSRC, "contour", "contour.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", CSRC, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exe():
    return build("contour_host", ["-O1"])


def host(exe, img, tmp_path, tag="c"):
    """the host build's result for an [H, W] float32 image, in the layout of contours_ref.contours plus "loops" """
    img = np.ascontiguousarray(img, np.float32)
    h, w = img.shape
    fin, fout = str(tmp_path / (tag + ".in")), str(tmp_path / (tag + ".out"))
    with open(fin, "wb") as f:
        f.write(struct.pack("<II", w, h))
        f.write(img.tobytes())
    subprocess.run([exe, fin, fout], check=True)
    raw = open(fout, "rb").read()
    nv, ns, nl = struct.unpack_from("<QQQ", raw, 0)
    at = 24

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(raw, dtype, n, at)
        at += a.nbytes
        return a
    res = {"vertices": take("<f4", 2 * nv).reshape(-1, 2), "segments": take("<u4", 2 * ns).reshape(-1, 2), "next": take("<u4", nv)}
    order, start, closed = take("<u4", nv), take("<u8", nl + 1), take("u1", nl)
    assert at == len(raw)
    res["loops"] = [([int(v) for v in order[int(start[k]):int(start[k + 1])]], bool(closed[k])) for k in range(nl)]
    return res


def same(got, want):
    assert got["vertices"].shape == want["vertices"].shape
    assert np.array_equal(got["vertices"].view(np.uint32), want["vertices"].view(np.uint32))          # by bits
    assert np.array_equal(got["segments"], want["segments"])
    assert np.array_equal(got["next"], want["next"])


def on_border(edge, w, h):
    kind, i, j = edge
    return (j == 0 or j == h - 1) if kind == "h" else (i == 0 or i == w - 1)


def properties(img, m):
    """what holds for every image, checked on the model's result `m` without its table"""
    h, w = img.shape
    segs, verts = m["segments"].astype(np.int64), m["vertices"].astype(np.float64)
    n = len(verts)
    out_deg, in_deg = np.bincount(segs[:, 0], minlength=n), np.bincount(segs[:, 1], minlength=n)
    assert out_deg.max(initial=0) <= 1 and in_deg.max(initial=0) <= 1
    for k, e in enumerate(m["edge_of"]):
        if not on_border(e, w, h):
            assert out_deg[k] == 1 and in_deg[k] == 1, (k, e)
    # next is the segments, and nothing else
    want = np.full(n, NONE, np.uint32)
    want[segs[:, 0]] = segs[:, 1]
    assert np.array_equal(m["next"], want)
    # the inside on the left: some inside corner of the cell lies strictly to the left of every segment.  (A segment of no length has
    # no left: a pixel of exactly 0 is outside and puts the vertices of its edges - t = 0 or 1 - on itself, two of them in one cell.
    # Its cross products are 0 by necessity; it must then sit on an outside corner.)
    for (a, b), (i, j) in zip(segs, m["cell_of"]):
        d = verts[b] - verts[a]
        corners = ((i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1))
        left = [d[0] * (cy - verts[a][1]) - d[1] * (cx - verts[a][0]) for cx, cy in corners if img[cy, cx] < 0]
        assert left, (i, j)
        if d[0] == 0 and d[1] == 0:
            assert any(verts[a][0] == cx and verts[a][1] == cy and not img[cy, cx] < 0 for cx, cy in corners), (i, j)
        else:
            assert max(left) > 0, (i, j)


CASES = {
    "disc": (K.disc, 40, 24, 0.0, None, None),
    "disc-z": (K.disc, 16, 16, 0.25, None, None),
    "annulus": (K.annulus, 40, 40, 0.0, None, None),
    "two-discs": (K.two_discs, 48, 32, 0.0, None, None),
    "sqrt-x": (K.sqrt_x, 16, 16, 0.0, None, None),
    "inv-square": (K.inv_square, 16, 8, 0.0, None, None),
    "var-disc": (K.var_disc, 24, 40, 0.0, None, {7: 0.55}),
    "bear": (K.bear, 64, 48, 0.0, K.BEAR_W2M_2D, None),
    "bear-z": (K.bear, 33, 37, 0.125, None, None),
}


@pytest.fixture(scope="module")
def images():
    return {name: K.image(make, w, h, z, w2m, vars_) for name, (make, w, h, z, w2m, vars_) in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_the_header_gives_what_the_model_gives(exe, images, tmp_path, name):
    img = images[name]
    m = R.contours(img)
    got = host(exe, img, tmp_path)
    print(name, img.shape, "vertices", len(m["vertices"]), "segments", len(m["segments"]), "loops", len(got["loops"]))
    assert len(m["vertices"]) > 0
    same(got, m)
    assert got["loops"] == R.loops(m["next"])
    properties(img, m)


def loop_areas(m):
    return [(closed, R.area(m["vertices"], ids)) for ids, closed in R.loops(m["next"])]


def clear_of_border(img):
    inside = img < 0
    return not (inside[0].any() or inside[-1].any() or inside[:, 0].any() or inside[:, -1].any())


@pytest.mark.parametrize("name,signs", [("disc", "+"), ("annulus", "+-"), ("two-discs", "++")])
def test_loops_and_areas(images, name, signs):
    img = images[name]
    assert clear_of_border(img)
    m = R.contours(img)
    areas = loop_areas(m)
    print(name, areas, "pixels inside", int((img < 0).sum()))
    assert all(closed for closed, _ in areas)
    assert "".join("+" if a > 0 else "-" for _, a in areas) == signs
    # contour and pixel staircase differ only inside cells that carry a segment, each of area 1
    assert abs(sum(a for _, a in areas) - int((img < 0).sum())) <= len(m["segments"])


def test_both_saddles_both_ways(exe, tmp_path):
    """x y - k and k - x y for both signs of k.  Pixel i of a width W sits at x = (i - W / 2) * 2 / min(W, H) (screen_to_world), so it is
    an ODD size that puts the origin in the middle of a cell, its corners at (+-p / 2, +-p / 2) with alternating signs of x y; on an
    even size the origin is a pixel and no cell of x y - k is a saddle for any k (the products at a cell's corners are integers
    times p^2 with p00 + p11 = p10 + p01 + 1: both of one diagonal can never lie strictly beyond both of the other)."""
    n = 15
    k = (2.0 / n) ** 2 / 8          # below a quarter of the pitch squared
    hist = {}
    for sign in (1, -1):
        for kk in (k, -k):
            img = K.image(K.saddle(sign, kk), n, n)
            m = R.contours(img)
            same(host(exe, img, tmp_path, f"s{sign}{kk > 0}"), m)
            properties(img, m)
            for key, v in m["hist"].items():
                hist[key] = hist.get(key, 0) + v
    print(hist)
    for key in ((5, True), (5, False), (10, True), (10, False)):
        assert hist.get(key, 0) >= 1, key


@pytest.mark.parametrize("name", ["sqrt-x", "inv-square"])
def test_ends_that_are_not_finite_take_the_middle(images, name):
    """sqrt(x) - 0.5 is NaN left of x = 0; 4 - 1 / (4 x)^2 is -inf on the column x = 0, which is column W / 2 of an EVEN width (pixel i
    sits at x = (i - W / 2) * 2 / min(W, H)), between columns that are outside"""
    img = images[name]
    assert not np.isfinite(img).all()
    m = R.contours(img)
    print(name, "t = 0.5 by rule:", m["t_half"], "of", len(m["vertices"]))
    assert m["t_half"] >= 1


def test_hand_made_images(exe, tmp_path):
    rng = np.random.default_rng(7)
    noise = rng.standard_normal((9, 13)).astype(np.float32)          # every case of the table, many saddles, open chains on every border
    noise[2, 3], noise[4, 4], noise[5, 1] = np.nan, np.inf, -np.inf
    wide = rng.standard_normal((3, 300)).astype(np.float32)         # edges and cells past one block of 256, rows ending inside a block
    for tag, img in (("noise", noise), ("wide", wide), ("tall", wide.T.copy())):
        m = R.contours(img)
        got = host(exe, img, tmp_path, tag)
        same(got, m)
        assert got["loops"] == R.loops(m["next"])
        properties(img, m)
    assert len(R.contours(noise)["hist"]) >= 16


@pytest.mark.parametrize("w,h", [(1, 1), (1, 8), (8, 1), (2, 2)])
def test_degenerate_sizes(exe, tmp_path, w, h):
    for tag, img in (("in", np.full((h, w), -1.0, np.float32)), ("out", np.full((h, w), 1.0, np.float32)), ("mix", np.where(np.arange(w * h).reshape(h, w) % 2 == 0, -1.0, 2.0).astype(np.float32))):
        m = R.contours(img)
        got = host(exe, img, tmp_path, tag)
        same(got, m)
        if tag != "mix":
            assert len(got["vertices"]) == 0 and len(got["segments"]) == 0 and got["loops"] == []
        if w < 2 or h < 2:
            assert len(got["segments"]) == 0 and (got["next"] == NONE).all()         # no cells: vertices nothing joins


def test_all_inside_and_all_outside(exe, tmp_path):
    for tag, v in (("in", -0.5), ("out", 0.5), ("nan", np.nan)):
        img = np.full((12, 20), v, np.float32)
        got = host(exe, img, tmp_path, tag)
        same(got, R.contours(img))
        assert len(got["vertices"]) == 0 and len(got["segments"]) == 0 and got["loops"] == []


# next: loop 5 -> 2 -> 7 -> 5, loop 1 -> 4 -> 1, chain 6 -> 0 -> 3, lone vertex 8
HAND_NEXT = np.array([3, 4, 7, NONE, 1, 2, 0, 5, NONE], np.uint32)
HAND_LOOPS = [([6, 0, 3], False), ([8], False), ([1, 4], True), ([2, 7, 5], True)]


def test_the_loop_follower_orders_as_defined(exe, tmp_path):
    assert R.loops(HAND_NEXT) == HAND_LOOPS
    got = [([int(v) for v in ids], closed) for ids, closed in F.contour_loops(HAND_NEXT)]           # fhip_contour_loops: no GPU call
    assert got == HAND_LOOPS
    fin, fout = str(tmp_path / "n.in"), str(tmp_path / "n.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<Q", len(HAND_NEXT)) + HAND_NEXT.tobytes())
    subprocess.run([exe, "--loops", fin, fout], check=True)
    raw = open(fout, "rb").read()
    ok, nl = struct.unpack_from("<QQ", raw, 0)
    assert ok == 1 and nl == 4
    order = np.frombuffer(raw, "<u4", 9, 16)
    start = np.frombuffer(raw, "<u8", nl + 1, 16 + 36)
    closed = np.frombuffer(raw, "u1", nl, 16 + 36 + 8 * (nl + 1))
    assert [([int(v) for v in order[int(start[k]):int(start[k + 1])]], bool(closed[k])) for k in range(nl)] == HAND_LOOPS
    assert F.contour_loops(np.zeros(0, np.uint32)) == []
    for bad in ([1, 1, NONE], [5, NONE]):          # two segments arriving at one vertex; an id past the end
        with pytest.raises(ValueError):
            F.contour_loops(np.array(bad, np.uint32))


def test_the_library_exports_the_entry_points():
    lib = C.CDLL(F.LIB_PATH)
    for name in ("fhip_contour2d", "fhip_contours_counts", "fhip_contours_vertices", "fhip_contours_segments", "fhip_contours_next",
                 "fhip_contours_vertices_dev", "fhip_contours_segments_dev", "fhip_contours_free", "fhip_contour_loops"):
        assert hasattr(lib, name) and name in F.EXPORTS and getattr(F.lib(), name).argtypes is not None, name
    assert callable(F.contour) and callable(F.slice_stack) and callable(F.Contours.svg) and callable(F.Contours.world)


def hand_made(width, height, vertices, nxt):
    """a Contours with its host arrays put there by hand (no device behind it)"""
    nxt = np.array(nxt, np.uint32)
    c = F.Contours(None, width, height, 0.0, len(vertices), int((nxt != NONE).sum()))
    segs = np.array([(k, t) for k, t in enumerate(nxt) if t != NONE], np.uint32).reshape(-1, 2)
    c._host = {"vertices": np.array(vertices, np.float32).reshape(-1, 2), "segments": segs, "next": nxt}
    return c


def svg_numbers(text):
    """(viewBox [x, y, w, h], [(closed, [(x, y), ...]) per subpath]) of Contours.svg's text"""
    import re
    box = [float(v) for v in re.search(r'viewBox="([^"]*)"', text).group(1).split()]
    d = re.search(r'<path fill-rule="evenodd" d="([^"]*)"', text).group(1)
    subs = []
    for part in d.split("M ")[1:]:
        closed = part.rstrip().endswith("Z")
        pts = [tuple(float(v) for v in p.split()) for p in part.replace("Z", "").strip().split(" L ")]
        subs.append((closed, pts))
    return box, subs


def test_svg_and_world_of_a_result_on_the_host(tmp_path):
    c = hand_made(4, 4, [[1, 1], [2, 1], [1.5, 2]], [1, 2, 0])
    assert [([int(v) for v in ids], closed) for ids, closed in c.loops()] == [([0, 1, 2], True)]
    assert c.areas() == [0.5]
    m = F.screen_to_world((4, 4))
    w = c.world()
    assert w.dtype == np.float32 and w.shape == (3, 2)
    for k in range(3):
        p = F.mat_mul(m, np.array([[c.vertices[k, 0], 0, 0], [c.vertices[k, 1], 0, 0], [1, 0, 0]], np.float32))[:2, 0]
        assert np.allclose(w[k], p, rtol=0, atol=1e-6)
    text = c.svg()
    assert text.count("<path") == 1 and 'fill-rule="evenodd"' in text and text.count("M ") == 1 and text.count(" L ") == 2 and text.count(" Z") == 1


def test_the_svg_is_the_image_as_displayed_not_its_mirror(tmp_path):
    """An asymmetric outline on a 40 x 24 image - an L whose foot points right, in rows 3 .. 15, plus an open chain in the last columns:
    SVG's y grows downward, so a vertex of a lower row index must get the smaller SVG y and one of a lower column the smaller x; the
    numbers are the world coordinates with y negated; the viewBox holds the whole pixel lattice of a W != H image."""
    W, H = 40, 24
    ell = [[5, 3], [5, 15], [20, 15], [20, 12], [8, 12], [8, 3]]          # pixel units; rows 3 (top of the stem) to 15 (the foot)
    verts = ell + [[38.5, 2], [39, 6.25]]
    c = hand_made(W, H, verts, [1, 2, 3, 4, 5, 0, 7, NONE])
    path = tmp_path / "ell.svg"
    text = c.svg(str(path))
    assert path.read_text() == text
    box, subs = svg_numbers(text)
    assert [(closed, len(pts)) for closed, pts in subs] == [(False, 2), (True, 6)]          # open chains first
    pts = {k: p for (_, ps), ids in zip(subs, ([6, 7], [0, 1, 2, 3, 4, 5])) for k, p in zip(ids, ps)}
    for a in range(len(verts)):
        for b in range(len(verts)):
            if verts[a][1] < verts[b][1]:
                assert pts[a][1] < pts[b][1], (a, b)          # the lower row index: nearer the top of the drawing
            if verts[a][0] < verts[b][0]:
                assert pts[a][0] < pts[b][0], (a, b)
    w = c.world()
    for k, (x, y) in pts.items():
        assert np.isclose(x, float(w[k, 0]), rtol=1e-7, atol=0) and np.isclose(y, -float(w[k, 1]), rtol=1e-7, atol=0)
    # the foot of the L points right and lies BELOW the stem's top in the drawing, as in the image
    assert pts[2][0] > pts[0][0] and pts[2][1] > pts[0][1]
    # every pixel centre of the image lies inside the viewBox, half a pixel clear of its sides, and the box is no larger than that
    m = F.screen_to_world((W, H)).astype(np.float64)
    xs = [m[0, 0] * i + m[0, 2] for i in (0, W - 1)]
    ys = [-(m[1, 1] * j + m[1, 2]) for j in (0, H - 1)]
    pitch = 2.0 / min(W, H)
    assert np.isclose(box[0], min(xs) - pitch / 2) and np.isclose(box[0] + box[2], max(xs) + pitch / 2)
    assert np.isclose(box[1], min(ys) - pitch / 2) and np.isclose(box[1] + box[3], max(ys) + pitch / 2)
    assert box[2] > 2.0 and abs(box[3] - 2.0) < 1e-6          # 40 x 24: wider than [-1, 1], the shorter side exactly 2
    assert all(box[0] < x < box[0] + box[2] and box[1] < y < box[1] + box[3] for x, y in pts.values())


def test_the_sanitized_build_runs_clean(images, tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined, once, on an image with every kind of cell and on the loop input"""
    exe = build("contour_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    rng = np.random.default_rng(11)
    img = rng.standard_normal((7, 300)).astype(np.float32)
    img[3, 5] = np.nan
    same(host(exe, img, tmp_path, "san"), R.contours(img))
    fin, fout = str(tmp_path / "sn.in"), str(tmp_path / "sn.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<Q", len(HAND_NEXT)) + HAND_NEXT.tobytes())
    subprocess.run([exe, "--loops", fin, fout], check=True)
