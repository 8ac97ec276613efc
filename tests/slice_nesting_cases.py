"""The hand-made meshes of the slice nesting's tests, shared by the host-build test and the device test.  Side walls alone make closed
loops under planes strictly inside a prism's z-range, so most cases are open prisms of a few quads: `prism(polygon, z0, z1)` is the
walls of a polygon given counter-clockwise - an outer boundary, area2 > 0 - or with `flip` a hole.  The hand-made cases keep every
coordinate dyadic with few bits and every prism's z-span a power of two with planes on a coarse dyadic grid, so that the crossings'
positions are dyadic with few bits too and the binary64 predicate is exact on them (slice_nesting_ref.check_exact).

The first triangle of a prism is (a0, b0, b1) for its polygon's first edge a -> b, and crossings are numbered by the edges' first
corners: the first prism of a soup therefore has crossing 0 - the leader of its loop on the lowest plane that cuts it - at its
polygon's SECOND vertex.  `leader_at` says so, and the tests that place things on a leader's row assert it."""
import functools

import numpy as np


def prism(polygon, z0, z1, flip=False):
    """-> float32 [2 m, 3, 3]: two triangles per edge of the polygon, normals outward for a counter-clockwise polygon"""
    pts = [(float(x), float(y)) for x, y in polygon]
    if flip:
        pts = [pts[0]] + pts[:0:-1]
    tris = []
    for k, a in enumerate(pts):
        b = pts[(k + 1) % len(pts)]
        a0, b0, b1, a1 = (*a, z0), (*b, z0), (*b, z1), (*a, z1)
        tris += [(a0, b0, b1), (a0, b1, a1)]
    return np.array(tris, np.float32)


def rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def square(cx, cy, h):
    return rect(cx - h, cy - h, cx + h, cy + h)


def diamond(cx, cy, r):
    return [(cx + r, cy), (cx, cy + r), (cx - r, cy), (cx, cy - r)]


def soup(*prisms):
    return np.ascontiguousarray(np.concatenate(prisms), np.float32)


def planes(*zs):
    return np.array(zs, np.float32)


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------------
CHAIN_HALF = (0.75, 0.5, 0.375, 0.25)
CHAIN_Z = (1.0, 0.5, 0.25, 0.125)          # prism k spans [-z, z]: spans 2, 1, 1/2, 1/4
CHAIN_PLANES = planes(-0.75, -0.375, -0.1875, 0.0, 0.1875, 0.375, 0.75)
CHAIN_MAX_DEPTH = [0, 1, 2, 3, 2, 1, 0]


def chain(reversed_prism=None):
    """four concentric square prisms, alternately flipped; `reversed_prism`: that one with the other winding"""
    return soup(*[prism(square(0.0, 0.0, h), -z, z, flip=(k % 2 == 1) != (k == reversed_prism)) for k, (h, z) in enumerate(zip(CHAIN_HALF, CHAIN_Z))]), CHAIN_PLANES


# ---- siblings ------------------------------------------------------------------------------------------------------------------------------------
def siblings():
    """an outer boundary, a hole, and two islands side by side in the hole: the right one, first in the soup, is lower than the left
    one, so its leader is level with the left one, hits it twice and is not inside it"""
    right = prism(rect(0.25, -0.125, 0.5, 0.125), -0.5, 0.5)
    left = prism(rect(-0.5, -0.25, -0.25, 0.25), -0.5, 0.5)
    return soup(right, left, prism(square(0.0, 0.0, 0.875), -0.5, 0.5), prism(square(0.0, 0.0, 0.75), -0.5, 0.5, flip=True)), planes(0.0)


# ---- the comb ------------------------------------------------------------------------------------------------------------------------------------
COMB_TEETH, LONG_COMB_TEETH = 40, 288
COMB_X0 = -0.8125          # tooth k spans x in [x0 + k pitch, x0 + k pitch + pitch / 2]


def comb(teeth=COMB_TEETH, pitch=1.0 / 32):
    """A C-shaped loop whose mouth opens to the right; in the mouth a comb of teeth that point up, and small squares: in the gaps after
    teeth 0 and 1 (the comb is hit 2 and 4 times), right of the comb (twice the teeth), and inside teeth 0 and 1 (1 and 3 times).  The C
    is hit twice by each of them.  40 teeth: the issue's comb.  288 teeth of pitch 1 / 256: 578 hits, a list too long for the wave's LDS"""
    c_shape = [(-0.9375, -0.5), (0.9375, -0.5), (0.9375, -0.25), (-0.875, -0.25), (-0.875, 0.25), (0.9375, 0.25), (0.9375, 0.5), (-0.9375, 0.5)]
    spine_lo, spine_hi, tip = -0.1875, -0.125, 0.125
    x1 = COMB_X0 + (teeth - 1) * pitch + pitch / 2
    pts = [(COMB_X0, spine_lo), (x1, spine_lo)]          # the spine's underside, then the teeth from the right
    for k in reversed(range(teeth)):
        x = COMB_X0 + k * pitch
        pts += [(x + pitch / 2, spine_hi)] if k < teeth - 1 else []
        pts += [(x + pitch / 2, tip), (x, tip)]
        pts += [(x, spine_hi)] if k > 0 else []
    h = pitch / 16
    probes = [square(COMB_X0 + k * pitch + 0.75 * pitch, 0.0, h) for k in (0, 1)]          # in the gaps
    probes += [square(0.625, 0.0, 1.0 / 64)]          # right of the comb, in the mouth
    probes += [square(COMB_X0 + k * pitch + 0.25 * pitch, 0.0, h) for k in (0, 1)]          # inside the teeth
    return soup(*[prism(p, -0.5, 0.5) for p in probes], prism(c_shape, -0.5, 0.5), prism(pts, -0.5, 0.5)), planes(0.0)


def long_comb():
    return comb(LONG_COMB_TEETH, 1.0 / 256)


def comb_multiplicities(teeth):
    """of the comb, per probe in the soup's order"""
    return [2, 4, 2 * teeth, 1, 3]


# ---- a vertex on the row -------------------------------------------------------------------------------------------------------------------------
ROW_Q = (0.0, 0.0)
# (cx, cy, r, the hits of the leader at ROW_Q): side vertices exactly on the row - left of it the ray passes through both, right of it,
# around it; the top vertex on the row, left - the ray touches - and right; the bottom vertex on the row, left - both segments at the
# vertex straddle - and right
ROW_DIAMONDS = ((-0.5, 0.0, 0.125, 2), (0.5, 0.0, 0.125, 0), (0.0625, 0.0, 0.125, 1), (-0.8125, -0.0625, 0.0625, 0), (0.8125, -0.0625, 0.0625, 0),
                (-0.25, 0.0625, 0.0625, 2), (0.25, 0.0625, 0.0625, 0))


def vertex_on_the_row():
    """the leader is the second vertex, ROW_Q, of the first prism's square; then the diamonds of ROW_DIAMONDS in their order"""
    w = 1.0 / 64
    first = prism(rect(ROW_Q[0] - w, ROW_Q[1], ROW_Q[0], ROW_Q[1] + w), -0.5, 0.5)
    return soup(first, *[prism(diamond(cx, cy, r), -0.5, 0.5) for cx, cy, r, _ in ROW_DIAMONDS]), planes(0.0)


# ---- horizontal and zero-length segments on the leader's row -----------------------------------------------------------------------------------------
def flat_on_the_row():
    """Every prism ends at z = 0, and the second plane is z = 0: it passes through the prisms' top vertices, so the crossings of a wall's
    vertical edge and of its diagonal share a position - zero-length segments.  Squares left of the leader (the first prism's second
    vertex, (0, 0)) with their top edge on its row, their bottom edge on its row, and one around it: horizontal segments on the row."""
    w = 1.0 / 32
    first = prism(rect(-w, 0.0, 0.0, w), -0.5, 0.0)
    others = [rect(-0.5, -0.25, -0.25, 0.0), rect(-0.875, 0.0, -0.625, 0.25), rect(-0.9375, -0.5, 0.5, 0.5), rect(0.125, -0.125, 0.25, 0.0)]
    return soup(first, *[prism(p, -0.5, 0.0) for p in others]), planes(-0.25, 0.0)


# ---- irregular loops -----------------------------------------------------------------------------------------------------------------------------
def shared_edge():
    """two cubes' walls that share a vertical edge - one irregular loop per plane - inside a hole of an outer boundary, beside an island
    with a hole of its own"""
    return soup(prism(square(0.0, 0.0, 0.875), -0.5, 0.5), prism(square(0.0, 0.0, 0.75), -0.5, 0.5, flip=True),
                prism(rect(-0.5, -0.25, -0.25, 0.0), -0.5, 0.5), prism(rect(-0.25, 0.0, 0.0, 0.25), -0.5, 0.5),
                prism(square(0.375, 0.0, 0.25), -0.5, 0.5), prism(square(0.375, 0.0, 0.125), -0.5, 0.5, flip=True),
                prism(square(-0.375, -0.125, 0.03125), -0.5, 0.5)), planes(-0.25, 0.25)          # (the last: inside the first cube)


# ---- crossing loops ------------------------------------------------------------------------------------------------------------------------------
def crossing():
    """two overlapping squares, neither's leader inside the other, and a small one in the overlap: it is inside both, both have depth 0,
    its parent is the one with the smaller id and it is improper"""
    return soup(prism(rect(-0.75, -0.5, 0.25, 0.5), -0.5, 0.5), prism(rect(-0.25, -0.25, 0.75, 0.75), -0.5, 0.5), prism(square(0.0, 0.0, 0.0625), -0.5, 0.5)), planes(0.0)


# ---- the field for the bands ---------------------------------------------------------------------------------------------------------------------
FIELD_PLANES = planes(-0.5, -0.25, 0.0, 0.25, 0.5, 0.875)
BANDS = (1, 2, 7, 64, 4096, 0)


@functools.lru_cache(maxsize=None)
def field():
    """[-1, 1]^2 subdivided recursively into boxes, which never overlap; in each leaf a prism - an axis-aligned rectangle, or a rotated
    one inside the leaf's inscribed circle - with up to three smaller ones nested in it, alternately flipped, each with a z-range of its
    own: about 200 loops on each of the five planes below 0.75, none of which cross.  A frame around all gives every plane the y-extent
    [-1, 1] exactly, and the leaves' corners are dyadic: segment ends lie exactly on the borders of 2, 64 and 4096 bands.  4096 bands are
    more than a plane's segments.  The sixth plane cuts two flat prisms alone, all of whose crossings have y = 0.5: a zero extent."""
    rng = np.random.default_rng(7)
    leaves = []

    def split(x0, y0, x1, y1, level):
        if level == 0 or (level < 3 and rng.random() < 0.3):
            leaves.append((x0, y0, x1, y1))
            return
        if (x1 - x0 >= y1 - y0):
            split(x0, y0, (x0 + x1) / 2, y1, level - 1), split((x0 + x1) / 2, y0, x1, y1, level - 1)
        else:
            split(x0, y0, x1, (y0 + y1) / 2, level - 1), split(x0, (y0 + y1) / 2, x1, y1, level - 1)
    split(-0.9375, -0.9375, 0.9375, 0.9375, 7)
    prisms = [prism(square(0.0, 0.0, 1.0), -0.75, 0.75), prism(square(0.0, 0.0, 0.96875), -0.75, 0.75, flip=True)]
    for x0, y0, x1, y1 in leaves:
        cx, cy, w, h = (x0 + x1) / 2, (y0 + y1) / 2, (x1 - x0) / 2, (y1 - y0) / 2
        rotated = rng.random() < 0.5
        angle = rng.random() * np.pi
        for k in range(int(rng.integers(1, 5))):
            s = 0.9375 - 0.25 * k          # the k-th nested one: the same shape, smaller; the first stays clear of the leaf's border
            z0, z1 = -0.75 + 0.3 * rng.random(), 0.75 - 0.3 * rng.random()
            if rotated:
                r = 0.85 * min(w, h) * s          # (half-sides r and r / 2: within r sqrt(5) / 2 of the centre)
                c, sn = np.cos(angle), np.sin(angle)
                poly = [(cx + r * (c * a - sn * b * 0.5), cy + r * (sn * a + c * b * 0.5)) for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
            else:
                poly = rect(cx - w * s, cy - h * s, cx + w * s, cy + h * s)
            prisms.append(prism(poly, z0, z1, flip=k % 2 == 1))
    flat = [prism([(-0.5, 0.5), (-0.25, 0.5)], 0.8125, 0.9375), prism([(0.25, 0.5), (0.5, 0.5)], 0.8125, 0.9375)]
    return soup(*prisms, *flat), FIELD_PLANES


def leader_at(slices, xy):
    """is crossing 0 the leader of a loop, and does it lie at xy?  `slices`: the reference's dict, or a MeshSlices' arrays as one"""
    return int(slices["loops"]["leader"][0]) == 0 and tuple(float(v) for v in np.asarray(slices["xy"]).reshape(-1, 2)[0]) == tuple(float(v) for v in xy)
