"""The shapes of the contour tests, each a function of the module that builds it (oracle or fidget_amd: the same Context API), and what
turns a 2D slice of one into the image the definition starts from: the oracle's pixel-perfect render2d."""
import numpy as np

import oracle as O
from conftest import model_path
from test_occupancy import BEAR_W2M

BEAR_W2M_2D = np.ascontiguousarray(BEAR_W2M[np.ix_((0, 1, 3), (0, 1, 3))])        # the same move of the region, as render2d's 3 x 3


def _r(c, cx=0.0, cy=0.0):
    return c.sqrt(c.add(c.square(c.sub(c.x(), cx)), c.square(c.sub(c.y(), cy))))


def disc(M, r=0.6, cx=0.0, cy=0.0):
    c = M.Context()
    return M.Shape(c, c.sub(_r(c, cx, cy), r))


def annulus(M):
    c = M.Context()
    r = _r(c)
    return M.Shape(c, c.max(c.sub(r, 0.7), c.sub(0.3, r)))


def two_discs(M):
    c = M.Context()
    return M.Shape(c, c.min(c.sub(_r(c, -0.45, 0.0), 0.3), c.sub(_r(c, 0.45, 0.125), 0.3)))


def saddle(sign, k):
    """x y - k (sign > 0) or k - x y: the four pixels around the origin of an odd-sized square image - pixel i sits at
    (i - W / 2) * 2 / W - alternate in sign for |k| below a quarter of the pixel pitch squared, and the mean of the four is -k (or k)"""
    def make(M):
        c = M.Context()
        xy = c.mul(c.x(), c.y())
        return M.Shape(c, c.sub(xy, k) if sign > 0 else c.sub(k, xy))
    return make


def sqrt_x(M):
    """sqrt(x) - 0.5: NaN for x < 0, so outside; inside for 0 <= x < 0.25"""
    c = M.Context()
    return M.Shape(c, c.sub(c.sqrt(c.x()), 0.5))


def inv_square(M):
    """4 - 1 / (4 x)^2: -inf where x = 0 - column W / 2 of an even width - and outside from |4 x| = 0.5 on, which the columns next to
    that one are while the pixel pitch 2 / min(W, H) is at least 1 / 8"""
    c = M.Context()
    x4 = c.mul(c.x(), 4.0)
    return M.Shape(c, c.sub(4.0, c.div(1.0, c.mul(x4, x4))))


def var_disc(M):
    c = M.Context()
    return M.Shape(c, c.sub(_r(c), c.var(7)))


def bear(M):
    return M.Shape.from_vm(model_path("bear.vm"))


def image(make, w, h, z=0.0, w2m=None, vars_=None):
    return O.render2d(make(O), w, h, z=z, pixel_perfect=True, world_to_model=w2m, vars=vars_)[0]
