"""The solids that test_thickness.py and test_thickness_gpu.py measure: name -> (bool [N, N, N] indexed [i, j, k], complement).  The local
thickness is taken of the set voxels, or with `complement` of the clear ones (the pores).  Each is the smallest shape at which a piece
of the library can go wrong; the depth is in the name."""
import functools

import numpy as np

import distance_ref as DR
import thickness_ref as TR
from test_components import hollow_box


def random_grid(depth, density, seed):
    N = 4 << depth
    return np.random.default_rng(seed).random((N, N, N)) < density


def cleared(depth, at):
    g = np.ones((4 << depth,) * 3, bool)
    g[at] = False
    return g


def balls(N, *spheres):
    """the union of the open balls (centre, squared radius)"""
    i, j, k = np.indices((N, N, N), sparse=True)
    g = np.zeros((N, N, N), bool)
    for (a, b, c), f in spheres:
        g |= (i - a) ** 2 + (j - b) ** 2 + (k - c) ** 2 < f
    return g


def box(N, lo, hi):
    g = np.zeros((N, N, N), bool)
    g[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    return g


def plates(axis, spanning, N=16):
    """two plates across `axis`, 6 voxels (1 .. 6) and 7 voxels (8 .. 14) thick: 2 .. 13 in the other two axes, or all of them"""
    g = np.zeros((N, N, N), bool)
    other = slice(None) if spanning else slice(2, 14)
    for a, b in ((1, 7), (8, 15)):
        g[tuple(slice(a, b) if ax == axis else other for ax in range(3))] = True
    return g


def fin_on_block():
    """a block of 8 x 12 x 12 with a fin two voxels thick standing on its +x face"""
    return box(16, (2, 2, 2), (10, 14, 14)) | box(16, (10, 7, 2), (15, 9, 14))


def tilted_slab():
    i, j, k = np.indices((32, 32, 32), sparse=True)
    g = np.abs(0.5 * i + 0.7 * j + 0.5 * k - 27) < 5
    return g & box(32, (3, 3, 3), (29, 29, 29))


def slab(axis, a, b, N=128):
    g = np.zeros((N, N, N), bool)
    g[tuple(slice(a, b) if ax == axis else slice(None) for ax in range(3))] = True
    return g


SLABS = {"d5-slab66-z": (2, 31, 97), "d5-slab66-x": (0, 40, 106)}          # axis, from, to: answered by thickness_ref.slab
GRIDS = {
    # depth 0: one word of 64 voxels, every ball clipped
    "d0-empty": (lambda: np.zeros((4, 4, 4), bool), False),
    "d0-clear000": (lambda: cleared(0, (0, 0, 0)), False),
    "d0-random0.5": (lambda: random_grid(0, 0.5, 21), False),
    # depth 1: balls across every brick face
    "d1-ball10": (lambda: balls(8, ((3, 4, 4), 10)), False),
    "d1-clear703": (lambda: cleared(1, (7, 0, 3)), False),
    "d1-random0.9": (lambda: random_grid(1, 0.9, 22), False),
    # depth 2: even and odd walls along every axis, a larger ball beside a smaller, a fin on a block
    **{f"d2-plates-{'ijk'[ax]}": (functools.partial(plates, ax, False), False) for ax in range(3)},
    **{f"d2-plates-{'ijk'[ax]}-spanning": (functools.partial(plates, ax, True), False) for ax in range(3)},
    "d2-two-balls": (lambda: balls(16, ((6, 7, 7), 30), ((11, 8, 8), 9)), False),
    "d2-fin-on-block": (fin_on_block, False),
    "d2-hollow-box": (hollow_box, False),
    "d2-random0.95": (lambda: random_grid(2, 0.95, 23), False),
    # depth 3
    "d3-two-balls-fin": (lambda: balls(32, ((10, 12, 12), 80), ((21, 18, 14), 30)) | box(32, (4, 15, 22), (28, 17, 30)), False),
    "d3-tilted-slab": (tilted_slab, False),
    "d3-random0.97": (lambda: random_grid(3, 0.97, 24), False),
    # depth 4: rows of every lane-group width, many small balls, the pores of a sparse bitmap
    "d4-part": (lambda: balls(64, ((22, 24, 24), 150), ((44, 40, 30), 40)) | box(64, (10, 30, 40), (54, 32, 60)) | box(64, (8, 8, 50), (40, 40, 53)), False),
    "d4-random0.97": (lambda: random_grid(4, 0.97, 25), False),
    "d4-pores0.03": (lambda: random_grid(4, 0.03, 26), True),
    # depth 5: rows of 65 voxels, every ball clipped by the grid, nothing pruned but off the two medial planes
    **{name: (functools.partial(slab, *spec), False) for name, spec in SLABS.items()},
}


@functools.lru_cache(maxsize=None)
def grid(name):
    g = GRIDS[name][0]()
    g.setflags(write=False)
    return g


def depth_of(name):
    return int(name[1])


@functools.lru_cache(maxsize=None)
def field_of(name):
    """the squared distance of every voxel to the nearest voxel outside the measured set, [i, j, k] (distance_ref.py)"""
    g, complement = grid(name), GRIDS[name][1]
    d2 = DR.edt(g if complement else ~g)
    d2.setflags(write=False)
    return d2


@functools.lru_cache(maxsize=None)
def reference(name):
    """T [i, j, k], computed once: every centre's ball (thickness_ref.by_centres), or the closed form for the slabs of depth 5"""
    if name in SLABS:
        axis, a, b = SLABS[name]
        N = len(grid(name))
        T = np.ascontiguousarray(np.broadcast_to(TR.slab(N, a, b).reshape([N if ax == axis else 1 for ax in range(3)]), (N, N, N)))
    else:
        T = TR.by_centres(field_of(name))
    T.setflags(write=False)
    return T
