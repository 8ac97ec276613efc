"""fhip_voxels_distance on the device against distance_ref.py: bitmaps made in numpy (voxels_ref.pack) and handed to the library as host
bricks and as a torch CUDA tensor, for the set bits and for their complement; the whole field, the summary and the thresholds at
t = 0, 1, 2, 3, max, max + 1 are compared with np.array_equal - every value is an integer.  Then a shape end to end with the offsets,
sub-ranges of layers, a caller's buffer for `within`, two runs, and the refused calls."""
import functools

import numpy as np
import pytest

import fidget_amd as F
import oracle as O
import distance_ref as DR
import occupancy_ref as R
import voxels_ref as V
from test_components import hollow_box
from test_mesh import sphere

pytestmark = pytest.mark.gpu

FIVE = [(3, 100, 64), (127, 0, 5), (64, 64, 64), (0, 127, 127), (90, 17, 33)]          # depth 5: five fixed voxels


@functools.lru_cache(maxsize=None)
def _torch():
    import torch
    return torch


def random_grid(depth, density, seed):
    N = 4 << depth
    return np.random.default_rng(seed).random((N, N, N)) < density


def points(depth, pts, fill=False):
    N = 4 << depth
    g = np.full((N, N, N), fill, bool)
    for p in pts:
        g[p] = not fill
    return g


def plane(axis, at, N=16):
    g = np.zeros((N, N, N), bool)
    g[tuple(at if a == axis else slice(None) for a in range(3))] = True
    return g


def line_along(axis, at, N=16):
    g = np.zeros((N, N, N), bool)
    g[tuple(slice(None) if a == axis else at[a] for a in range(3))] = True
    return g


# name -> (grid, complements to run: the depth-5 grids are made for one foreground each)
GRIDS = {
    # depth 0: one brick
    "d0-empty": lambda: np.zeros((4, 4, 4), bool),
    "d0-full": lambda: np.ones((4, 4, 4), bool),
    "d0-voxel000": lambda: points(0, [(0, 0, 0)]),
    "d0-voxel333": lambda: points(0, [(3, 3, 3)]),
    "d0-random0.5": lambda: random_grid(0, 0.5, 1),
    # depth 1: every brick boundary
    "d1-voxel000": lambda: points(1, [(0, 0, 0)]),
    "d1-voxel777": lambda: points(1, [(7, 7, 7)]),
    "d1-across-x": lambda: points(1, [(3, 2, 5), (4, 2, 5)]),
    "d1-across-z": lambda: points(1, [(6, 1, 3), (6, 1, 4)]),
    "d1-random0.05": lambda: random_grid(1, 0.05, 2),
    # depth 2: whole rows, columns and planes without foreground
    "d2-random0.01": lambda: random_grid(2, 0.01, 3),
    "d2-plane-i": lambda: plane(0, 5),
    "d2-plane-j": lambda: plane(1, 11),
    "d2-plane-k": lambda: plane(2, 0),
    "d2-line-i": lambda: line_along(0, (0, 3, 12)),
    "d2-line-j": lambda: line_along(1, (15, 0, 6)),
    "d2-line-k": lambda: line_along(2, (7, 8, 0)),
    "d2-hollow-box": hollow_box,
    # depth 4: columns as long as a wave, a layer over several blocks
    "d4-random0.001": lambda: random_grid(4, 0.001, 4),
    "d4-random0.2": lambda: random_grid(4, 0.2, 5),
    "d4-random0.9": lambda: random_grid(4, 0.9, 6),
    "d4-full": lambda: np.ones((64, 64, 64), bool),
    # depth 5: columns longer than a wave - the stacks in the workspace; the direct-definition reference
    "d5-five": lambda: points(5, FIVE),
    "d5-five-cleared": lambda: points(5, FIVE, fill=True),
}
ONE_FOREGROUND = {"d5-five": False, "d5-five-cleared": True}
CASES = [(name, c) for name in GRIDS for c in (False, True) if ONE_FOREGROUND.get(name, c) == c]


@functools.lru_cache(maxsize=None)
def grid(name):
    g = GRIDS[name]()
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def reference(name, complement):
    fg = grid(name) != complement
    d2 = DR.direct(fg) if name.startswith("d5-") else DR.edt(fg)
    d2.setflags(write=False)
    return d2


@functools.lru_cache(maxsize=None)
def bricks_of(name):
    b = V.pack(grid(name))
    b.setflags(write=False)
    return b


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


def to_host(hip, a):
    if isinstance(a, np.ndarray):
        return a
    hip.sync()
    return a.cpu().numpy()


def bricks_host(vox):
    return to_host(vox._hip, vox.bricks).view(np.uint64)


def compare(vox, d2, complement):
    """the field, the summary and the six thresholds of `vox.distance(complement)` against the reference field d2 [i, j, k]"""
    N = vox.grid
    dist = vox.distance(complement)
    got = to_host(vox._hip, dist.slices(0, N))
    want = DR.field(d2)
    print(f"field: values that differ {int((got.view(np.uint32) != want).sum())} of {want.size}")
    assert got.shape == (N, N, N) and got.dtype == (np.uint32 if not vox.on_device else np.int32)
    assert np.array_equal(got.view(np.uint32), want)
    m, arg, n = DR.summary(d2)
    print(f"summary: reference {(m, arg, n)}, device {(dist.max_squared, dist.argmax, dist.n)}")
    assert (dist.max_squared, dist.argmax, dist.n) == (m, arg, n)
    assert (dist.depth, dist.grid, dist.complement) == (vox.depth, N, complement)
    for t in (0, 1, 2, 3, m, m + 1):
        w, b = dist.within(squared=t), dist.beyond(squared=t)
        assert w.on_device == vox.on_device and w.depth == vox.depth and w.cells is None
        assert np.array_equal(bricks_host(w), V.pack(DR.within(d2, t))), ("within", t)
        assert np.array_equal(bricks_host(b), V.pack(DR.beyond(d2, t))), ("beyond", t)
    return dist


@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("name,complement", CASES)
def test_grids(name, complement, where):
    d2 = reference(name, complement)
    dist = compare(voxels(bricks_of(name), where), d2, complement)
    fg = grid(name) != complement
    if not fg.any():
        assert (dist.max_squared, dist.argmax, dist.n) == (0, None, 0)
        assert (to_host(dist._hip, dist.slices(0, 4)).view(np.int32) == -1).all()
    if fg.all():
        assert (dist.max_squared, dist.argmax, dist.n) == (0, (0, 0, 0), fg.size)
    if name == "d0-voxel333" and not complement:
        assert dist.max_squared == 27 and dist.argmax == (0, 0, 0)
    if name == "d5-five":
        assert dist.n == 5 and dist.max_squared > 64 ** 2


def test_the_field_in_place():
    """the whole field through __cuda_array_interface__, without a copy-out"""
    torch = _torch()
    name = "d2-random0.01"
    vox = voxels(bricks_of(name), "torch")
    dist = vox.distance()
    arr = dist.squared_device
    assert arr.shape == (16, 16, 16) and arr.__cuda_array_interface__["typestr"] == "<u4"
    whole = dist.slices(0, 16)
    assert arr.ptr != whole.data_ptr()
    vox._hip.sync()
    as_i4 = dict(arr.__cuda_array_interface__, typestr="<i4")       # (the values as int32: every torch takes that)
    t = torch.as_tensor(type("A", (), {"__cuda_array_interface__": as_i4, "_keep": arr})(), device="cuda")
    assert t.data_ptr() == arr.ptr and torch.equal(t, whole)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), DR.field(reference(name, False)))


def test_a_shape_end_to_end():
    """a sphere voxelized into a torch tensor: its field, and the offsets made of it"""
    torch = _torch()
    depth = 4
    c = F.Context()
    vox = F.voxelize(F.Shape(c, sphere(c, (0.0, 0.0, 0.0), 0.6)), depth, out=torch.zeros(8 * 8 ** depth, dtype=torch.uint8, device="cuda"))
    oc = O.Context()
    inside = R.brute_force(O.Shape(oc, sphere(oc, (0.0, 0.0, 0.0), 0.6)), depth)
    assert vox.on_device and np.array_equal(bricks_host(vox), V.pack(inside))
    out_d2, in_d2 = DR.edt(inside), DR.edt(~inside)          # to the solid; to its complement
    compare(vox, out_d2, False)
    compare(vox, in_d2, True)

    def bits(v):
        return V.unpack(bricks_host(v))
    grown, shrunk = bits(vox.offset(2)), bits(vox.offset(-2))
    assert np.array_equal(grown, DR.within(out_d2, 4)) and np.array_equal(shrunk, DR.beyond(in_d2, 4))
    assert (grown >= inside).all() and grown.sum() > inside.sum() and (shrunk <= inside).all() and 0 < shrunk.sum() < inside.sum()
    assert np.array_equal(bits(vox.offset(0)), inside)
    closed, opened = bits(vox.closed(1)), bits(vox.opened(1))
    assert (closed >= inside).all() and (inside >= opened).all()
    # a speck beside the solid: opening drops it
    speck = inside.copy()
    speck[2, 3, 60] = True
    assert not inside[0:5, 1:6, 58:63].any()
    t = torch.from_numpy(V.pack(speck).view(np.int64)).cuda()
    torch.cuda.synchronize()
    cleaned = bits(F.Voxels(vox._hip, t, depth, None).opened(1.5))
    assert not cleaned[2, 3, 60] and cleaned.any() and (cleaned <= inside).all()
    # opening is the reference's: shrink by beyond(floor(1.5^2)), grow by within(2)
    core = DR.beyond(DR.edt(~speck), 2)
    assert np.array_equal(cleaned, DR.within(DR.edt(core), 2))


@pytest.mark.parametrize("where", ["host", "torch"])
def test_a_sub_range_of_layers(where):
    """layers 5 .. 10 of a grid of 16, neither end on a brick boundary; into a buffer of the caller's with room to spare"""
    name = "d2-random0.01"
    want = DR.field(reference(name, False))
    vox = voxels(bricks_of(name), where)
    dist = vox.distance()
    got = to_host(vox._hip, dist.slices(5, 11))
    assert got.shape == (6, 16, 16) and np.array_equal(got.view(np.uint32), want[5:11])
    assert dist.slices(7, 7).shape == (0, 16, 16)
    if where == "torch":
        torch = _torch()
        out = torch.full((6 * 256 + 8,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert dist.slices(5, 11, out=out) is out
        flat = to_host(vox._hip, out)
        assert np.array_equal(flat[:-8].reshape(6, 16, 16).view(np.uint32), want[5:11]) and (flat[-8:] == -7).all()


@pytest.mark.parametrize("where", ["host", "torch"])
def test_within_into_a_buffer_of_the_callers(where):
    """a buffer full of 0xA5 and longer than the bitmap: all of the bitmap is written and nothing beyond it"""
    name = "d2-random0.01"
    d2 = reference(name, False)
    vox = voxels(bricks_of(name), where)
    dist = vox.distance()
    want = V.pack(DR.within(d2, 5))
    words = 4 ** 3
    assert 0 < int(DR.within(d2, 5).sum()) < 16 ** 3 and (want == 0).any()          # words that must be written as zeros
    if where == "host":
        out = np.full(words + 8, 0xA5A5A5A5A5A5A5A5, np.uint64)
        part = dist.within(squared=5, out=out)
        assert np.shares_memory(part.bricks, out) and (out[words:] == 0xA5A5A5A5A5A5A5A5).all()
        got = part.bricks
    else:
        torch = _torch()
        out = torch.full((8 * words + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        part = dist.within(squared=5, out=out)
        assert part.on_device and part.bricks.data_ptr() == out.data_ptr()
        flat = to_host(vox._hip, out)
        assert (flat[8 * words:] == 0xA5).all()
        got = flat[:8 * words].view(np.uint64).reshape(4, 4, 4)
    assert got.shape == (4, 4, 4) and np.array_equal(got, want)
    assert np.array_equal(bricks_host(dist.within(r=2.4)), want)          # floor(2.4^2) = 5


def test_two_runs_give_the_same_field():
    vox = voxels(bricks_of("d4-random0.001"), "torch")
    a, b = vox.distance(), vox.distance()
    assert (a.max_squared, a.argmax, a.n) == (b.max_squared, b.argmax, b.n)
    fa, fb = a.slices(0, 64), b.slices(0, 64)
    vox._hip.sync()
    assert _torch().equal(fa, fb)


def test_refusals():
    """the statuses of the refused calls, and that the context works after them"""
    torch = _torch()
    name = "d1-random0.05"
    vox = voxels(bricks_of(name), "host")
    with pytest.raises(F.FidgetHipError) as e:
        F.Voxels(vox._hip, np.zeros(1, np.uint64), 9, None).distance()
    assert e.value.status == 6 and "depth" in str(e.value)          # FHIP_ERR_UNSUPPORTED
    dist = vox.distance()
    for k0, k1 in ((0, 9), (5, 4)):          # k1 > N; k0 > k1
        with pytest.raises(F.FidgetHipError) as e:
            dist.slices(k0, k1)
        assert e.value.status == 6 and "k0 <= k1" in str(e.value)
    with pytest.raises(F.FidgetHipError) as e:
        dist.within(squared=0xFFFFFFFF)
    assert e.value.status == 6 and "0xFFFFFFFE" in str(e.value)
    with pytest.raises(F.FidgetHipError) as e:
        dist.beyond(squared=1 << 32)
    assert e.value.status == 6
    for kw in ({}, {"r": 1.0, "squared": 1}):
        with pytest.raises(ValueError):
            dist.within(**kw)
        with pytest.raises(ValueError):
            dist.beyond(**kw)
    # a bitmap on the device that is not 8-byte aligned; layers on the device that are not 16-byte aligned
    raw = torch.zeros(8 * 8 + 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    odd = F.Voxels(vox._hip, raw[4:4 + 64], 1, None)
    assert odd.bricks.data_ptr() % 8 == 4
    with pytest.raises(F.FidgetHipError) as e:
        odd.distance()
    assert e.value.status == 6 and "aligned" in str(e.value)
    dev = voxels(bricks_of(name), "torch")
    ddist = dev.distance()
    room = torch.zeros(8 * 64 + 4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert room[1:].data_ptr() % 16 == 4
    with pytest.raises(F.FidgetHipError) as e:
        ddist.slices(0, 8, out=room[1:1 + 8 * 64])
    assert e.value.status == 6 and "aligned" in str(e.value)
    with pytest.raises(F.FidgetHipError) as e:
        ddist.within(squared=1, out=raw[4:4 + 64])
    assert e.value.status == 6 and "aligned" in str(e.value)
    compare(dev, reference(name, True), True)          # the context still works
