"""fhip_distance_thickness on the device against thickness_ref.py: the solids of thickness_grids.py packed in numpy (voxels_ref.pack) and
handed to the library as host bricks and, for a subset, as a torch CUDA tensor.  Per grid the whole field, a sub-range of layers, the
summary, `thin` / `within` / `beyond` at t = 1, 2, min, max - 1, max, a histogram, the field in place, a second run and a caller's
buffer for `thin` are compared with np.array_equal - every value is an integer.  Then a shape end to end, and the refused calls."""
import functools

import numpy as np
import pytest

import fidget_amd as F
import oracle as O
import distance_ref as DR
import occupancy_ref as R
import thickness_grids as G
import thickness_ref as TR
import voxels_ref as V
from test_mesh import sphere

pytestmark = pytest.mark.gpu

ON_TORCH = ("d0-clear000", "d1-ball10", "d2-fin-on-block", "d2-plates-i", "d3-tilted-slab", "d4-pores0.03", "d5-slab66-x")
CASES = [(name, "host") for name in G.GRIDS] + [(name, "torch") for name in ON_TORCH]


@functools.lru_cache(maxsize=None)
def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def bricks_of(name):
    b = V.pack(G.grid(name))
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


def compare(vox, T, complement):
    """everything `vox.thickness(complement)` offers against the reference field T [i, j, k]"""
    N, hip = vox.grid, vox._hip
    th = vox.thickness(complement)
    want = TR.field(T)
    got = to_host(hip, th.slices(0, N))
    print(f"field: values that differ {int((got.view(np.uint32) != want).sum())} of {want.size}; balls {th.balls} of {th.centres} centres")
    assert isinstance(th, F.ThicknessField) and got.shape == (N, N, N) and got.dtype == (np.uint32 if not vox.on_device else np.int32)
    assert np.array_equal(got.view(np.uint32), want)
    k0, k1 = N // 4 + 1, N - N // 4 - 1          # neither end on a brick boundary
    assert np.array_equal(to_host(hip, th.slices(k0, k1)).view(np.uint32), want[k0:k1])
    hi, arg_hi, lo, arg_lo, n = TR.summary(T)
    print(f"summary: reference {(hi, arg_hi, lo, arg_lo, n)}, device {(th.max_squared, th.argmax, th.min_squared, th.argmin, th.n)}")
    assert (th.max_squared, th.argmax, th.min_squared, th.argmin, th.n) == (hi, arg_hi, lo, arg_lo, n)
    assert (th.depth, th.grid) == (vox.depth, N)
    dist = vox.distance(complement=not complement)
    assert th.n == N ** 3 - dist.n == th.centres and (0 < th.balls <= th.centres if n else th.balls == 0)
    for t in sorted({1, 2, lo or 1, max(hi - 1, 0), hi}):
        for what, bits in (("thin", TR.thin(T, t)), ("within", TR.within(T, t)), ("beyond", TR.beyond(T, t))):
            part = getattr(th, what)(squared=t)
            assert part.on_device == vox.on_device and part.depth == vox.depth and part.cells is None
            assert np.array_equal(bricks_host(part), V.pack(bits)), (what, t)
    edges = sorted([0, 1, 2, 5, hi, hi + 1])          # (ascending also where the largest value is below 5)
    counts = to_host(hip, th.histogram(edges))
    assert counts.dtype == (np.int64 if vox.on_device else np.uint64) and np.array_equal(counts.astype(np.uint64), TR.histogram(T, edges)), (edges, counts)
    assert int(counts.sum()) == N ** 3          # from 0 to the largest value: every voxel once
    # the field in place
    arr = th.squared_device
    assert arr.shape == (N, N, N) and arr.__cuda_array_interface__["typestr"] == "<u4"
    torch = _torch()
    as_i4 = dict(arr.__cuda_array_interface__, typestr="<i4")       # (the values as int32: every torch takes that)
    hip.sync()
    inplace = torch.as_tensor(type("A", (), {"__cuda_array_interface__": as_i4, "_keep": arr})(), device="cuda")
    assert inplace.data_ptr() == arr.ptr and np.array_equal(inplace.cpu().numpy().view(np.uint32), want)
    # a second run: the same bits
    again = vox.thickness(complement)
    assert (again.max_squared, again.argmax, again.min_squared, again.argmin, again.n) == (hi, arg_hi, lo, arg_lo, n)
    assert np.array_equal(to_host(hip, again.slices(0, N)).view(np.uint32), want)
    # `thin` into a buffer of the caller's, full of 0xA5 and longer than the bitmap
    words = (N // 4) ** 3
    want_thin = V.pack(TR.thin(T, 2))
    if vox.on_device:
        out = torch.full((8 * words + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        part = th.thin(squared=2, out=out)
        flat = to_host(hip, out)
        assert part.bricks.data_ptr() == out.data_ptr() and (flat[8 * words:] == 0xA5).all()
        assert np.array_equal(flat[:8 * words].view(np.uint64).reshape(want_thin.shape), want_thin)
    else:
        out = np.full(words + 8, 0xA5A5A5A5A5A5A5A5, np.uint64)
        part = th.thin(squared=2, out=out)
        assert np.shares_memory(part.bricks, out) and (out[words:] == 0xA5A5A5A5A5A5A5A5).all() and np.array_equal(part.bricks, want_thin)
    assert np.array_equal(bricks_host(th.thin(r=1.5)), want_thin)          # floor(1.5^2) = 2
    return th


@pytest.mark.parametrize("name,where", CASES)
def test_grids(name, where):
    complement = G.GRIDS[name][1]
    T = G.reference(name)
    th = compare(voxels(bricks_of(name), where), T, complement)
    if name == "d0-empty":
        assert (th.max_squared, th.argmax, th.min_squared, th.argmin, th.n, th.balls) == (0, (0, 0, 0), None, None, 0, 0)
    if name == "d0-clear000":
        assert th.max_squared == 27 and th.argmax == (1, 0, 0)
    if name == "d2-fin-on-block":          # the fin does not inherit the block's value
        assert np.array_equal(V.unpack(bricks_host(th.thin(squared=1)))[12:15, 7:9, 4:12], np.ones((3, 2, 8), bool))
    if name.startswith("d2-plates"):          # 6 and 7 voxels thick: 3^2 and 4^2; a finite plate is thinner towards its rim
        assert th.max_squared == 16 and (th.min_squared == 9) == name.endswith("spanning")
    if name in G.SLABS:          # 66 thick: 33^2, rows of 65 voxels; the two medial planes alone are painted
        assert th.max_squared == 33 ** 2 and th.balls == 2 * 128 * 128


def test_a_shape_end_to_end():
    """a sphere voxelized into a torch tensor: the thickness of the solid and the width of the space around it"""
    torch = _torch()
    depth = 3
    c = F.Context()
    vox = F.voxelize(F.Shape(c, sphere(c, (0.1, 0.0, -0.1), 0.6)), depth, out=torch.zeros(8 * 8 ** depth, dtype=torch.uint8, device="cuda"))
    oc = O.Context()
    inside = R.brute_force(O.Shape(oc, sphere(oc, (0.1, 0.0, -0.1), 0.6)), depth)
    assert vox.on_device and np.array_equal(V.unpack(bricks_host(vox)), inside) and np.array_equal(vox.inside(), inside)
    walls = compare(vox, TR.by_centres(DR.edt(~inside)), False)
    compare(vox, TR.by_centres(DR.edt(inside)), True)
    assert 8 ** 2 < walls.max_squared <= 11 ** 2 and walls.n == int(inside.sum())          # a ball of radius 0.6 * 16 = 9.6 voxels


def test_refusals():
    """the statuses of the refused calls, and that the context works after them"""
    full = voxels(V.pack(np.ones((4, 4, 4), bool)), "host")
    with pytest.raises(F.FidgetHipError) as e:
        full.thickness()          # no clear voxel: no bounded ball
    assert e.value.status == 6 and "foreground" in str(e.value)
    with pytest.raises(F.FidgetHipError) as e:
        voxels(V.pack(np.zeros((4, 4, 4), bool)), "host").thickness(complement=True)
    assert e.value.status == 6 and "foreground" in str(e.value)
    hip = full._hip
    h = F.C.c_void_p()
    assert F.lib().fhip_distance_thickness(hip._h, None, F.C.byref(h)) == 5 and not h.value          # FHIP_ERR_BAD_TAPE
    th = voxels(bricks_of("d1-ball10"), "host").thickness()
    assert F.lib().fhip_distance_thickness(hip._h, th._owner.h, None) == 5
    assert F.lib().fhip_distance_thickness(hip._h, th._owner.h, F.C.byref(h)) == 6 and not h.value          # a thickness of a thickness
    with pytest.raises(F.FidgetHipError):
        th.thickness()
    for edges in ([1], [3, 2], [-1, 2], list(range(1025))):
        with pytest.raises(ValueError):
            th.histogram(edges)
    assert F.lib().fhip_thickness_histogram(hip._h, None, None, 2, None, 0) == 5
    two = np.array([3, 2], np.uint32)
    out = np.zeros(1, np.uint64)
    assert F.lib().fhip_thickness_histogram(hip._h, th._owner.h, two.ctypes.data_as(F.C.c_void_p), 2, out.ctypes.data_as(F.C.c_void_p), 0) == 6
    with pytest.raises(F.FidgetHipError) as e:
        th.thin(squared=0xFFFFFFFF)
    assert e.value.status == 6
    with pytest.raises(ValueError):
        th.thin()
    assert th.histogram(list(range(1024))).shape == (1023,)
    compare(voxels(bricks_of("d1-ball10"), "host"), G.reference("d1-ball10"), False)          # the context still works
