"""fhip_shape_voxels on the device against occupancy_ref.py's `inside[i, j, k]` packed by voxels_ref.py: the bitmaps are compared with
np.array_equal, word for word.  (a) is the brute-force array over all N^3 centres, (b) the octree recursion that defines the result;
tests/test_occupancy.py and tests/test_voxels.py hold the two to each other for the shapes compared against (a) here.  The octree's
counters are (b)'s where (b) is computed.  Layer images and layer counts are compared with the same arrays, from bricks on the host and
from bricks left on the device."""
import functools

import numpy as np
import pytest

import fidget_amd as F
import oracle as O
import occupancy_ref as R
import voxels_ref as V
from conftest import model_path
from test_many_inputs import spheres
from test_many_inputs_gpu import sphere_vars
from test_occupancy import BEAR_W2M, sphere_shape
from test_occupancy_gpu import constant, perspective, rotation, var_sphere, vm
from test_spills import many_live_values
from test_voxels import half_space

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _torch():
    import torch
    return torch


def device_buffer(words, extra=0, fill=0xA5):
    """a torch CUDA uint8 tensor of 8 * words + extra bytes, every byte `fill`"""
    torch = _torch()
    t = torch.full((8 * words + extra,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def host_words(t):
    return t.cpu().numpy().view(np.uint64)


def check(make, depth, w2m=None, vars_=None, against="b", out=None):
    """the device's bitmap for this case == pack(the reference's inside array); counters == (b)'s where computed; -> (Voxels, inside)"""
    s, o = make(F), make(O)
    vox = F.voxelize(s, depth, world_to_model=w2m, vars=vars_, out=out)
    B = 1 << depth
    assert (vox.depth, vox.grid) == (depth, 4 * B) and tuple(vox.bricks.shape) == (B, B, B)
    if against == "a":
        inside = R.brute_force(o, depth, w2m, vars_)
    else:
        inside, counts, _ = R.recursion(o, depth, w2m, vars_)
        print("reference counters", counts, "device", vox.cells)
        assert vox.cells == counts
    got = host_words(vox.bricks) if vox.on_device else vox.bricks
    want = V.pack(inside)
    print("inside voxels: reference", int(inside.sum()), "device", V.popcount(got), "words that differ", int((got != want).sum()))
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    return vox, inside


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_sphere(depth):
    """depth 0: one brick on a grid of 4, the root itself the leaf cell"""
    vox, inside = check(lambda M: sphere_shape(M, 0.5), depth)
    assert np.array_equal(vox.inside(), inside)
    if depth == 0:
        assert vox.bricks.shape == (1, 1, 1) and vox.cells == {"cells": 1, "full": 0, "empty": 0, "leaf_cells": 1} and vox.n == 8
    if depth == 3:
        assert vox.n == 2176 == F.occupancy(sphere_shape(F, 0.5), 3).n == V.popcount(vox.bricks)
        assert (vox.cells["full"], vox.cells["empty"], vox.cells["leaf_cells"]) == (8, 200, 80)


@pytest.mark.parametrize("where", ["host", "torch"])
def test_out_is_written_completely(where):
    """`out` full of 0xA5 bytes: +1 everywhere leaves 512 zero words (nothing but the clearing pass writes), -1 everywhere 512 words of all
    ones (the root Full: one box); bytes beyond the bitmap stay as they were"""
    for value, word in ((1.0, 0), (-1.0, 0xFFFFFFFFFFFFFFFF)):
        if where == "host":
            out = np.full(512 + 8, 0xA5A5A5A5A5A5A5A5, np.uint64)
            vox = F.voxelize(constant(value)(F), 3, out=out)
            got, rest = vox.bricks, out[512:]
            assert np.shares_memory(got, out) and (rest == 0xA5A5A5A5A5A5A5A5).all()
        else:
            out = device_buffer(512, extra=64)
            vox = F.voxelize(constant(value)(F), 3, out=out)
            assert vox.on_device and vox.bricks.data_ptr() == out.data_ptr()
            got = host_words(vox.bricks)
            assert (out[4096:].cpu().numpy() == 0xA5).all()
        assert got.shape == (8, 8, 8) and (got == np.uint64(word)).all()
        assert vox.cells == {"cells": 1, "full": int(value < 0), "empty": int(value > 0), "leaf_cells": 0}
        assert vox.n == (32 ** 3 if value < 0 else 0)


def test_full_cells_with_rows_of_two_and_one_words():
    vox, _ = check(lambda M: sphere_shape(M, 0.9), 3)
    assert vox.cells["full"] == 32          # 8 of level 2 (rows of 2 words) and 24 of level 3 (single words), tests/test_occupancy.py


def test_full_cells_with_rows_of_eight_words():
    """sphere 0.9 at depth 5: Full cells from level 2 (8^3 words) down.  To a host array (the library's own buffer), to a 16-byte aligned
    device buffer (16 bytes per lane) and to one that is only 8-byte aligned (8 bytes per lane): the same words"""
    make = lambda M: sphere_shape(M, 0.9)        # noqa: E731
    vox, inside = check(make, 5, against="a")
    _, counts, full_per_level = R.recursion(make(O), 5)
    assert vox.cells == counts and full_per_level[2] > 0
    words = 32 ** 3
    aligned = device_buffer(words)
    assert aligned.data_ptr() % 16 == 0
    on_dev = F.voxelize(make(F), 5, out=aligned)
    odd = device_buffer(words, extra=8)[8:]
    assert odd.data_ptr() % 16 == 8
    on_dev_odd = F.voxelize(make(F), 5, out=odd)
    assert np.array_equal(host_words(on_dev.bricks), vox.bricks) and np.array_equal(host_words(on_dev_odd.bricks), vox.bricks)
    assert on_dev.cells == on_dev_odd.cells == vox.cells and on_dev.n == on_dev_odd.n == int(inside.sum())


def test_half_space_full_octants():
    """x - 0.25 at depth 4: the four octants of x < 0 are Full at level 1, 8^3 words each"""
    vox, inside = check(half_space, 4, against="a")
    _, counts, full_per_level = R.recursion(half_space(O), 4)
    assert full_per_level[1] == 4 and vox.cells == counts
    assert (vox.bricks[:, :, :8] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and vox.n == 40 * 64 * 64


@pytest.mark.parametrize("name,w2m", [("gyroid-sphere.vm", None), ("colonnade.vm", None), ("bear.vm", BEAR_W2M)])
def test_models(name, w2m):
    check(vm(name), 3, w2m, against="a")
    check(vm(name), 3, w2m, against="b")      # ... and the counters


@pytest.mark.parametrize("matrix", [rotation, perspective])
def test_transforms(matrix):
    check(lambda M: sphere_shape(M, 0.5), 3, matrix())


def test_a_variable():
    vox, _ = check(var_sphere, 3, vars_={7: 0.625})
    assert vox.n > 2176
    with pytest.raises(ValueError, match="MissingVar"):
        F.voxelize(var_sphere(F), 3)


def test_more_than_16_inputs():
    """the bound-tape path"""
    vals = sphere_vars(80)
    make = lambda M: M.Shape(*spheres(M, 80))        # noqa: E731
    assert make(F).var_count() > 16
    check(make, 3, vars_=vals)


def test_more_leaf_cells_than_blocks():
    """gyroid-sphere at depth 6: 79 226 leaf cells for at most 4 096 blocks, every block some twenty cells in turn.  Against (a)"""
    vox, _ = check(vm("gyroid-sphere.vm"), 6, against="a")
    assert vox.cells["leaf_cells"] == 79226 > 4096 and vox.n == 655036


@pytest.mark.parametrize("name,depth", [("colonnade.vm", 5), ("prospero.vm", 7)])
def test_simplification_does_not_matter(name, depth):
    """the tape simplified on the way down (prospero at depth 7: twice) or not at all: the same bitmap, device against device"""
    torch = _torch()
    s = F.Shape.from_vm(model_path(name))
    words = 8 ** depth
    default = F.voxelize(s, depth, out=device_buffer(words))
    with s.hip.options(mesh_simplify_min_ops=0):
        plain = F.voxelize(s, depth, out=device_buffer(words, fill=0x5A))
    assert default.on_device and plain.on_device and default.bricks.data_ptr() != plain.bricks.data_ptr()
    assert torch.equal(default.bricks, plain.bricks)
    assert default.cells == plain.cells
    n = F.occupancy(s, depth).n
    print("inside voxels", default.n, plain.n, "occupancy", n)
    assert default.n == plain.n == n > 0


@functools.lru_cache(maxsize=None)
def _slice_case(name, depth):
    make = (lambda M: sphere_shape(M, 0.5)) if name == "sphere" else vm(name)
    s = make(F)
    inside = R.brute_force(make(O), depth)
    host = F.voxelize(s, depth)
    dev = F.voxelize(s, depth, out=device_buffer(8 ** depth))
    assert np.array_equal(host.bricks, V.pack(inside)) and np.array_equal(host_words(dev.bricks), host.bricks)
    return host, dev, inside


@pytest.mark.parametrize("name,depth,k0,k1", [("sphere", 0, 0, 4), ("sphere", 2, 5, 11), ("gyroid-sphere.vm", 3, 0, 32), ("sphere", 1, 3, 4)])
def test_slices(name, depth, k0, k1):
    """depth 0: rows of 4 bytes, shorter than a wave; depth 2 layers 5..10: neither end on a brick boundary; depth 1: rows of two bricks"""
    torch = _torch()
    host, dev, inside = _slice_case(name, depth)
    N = 4 << depth
    want = V.slices(inside, k0, k1)
    got = host.slices(k0, k1)
    assert got.dtype == np.uint8 and got.shape == (k1 - k0, N, N) and np.array_equal(got, want)
    assert want.any() and not want.all()
    out = torch.full(((k1 - k0) * N * N + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert dev.slices(k0, k1, out=out) is out
    dev._hip.sync()
    flat = out.cpu().numpy()
    assert np.array_equal(flat[:-16].reshape(k1 - k0, N, N), want) and (flat[-16:] == 0xA5).all()
    fresh = dev.slices(k0, k1)          # a tensor of the call's own
    dev._hip.sync()
    assert fresh.is_cuda and tuple(fresh.shape) == (k1 - k0, N, N) and np.array_equal(fresh.cpu().numpy(), want)
    assert host.slices(k0, k0).shape == (0, N, N)          # k0 == k1: nothing


@pytest.mark.parametrize("name,depth", [("sphere", 0), ("sphere", 2), ("gyroid-sphere.vm", 3)])
def test_layer_counts(name, depth):
    host, dev, inside = _slice_case(name, depth)
    want = V.layer_counts(inside)
    got = host.layer_counts()
    assert got.shape == (4 << depth,) and np.array_equal(got.astype(np.int64), want)
    assert int(got.sum()) == host.n == int(inside.sum())
    on_dev = dev.layer_counts()
    dev._hip.sync()
    assert on_dev.is_cuda and np.array_equal(on_dev.cpu().numpy(), want) and dev.n == host.n


def test_layer_counts_of_a_large_slab():
    """gyroid-sphere at depth 6: 64 x 64 bricks per slab, 16 partials per layer group"""
    s = F.Shape.from_vm(model_path("gyroid-sphere.vm"))
    vox = F.voxelize(s, 6)
    got = vox.layer_counts()
    want = V.layer_counts(vox.inside())         # (the bitmap itself is held to brute force by test_more_leaf_cells_than_blocks)
    assert np.array_equal(got.astype(np.int64), want) and int(got.sum()) == 655036


def test_two_runs_give_the_same_bitmap():
    s = F.Shape.from_vm(model_path("gyroid-sphere.vm"))
    a, b = F.voxelize(s, 5), F.voxelize(s, 5)
    assert a.bricks is not b.bricks and np.array_equal(a.bricks, b.bricks) and a.cells == b.cells and a.n == b.n > 0


def test_refusals():
    """the statuses and messages of the refused calls, and that the context works after them"""
    s = sphere_shape(F, 0.5)
    with pytest.raises(F.FidgetHipError) as e:
        F.voxelize(s, 11)
    assert e.value.status == 6 and "depth" in str(e.value)          # FHIP_ERR_UNSUPPORTED
    big = many_live_values(F)
    with pytest.raises(F.FidgetHipError) as e:
        F.voxelize(big, 2)
    assert e.value.status == 6 and "LDS" in str(e.value)
    c = F.Context()
    with pytest.raises(F.FidgetHipError) as e:
        F.voxelize(F.Shape(c, roots=[c.x(), c.y()]), 2)
    assert e.value.status == 5          # FHIP_ERR_BAD_TAPE: one output
    vox = F.voxelize(s, 2)
    for k0, k1 in ((0, 17), (5, 4)):          # k1 > N; k0 > k1
        with pytest.raises(F.FidgetHipError) as e:
            vox.slices(k0, k1)
        assert e.value.status == 6 and "k0 <= k1" in str(e.value)
    again = F.voxelize(s, 3)          # the context still works
    assert again.n == 2176 and vox.slices(0, 16).shape == (16, 16, 16)
