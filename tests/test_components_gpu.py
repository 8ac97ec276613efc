"""fhip_voxels_components on the device against components_ref.py: bitmaps made in numpy (voxels_ref.pack) and handed to the library as
host bricks and as a torch CUDA tensor; the number of components, the whole table (sizes, seeds, bounds, border flags) and the label
images of every layer are compared with np.array_equal - ids included, which the interface fixes - for connectivity 6 and 26, for the
set bits and for their complement.  Then a shape end to end, `extract`, sub-ranges of layers and the refused calls."""
import functools

import numpy as np
import pytest

import fidget_amd as F
import oracle as O
import components_ref as CR
import occupancy_ref as R
import voxels_ref as V
from test_components import hollow_box
from test_mesh import sphere

pytestmark = pytest.mark.gpu

DIRECTIONS = [d for d in CR.offsets(26) if (d[2], d[1], d[0]) > (0, 0, 0)]          # the 13 of the positive half: 3 faces, 6 edges, 4 corners


@functools.lru_cache(maxsize=None)
def _torch():
    import torch
    return torch


def random_grid(depth, density, seed):
    N = 4 << depth
    return np.random.default_rng(seed).random((N, N, N)) < density


def checkerboard(depth):
    i, j, k = np.indices(((4 << depth),) * 3)
    return (i + j + k) % 2 == 0


def across(d):
    """two voxels of a grid of 8 that meet only across the brick boundary in direction d: the first in the brick the step leaves, on the
    layers that touch (coordinate 3 | 4 for +1, 4 | 3 for -1), both at 2 along the axes without a step"""
    a = [3 if v > 0 else 4 if v < 0 else 2 for v in d]
    b = [p + v for p, v in zip(a, d)]
    g = np.zeros((8, 8, 8), bool)
    g[tuple(a)] = g[tuple(b)] = True
    assert [p // 4 for p in a] != [p // 4 for p in b]
    return g


def serpentine():
    """one voxel wide through the whole grid of 16: in every even layer the even rows joined at alternating ends, the layers joined at
    alternating corners - one component under either connectivity, a single chain of 1087 voxels under 6"""
    g = np.zeros((16, 16, 16), bool)
    for k in range(0, 16, 2):
        g[:, 0::2, k] = True
        for r, j in enumerate(range(1, 15, 2)):
            g[15 if r % 2 == 0 else 0, j, k] = True
        if k + 1 < 15:
            g[0, 14 if (k // 2) % 2 == 0 else 0, k + 1] = True
    return g


GRIDS = {
    # depth 0: one brick
    "d0-empty": lambda: np.zeros((4, 4, 4), bool),
    "d0-full": lambda: np.ones((4, 4, 4), bool),
    "d0-checkerboard": lambda: checkerboard(0),
    "d0-random0.5": lambda: random_grid(0, 0.5, 1),
    # depth 1: 8 bricks, every pair of them a boundary
    "d1-random0.1": lambda: random_grid(1, 0.1, 2),
    "d1-random0.3": lambda: random_grid(1, 0.3, 3),
    "d1-random0.6": lambda: random_grid(1, 0.6, 4),
    **{"d1-across%+d%+d%+d" % d: (lambda d=d: across(d)) for d in DIRECTIONS},
    # depth 2: an interior brick with all 26 neighbours
    "d2-random0.25": lambda: random_grid(2, 0.25, 5),
    "d2-serpentine": serpentine,
    "d2-hollow-box": hollow_box,
    "d2-full": lambda: np.ones((16, 16, 16), bool),
    # depth 4: 4 096 bricks - the prefix sums take two blocks and recurse
    "d4-random0.2": lambda: random_grid(4, 0.2, 6),
    "d4-full": lambda: np.ones((64, 64, 64), bool),
}


@functools.lru_cache(maxsize=None)
def grid(name):
    g = GRIDS[name]()
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def reference(name, conn, complement):
    return CR.components(CR.foreground(grid(name), complement), conn)


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


def compare(vox, ref, conn, complement):
    comps = vox.components(conn, complement)
    N = vox.grid
    print(f"components: reference {ref.count}, device {comps.count}; nodes {comps.nodes}; foreground voxels: reference {int((ref.labels >= 0).sum())}, device {comps.n}")
    assert comps.count == ref.count and comps.n == int((ref.labels >= 0).sum()) and comps.nodes >= comps.count
    assert comps.sizes.dtype == np.uint64 and np.array_equal(comps.sizes, ref.sizes)
    for name in ("seeds", "lo", "hi"):
        got = getattr(comps, name)
        assert got.dtype == np.uint32 and got.shape == (ref.count, 3) and np.array_equal(got, getattr(ref, name)), name
    assert comps.border.dtype == bool and np.array_equal(comps.border, ref.border)
    lab = to_host(vox._hip, comps.label_slices(0, N))
    want = np.ascontiguousarray(ref.labels.transpose(2, 1, 0))
    print("label images: voxels that differ", int((lab != want).sum()))
    assert lab.dtype == np.int32 and lab.shape == (N, N, N) and np.array_equal(lab, want)
    return comps


@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("complement", [False, True])
@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("name", list(GRIDS))
def test_grids(name, conn, complement, where):
    ref = reference(name, conn, complement)
    comps = compare(voxels(bricks_of(name), where), ref, conn, complement)
    if name == "d0-checkerboard" and not complement:
        assert (comps.count, comps.nodes) == ((32, 32) if conn == 6 else (1, 1))
    if name.startswith("d1-across") and not complement:
        steps = sum(c in "+-" for c in name[len("d1-across"):].replace("+0", ""))
        assert comps.count == (1 if conn == 26 or steps == 1 else 2) and comps.nodes == 2
    if name == "d2-serpentine" and not complement:
        assert comps.count == 1 and int(comps.sizes[0]) == 1087 and comps.nodes > 100
    if name == "d2-hollow-box" and complement and conn == 6:
        assert comps.border.tolist() == [True, False] and int(comps.sizes[1]) == 8 ** 3          # one cavity
    if name.endswith("-full"):
        assert (comps.count, comps.largest() if comps.count else None) == ((0, None) if complement else (1, 0))
        assert comps.nodes == (0 if complement else 8 ** vox_depth(name))


def vox_depth(name):
    return int(name[1])


def two_spheres(M):
    c = M.Context()
    return M.Shape(c, c.min(sphere(c, (-0.45, -0.4, -0.35), 0.4), sphere(c, (0.5, 0.45, 0.4), 0.3)))


def test_a_shape_end_to_end():
    """two disjoint spheres voxelized into a torch tensor: two components, the larger one extracted and counted"""
    torch = _torch()
    depth = 3
    out = torch.full((8 * 8 ** depth,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = two_spheres(F)
    vox = F.voxelize(s, depth, out=out)
    inside = R.brute_force(two_spheres(O), depth)
    assert vox.on_device and np.array_equal(to_host(vox._hip, vox.bricks).view(np.uint64), V.pack(inside))
    ref = CR.components(inside, 6)
    comps = vox.components()
    print("sizes: reference", ref.sizes.tolist(), "device", comps.sizes.tolist(), "occupancy", F.occupancy(s, depth).n)
    assert comps.count == ref.count == 2 and int(comps.sizes.sum()) == F.occupancy(s, depth).n == comps.n
    assert np.array_equal(comps.sizes, ref.sizes) and not comps.border.any()
    big = comps.largest()
    assert big == int(np.argmax(ref.sizes)) and comps.sizes[big] > comps.sizes[1 - big]
    part = comps.extract([big])
    assert part.on_device and part.depth == depth and part.bricks.data_ptr() != vox.bricks.data_ptr()
    assert np.array_equal(to_host(vox._hip, part.bricks).view(np.uint64), V.pack(ref.labels == big))
    counts = to_host(vox._hip, part.layer_counts())
    assert int(counts.sum()) == int(comps.sizes[big])
    voids = vox.components(6, complement=True)          # two solid balls enclose nothing
    assert voids.count == 1 and voids.border.all() and voids.n == 32 ** 3 - comps.n


@pytest.mark.parametrize("where", ["host", "torch"])
def test_a_sub_range_of_layers(where):
    """layers 5 .. 10 of a grid of 16, neither end on a brick boundary; into a buffer of the caller's with room to spare"""
    name, conn = "d2-random0.25", 26
    ref = reference(name, conn, False)
    vox = voxels(bricks_of(name), where)
    comps = vox.components(conn)
    want = np.ascontiguousarray(ref.labels.transpose(2, 1, 0))
    got = to_host(vox._hip, comps.label_slices(5, 11))
    assert got.shape == (6, 16, 16) and np.array_equal(got, want[5:11]) and (got >= 0).any() and (got < 0).any()
    assert comps.label_slices(7, 7).shape == (0, 16, 16)
    if where == "torch":
        torch = _torch()
        out = torch.full((6 * 256 + 8,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert comps.label_slices(5, 11, out=out) is out
        flat = to_host(vox._hip, out)
        assert np.array_equal(flat[:-8].reshape(6, 16, 16), want[5:11]) and (flat[-8:] == -7).all()


@pytest.mark.parametrize("complement", [False, True])
@pytest.mark.parametrize("where", ["host", "torch"])
def test_extract(where, complement):
    name, conn = ("d1-random0.6" if complement else "d2-random0.25"), 6          # (19 and 323 components)
    ref = reference(name, conn, complement)
    vox = voxels(bricks_of(name), where)
    comps = vox.components(conn, complement)
    B = 1 << vox.depth
    words = B ** 3
    assert comps.count == ref.count > 3
    ids = [int(np.argmax(ref.sizes)), ref.count - 1, 1]
    want = V.pack(np.isin(ref.labels, ids))
    # into a buffer full of 0xA5 and longer than the bitmap: all of the bitmap and nothing beyond it
    if where == "host":
        out = np.full(words + 8, 0xA5A5A5A5A5A5A5A5, np.uint64)
        part = comps.extract(ids, out=out)
        assert np.shares_memory(part.bricks, out) and (out[words:] == 0xA5A5A5A5A5A5A5A5).all()
        got = part.bricks
    else:
        torch = _torch()
        out = torch.full((8 * words + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        part = comps.extract(ids, out=out)
        assert part.on_device and part.bricks.data_ptr() == out.data_ptr()
        flat = to_host(vox._hip, out)
        assert (flat[8 * words:] == 0xA5).all()
        got = flat[:8 * words].view(np.uint64).reshape(B, B, B)
    assert got.shape == (B, B, B) and np.array_equal(got, want)
    assert int(to_host(vox._hip, part.layer_counts()).sum()) == sum(int(ref.sizes[c]) for c in set(ids))
    nothing, everything = comps.extract([]), comps.extract(range(comps.count))
    assert not to_host(vox._hip, nothing.bricks).any()
    foreground = V.pack(CR.foreground(grid(name), complement))
    assert np.array_equal(to_host(vox._hip, everything.bricks).view(np.uint64), foreground)
    assert np.array_equal(to_host(vox._hip, comps.extract(np.array(ids[::-1] + ids)).bricks).view(np.uint64), want)          # any order, repeats


def test_two_runs_give_the_same_labels():
    vox = voxels(bricks_of("d4-random0.2"), "torch")
    a, b = vox.components(26), vox.components(26)
    assert a.count == b.count and np.array_equal(a.sizes, b.sizes) and np.array_equal(a.seeds, b.seeds)
    la, lb = a.label_slices(0, 64), b.label_slices(0, 64)
    vox._hip.sync()
    assert _torch().equal(la, lb)


def test_refusals():
    """the statuses of the refused calls, and that the context works after them"""
    torch = _torch()
    name = "d1-random0.3"
    vox = voxels(bricks_of(name), "host")
    with pytest.raises(F.FidgetHipError) as e:
        vox.components(18)
    assert e.value.status == 6 and "connectivity" in str(e.value)          # FHIP_ERR_UNSUPPORTED
    comps = vox.components(6)
    for ids in ([comps.count], [0, comps.count + 5], [-1]):
        with pytest.raises(F.FidgetHipError) as e:
            comps.extract(ids)
        assert e.value.status == 6 and "id" in str(e.value)
    for k0, k1 in ((0, 9), (5, 4)):          # k1 > N; k0 > k1
        with pytest.raises(F.FidgetHipError) as e:
            comps.label_slices(k0, k1)
        assert e.value.status == 6 and "k0 <= k1" in str(e.value)
    # a bitmap on the device that is not 8-byte aligned; label images on the device that are not 16-byte aligned
    raw = torch.zeros(8 * 8 + 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    odd = F.Voxels(vox._hip, raw[4:4 + 64], 1, None)
    assert odd.bricks.data_ptr() % 8 == 4
    with pytest.raises(F.FidgetHipError) as e:
        odd.components(6)
    assert e.value.status == 6 and "aligned" in str(e.value)
    dev = voxels(bricks_of(name), "torch")
    dcomps = dev.components(6)
    room = torch.zeros(8 * 64 + 4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert room[1:].data_ptr() % 16 == 4
    with pytest.raises(F.FidgetHipError) as e:
        dcomps.label_slices(0, 8, out=room[1:1 + 8 * 64])
    assert e.value.status == 6 and "aligned" in str(e.value)
    with pytest.raises(F.FidgetHipError) as e:
        F.Voxels(vox._hip, np.zeros(1, np.uint64), 11, None).components()
    assert e.value.status == 6 and "depth" in str(e.value)
    again = compare(dev, reference(name, 26, True), 26, True)          # the context still works
    assert again.count >= 1
