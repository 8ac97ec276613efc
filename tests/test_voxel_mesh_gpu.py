"""fhip_voxels_mesh and fhip_voxels_surface on the device against voxel_mesh_ref.py: bitmaps made in numpy (voxels_ref.pack) and handed to
the library as host bricks and as a torch CUDA tensor; triangles, vertices and the ten numbers of the summary are compared with
np.array_equal - the indices are integers and the coordinates exact.  Then what a caller does with the mesh (STL, resident arrays,
gradients at the vertices), a shape end to end, two runs, the refused calls and the overflow."""
import ctypes as C
import functools

import numpy as np
import pytest

import fidget_amd as F
import voxel_mesh_ref as MR
import voxels_ref as V
from stl_ref import stl_bytes
from test_many_inputs_gpu import same_f32
from test_mesh import sphere
from test_voxel_mesh import box, hollow_box16, square_ring16, voxels_at

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _torch():
    import torch
    return torch


def random_grid(depth, density, seed):
    N = 4 << depth
    return np.random.default_rng(seed).random((N, N, N)) < density


def sparse_256():
    g = box(256, (100, 3, 250), (140, 9, 256))
    g[0, 0, 0] = g[255, 255, 255] = True
    return g


GRIDS = {
    # depth 0: one brick, every face of it on the grid's border
    "d0-empty": lambda: np.zeros((4, 4, 4), bool),
    "d0-full": lambda: np.ones((4, 4, 4), bool),
    "d0-voxel000": lambda: voxels_at(4, [(0, 0, 0)]),
    "d0-voxel333": lambda: voxels_at(4, [(3, 3, 3)]),
    "d0-random0.5": lambda: random_grid(0, 0.5, 1),
    # depth 1: pairs across every brick boundary - no face between them; pinches across brick boundaries - shared vertices; corner brick B
    "d1-across-x": lambda: voxels_at(8, [(3, 2, 5), (4, 2, 5)]),
    "d1-across-y": lambda: voxels_at(8, [(2, 3, 5), (2, 4, 5)]),
    "d1-across-z": lambda: voxels_at(8, [(6, 1, 3), (6, 1, 4)]),
    "d1-edge-only": lambda: voxels_at(8, [(3, 3, 5), (4, 4, 5)]),
    "d1-corner-only": lambda: voxels_at(8, [(3, 3, 3), (4, 4, 4)]),
    "d1-voxel777": lambda: voxels_at(8, [(7, 7, 7)]),
    "d1-random0.05": lambda: random_grid(1, 0.05, 2),
    "d1-random0.5": lambda: random_grid(1, 0.5, 3),
    # depth 2
    "d2-hollow-box": hollow_box16,
    "d2-square-ring": square_ring16,
    "d2-plane-k0": lambda: box(16, (0, 0, 0), (16, 16, 1)),
    "d2-plane-i15": lambda: box(16, (15, 0, 0), (16, 16, 16)),
    # depth 4: 4 096 bricks and 17^3 corner bricks - the scans span blocks
    "d4-random0.001": lambda: random_grid(4, 0.001, 4),
    "d4-random0.2": lambda: random_grid(4, 0.2, 5),
    "d4-random0.9": lambda: random_grid(4, 0.9, 6),
    "d4-full": lambda: np.ones((64, 64, 64), bool),
    # depth 6, sparse: 262 144 bricks - more than two levels of a scan of 2 048 a block cover
    "d6-sparse": sparse_256,
}
KNOWN = {"d0-full": (96, 98, 192, 2), "d0-voxel000": (6, 8, 12, 2), "d1-across-x": (10, 12, 20, 2), "d1-edge-only": (12, 14, 23, 3),
         "d1-corner-only": (12, 15, 24, 3), "d2-hollow-box": (1248, 1252, 2496, 4), "d2-square-ring": (336, 336, 672, 0)}          # F, V, E, euler


@functools.lru_cache(maxsize=None)
def grid(name):
    g = GRIDS[name]()
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def reference(name):
    """(vertices, triangles, summary) of the reference, computed once and read-only"""
    verts, tris, s = MR.mesh_and_summary(grid(name))
    verts.setflags(write=False)
    tris.setflags(write=False)
    return verts, tris, tuple(s)


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


def raw_summary(s):
    return s.faces + (s.vertices, s.edges, s.n_faces, s.n)


def compare(vox, want):
    """`vox.mesh()` and `vox.surface()` against the reference's (vertices, triangles, summary) -> the mesh"""
    verts, tris, summary = want[0], want[1], tuple(want[2])
    s = vox.surface()
    print(f"summary: reference {summary}, device {raw_summary(s)}")
    assert raw_summary(s) == summary
    assert s.euler == summary[6] - summary[7] + summary[8] and s.area == summary[8] * (2.0 / vox.grid) ** 2
    m = vox.mesh()
    print(f"mesh: {len(m.vertices)} vertices of {len(verts)}, {len(m.triangles)} triangles of {len(tris)}")
    assert m.vertices.dtype == np.float32 and m.triangles.dtype == np.uint64
    assert m.vertices.shape == verts.shape and m.triangles.shape == tris.shape
    assert np.array_equal(m.vertices.view(np.uint32), verts.view(np.uint32))
    assert np.array_equal(m.triangles, tris)
    assert m.counts == {"cells": 0, "full": 0, "empty": 0, "leaf_cells": 0, "levels": 0}
    return m


@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_grids(name, where):
    want = reference(name)
    m = compare(voxels(bricks_of(name), where), want)
    s = want[2]
    if name in KNOWN:
        assert (s[8], s[6], s[7], s[6] - s[7] + s[8]) == KNOWN[name]
    if name == "d0-empty":
        assert len(m.triangles) == 0 and len(m.vertices) == 0 and len(m.stl()) == 84
        assert m.vertices_device() is None and m.triangles_device() is None
    if name == "d6-sparse":
        assert (s[8], s[6]) == (1044, 1050)
    if name == "d1-voxel777":
        assert (MR.lattice(m.vertices, 8) == 8).all(axis=1).any()          # lattice corner (N, N, N): corner brick B on every axis


@pytest.mark.parametrize("where", ["host", "torch"])
@pytest.mark.parametrize("name", ["d0-empty", "d1-corner-only", "d4-random0.2"])
def test_stl_and_the_resident_arrays(name, where):
    torch = _torch()
    verts, tris, _ = reference(name)
    vox = voxels(bricks_of(name), where)
    m = vox.mesh()
    ref = stl_bytes(verts, tris)
    got = m.stl()
    assert got.shape == ref.shape and np.array_equal(got, ref)
    out = torch.full((len(ref) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert m.stl(out=out) is out
    vox._hip.sync()
    flat = out.cpu().numpy()
    assert np.array_equal(flat[:len(ref)], ref) and (flat[len(ref):] == 0xA5).all()
    if len(tris) == 0:
        return
    dv, dt = m.vertices_device(), m.triangles_device()
    assert dv.shape == verts.shape and dt.shape == tris.shape
    tv = torch.as_tensor(dv, device="cuda")
    assert tv.data_ptr() == dv.ptr and np.array_equal(tv.cpu().numpy().view(np.uint32), verts.view(np.uint32))
    ti = dict(dt.__cuda_array_interface__, typestr="<i8")       # (the indices as int64: every torch takes that)
    tt = torch.as_tensor(type("A", (), {"__cuda_array_interface__": ti, "_keep": dt})(), device="cuda")
    assert tt.data_ptr() == dt.ptr and np.array_equal(tt.cpu().numpy().astype(np.uint64), tris)


def test_a_shape_end_to_end():
    """a sphere voxelized into a torch tensor, meshed; grown by two voxels, meshed again"""
    torch = _torch()
    depth = 3
    c = F.Context()
    shape = F.Shape(c, sphere(c, (0.0, 0.0, 0.0), 0.6))
    vox = F.voxelize(shape, depth, out=torch.zeros(8 * 8 ** depth, dtype=torch.uint8, device="cuda"))
    assert vox.on_device and vox.n > 0
    inside = vox.inside()
    m = compare(vox, MR.mesh_and_summary(inside))
    assert MR.six_volumes(MR.lattice(m.vertices, vox.grid), m.triangles) == 6 * vox.n
    assert MR.edges_balanced(m.triangles)
    s = vox.surface()
    assert s.euler == 2 and s.n == vox.n
    v = m.vertices
    got = m.vertex_grads(shape)
    own = np.asarray(shape.eval_grad_slice(v[:, 0], v[:, 1], v[:, 2])).reshape(-1, 4)
    assert got.shape == (len(v), 4) and same_f32(got, own)
    grown = vox.offset(2)
    gm, gs = grown.mesh(), grown.surface()
    assert gs.n_faces > s.n_faces and len(gm.triangles) == 2 * gs.n_faces > len(m.triangles) and gs.euler == 2


def test_a_void_extracted_and_meshed_on_its_own():
    """the hollow box's complement has two parts; the one away from the border is the cavity [4, 12)^3, meshed as a solid"""
    vox = voxels(bricks_of("d2-hollow-box"), "torch")
    comps = vox.components(connectivity=6, complement=True)
    assert comps.count == 2 and comps.border.tolist().count(False) == 1
    cavity = comps.extract([int(np.flatnonzero(~comps.border)[0])])
    want = MR.mesh_and_summary(box(16, 4, 12))
    m = compare(cavity, want)
    assert want[2][8] == 6 * 64 and want[2][6] == 6 * 64 + 2 and len(m.triangles) == 2 * 6 * 64
    assert vox.surface().euler == 4 and cavity.surface().euler == 2


def test_two_runs_give_the_same_arrays():
    vox = voxels(bricks_of("d4-random0.2"), "torch")
    a, b = vox.mesh(), vox.mesh()
    assert np.array_equal(a.triangles, b.triangles) and np.array_equal(a.vertices.view(np.uint32), b.vertices.view(np.uint32))
    assert raw_summary(vox.surface()) == raw_summary(vox.surface())


def test_refusals():
    """the refused calls - before any launch - and that the context works after them"""
    torch = _torch()
    name = "d1-random0.05"
    vox = voxels(bricks_of(name), "host")
    hip = vox._hip
    too_deep = F.Voxels(hip, np.zeros(1, np.uint64), 11, None)
    for call in (too_deep.mesh, too_deep.surface):
        with pytest.raises(F.FidgetHipError) as e:
            call()
        assert e.value.status == 6 and "depth" in str(e.value)          # FHIP_ERR_UNSUPPORTED
    h, out = C.c_void_p(), np.zeros(10, np.uint64)
    for on_device in (0, 1):          # a NULL bitmap
        assert F.lib().fhip_voxels_mesh(hip._h, None, 1, on_device, C.byref(h)) == 6 and not h.value
        assert F.lib().fhip_voxels_surface(hip._h, None, 1, on_device, F._p(out)) == 6
    assert F.lib().fhip_voxels_mesh(hip._h, F._p(vox.bricks), 1, 0, None) == 5          # no place for the result: FHIP_ERR_BAD_TAPE
    assert F.lib().fhip_voxels_surface(hip._h, F._p(vox.bricks), 1, 0, None) == 5
    assert F.lib().fhip_voxels_mesh(None, F._p(vox.bricks), 1, 0, C.byref(h)) == 5 and F.lib().fhip_voxels_surface(None, F._p(vox.bricks), 1, 0, F._p(out)) == 5
    raw = torch.zeros(8 * 8 + 8, dtype=torch.uint8, device="cuda")          # a bitmap on the device that is not 8-byte aligned
    torch.cuda.synchronize()
    odd = F.Voxels(hip, raw[4:4 + 64], 1, None)
    assert odd.bricks.data_ptr() % 8 == 4
    for call in (odd.mesh, odd.surface):
        with pytest.raises(F.FidgetHipError) as e:
            call()
        assert e.value.status == 6 and "aligned" in str(e.value)
    compare(vox, reference(name))          # the context still works


def test_overflow():
    """the 3-D checkerboard at depth 8 - one constant word - has 6 * 2^29 faces: more than 2^32 triangles.  The summary counts them;
    the mesh is refused from the counting pass's totals; a small call after it works."""
    torch = _torch()
    lx, ly, lz = np.indices((4, 4, 4))
    word = int((np.uint64(1) << (lx + 4 * ly + 16 * lz).astype(np.uint64))[(lx + ly + lz) % 2 == 0].sum())
    assert bin(word).count("1") == 32
    t = torch.full((256, 256, 256), word - (1 << 64) if word >> 63 else word, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    vox = F.Voxels(F.default_context(), t, 8, None)
    s = vox.surface()
    assert s.faces == (1 << 29,) * 6 and s.n == 1 << 29 and s.n_faces == 6 << 29
    with pytest.raises(F.FidgetHipError) as e:
        vox.mesh()
    assert e.value.status == 10          # FHIP_ERR_OVERFLOW
    del t, vox
    compare(voxels(bricks_of("d1-random0.05"), "torch"), reference("d1-random0.05"))
