"""fhip_triangles_voxels and fhip_mesh_voxels on the device against mesh_voxels_ref.py: meshes made in numpy and handed to the library
as host arrays and as torch CUDA tensors, indexed and as a soup, to a host `out` and a device `out`; every bitmap and every number of
`info` is compared with np.array_equal / ==.  Then the boundary mesh of a voxelized shape voxelized back - the original bitmap, bit for
bit, through the resident arrays and through an STL file's bytes - what is made of the result, two runs, the refused calls."""
import functools

import numpy as np
import pytest
from conftest import model_path

import fidget_amd as F
import mesh_voxels_ref as MV
import voxels_ref as V
from test_directional_gpu import pack
from test_mesh import sphere
from test_mesh_voxels import box_mesh, octahedron, rejected_mesh, sliver_and_flat, spanning16, tetrahedra, together

pytestmark = pytest.mark.gpu
TURN = np.array([[0.6, -0.8, 0.0, 0.05], [0.8, 0.6, 0.0, -0.1], [0.0, 0.0, 1.1, 0.02]])


@functools.lru_cache(maxsize=None)
def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (depth, vertices, triangles, matrix, the reference's packed bitmap, its info); computed once, shared"""
    depth, v, t, m = {
        "tetrahedra0": lambda: (0, *tetrahedra(5, 20), None),
        "octahedron0": lambda: (0, *octahedron(4, 2, 1), None),
        "tetrahedra2": lambda: (2, *together(tetrahedra(20, 7), sliver_and_flat()), None),          # 82 triangles: no multiple of 64
        "turned1": lambda: (1, *tetrahedra(6, 9, 1.0), TURN),
        "tetrahedra6": lambda: (6, *tetrahedra(6, 31), None),
        "spanning7": lambda: (7, *spanning16(), None),
    }[name]()
    inside, info = MV.voxelize(v, t, 4 << depth, m)
    return depth, v, t, m, (V.pack(inside) if depth < 3 else pack(inside)), info


def on_host(bricks):
    return bricks if isinstance(bricks, np.ndarray) else bricks.cpu().numpy().view(np.uint64)


def run(name, form, where, out_where):
    depth, v, t, m, want, info = case(name)
    torch, B = _torch(), 1 << depth
    mesh = (v, t) if form == "indexed" else MV.soup(v, t)
    if where == "device":
        mesh = (torch.from_numpy(v).cuda(), torch.from_numpy(t.astype(np.int64)).cuda()) if form == "indexed" else torch.from_numpy(mesh).cuda()
    out = None
    if out_where == "device":
        out = torch.full((B, B, B), -1, dtype=torch.int64, device="cuda")
    elif out_where == "host":
        out = np.full((B, B, B), ~np.uint64(0), np.uint64)
    got = F.voxelize_mesh(mesh, depth, mesh_to_world=m, out=out)
    assert got.on_device == (out_where == "device") and got.depth == depth
    assert np.array_equal(on_host(got.bricks), want)
    assert got.mesh_info == info and got.n == info["set_voxels"] and got.cells == {"cells": 0, "full": 0, "empty": 0, "leaf_cells": 0}
    return got


@pytest.mark.parametrize("where,out_where", [("host", None), ("host", "device"), ("device", "host"), ("device", "device")])
@pytest.mark.parametrize("form", ["indexed", "soup"])
@pytest.mark.parametrize("name", ["tetrahedra0", "octahedron0"])
def test_one_brick(name, form, where, out_where):
    got = run(name, form, where, out_where)
    if name == "octahedron0":          # the half-open reading: [-1, 1) on the middle row alone
        assert got.mesh_info["set_voxels"] == 2 and got.mesh_info["open_rows"] == 0


@pytest.mark.parametrize("form,where,out_where", [("indexed", "host", None), ("soup", "device", "device")])
def test_rows_of_four_bricks_sixteen_to_a_wave(form, where, out_where):
    got = run("tetrahedra2", form, where, out_where)
    assert got.mesh_info["triangles"] == 82 and got.mesh_info["flat"] == 1 and got.mesh_info["open_rows"] == 0


def test_the_matrix_is_applied_before_the_snap():
    run("turned1", "indexed", "host", None)
    run("turned1", "soup", "device", "device")


def test_a_row_is_exactly_one_wave():
    run("tetrahedra6", "indexed", "device", "device")


def test_rows_in_two_chunks_and_one_triangle_over_many_waves():
    got = run("spanning7", "indexed", "host", "device")
    info = got.mesh_info
    assert info["triangles"] == 16 and info["W"] > 10000 * info["triangles"] and info["clipped"] > 0 and info["open_rows"] == 0


@functools.lru_cache(maxsize=None)
def gyroid(depth):
    v = F.voxelize(F.Shape.from_vm(model_path("gyroid-sphere.vm")), depth)
    return v, v.mesh()


@pytest.mark.parametrize("depth", [4, 5])
def test_the_boundary_mesh_voxelizes_back_to_the_bitmap(depth):
    v, m = gyroid(depth)
    back = m.voxelize(depth)          # the resident arrays
    assert np.array_equal(back.bricks, v.bricks)
    info = back.mesh_info
    assert info["triangles"] == len(m.triangles) and info["open_rows"] == 0 and info["rejected"] == 0 and info["set_voxels"] == v.n
    if depth == 4:
        assert info["triangles"] > 50000
        soup = F.read_stl(m.stl())          # ... and the file's bytes, as a stranger's mesh arrives
        assert soup.shape == (len(m.triangles), 3, 3) and np.array_equal(soup, m.vertices[m.triangles.astype(np.int64)])
        again = F.voxelize_mesh(soup, depth)
        assert np.array_equal(again.bricks, v.bricks) and again.mesh_info == info
        # two runs, on the device: the same bits
        torch = _torch()
        a = m.voxelize(depth, out=torch.empty(16 ** 3, dtype=torch.int64, device="cuda"))
        b = m.voxelize(depth, out=torch.empty(16 ** 3, dtype=torch.int64, device="cuda"))
        assert torch.equal(a.bricks, b.bricks) and np.array_equal(on_host(a.bricks), v.bricks)


def test_what_is_made_of_a_bitmap_runs_on_the_result():
    v, m = gyroid(4)
    for out in (None, _torch().empty(16 ** 3, dtype=_torch().int64, device="cuda")):
        back = m.voxelize(4, out=out)
        c, c0 = back.components(), v.components()
        assert c.count == c0.count and c.n == c0.n
        assert np.array_equal(on_host(back.overhangs().bricks), v.overhangs().bricks)
        assert repr(back.thickness()) == repr(v.thickness())


def test_a_built_mesh_of_a_sphere_closes():
    """the mesh of a sphere of radius 0.8 closes inside the cube: no open row, from the resident arrays and from the host's"""
    c = F.Context()
    s = F.Shape(c, sphere(c, (0.0, 0.0, 0.0), 0.8))
    on, off = F.build_mesh(s, 4), F.build_mesh(s, 4, keep_device=False)
    assert on.vertices_device() is not None and off.vertices_device() is None
    a, b = on.voxelize(4), off.voxelize(4)
    assert a.mesh_info["open_rows"] == 0 and a.mesh_info["rejected"] == 0 and a.mesh_info["set_voxels"] > 0
    assert np.array_equal(a.bricks, b.bricks) and a.mesh_info == b.mesh_info


def test_more_than_2_to_the_32_items_of_work():
    """The prefix sums of the column counts are 32-bit sums and the flags of where they wrapped: 1301 copies of a sliver along the yz
    diagonal - its box is the whole grid of 2048^2 columns at depth 9, some ten thousand of them covered - come first, so every item of the
    tetrahedra that follow lies beyond 2^32.  1300 of the copies cancel: the bitmap is that of ONE sliver and the tetrahedra, which
    the library makes with W far below 2^32 (and that path is held to the reference above); the counts are sums."""
    torch, depth, copies = _torch(), 9, 1301
    sliver = np.array([[-0.3, -1.35, -1.35], [0.4, 1.35, 1.35], [0.1, 1.35, 1.34]], np.float32)          # ten voxels wide at its far end: some 10 000 columns
    v, t = tetrahedra(3, 41)
    few = np.concatenate([sliver, MV.soup(v, t).reshape(-1, 3)])
    many = np.concatenate([np.tile(sliver, (copies, 1)), MV.soup(v, t).reshape(-1, 3)])
    a = F.voxelize_mesh(few.reshape(-1, 3, 3), depth, out=torch.empty(1 << 27, dtype=torch.int64, device="cuda"))
    b = F.voxelize_mesh(many.reshape(-1, 3, 3), depth, out=torch.empty(1 << 27, dtype=torch.int64, device="cuda"))
    one = F.voxelize_mesh(sliver.reshape(1, 3, 3), depth, out=torch.empty(1 << 27, dtype=torch.int64, device="cuda")).mesh_info
    assert one["W"] > 3_300_000 and 0 < one["crossings"] < 20000 and a.mesh_info["set_voxels"] > one["set_voxels"] > 0
    assert b.mesh_info["W"] == a.mesh_info["W"] + (copies - 1) * one["W"] > 1 << 32
    for key in ("crossings", "clipped"):
        assert b.mesh_info[key] == a.mesh_info[key] + (copies - 1) * one[key], key
    assert b.mesh_info["triangles"] == copies + 12 and b.mesh_info["flat"] == 0 and b.mesh_info["rejected"] == 0
    assert torch.equal(a.bricks, b.bricks) and b.mesh_info["open_rows"] == a.mesh_info["open_rows"] and b.mesh_info["set_voxels"] == a.mesh_info["set_voxels"]


def test_trim_gives_the_scratch_back():
    """The call's scratch, 64 bytes per triangle, stays with the context - the buffer of the mesher's leaf records - and fhip_ctx_trim
    gives it back: 2 M triangles leave at least 128 MB behind, which a second call does not add to and trim returns."""
    import os
    torch = _torch()
    alone = not os.environ.get("PYTEST_XDIST_WORKER")          # (free device memory is the DEVICE's: with other test processes on it the readings mean nothing)
    T = 2_000_000
    soup = torch.from_numpy(np.tile(MV.soup(*tetrahedra(1, 3)), (T // 4, 1, 1))).cuda()
    out = torch.empty(8 ** 3, dtype=torch.int64, device="cuda")
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    first = F.voxelize_mesh(soup, 3, out=out, hip=hip)
    held = free0 - torch.cuda.mem_get_info()[0]
    again = F.voxelize_mesh(soup, 3, out=out, hip=hip)
    held_again = free0 - torch.cuda.mem_get_info()[0]
    hip.trim()
    after = free0 - torch.cuda.mem_get_info()[0]
    assert first.mesh_info == again.mesh_info and first.mesh_info["triangles"] == T and not bool(first.bricks.any())          # an even number of copies
    # (the buffer only grows and the second call needs no more: nothing is added but what the runtime may allocate for itself, allowed 16 MB)
    assert not alone or (held >= 64 * T and held_again <= held + (16 << 20) and after <= held_again - 64 * T), (held, held_again, after)
    assert F.voxelize_mesh(soup, 3, out=out, hip=hip).mesh_info == first.mesh_info          # whatever is needed again is made again
    del hip


def test_a_pair_may_be_a_list():
    depth, v, t, m, want, info = case("tetrahedra0")
    assert np.array_equal(F.voxelize_mesh([v, t], depth).bricks, want)
    with pytest.raises(TypeError, match="a pair"):
        F.voxelize_mesh([v, t, t], depth)


def test_no_triangles_give_an_empty_bitmap():
    out = np.full((2, 2, 2), ~np.uint64(0), np.uint64)
    got = F.voxelize_mesh((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint64)), 1, out=out)
    assert not out.any() and got.mesh_info == dict.fromkeys(MV.INFO, 0)


def test_refused_calls():
    v, t = rejected_mesh()
    with pytest.raises(ValueError, match=r"3 of 7 triangles rejected.*\[-1\.5, 1\.5\]"):
        F.voxelize_mesh((v, t), 1)
    out = np.full(8, 0xABABABABABABABAB, np.uint64)
    with pytest.raises(F.FidgetHipError, match="depth above 10"):
        F.voxelize_mesh(box_mesh(-0.5, 0.5), 11, out=out)
    assert (out == 0xABABABABABABABAB).all()
