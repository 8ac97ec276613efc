"""fhip_topology_slices on the device against mesh_slices_ref.py, run on the Topology's own arrays.  Every integer array and the bits of
the positions are compared with np.array_equal; a loop's area2 against math.fsum within n 2^-52 sum |term| for its n segments, the
bound of n rounded additions in any order.  The meshes: the boundary meshes of a random bitmap and of a ball, a one-voxel cube under
300 planes - more crossings on one edge than a workgroup has lanes - and build_mesh of a sphere; cross-checks against
Voxels.outlines and Voxels.layer_counts; inputs on the host and on the device, as a soup and as a pair, twice; refused calls."""
import functools

import numpy as np
import pytest

import fidget_amd as F
import mesh_slices_ref as SR
import voxels_ref as V
from test_mesh import sphere
from test_mesh_slices import bitmap, centre_planes, cube_planes, voxel_mesh

pytestmark = pytest.mark.gpu
ARRAYS = ("plane", "edge", "next", "loop_of", "degree")
LOOP_COLUMNS = ("leader", "plane", "crossings", "segments", "irregular")


def check(got, name=""):
    """a MeshSlices against the reference's slices of the same indexed mesh: -> the reference's dict"""
    want = SR.slices(got.topology.vertices, got.topology.triangles, got.zs)
    assert {k: got.counts[k] for k in SR.COUNTS} == want["counts"], name
    assert got.xy.dtype == np.float32 and got.xy.shape == want["xy"].shape and np.array_equal(got.xy.view(np.uint32), want["xy"].view(np.uint32)), name
    for key in ARRAYS:
        a = getattr(got, key)
        assert a.dtype == want[key].dtype and a.shape == want[key].shape and np.array_equal(a, want[key]), (name, key)
    for key in LOOP_COLUMNS:
        assert got.loops[key].dtype == np.uint32 and np.array_equal(got.loops[key], want["loops"][key]), (name, key)
    for key in ("lo", "hi"):
        assert np.array_equal(got.loops[key].view(np.uint32), want["loops"][key].view(np.uint32)), (name, key)
    for key in ("crossings", "segments", "loops"):
        assert got.per_plane[key].dtype == np.uint64 and np.array_equal(got.per_plane[key], want["per_plane"][key]), (name, key)
    err = np.abs(got.loops["area2"] - want["loops"]["area2"])
    bound = want["loops"]["segments"] * 2.0 ** -52 * want["loops"]["area2_abs"]
    print(f"{name}: {got.counts}, area2 error / bound {np.max(err / np.maximum(bound, 1e-300), initial=0):.3g}")
    assert np.all(err <= bound), name
    return want


@functools.lru_cache(maxsize=None)
def case(name):
    """-> MeshSlices"""
    if name in ("random 8", "ball"):
        return F.mesh_slices(voxel_mesh(name), centre_planes(bitmap(name).shape[0]))
    if name == "cube":
        return F.mesh_slices(voxel_mesh("cube"), cube_planes(300))
    assert name == "sphere"
    c = F.Context()
    return F.build_mesh(F.Shape(c, sphere(c, (0.0, 0.0, 0.0), 0.5)), 2).slices(np.linspace(-0.55, 0.55, 12).astype(np.float32))


# ---- 7. every array equal to the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random 8", "ball", "cube", "sphere"])
def test_the_device_is_the_reference(name):
    got = case(name)
    want = check(got, name)
    if name == "random 8":
        assert want["counts"] == {"planes": 8, "vertices": 798, "segments": 816, "loops": 54, "irregular": 18}
    if name == "cube":          # the bottom face's plane cuts nothing; the other 299 cut the four vertical edges and the four side faces' diagonals
        assert got.counts["vertices"] == 8 * 299 and got.counts["loops"] == 299 and got.per_plane["crossings"].tolist() == [0] + [8] * 299
        assert np.bincount(got.edge[:, 0].astype(np.int64) * 8 + got.edge[:, 1]).max() == 299 > 256
        assert got.loops["area2"].tolist() == [0.5] * 299
    if name == "sphere":
        assert got.counts["vertices"] > 0 and got.topology.counts["triangles"] > 12
    polys, skipped = got.polygons(int(got.loops["plane"][0]))
    ref_polys, ref_skipped = SR.polygons(want, int(got.loops["plane"][0]))
    assert skipped == ref_skipped and len(polys) == len(ref_polys) and all(np.array_equal(a, b) for a, b in zip(polys, ref_polys))


# ---- 8. cross-checks of existing features -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ball", "sphere"])
def test_a_closed_manifold_mesh_gives_closed_polygons(name):
    got = case(name)
    assert got.counts["irregular"] == 0 and got.counts["vertices"] == got.counts["segments"]
    assert np.array_equal(np.sort(got.next), np.arange(got.counts["vertices"]))          # a permutation
    assert (got.degree == 0x11).all() and (name != "ball" or (got.loops["area2"] > 0).all())          # a ball has no holes
    for p in range(got.counts["planes"]):
        polys, skipped = got.polygons(p)
        assert skipped == 0 and len(polys) == got.per_plane["loops"][p]
    text = got.svg(int(got.loops["plane"][0]))
    assert text.startswith("<svg") and text.count("<path") == int(got.per_plane["loops"][got.loops["plane"][0]])


@pytest.mark.parametrize("name", ["random 8", "ball"])
def test_cross_sections_against_the_bitmap(name):
    """the bitmap's own boundary mesh (Voxels.mesh), cut at the layers' centres: the area of every cross-section is the layer's count of
    voxels, exactly - every term is a multiple of 1 / N^2 - and for the ball, whose layers have no pixels that touch at a corner alone,
    the loops are as many as the layer's outlines"""
    g = bitmap(name)
    N = g.shape[0]
    vox = F.Voxels(F.default_context(), V.pack(g), N.bit_length() - 3, None)
    got = vox.mesh().slices(centre_planes(N))
    check(got, name + ", Voxels.mesh")
    area2 = np.array([got.loops["area2"][got.loops_of(p)].sum() for p in range(N)])
    assert np.array_equal(area2 / 2 * (N / 2) ** 2, vox.layer_counts().astype(np.float64))
    if name == "ball":
        assert np.array_equal(got.per_plane["loops"], np.diff(vox.outlines(0, N).loop_start))


# ---- 9. inputs and errors --------------------------------------------------------------------------------------------------------------------------
def same(a, b, but=()):
    assert {k: a.counts[k] for k in SR.COUNTS} == {k: b.counts[k] for k in SR.COUNTS}
    assert np.array_equal(a.xy.view(np.uint32), b.xy.view(np.uint32))
    for key in ARRAYS:
        assert key in but or np.array_equal(getattr(a, key), getattr(b, key)), key
    for key in LOOP_COLUMNS + ("lo", "hi"):
        assert np.array_equal(a.loops[key], b.loops[key]), key
    for key in a.per_plane:
        assert np.array_equal(a.per_plane[key], b.per_plane[key]), key


def test_inputs_on_the_host_and_on_the_device_as_a_soup_and_as_a_pair_twice():
    import torch
    v, t = voxel_mesh("random 8")
    zs = centre_planes(8)
    host = case("random 8")
    same(host, F.mesh_slices(voxel_mesh("random 8"), zs))          # two runs
    same(host, F.mesh_slices((torch.from_numpy(v).cuda(), torch.from_numpy(t.astype(np.int64)).cuda()), zs))
    soup = v[t.astype(np.int64)]          # [T, 3, 3]: welded, the vertices numbered by their first corners
    by_soup = F.mesh_slices(soup, zs)
    same(by_soup, F.mesh_slices(torch.from_numpy(soup).cuda(), zs))
    same(by_soup, F.mesh_slices((v, t), zs, weld=True))
    same(by_soup, host, but=("edge",))          # the same crossings in the same order, on edges named by other vertex ids
    check(by_soup, "soup")
    same(host, F.mesh_slices(host.topology, zs))          # a Topology is cut as it is
    # the device arrays are the host copies
    for got in (host, by_soup):
        n = got.counts["vertices"]
        assert np.array_equal(torch.as_tensor(got.xy_device(), device="cuda").cpu().numpy().view(np.uint32), got.xy.view(np.uint32))
        for what, host_copy in (("next", got.next), ("loop_of", got.loop_of), ("plane", got.plane)):
            d = getattr(got, what + "_device")()
            assert d.shape == (n,) and np.array_equal(torch.as_tensor(d, device="cuda").cpu().numpy().view(np.uint32), host_copy), what


def test_empty_results_and_refused_calls():
    cube = voxel_mesh("cube")
    none = F.mesh_slices(cube, [])
    assert none.counts == dict.fromkeys(F.SLICES_COUNTS, 0) and none.xy.shape == (0, 2) and none.xy_device() is None and none.loops["leader"].shape == (0,)
    missed = F.mesh_slices(cube, [-2.0, 0.5, 1.0])          # below the cube, and twice above it
    assert missed.counts == dict(dict.fromkeys(F.SLICES_COUNTS, 0), planes=3) and missed.per_plane["crossings"].tolist() == [0, 0, 0] and missed.next.shape == (0,)
    assert missed.polygons(1) == ([], 0) and missed.zs.tolist() == [-2.0, 0.5, 1.0]
    with pytest.raises(IndexError):
        missed.polygons(3)
    assert F.mesh_slices(np.zeros((0, 3, 3), np.float32), [0.0]).counts["vertices"] == 0
    for zs in ([0.0, -0.25], [-0.25, -0.25], [-0.25, np.nan], [np.inf], [-0.0, 0.0]):
        with pytest.raises(F.FidgetHipError) as err:
            F.mesh_slices(cube, zs)
        assert err.value.status == 6 and "strictly ascending" in str(err.value)
    with pytest.raises(F.FidgetHipError) as err:
        F.mesh_slices(cube, [-0.25], table_log2=1)
    assert err.value.status == 10 and "table is full" in str(err.value)
    with pytest.raises(F.FidgetHipError) as err:
        F.mesh_slices(cube, [-0.25], table_log2=33)
    assert err.value.status == 6
    tight = F.mesh_slices(cube, [-0.25], table_log2=3)          # 8 crossing edges in 8 slots
    check(tight, "after the refused calls, a full table")
    assert tight.counts["edge_slots"] == 8 and tight.counts["vertices"] == 8
