"""fhip_triangles_topology and fhip_mesh_topology on the device against mesh_topology_ref.py.  Every integer output - the counts, the
vertices' bits, the triangles, a shell per triangle, the integer and bound columns of the shells, the four edge lists - is compared with
np.array_equal / ==; the two float64 columns against math.fsum within the bound of any order of summation.  The meshes: the hand
meshes of test_mesh_topology.py, tetrahedra on a lattice whole, thinned and cut short at the block's edges, the boundary meshes of
bitmaps indexed, as the soup of their STL file and from the Mesh's resident arrays; inputs on the device; two runs and a shuffle;
tables at load factor near 1 and one size too small; the cross-checks of voxelize_mesh, Voxels.mesh and build_mesh; refused calls."""
import functools

import numpy as np
import pytest
from conftest import model_path

import fidget_amd as F
import mesh_topology_ref as MT
import oracle as O
import voxels_ref as V
from test_mesh import sphere
from test_mesh_topology import bitmaps, hand_meshes, lattice_tetrahedra, pow2_at_least, signed_zeros, soup, tetrahedron, thinned

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def gamma(n):
    """|computed sum - exact sum| <= gamma(n) sum |term| for n terms added in any order (Higham, Accuracy and Stability, 4.2)"""
    return n * U / (1 - n * U)


@functools.lru_cache(maxsize=None)
def _torch():
    import torch
    return torch


def check(got, want, name=""):
    """a Topology against the reference's dict: every integer equal, the float columns within their bounds"""
    assert {k: got.counts[k] for k in MT.COUNTS} == want["counts"], name
    assert got.closed == MT.closed(want) and got.manifold == MT.manifold(want) and got.euler == MT.euler(want)
    assert got.vertices.dtype == np.float32 and np.array_equal(got.vertices.view(np.uint32), want["vertices"].view(np.uint32)), name
    assert got.triangles.dtype == np.uint64 and np.array_equal(got.triangles, want["triangles"]), name
    assert got.triangle_shell.dtype == np.uint32 and np.array_equal(got.triangle_shell, want["triangle_shell"]), name
    s, w = got.shells, want["shells"]
    for col in ("triangles", "first", "unbalanced"):
        assert s[col].dtype == w[col].dtype and np.array_equal(s[col], w[col]), (name, col)
    for col in ("lo", "hi"):
        assert np.array_equal(s[col].view(np.uint32), w[col].view(np.uint32)), (name, col)
    for kind in MT.KINDS:
        e = got.edges(kind)
        assert e.dtype == np.uint32 and e.shape == (want["counts"][kind], 2) and np.array_equal(e, want["edges"][kind]), (name, kind)
    n = w["triangles"].astype(np.float64)
    err_v, err_a = np.abs(s["volume6"] - w["volume6"]), np.abs(s["area2"] - w["area2"])
    bound_v, bound_a = gamma(n) * w["volume6_abs"], gamma(n) * w["area2_abs"] + 2.0 ** -52 * w["area2_abs"]          # (a device sqrt within 1 ulp)
    print(f"{name}: volume6 error / bound {np.max(err_v / np.maximum(bound_v, 1e-300), initial=0):.3g}, area2 {np.max(err_a / np.maximum(bound_a, 1e-300), initial=0):.3g}")
    assert np.all(err_v <= bound_v) and np.all(err_a <= bound_a), name
    assert abs(got.volume - sum(w["volume6"]) / 6) <= (gamma(len(n) + 1) * sum(np.abs(w["volume6"])) + sum(bound_v)) / 6
    assert abs(got.area - sum(w["area2"]) / 2) <= (gamma(len(n) + 1) * sum(w["area2"]) + sum(bound_a)) / 2


# ---- every integer output equal to the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hand_meshes()))
def test_hand_meshes(name):
    v, t, weld = hand_meshes()[name]
    got = F.mesh_topology(v if t is None else (v, t), weld=weld)
    check(got, MT.topology(v, t, weld), name)
    if name == "nested cubes":
        assert got.shells["volume6"].tolist() == [48.0, -6.0] and got.volume == 7.0 and got.area == 30.0
    if name in ("nothing", "no soup"):
        assert got.vertices_device() is None and got.triangles.shape == (0, 3) and got.volume == 0.0


@functools.lru_cache(maxsize=None)
def tets():
    return lattice_tetrahedra(300)          # 1200 triangles


@pytest.mark.parametrize("thin", [False, True])
@pytest.mark.parametrize("n", [1200, 257, 256, 255, 1, 0])
def test_lattice_tetrahedra(n, thin):
    """3600 corners are several blocks; 255, 256 and 257 triangles end a block of 256 lanes before, at and after its last lane"""
    tris = (thinned(tets()) if thin else tets())[:n]
    want = MT.topology(tris)
    check(F.mesh_topology(tris), want, f"{n} {thin}")
    if n > 1:          # ... and indexed, welded or not, from the reference's own indexed mesh
        pair = (want["vertices"], want["triangles"])
        check(F.mesh_topology(pair), MT.topology(*pair), f"{n} {thin} indexed")
        check(F.mesh_topology(pair, weld=True), MT.topology(*pair, True), f"{n} {thin} indexed, welded")


@functools.lru_cache(maxsize=None)
def voxel_case(name):
    """-> (Voxels, its boundary Mesh): the bitmaps of test_mesh_topology.py at depth 1, gyroid-sphere voxelized at depth 3"""
    if name == "gyroid":
        vox = F.voxelize(F.Shape.from_vm(model_path("gyroid-sphere.vm")), 3)
    else:
        vox = F.Voxels(F.default_context(), V.pack(bitmaps()[name]), 1, None)
    return vox, vox.mesh()


@pytest.mark.parametrize("name", ["touching", "sparse", "dense", "gyroid"])
def test_boundary_meshes_three_ways(name):
    vox, m = voxel_case(name)
    euler = vox.surface().euler
    want = MT.topology(m.vertices, m.triangles)
    assert m.vertices_device() is not None
    by_handle, by_pair = m.topology(), F.mesh_topology((m.vertices, m.triangles))
    for got in (by_handle, by_pair):
        check(got, want, name)
        assert got.closed and got.counts["boundary"] == 0 and got.euler == euler
    tris = F.read_stl(m.stl())
    got = F.mesh_topology(tris)
    check(got, MT.topology(tris), name + ", soup")
    assert got.closed and got.counts["boundary"] == 0 and got.euler == euler
    assert {k: got.counts[k] for k in MT.COUNTS} == {k: by_pair.counts[k] for k in MT.COUNTS}          # a voxel mesh has no two vertices in one place
    if name == "touching":
        assert (got.counts["vertices"], got.counts["edges"], got.counts["nonmanifold"], got.counts["shells"], got.euler) == (14, 35, 1, 1, 3)
    if name == "gyroid":
        assert got.counts["triangles"] > 3000 and got.volume * (32 ** 3 / 8) == vox.n          # every term a multiple of 2^-15: the sums are exact


# ---- inputs on the device, views of the results ----------------------------------------------------------------------------------------------
def same(a, b):
    assert a.counts == b.counts
    assert np.array_equal(a.vertices.view(np.uint32), b.vertices.view(np.uint32)) and np.array_equal(a.triangles, b.triangles) and np.array_equal(a.triangle_shell, b.triangle_shell)
    for col in ("triangles", "first", "unbalanced", "lo", "hi"):
        assert np.array_equal(a.shells[col], b.shells[col]), col
    for kind in MT.KINDS:
        assert np.array_equal(a.edges(kind), b.edges(kind)), kind


def test_inputs_on_the_device_and_views_of_the_results():
    torch = _torch()
    tris = thinned(tets())
    host = F.mesh_topology(tris)
    dev = F.mesh_topology(torch.from_numpy(tris).cuda())
    same(host, dev)
    pair = (host.vertices, host.triangles)
    pair_host = F.mesh_topology(pair)
    pair_dev = F.mesh_topology((torch.from_numpy(pair[0]).cuda(), torch.from_numpy(pair[1].astype(np.int64)).cuda()))
    same(pair_host, pair_dev)
    for t in (dev, pair_dev):
        assert np.array_equal(torch.as_tensor(t.vertices_device(), device="cuda").cpu().numpy().view(np.uint32), t.vertices.view(np.uint32))
        iface = dict(t.triangles_device().__cuda_array_interface__, typestr="<i8")
        holder = type("A", (), {"__cuda_array_interface__": iface})()
        assert np.array_equal(torch.as_tensor(holder, device="cuda").cpu().numpy().view(np.uint64), t.triangles)
        iface = dict(t.triangle_shell_device().__cuda_array_interface__, typestr="<i4")
        holder = type("A", (), {"__cuda_array_interface__": iface})()
        assert np.array_equal(torch.as_tensor(holder, device="cuda").cpu().numpy().view(np.uint32), t.triangle_shell)
        for kind in MT.KINDS:
            e = t.edges(kind, device=True)
            assert e.is_cuda and np.array_equal(e.cpu().numpy().view(np.uint32), t.edges(kind))


# ---- run to run ------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_a_shuffle_give_the_same_integers():
    tris = thinned(tets())
    a, b = F.mesh_topology(tris), F.mesh_topology(tris)
    same(a, b)
    order = np.random.default_rng(2).permutation(len(tris))
    c = F.mesh_topology(tris[order])
    check(c, MT.topology(tris[order]), "shuffled")
    assert {k: c.counts[k] for k in MT.COUNTS} == {k: a.counts[k] for k in MT.COUNTS}
    # mapped back: the same partition into shells, the same rows for the same shells
    shell_a, shell_c = a.triangle_shell[order], c.triangle_shell
    assert np.array_equal(shell_a == MT.NO_SHELL, shell_c == MT.NO_SHELL)
    live = shell_c != MT.NO_SHELL
    to_a = np.full(c.counts["shells"], -1, np.int64)
    to_a[shell_c[live]] = shell_a[live]
    assert np.array_equal(to_a[shell_c[live]], shell_a[live]) and len(np.unique(to_a)) == a.counts["shells"]
    for col in ("triangles", "unbalanced", "lo", "hi"):
        assert np.array_equal(c.shells[col], a.shells[col][to_a]), col
    # the welded vertices are the same points
    assert sorted(map(tuple, c.vertices.tolist())) == sorted(map(tuple, a.vertices.tolist()))


# ---- table_log2 ---------------------------------------------------------------------------------------------------------------------------------
def test_tables_at_load_factor_near_one_and_one_size_too_small():
    hip = F.default_context()
    tris = tets()
    want = MT.topology(tris)
    n_v, n_e = want["counts"]["vertices"], want["counts"]["edges"]
    assert n_v == 125 and n_e > 256
    tight = pow2_at_least(n_e)          # the least power of two at or above the edges: the vertices fit too
    got = F.mesh_topology(tris, table_log2=tight)
    check(got, want, "tight")
    assert got.counts["vertex_slots"] == got.counts["edge_slots"] == 1 << tight and n_e / (1 << tight) > 0.5
    pair = (want["vertices"], want["triangles"])
    got = F.mesh_topology(pair, table_log2=tight)
    check(got, MT.topology(*pair), "tight, indexed")
    assert got.counts["vertex_slots"] == 0
    # the 125 vertices in 128 slots: a load of 0.98 - the edges, indexed, need their own size
    v7 = F.mesh_topology(tris[:40], table_log2=pow2_at_least(max(MT.topology(tris[:40])["counts"][k] for k in ("vertices", "edges"))))
    check(v7, MT.topology(tris[:40]), "tight, 40")
    for mesh, log2 in ((tris, 6), (tris, tight - 1), (pair, tight - 1)):
        with pytest.raises(F.FidgetHipError) as err:
            F.mesh_topology(mesh, table_log2=log2)
        assert err.value.status == 10 and "Overflow" in str(err.value) and "table is full" in str(err.value)
        check(F.mesh_topology(tetrahedron()), MT.topology(*tetrahedron()), "after an overflow")          # the context works on
    hip.sync()


def test_the_scratch_is_the_contexts_and_a_result_outlives_a_trim():
    """the tables and the per-corner arrays live in the context's buffer: fhip_ctx_trim gives them back, a result made before - its
    arrays are its own - still answers, and the next call makes its scratch anew"""
    hip = F.default_context()
    tris = thinned(tets())
    want = MT.topology(tris)
    before = F.mesh_topology(tris)
    hip.check(F.lib().fhip_ctx_trim(hip._h))
    check(before, want, "made before the trim")          # the arrays are read only now
    check(F.mesh_topology(tris), want, "made after the trim")


# ---- cross-checks of existing features ---------------------------------------------------------------------------------------------------------
def test_a_voxel_boundary_mesh_is_balanced_and_goes_back_into_voxelize_mesh():
    vox, m = voxel_case("gyroid")
    t = m.topology()
    assert t.counts["unbalanced"] == 0 and t.closed
    tris = F.read_stl(m.stl())
    welded = F.mesh_topology(tris)
    a = F.voxelize_mesh((welded.vertices, welded.triangles), 3)
    b = F.voxelize_mesh(tris, 3)
    assert np.array_equal(a.bricks, b.bricks) and np.array_equal(a.bricks, vox.bricks) and a.mesh_info == b.mesh_info
    torch = _torch()
    held = dict(welded.triangles_device().__cuda_array_interface__, typestr="<i8")
    on_device = (torch.as_tensor(welded.vertices_device(), device="cuda"), torch.as_tensor(type("A", (), {"__cuda_array_interface__": held})(), device="cuda"))
    c = F.voxelize_mesh(on_device, 3)
    assert np.array_equal(c.bricks, vox.bricks)


def test_build_mesh_of_a_sphere_against_the_reference_on_the_oracles_mesh():
    """Manifold dual contouring claims a manifold mesh.  The reference on the oracle's mesh of the same sphere, worked out without a
    device, says: closed and manifold, one shell, Euler number 2 - and the device must say what the reference says, whatever that is."""
    oc = O.Context()
    ot, ov = O.Octree(O.Shape(oc, sphere(oc, (0.0, 0.0, 0.0), 0.5)), 4).walk_dual()
    want = MT.topology(np.asarray(ov, np.float32).reshape(-1, 3), np.asarray(ot, np.uint64).reshape(-1, 3))
    c = F.Context()
    m = F.build_mesh(F.Shape(c, sphere(c, (0.0, 0.0, 0.0), 0.5)), 4)
    assert np.array_equal(m.triangles, np.asarray(ot, np.uint64).reshape(-1, 3)) and np.array_equal(m.vertices.view(np.uint32), np.asarray(ov, np.float32).reshape(-1, 3).view(np.uint32))
    got = m.topology()
    check(got, want, "sphere 4")
    print("build_mesh(sphere, 4):", want["counts"], "closed", MT.closed(want), "manifold", MT.manifold(want), "euler", MT.euler(want))
    assert abs(got.volume - 4 / 3 * np.pi * 0.125) < 0.01 and abs(got.area - np.pi) < 0.05


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------------
def test_refused_calls():
    hip = F.default_context()
    v, t = tetrahedron()
    bad = v.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="3 of 4 triangles rejected"):
        F.mesh_topology((bad, t))
    far = t.copy()
    far[2, 0] = 4
    with pytest.raises(ValueError, match="1 of 4 triangles rejected"):
        F.mesh_topology((v, far))
    bad[3, 1] = -np.inf
    with pytest.raises(ValueError, match="3 of 4 triangles rejected"):
        F.mesh_topology(soup(bad, t))
    with pytest.raises(ValueError, match="welded"):
        F.mesh_topology(signed_zeros(), weld=False)
    L, C = F.lib(), __import__("ctypes")
    h = C.c_void_p()
    # the limits are decided on the numbers alone, before anything is read: 3 T <= 2^32 - 2 and, indexed, n_vertices <= 2^32 - 2
    assert L.fhip_triangles_topology(hip._h, F._p(v), 4, F._p(t), (2 ** 32 - 2) // 3 + 1, 0, 0, 0, C.byref(h)) == 10 and not h.value
    assert L.fhip_triangles_topology(hip._h, F._p(v), 2 ** 32 - 1, F._p(t), 4, 0, 0, 0, C.byref(h)) == 10 and not h.value
    assert L.fhip_triangles_topology(hip._h, F._p(v), 4, None, 1, 0, 0, 0, C.byref(h)) == 6 and not h.value          # a soup, not welded
    assert L.fhip_triangles_topology(hip._h, F._p(v), 4, F._p(t), 4, 0, 0, 33, C.byref(h)) == 6 and not h.value
    assert L.fhip_triangles_topology(hip._h, F._p(v), 4, F._p(t), 4, 0, 0, 0, None) == 5
    assert L.fhip_topology_edges(hip._h, None, 0, None, 0) == 5
    ok = F.mesh_topology((v, t))
    assert L.fhip_topology_edges(hip._h, ok._owner.h, 4, None, 0) == 6
    check(ok, MT.topology(v, t), "after the refused calls")
