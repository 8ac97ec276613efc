"""Mesh export on the device: fhip_mesh_stl against the numpy restatement of Mesh::write_stl (tests/stl_ref.py) byte for byte - from
resident arrays (context option mesh_keep_device) and from uploaded host arrays -, the packing kernel on triangle counts a mesh does not
give, fhip_mesh_vertex_grads against the oracle's gradient evaluator and the library's own, and the resident arrays through torch.

The tape whose register file exceeds LDS (tests/test_spills.py's 303 live values) cannot be meshed itself - fhip_mesh_build refuses
such a tape ("register file exceeds LDS") - so its gradients are taken at the vertices of a sphere's depth-3 mesh."""
import ctypes as C

import numpy as np
import pytest

import fidget_amd as F
import oracle as O
from conftest import model_path
from stl_ref import stl_bytes
from test_many_inputs import spheres
from test_many_inputs_gpu import same_f32, sphere_vars
from test_mesh import sphere
from test_spills import many_live_values

pytestmark = pytest.mark.gpu


def _sphere(M, r=0.5):
    c = M.Context()
    return M.Shape(c, sphere(c, (0.0, 0.0, 0.0), r))


def _var_sphere(M):
    c = M.Context()
    x, y, z = c.x(), c.y(), c.z()
    return M.Shape(c, c.sub(c.sqrt(c.add(c.add(c.square(x), c.square(y)), c.square(z))), c.var(7)))


BEAR_W2M = np.eye(4, dtype=np.float32)
BEAR_W2M[:2, 3] = 0.125          # bear.vm reaches x, y = 1 and stops at -0.75 (octree.rs:1532-1560): the region moved to [-0.875, 1.125]
# name -> (shape builder for either module, depth, world_to_model, vars)
CASES = {
    "sphere3": (_sphere, 3, None, None),
    "sphere5": (_sphere, 5, None, None),
    "gyroid-sphere5": (lambda M: M.Shape.from_vm(model_path("gyroid-sphere.vm")), 5, None, None),
    "colonnade5": (lambda M: M.Shape.from_vm(model_path("colonnade.vm")), 5, None, None),
    "bear5": (lambda M: M.Shape.from_vm(model_path("bear.vm")), 5, BEAR_W2M, None),
    "var-sphere4": (_var_sphere, 4, None, {7: 0.625}),
}
_built = {}


def built(name):
    """(shape, resident mesh, uploaded mesh): each case is built once, with keep_device on and off"""
    if name not in _built:
        make, depth, w2m, vars_ = CASES[name]
        s = make(F)
        _built[name] = (s, F.build_mesh(s, depth, world_to_model=w2m, vars=vars_, keep_device=True),
                        F.build_mesh(s, depth, world_to_model=w2m, vars=vars_, keep_device=False))
    return _built[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_stl_equals_the_restatement(name):
    make, depth, w2m, vars_ = CASES[name]
    s, on, off = built(name)
    tris, verts, _ = F.mesh(s, depth, world_to_model=w2m, vars=vars_)
    assert len(tris) > 0 and len(verts) > 0
    for m in (on, off):
        assert (m.triangles == tris).all() and (m.vertices.view(np.uint32) == verts.view(np.uint32)).all()
    assert on.vertices_device() is not None and on.triangles_device() is not None
    assert off.vertices_device() is None and off.triangles_device() is None
    ref = stl_bytes(verts, tris)
    for m in (on, off):
        got = m.stl()
        assert got.dtype == np.uint8 and len(got) == 84 + 50 * len(tris) == len(ref)
        bad = np.flatnonzero(got != ref)
        assert not len(bad), f"{len(bad)} bytes differ, the first at {bad[0]}"


def test_write_stl(tmp_path):
    _, on, _ = built("sphere3")
    p = tmp_path / "sphere.stl"
    on.write_stl(str(p))
    assert p.read_bytes() == stl_bytes(on.vertices, on.triangles).tobytes()


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 513, 1001])
def test_packing_on_counts_a_mesh_does_not_give(n):
    """one partial block, the block's edges, odd counts (the 16-bit tail), several blocks; 64 guard bytes behind the file stay as they were"""
    rng = np.random.default_rng(100 + n)
    n_verts = 97
    verts = rng.uniform(-1, 1, (n_verts, 3)).astype(np.float32)
    tris = rng.integers(0, n_verts, (n, 3)).astype(np.uint64)
    size = 84 + 50 * n
    out = np.full(size + 64, 0xA5, np.uint8)
    hip = F.default_context()
    hip.check(F.lib().fhip_debug_stl_pack(hip._h, F._p(verts), n_verts, F._p(tris), n, F._p(out)))
    assert (out[size:] == 0xA5).all(), "bytes behind the file were written"
    ref = stl_bytes(verts, tris)
    bad = np.flatnonzero(out[:size] != ref)
    assert not len(bad), f"{len(bad)} bytes differ, the first at {bad[0]}"


def test_an_empty_shape():
    c = F.Context()
    s = F.Shape(c, c.constant(1.0))
    for keep in (True, False):
        m = F.build_mesh(s, 3, keep_device=keep)
        assert len(m.triangles) == 0 and len(m.vertices) == 0
        assert (m.stl() == stl_bytes(m.vertices, m.triangles)).all() and len(m.stl()) == 84
        g = m.vertex_grads(s)
        assert g.shape == (0, 4) and g.dtype == np.float32
        s.hip.sync()


def test_device_output_and_resident_arrays():
    torch = pytest.importorskip("torch")
    s, on, off = built("gyroid-sphere5")
    hip = s.hip
    n_bytes, n_verts = 84 + 50 * len(on.triangles), len(on.vertices)
    for m in (on, off):
        stl = torch.full((n_bytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        grads = torch.zeros((n_verts, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert m.stl(out=stl) is stl and m.vertex_grads(s, out=grads) is grads
        hip.sync()
        assert (stl[:n_bytes].cpu().numpy() == m.stl()).all() and (stl[n_bytes:].cpu().numpy() == 0xA5).all()
        assert same_f32(grads.cpu().numpy(), m.vertex_grads(s))
    dv, dt = on.vertices_device(), on.triangles_device()
    assert dv.shape == (n_verts, 3) and dt.shape == (len(on.triangles), 3)
    tv = torch.as_tensor(dv, device="cuda")
    assert tv.data_ptr() == dv.ptr and (tv.cpu().numpy().view(np.uint32) == on.vertices.view(np.uint32)).all()
    ti = dict(dt.__cuda_array_interface__, typestr="<i8")       # (the indices as int64: every torch takes that)
    tt = torch.as_tensor(type("A", (), {"__cuda_array_interface__": ti, "_keep": dt})(), device="cuda")
    assert tt.data_ptr() == dt.ptr and (tt.cpu().numpy().astype(np.uint64) == on.triangles).all()
    assert off.vertices_device() is None and off.triangles_device() is None


def _grads_three_ways(mesh, fshape, oshape, vars_=None):
    v = mesh.vertices
    assert len(v) > 0
    got = mesh.vertex_grads(fshape, vars=vars_)
    assert got.shape == (len(v), 4) and got.dtype == np.float32
    want = oshape.eval_grad_slice(v[:, 0], v[:, 1], v[:, 2], vars_)
    own = fshape.eval_grad_slice(v[:, 0], v[:, 1], v[:, 2], vars_)
    assert same_f32(got, np.asarray(want).reshape(-1, 4)), "differs from the oracle's gradient evaluator"
    assert same_f32(got, np.asarray(own).reshape(-1, 4)), "differs from fhip_grad_eval"


@pytest.mark.parametrize("name", sorted(set(CASES) - {"sphere3"}))
def test_vertex_grads_equal_the_oracle_and_the_evaluator(name):
    make, depth, w2m, vars_ = CASES[name]
    s, on, off = built(name)
    o = make(O)
    _grads_three_ways(on, s, o, vars_)
    assert same_f32(off.vertex_grads(s, vars=vars_), on.vertex_grads(s, vars=vars_))      # (uploaded vertices: the same result)


def test_vertex_grads_of_a_tape_with_more_than_16_inputs():
    vals = sphere_vars(80)
    s, o = F.Shape(*spheres(F, 80)), O.Shape(*spheres(O, 80))
    assert s.var_count() > 16
    m = F.build_mesh(s, 4, vars=vals)
    _grads_three_ways(m, s, o, vals)


def test_vertex_grads_with_the_register_file_in_global_memory():
    s, o = many_live_values(F), many_live_values(O)
    assert s.slot_count() * 64 * 16 > 160 * 1024
    _, on, off = built("sphere3")
    assert len(on.vertices) > 64        # (more than one block)
    _grads_three_ways(on, s, o)
    assert same_f32(off.vertex_grads(s), on.vertex_grads(s))


def test_errors():
    s, on, _ = built("sphere3")
    c = F.Context()
    two = F.Shape(c, roots=[c.x(), c.y()])
    with pytest.raises(F.FidgetHipError) as e:
        on.vertex_grads(two)
    assert e.value.status == 5          # FHIP_ERR_BAD_TAPE
    vs, von, _ = built("var-sphere4")
    with pytest.raises(ValueError, match="MissingVar"):        # as F.mesh / fhip_mesh_build report it
        F.mesh(vs, 4)
    with pytest.raises(ValueError, match="MissingVar"):
        von.vertex_grads(vs)
