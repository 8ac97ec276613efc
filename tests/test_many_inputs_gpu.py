"""Tapes of more than 16 variables on the device: the trait-level evaluators bit for bit with the oracle, and renders and meshes - which
run the tape's bound tape (capi_bound.hpp) - equal to the oracle's render or mesh of the same function.  (The oracle's renders and
meshes bind at most 16 variables themselves, so its side of a render comparison is the model built with the values as constants:
prospero.vm itself for the prospero model.)"""
import numpy as np
import pytest

import fidget_amd as F
import oracle as O
from conftest import model_path
from test_gpu_parity import bench_camera
from test_many_inputs import prospero_with_vars, spheres

pytestmark = pytest.mark.gpu


def same_f32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


def sphere_vars(n_vars, seed=0):
    """centres in [-0.7, 0.7], radii in [0.1, 0.3]"""
    rng = np.random.default_rng(seed)
    return {i: float(np.float32(rng.uniform(0.1, 0.3) if i % 4 == 3 else rng.uniform(-0.7, 0.7))) for i in range(n_vars)}


def trans_model(M, n_vars, consts=None):
    """a blobby field with sin / cos / exp / atan2 of the variables and the axes"""
    c = M.Context()
    x, y, z = c.x(), c.y(), c.z()
    r = c.sub(c.add(c.add(c.square(x), c.square(y)), c.square(z)), c.constant(0.5))
    for i in range(n_vars):
        v = c.var(i) if consts is None else c.constant(consts[i])
        t = [c.sin(c.mul(x, v)), c.cos(c.mul(y, v)), c.exp(c.mul(z, v)), c.atan2(c.add(x, v), c.sub(y, v))][i % 4]
        r = c.add(r, c.mul(t, c.constant(0.01)))
    return c, r


def trans_vars(n_vars, seed=1):
    rng = np.random.default_rng(seed)
    return {i: float(np.float32(rng.uniform(-1.0, 1.0))) for i in range(n_vars)}


MODELS = {
    "spheres80": (lambda M, k=None: spheres(M, 80, consts=k), lambda: sphere_vars(80)),
    "trans24": (lambda M, k=None: trans_model(M, 24, consts=k), lambda: trans_vars(24)),
    "prospero40": (lambda M, k=None: prospero_with_vars(M, 40)[:2] if k is None else None, lambda: prospero_with_vars(F, 40)[2]),
}


def both(name):
    build, vals = MODELS[name]
    return F.Shape(*build(F)), O.Shape(*build(O)), vals()


def oracle_const(name, vals):
    """the oracle's shape of the same function with the values as constants"""
    if name == "prospero40":
        return O.Shape.from_vm(model_path("prospero.vm"))
    return O.Shape(*MODELS[name][0](O, vals))


# ---- trait-level evaluators ---------------------------------------------------------------------------------------------------
def slot_vectors(p, vals, rng, n):
    """n random points: per slot of the tape its value (axes random in [-1, 1], variables their value jittered)"""
    nv = p.var_count()
    out = np.zeros((n, nv), np.float32)
    for i in range(n):
        for a in range(3):
            out[i, p.axis_index(a)] = rng.uniform(-1, 1)
        for k, v in vals.items():
            out[i, p.var_index(k)] = np.float32(v * rng.uniform(0.9, 1.1))
    return out


@pytest.mark.parametrize("name", sorted(MODELS))
def test_evaluators_bit_for_bit(name):
    p, o, vals = both(name)
    assert p.var_count() > 16
    rng = np.random.default_rng(5)
    pts = slot_vectors(p, vals, rng, 64)
    batch = [[(float(v) - 0.05, float(v) + 0.05) for v in row] for row in pts]
    got = p.eval_interval_batch(batch)
    for b, (iv, tr) in zip(batch, got):
        (lo, hi), tr2 = o.eval_interval_batch([b])[0]
        assert same_f32([iv[0], iv[1]], [lo, hi])
        assert (tr is None) == (tr2 is None) and (tr is None or (tr == tr2).all())
        if tr is not None:        # simplify with the trace, as the oracle
            from test_host_frontend import canon_oracle, canon_product
            assert canon_product(p.simplify(tr)) == canon_oracle(o.simplify(tr))
    for row in pts[:16]:
        a, ta = p.eval_point_raw(row.tolist())
        b, tb = o.eval_point_raw(row.tolist())
        assert same_f32(a, b) and ((ta is None) == (tb is None)) and (ta is None or (ta == tb).all())
    cols = [pts[:, s].copy() for s in range(pts.shape[1])]
    assert same_f32(p.eval_float_slice_raw(cols), o.eval_float_slice_raw(cols))
    grads = []
    for s in range(pts.shape[1]):
        g = np.zeros((len(pts), 4), np.float32)
        g[:, 0] = pts[:, s]
        if s in [p.axis_index(a) for a in range(3)]:
            g[:, 1 + [p.axis_index(a) for a in range(3)].index(s)] = 1.0
        grads.append(g.reshape(-1))
    assert same_f32(p.eval_grad_slice_raw(grads), o.eval_grad_slice_raw(grads))


def test_evaluators_on_bytecode_with_slots_up_to_302():
    oc, orr = spheres(O, 300, axes_last=True)
    o = O.Shape(oc, orr)
    words, _, _ = o.bytecode()
    p = F.Shape.from_bytecode(words, axis_slots=[o.axis_index(a) for a in range(3)])
    assert p.var_count() == 303
    rng = np.random.default_rng(8)
    pts = rng.uniform(-1, 1, (200, 303)).astype(np.float32)
    cols = [pts[:, s].copy() for s in range(303)]
    assert same_f32(p.eval_float_slice_raw(cols), o.eval_float_slice_raw(cols))
    for row in pts[:8]:
        a, ta = p.eval_interval_raw([(float(v), float(v) + 0.01) for v in row])
        b, tb = o.eval_interval_raw([(float(v), float(v) + 0.01) for v in row])
        assert same_f32(a, b) and ((ta is None) == (tb is None)) and (ta is None or (ta == tb).all())


# ---- renders and meshes -------------------------------------------------------------------------------------------------------
def rotated():
    return bench_camera(0.0)


def same_3d(a, b):
    assert b["depth"].max() > 0
    assert (a["depth"] == b["depth"]).all(), f"{(a['depth'] != b['depth']).sum()} depths differ"
    assert same_f32(a["normal"], b["normal"]), "normals differ"


@pytest.mark.parametrize("name", sorted(MODELS))
def test_render2d_equals_oracle(name):
    p, _, vals = both(name)
    m = np.array([[0.8, -0.6, 0.05], [0.6, 0.8, -0.1], [0, 0, 1]], np.float32)
    a = F.render2d(p, 512, vars=vals, world_to_model=m)[0]
    b = O.render2d(oracle_const(name, vals), 512, world_to_model=m, tile_sizes=F.HIP_TILES_2D)[0]
    assert same_f32(a, b)


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("persp", [0.0, 0.3])
def test_render3d_equals_oracle(name, persp):
    p, _, vals = both(name)
    m = bench_camera(persp)
    same_3d(F.render3d(p, 256, vars=vals, world_to_model=m)[0], O.render3d(oracle_const(name, vals), 256, world_to_model=m)[0])


def test_prospero_with_variables_renders_as_prospero():
    """prospero.vm with 40 constants as variables bound to the same values: its image is prospero's own"""
    p, _, vals = both("prospero40")
    ref = F.Shape.from_vm(model_path("prospero.vm"))
    assert (F.render2d(p, 512, vars=vals)[0].view(np.uint32) == F.render2d(ref, 512)[0].view(np.uint32)).all()
    same_3d(F.render3d(p, 256, vars=vals)[0], F.render3d(ref, 256)[0])


def test_render3d_block_merged_and_shard():
    import torch
    p, _, vals = both("spheres80")
    m = rotated()
    b = O.render3d(oracle_const("spheres80", vals), 256, world_to_model=m)[0]
    parts = []
    for i in range(8):
        t = torch.zeros((256, 256, 4), dtype=torch.int32, device="cuda")
        F.render3d(p, 256, vars=vals, world_to_model=m, out=t, block=(i, (2, 2, 2)))
        parts.append(t)
    torch.cuda.synchronize()
    p.hip.sync()
    for col in range(4):          # (block col + 4: the front half of the column's z range; outside its columns a block is all zeros)
        F.merge_depth(parts[col + 4], parts[col], 256, hip=p.hip)
    p.hip.sync()
    full = parts[4] + parts[5] + parts[6] + parts[7]
    torch.cuda.synchronize()
    a = full.cpu().numpy().view(np.uint32).reshape(256, 256, 4)
    assert (a[:, :, 3] == b["depth"]).all()
    assert same_f32(a[:, :, :3].copy().view(np.float32), b["normal"])
    shards = [F.render3d(p, 256, vars=vals, world_to_model=m, shard=s, n_shards=2)[0] for s in range(2)]
    d = np.maximum(shards[0]["depth"], shards[1]["depth"])
    assert (d == b["depth"]).all()


@pytest.mark.parametrize("name", ["spheres80", "trans24"])
def test_mesh_equals_oracle(name):
    p, _, vals = both(name)
    m = rotated()
    tris, verts, _ = F.mesh(p, 7, world_to_model=m, vars=vals)
    t, v = O.Octree(oracle_const(name, vals), 7, world_to_model=m).walk_dual()
    t, v = np.asarray(t, np.uint64).reshape(-1, 3), np.asarray(v, np.float32).reshape(-1, 3)
    assert len(t) > 100 and tris.shape == t.shape and verts.shape == v.shape
    assert (tris == t).all() and same_f32(verts, v)


def test_queued_frames_with_changing_values():
    """more asynchronous frames than the context's four buffer sets, each with other values, then one sync: every frame is the
    oracle's (a set holds the bound tape its frame reads until that frame is over)"""
    import torch
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    p = F.Shape(*spheres(F, 80), hip=hip)
    frames = [sphere_vars(80, seed=10 + k) for k in range(12)]
    outs = [torch.zeros((128, 128, 4), dtype=torch.int32, device="cuda") for _ in frames]
    outs2d = [torch.zeros((256, 256), dtype=torch.float32, device="cuda") for _ in frames]
    for k, vals in enumerate(frames):
        F.render3d(p, 128, vars=vals, out=outs[k])
        F.render2d(p, 256, vars=vals, out=outs2d[k])
    torch.cuda.synchronize()
    hip.sync()
    for k, vals in enumerate(frames):
        o = oracle_const("spheres80", vals)
        b = O.render3d(o, 128)[0]
        a = outs[k].cpu().numpy().view(np.uint32).reshape(128, 128, 4)
        assert (a[:, :, 3] == b["depth"]).all(), f"frame {k}"
        assert same_f32(a[:, :, :3].copy().view(np.float32), b["normal"])
        b2 = O.render2d(o, 256, tile_sizes=F.HIP_TILES_2D)[0]
        assert same_f32(outs2d[k].cpu().numpy(), b2), f"2D frame {k}"


def test_missing_variable_of_many():
    p = F.Shape(*spheres(F, 80))
    vals = sphere_vars(80)
    del vals[57]
    with pytest.raises(ValueError, match="MissingVar"):
        F.render2d(p, 64, vars=vals)
    with pytest.raises(ValueError, match="MissingVar"):
        F.render3d(p, 64, vars=vals)
    with pytest.raises(Exception):
        F.mesh(p, 3, vars=vals)
    vals[57] = 0.2
    vals[1000] = 3.0          # a key the tape does not read: ignored
    F.render2d(p, 64, vars=vals)
