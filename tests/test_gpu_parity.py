"""GPU parity: the HIP renderers (through the C ABI) against the CPU oracle on the same inputs.

Bar (north star): interval pruning decisions and occupancy bit-exact, f32 values within 1 ulp.
For models without transcendentals (prospero, hi, colonnade, quarter) EVERYTHING is compared
bit for bit (pixels, fills incl. their recursion level, depth, normals)."""
import os

import numpy as np
import pytest

import fidget_amd as F
import oracle as O
from conftest import model_path, ROOT

pytestmark = pytest.mark.gpu


def both(name):
    return F.Shape.from_vm(model_path(name)), O.Shape.from_vm(model_path(name))


def same_bits_f32(a, b):
    a, b = a.view(np.uint32), b.view(np.uint32)
    nan = (np.isnan(a.view(np.float32)) & np.isnan(b.view(np.float32)))
    return ((a == b) | nan | ((a.view(np.float32) == 0) & (b.view(np.float32) == 0))).all()  # +-0, NaN payload: float equality


@pytest.mark.parametrize("name,size", [("hi.vm", 256), ("prospero.vm", 256), ("prospero.vm", 1024), ("quarter.vm", 128),
                                       ("prospero.vm", 100), ("colonnade.vm", 200),
                                       ("prospero.vm", 4096)])   # 4096: BASELINE.json configuration 2 at full size
def test_render2d_bit_exact(name, size):
    """the HIP shape's own 2D hint (128 / 16, fidget-jit's: 64 children per parent, the split tile stage with the assembly
    kernels) and the VM shape's (128 / 32 / 8: 16 children, the one-kernel tile stage), each against the oracle with the same
    tile sizes - fills carry the level they were decided at"""
    p, o = both(name)
    for ts in (None, F.VM_TILES_2D):
        a = F.render2d(p, size, tile_sizes=ts)[0]
        b = O.render2d(o, size, tile_sizes=ts or F.HIP_TILES_2D)[0]
        assert a.shape == b.shape
        assert same_bits_f32(a, b), f"{ts}: {(a.view(np.uint32) != b.view(np.uint32)).sum()} pixels differ"
        assert (F.pixel_fill_depth(a) == O.pixel_fill_depth(b)).all()


def test_render2d_pixel_perfect_and_rect():
    p, o = both("prospero.vm")
    for ts in (None, F.VM_TILES_2D):
        a = F.render2d(p, 192, 128, pixel_perfect=True, tile_sizes=ts)[0]
        b = O.render2d(o, 192, 128, pixel_perfect=True, tile_sizes=ts or F.HIP_TILES_2D)[0]
        assert same_bits_f32(a, b)
        a = F.render2d(p, 200, 136, tile_sizes=ts)[0]
        b = O.render2d(o, 200, 136, tile_sizes=ts or F.HIP_TILES_2D)[0]
        assert same_bits_f32(a, b)


@pytest.mark.parametrize("name,size", [("prospero.vm", 128), ("prospero.vm", 256), ("colonnade.vm", 128), ("colonnade.vm", 256),
                                       ("tanglecube.vm", 64)])
def test_render3d_bit_exact(name, size):
    p, o = both(name)
    a = F.render3d(p, size)[0]
    b = O.render3d(o, size)[0]
    assert (a["depth"] == b["depth"]).all(), f"{(a['depth'] != b['depth']).sum()} depths differ"
    assert same_bits_f32(a["normal"], b["normal"])


def test_render3d_headline_config_full_size():
    """BASELINE.json's metric configuration itself: prospero.vm at 1024^3, bit for bit against the oracle
    (0.7 s on the GPU box's host cores), plus what must hold at any size: the image does not change from
    one frame to the next (resident tapes, recycled arena), saturated columns carry (D, [0, 0, 1])
    (voxel.rs:536-542), and the two halves of a two-way shard are disjoint and sum to the image."""
    n = 1024
    p, o = both("prospero.vm")
    a = F.render3d(p, n)[0]
    b = O.render3d(o, n)[0]
    assert (a["depth"] == b["depth"]).all(), f"{(a['depth'] != b['depth']).sum()} depths differ"
    assert same_bits_f32(a["normal"], b["normal"])
    again = F.render3d(p, n)[0]
    assert (again["depth"] == a["depth"]).all() and same_bits_f32(again["normal"], a["normal"])
    sat = a["depth"] == n
    assert sat.any() and (a["normal"][sat] == np.array([0, 0, 1], np.float32)).all()
    halves = [F.render3d(p, n, shard=r, n_shards=2)[0] for r in (0, 1)]
    h0, h1 = (h.view(np.uint32).reshape(n, n, 4) for h in halves)
    assert not ((h0 != 0).any(axis=2) & (h1 != 0).any(axis=2)).any()
    assert ((h0 + h1) == a.view(np.uint32).reshape(n, n, 4)).all()




@pytest.mark.parametrize("size", [64, 128, 256, 512])   # 512: BASELINE.json configuration 3 at full size
def test_render3d_bear(size):
    # transcendental opcodes (exp / ln / sin / cos): the device runs the host libm's routines (trans_libm.hpp), so the normals are the
    # oracle's bit for bit like everything else (until round 4 the device rounded once from f64: up to 7.2 ulp of the gradient's scale)
    p, o = both("bear.vm")
    a = F.render3d(p, size)[0]
    b = O.render3d(o, size)[0]
    nd = int((a["depth"] != b["depth"]).sum())
    assert nd == 0, f"{nd} depths differ"
    ne = int((a["normal"].view(np.uint32) != b["normal"].view(np.uint32)).sum())
    assert ne == 0, f"{ne} normal components differ"


@pytest.mark.gpu
@pytest.mark.parametrize("arena_mb", [2, 8])
def test_render3d_survives_a_full_tape_arena(arena_mb):
    """When the tape arena runs out the children keep their parent's tape (no pruning): slower, same
    image.  Runs in a fresh process because the arena size is read when the context is created."""
    import subprocess, sys, textwrap
    code = textwrap.dedent(f"""
        import os, sys
        sys.path.insert(0, {ROOT!r})
        os.environ["FHIP_ARENA_MB"] = "{arena_mb}"
        import numpy as np, fidget_amd as F, oracle as O
        m = os.path.join({ROOT!r}, "models", "prospero.vm")
        a = F.render3d(F.Shape.from_vm(m), 256)[0]
        b = O.render3d(O.Shape.from_vm(m), 256)[0]
        assert (a["depth"] == b["depth"]).all() and (a["normal"].view(np.uint32) == b["normal"].view(np.uint32)).all()
        c = F.default_context().counters()
        print("overflows", c["arena_overflow"] if c else "?")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_cancel_token():
    """render/config.rs:38-80 CancelToken: a cancelled context refuses to render (the reference returns
    None), and renders again once reset; non-rectangular volumes and larger-than-slab counts still work."""
    hip = F.HipContext(0)
    s = F.Shape.from_vm(model_path("hi.vm"), hip=hip)
    hip.cancel()
    with pytest.raises(F.FidgetHipError) as e:
        F.render3d(s, 64)
    assert "cancel" in str(e.value).lower()
    with pytest.raises(F.FidgetHipError):
        F.render2d(s, 64)
    hip.cancel_reset()
    a = F.render3d(s, 64)[0]
    b = O.render3d(O.Shape.from_vm(model_path("hi.vm")), 64)[0]
    assert (a["depth"] == b["depth"]).all()


@pytest.mark.gpu
def test_cancel_flag_of_the_caller():
    """fhip_cancel_watch: the context reads a one-byte flag of the caller's beside its own - fidget_core's CancelToken is an
    Arc<AtomicBool> whose address the Rust crate passes for the duration of a render (rust/fidget-hip/src/render.rs Watch; voxel.rs:573-590
    cancel_render).  Set: the render refuses; cleared, or no longer watched: it renders the oracle's image."""
    hip = F.HipContext(0)
    s = F.Shape.from_vm(model_path("hi.vm"), hip=hip)
    flag = np.zeros(1, np.uint8)
    hip.cancel_watch(flag)
    want = O.render3d(O.Shape.from_vm(model_path("hi.vm")), 64)[0]
    assert (F.render3d(s, 64)[0]["depth"] == want["depth"]).all()
    flag[0] = 1
    with pytest.raises(F.FidgetHipError) as e:
        F.render3d(s, 64)
    assert "cancel" in str(e.value).lower()
    with pytest.raises(F.FidgetHipError):
        F.render2d(s, 64)
    hip.cancel_watch(None)
    assert (F.render3d(s, 64)[0]["depth"] == want["depth"]).all()
    hip.cancel_watch(flag)
    flag[0] = 0
    assert (F.render3d(s, 64)[0]["depth"] == want["depth"]).all()
    hip.cancel_watch(None)


@pytest.mark.gpu
@pytest.mark.parametrize("whd", [(200, 120, 300), (96, 256, 64), (33, 47, 129)])
def test_render3d_non_cubic(whd):
    w, h, d = whd
    p, o = both("colonnade.vm")
    a = F.render3d(p, w, h, d)[0]
    b = O.render3d(o, w, h, d)[0]
    assert a.shape == b.shape == (h, w)
    assert (a["depth"] == b["depth"]).all(), f"{(a['depth'] != b['depth']).sum()} depths differ"
    assert same_bits_f32(a["normal"], b["normal"])


@pytest.mark.gpu
def test_render3d_without_tape_groups():
    """The root level as one tape (FHIP_NO_TAPE_GROUPS=1; the default splits it, see test_groups.py): same image."""
    import subprocess, sys, textwrap
    code = textwrap.dedent(f"""
        import os, sys
        sys.path.insert(0, {ROOT!r})
        os.environ["FHIP_NO_TAPE_GROUPS"] = "1"
        import numpy as np, fidget_amd as F, oracle as O
        m = os.path.join({ROOT!r}, "models", "prospero.vm")
        for n in (128, 256):
            a = F.render3d(F.Shape.from_vm(m), n)[0]
            b = O.render3d(O.Shape.from_vm(m), n)[0]
            assert (a["depth"] == b["depth"]).all() and (a["normal"].view(np.uint32) == b["normal"].view(np.uint32)).all(), n
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- rotated and projective cameras (shape/mod.rs:906-946 Transformable: every row divided by row 3) ----------------
def bench_camera(perspective=0.3):
    """world_to_model of the reference's own voxel benchmark (fidget/benches/voxel.rs:6-53):
    roll(30 deg about z) * pitch(60 deg about x) * scale(1 / 0.7) * camera with `perspective` at (3, 2)"""
    def rot(axis, deg):
        c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
        m = np.eye(4)
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
        return m
    cam = np.eye(4)
    cam[3, 2] = perspective
    return (rot(2, 30) @ rot(0, 60) @ np.diag([1 / 0.7, 1 / 0.7, 1 / 0.7, 1.0]) @ cam).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("model,size,persp", [("colonnade.vm", 256, 0.3), ("colonnade.vm", 200, 0.0), ("prospero.vm", 256, 0.3),
                                              ("prospero.vm", 512, 0.15), ("tanglecube.vm", 128, 0.5)])
def test_render3d_rotated_and_perspective(model, size, persp):
    """non-diagonal and projective world_to_model through the whole device path (interval transform, the assembly leaf
    interpreter's divide-by-w, gradients): depth and normals bit-exact (no transcendental opcode in these models)"""
    p, o = both(model)
    m = bench_camera(persp)
    a = F.render3d(p, size, world_to_model=m)[0]
    b = O.render3d(o, size, world_to_model=m)[0]
    assert b["depth"].max() > 0 and (b["depth"] == 0).any()
    assert (a["depth"] == b["depth"]).all(), f"{(a['depth'] != b['depth']).sum()} depths differ"
    same = (a["normal"] == b["normal"]) | (np.isnan(a["normal"]) & np.isnan(b["normal"]))
    assert same.all(), f"{(~same).any(axis=2).sum()} normals differ"


@pytest.mark.gpu
def test_render3d_reference_bench_camera_full_size():
    """the reference benchmark's own configuration: colonnade.vm at 1024^3 under the perspective camera"""
    p, o = both("colonnade.vm")
    m = bench_camera(0.3)
    a = F.render3d(p, 1024, world_to_model=m)[0]
    b = O.render3d(o, 1024, world_to_model=m)[0]
    assert (a["depth"] == b["depth"]).all()
    assert ((a["normal"] == b["normal"]) | (np.isnan(a["normal"]) & np.isnan(b["normal"]))).all()


@pytest.mark.gpu
def test_render3d_frames_in_flight():
    """Asynchronous renders are pipelined across frames (four buffer sets per context, the coarse levels of frame n + 1
    beside the slabs of frame n): a queue of frames of different shapes, sizes and cameras, nothing waited for in between,
    gives the images the oracle gives, every one of them; a synchronous render in the middle of the queue as well."""
    import torch
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    jobs = [("prospero.vm", 512, None), ("colonnade.vm", 256, bench_camera(0.3)), ("prospero.vm", 512, None), ("tanglecube.vm", 128, None),
            ("colonnade.vm", 512, None), ("prospero.vm", 256, bench_camera(0.15)), ("prospero.vm", 1024, None), ("prospero.vm", 1024, None),
            ("colonnade.vm", 256, None)]
    shapes = {m: F.Shape.from_vm(model_path(m), hip=hip) for m, _, _ in jobs}
    outs = [torch.zeros((n, n, 4), dtype=torch.int32, device="cuda") for _, n, _ in jobs]
    mid = None
    for rep in range(2):           # the second round reuses both sets with every buffer already sized
        for i, (m, n, cam) in enumerate(jobs):
            F.render3d(shapes[m], n, world_to_model=cam, out=outs[i])
            if rep == 1 and i == 4:
                mid = F.render3d(shapes["tanglecube.vm"], 64)[0]       # host output: waits for its own frame only
    torch.cuda.synchronize()
    hip.sync()
    oshape = {m: O.Shape.from_vm(model_path(m)) for m in shapes}
    for i, (m, n, cam) in enumerate(jobs):
        b = O.render3d(oshape[m], n, world_to_model=cam)[0]
        a = outs[i].cpu().numpy().view(np.uint32).reshape(n, n, 4)
        assert (a[:, :, 3] == b["depth"]).all(), f"frame {i} ({m} {n}): {(a[:, :, 3] != b['depth']).sum()} depths differ"
        an = a[:, :, :3].copy().view(np.float32)
        assert ((an == b["normal"]) | (np.isnan(an) & np.isnan(b["normal"]))).all(), f"frame {i} ({m} {n}): normals differ"
    b = O.render3d(oshape["tanglecube.vm"], 64)[0]
    assert (mid["depth"] == b["depth"]).all() and same_bits_f32(mid["normal"], b["normal"])


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"FHIP_COLUMN_GROUP": "0"}, {"FHIP_COLUMN_GROUP": "1", "FHIP_ROOT32_MAX": "0"}, {"FHIP_COLUMN_GROUP": "3", "FHIP_NO_ZREP": "1"},
                                 {"FHIP_COLUMN_GROUP": "6", "FHIP_NO_COLUMN_INV": "1"},
                                 {"FHIP_SLAB_LAYERS": "1"}, {"FHIP_SLAB_LAYERS": "2", "FHIP_NO_ZREP": "2"}, {"FHIP_FRAME_LANES": "0"}, {"FHIP_NO_COLUMN_INV": "1"},
                                 {"FHIP_COLUMN_WALK": "0"}, {"FHIP_COLUMN_WALK": "2", "FHIP_FRAME_LANES": "0"}, {"FHIP_COLUMN_WALK": "2", "FHIP_NO_COLUMN_INV": "1"}])
def test_render3d_frames_in_flight_under_the_pipeline_options(env, monkeypatch):
    """The frame pipeline's switches (the leaf kernel's column groups, z-slab thickness, the library's tile choice, sharing of tiles along z, frame lanes,
    the column-invariance short cuts, the leaf kernel by layers or by footprint columns) decide WHEN and WHERE a frame's kernels run, never what they compute: a queue of frames of different
    shapes, sizes and cameras gives the oracle's images under every setting.  (Round 5 fixed the switches of rounds 2-4 whose measurement
    was settled - where the slab's small kernels run, what the side stream carries, issue priority ... - at their measured values.)"""
    import torch
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # (a context reads the environment once, when it is created)
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    for k, v in env.items():
        assert hip.option(k[5:].lower()) == int(v)
    jobs = [("prospero.vm", 512, None), ("colonnade.vm", 256, bench_camera(0.3)), ("prospero.vm", 1024, None), ("tanglecube.vm", 128, None),
            ("prospero.vm", 1024, None), ("colonnade.vm", 512, None), ("prospero.vm", 256, bench_camera(0.15))]
    shapes = {m: F.Shape.from_vm(model_path(m), hip=hip) for m, _, _ in jobs}
    outs = [torch.zeros((n, n, 4), dtype=torch.int32, device="cuda") for _, n, _ in jobs]
    for rep in range(3):
        for i, (m, n, cam) in enumerate(jobs):
            F.render3d(shapes[m], n, world_to_model=cam, out=outs[i])
    torch.cuda.synchronize()
    hip.sync()
    oshape = {m: O.Shape.from_vm(model_path(m)) for m in shapes}
    for i, (m, n, cam) in enumerate(jobs):
        b = O.render3d(oshape[m], n, world_to_model=cam)[0]
        a = outs[i].cpu().numpy().view(np.uint32).reshape(n, n, 4)
        assert (a[:, :, 3] == b["depth"]).all(), f"frame {i} ({m} {n}): {(a[:, :, 3] != b['depth']).sum()} depths differ"
        an = a[:, :, :3].copy().view(np.float32)
        assert ((an == b["normal"]) | (np.isnan(an) & np.isnan(b["normal"]))).all(), f"frame {i} ({m} {n}): normals differ"


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [3, 4, 2, 0])
def test_render3d_frame_lanes(lanes):
    """Option frame_lanes: queued frames whose kernels are the `_t` ones (tapes with transcendental opcodes) run WHOLE, on child
    contexts in turn, and come back through a copy on the caller's stream.  A queue that mixes such frames - different shapes, sizes,
    cameras - with frames of the stage pipeline (prospero) and a host-output frame in the middle gives the oracle's images, frame by
    frame; the counter says the lanes were really taken, and not with the option off."""
    import torch
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    hip.set_option("frame_lanes", lanes)
    jobs = [("bear.vm", 256, None), ("bear.vm", 128, bench_camera(0.3)), ("gyroid-sphere.vm", 256, None), ("prospero.vm", 512, None),
            ("bear.vm", 256, bench_camera(0.15)), ("gyroid-sphere.vm", 128, bench_camera(0.3)), ("bear.vm", 192, None), ("bear.vm", 256, None),
            ("prospero.vm", 256, None), ("gyroid-sphere.vm", 256, None)]
    shapes = {m: F.Shape.from_vm(model_path(m), hip=hip) for m, _, _ in jobs}
    outs = [torch.zeros((n, n, 4), dtype=torch.int32, device="cuda") for _, n, _ in jobs]
    mid = None
    for rep in range(3):
        for i, (m, n, cam) in enumerate(jobs):
            F.render3d(shapes[m], n, world_to_model=cam, out=outs[i])
            if rep == 1 and i == 5:
                mid = F.render3d(shapes["bear.vm"], 64)[0]       # host output: the stage pipeline, waits for its own frame only
    hip.sync()
    torch.cuda.synchronize()
    taken = F.lib().fhip_debug_lane_frames(hip._h)
    assert (taken >= 12) if lanes >= 2 else (taken == 0), taken
    oshape = {m: O.Shape.from_vm(model_path(m)) for m in shapes}
    for i, (m, n, cam) in enumerate(jobs):
        b = O.render3d(oshape[m], n, world_to_model=cam)[0]
        a = outs[i].cpu().numpy().view(np.uint32).reshape(n, n, 4)
        assert (a[:, :, 3] == b["depth"]).all(), f"frame {i} ({m} {n}): {(a[:, :, 3] != b['depth']).sum()} depths differ"
        an = a[:, :, :3].copy().view(np.float32)
        assert ((an == b["normal"]) | (np.isnan(an) & np.isnan(b["normal"]))).all(), f"frame {i} ({m} {n}): normals differ"
    b = O.render3d(oshape["bear.vm"], 64)[0]
    assert (mid["depth"] == b["depth"]).all() and same_bits_f32(mid["normal"], b["normal"])
    # a switch between frames: the lanes are given up and made again under the new options
    hip.set_option("no_column_inv", 1)
    for i, (m, n, cam) in enumerate(jobs[:3] * 2):
        F.render3d(shapes[m], n, world_to_model=cam, out=outs[i % 3])
    hip.sync()
    for i, (m, n, cam) in enumerate(jobs[:3]):
        b = O.render3d(oshape[m], n, world_to_model=cam)[0]
        a = outs[i].cpu().numpy().view(np.uint32).reshape(n, n, 4)
        assert (a[:, :, 3] == b["depth"]).all()
    del shapes, hip


@pytest.mark.gpu
@pytest.mark.parametrize("model,n", [("colonnade.vm", 256), ("prospero.vm", 512)])
def test_render3d_arrangement_tuner(model, n):
    """A run of queued frames of one kind is measured under the stage pipeline, on the lanes and under the stage pipeline again, and the
    faster arrangement kept (capi_render.hpp lane_mode): every frame of the run - whichever arrangement it fell to - is the oracle's image,
    the tuner reaches its decision, and a frame of another kind in between only restarts a window."""
    import torch
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    shape, other = F.Shape.from_vm(model_path(model), hip=hip), F.Shape.from_vm(model_path("tanglecube.vm"), hip=hip)
    outs = [torch.zeros((n, n, 4), dtype=torch.int32, device="cuda") for _ in range(7)]
    o2 = torch.zeros((64, 64, 4), dtype=torch.int32, device="cuda")
    ms, ln = (F.C.c_float * 3)(), F.C.c_int(0)
    for i in range(90):
        F.render3d(shape, n, out=outs[i % 7])
        if i == 20:
            F.render3d(other, 64, out=o2)
    hip.sync()
    assert F.lib().fhip_debug_lane_tune(hip._h, ms, F.C.byref(ln)) == 4 and min(ms) > 0.0, list(ms)
    b = O.render3d(O.Shape.from_vm(model_path(model)), n)[0]
    for o in outs:
        a = o.cpu().numpy().view(np.uint32).reshape(n, n, 4)
        assert (a[:, :, 3] == b["depth"]).all() and same_bits_f32(a[:, :, :3].copy().view(np.float32), b["normal"])
    taken = F.lib().fhip_debug_lane_frames(hip._h)
    assert taken >= 10          # (the lanes' window at least)
    # (a frame takes the lanes only while the frame before it is still under way, capi_render.hpp lanes_possible: the stream is held busy
    # so that every one of the 12 is queued behind work whatever the host's pace - the first, behind a finished frame, is a frame alone)
    torch.cuda._sleep(200_000_000)
    for i in range(12):         # decided: the run goes on in the arrangement kept
        F.render3d(shape, n, out=outs[i % 7])
    hip.sync()
    now = F.lib().fhip_debug_lane_frames(hip._h)
    assert now - taken in ((10, 11, 12) if ln.value else (0,)), (taken, now, ln.value)
    del shape, other, hip


@pytest.mark.gpu
def test_frame_lanes_that_cannot_be_had_fall_back_to_the_stage_pipeline():
    """The lanes need device memory of their own (a child context's buffers); when that fails the frame is rendered under the stage pipeline
    and the context gives its lanes up - the caller sees frames, not an error (option lanes_fail provokes the failure)."""
    import torch
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    hip.set_option("lanes_fail", 1)
    shape = F.Shape.from_vm(model_path("bear.vm"), hip=hip)
    outs = [torch.zeros((128, 128, 4), dtype=torch.int32, device="cuda") for _ in range(3)]
    o2 = torch.zeros((256, 256), dtype=torch.float32, device="cuda")
    for i in range(9):
        F.render3d(shape, 128, out=outs[i % 3])
        F.render2d(shape, 256, out=o2)
    hip.sync()
    assert hip.lane_frames() == 0 and hip.option("frame_lanes") == 0
    b = O.render3d(O.Shape.from_vm(model_path("bear.vm")), 128)[0]
    for o in outs:
        a = o.cpu().numpy().view(np.uint32).reshape(128, 128, 4)
        assert (a[:, :, 3] == b["depth"]).all() and same_bits_f32(a[:, :, :3].copy().view(np.float32), b["normal"])
    assert same_bits_f32(o2.cpu().numpy(), O.render2d(O.Shape.from_vm(model_path("bear.vm")), 256, tile_sizes=F.HIP_TILES_2D)[0])
    del shape, hip


@pytest.mark.gpu
def test_render3d_lanes_for_parts_of_a_frame():
    """Shards and blocks - what a rank of a multi-GPU job renders - queued back to back take the lanes like whole frames :
    every part, whichever arrangement its frames fell to, equals the part rendered alone by a context without lanes, and the parts of a
    split still merge to the oracle's frame."""
    import torch
    n = 512
    ref_ctx = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    ref_ctx.set_option("frame_lanes", 0)
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    sa, sb = F.Shape.from_vm(model_path("prospero.vm"), hip=ref_ctx), F.Shape.from_vm(model_path("prospero.vm"), hip=hip)
    parts = [{"block": (i, (2, 2, 2))} for i in range(8)] + [{"shard": 1, "n_shards": 4}]
    outs = [torch.zeros((n, n, 4), dtype=torch.int32, device="cuda") for _ in parts]
    for rep in range(3):                         # mixed: the prior (stage pipeline) ...
        for kw, o in zip(parts, outs):
            F.render3d(sb, n, out=o, **kw)
    for kw, o in zip(parts[6:8], outs[6:8]):       # ... and runs of one kind, long enough for the tuner to take them through the lanes
        for i in range(60):
            F.render3d(sb, n, out=o, **kw)
    hip.sync()
    assert F.lib().fhip_debug_lane_frames(hip._h) >= 20
    for kw, o in zip(parts, outs):
        alone = torch.zeros((n, n, 4), dtype=torch.int32, device="cuda")
        F.render3d(sa, n, out=alone, **kw)
        ref_ctx.sync()
        assert torch.equal(o, alone), kw
    # front to back over the two z halves of every column block, then the union of the four column blocks: the whole frame
    img = None
    for ix in range(2):
        for iy in range(2):
            front, back = outs[ix + 2 * iy + 4].clone(), outs[ix + 2 * iy]
            F.merge_depth(front, back, n, hip=hip)
            img = front if img is None else img + front          # (the column blocks are disjoint and a part's image is zero outside its block)
    hip.sync()
    whole = torch.zeros((n, n, 4), dtype=torch.int32, device="cuda")
    F.render3d(sa, n, out=whole)
    ref_ctx.sync()
    assert torch.equal(img[..., 3], whole[..., 3])
    assert torch.equal(img, whole)          # depths AND normals (the merged frame was compared by depth only)
    del sa, sb, hip, ref_ctx


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [3, 0])
def test_render2d_frame_lanes(lanes):
    """... and every queued 2D frame with a device output (a 2D frame has no stage pipeline to lose): a queue of 2D frames of different
    models, sizes, z and pixel_perfect, with 3D frames in between, against the oracle frame by frame."""
    import torch
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    hip.set_option("frame_lanes", lanes)
    jobs = [("prospero.vm", 1024, 0.0, False), ("hi.vm", 256, 0.0, False), ("bear.vm", 512, 0.1, False), ("prospero.vm", 512, 0.0, True),
            ("colonnade.vm", 512, 0.2, False), ("gyroid-sphere.vm", 256, 0.0, False), ("prospero.vm", 2048, 0.0, False), ("quarter.vm", 128, 0.0, True)]
    shapes = {m: F.Shape.from_vm(model_path(m), hip=hip) for m, _, _, _ in jobs}
    outs = [torch.zeros((n, n), dtype=torch.float32, device="cuda") for _, n, _, _ in jobs]
    out3 = torch.zeros((128, 128, 4), dtype=torch.int32, device="cuda")
    for rep in range(3):
        for i, (m, n, z, pp) in enumerate(jobs):
            F.render2d(shapes[m], n, z=z, pixel_perfect=pp, out=outs[i])
            if i == 4:
                F.render3d(shapes["bear.vm"], 128, out=out3)
    hip.sync()
    torch.cuda.synchronize()
    taken = F.lib().fhip_debug_lane_frames(hip._h)
    assert (taken >= 20) if lanes >= 2 else (taken == 0), taken
    for i, (m, n, z, pp) in enumerate(jobs):
        b = O.render2d(O.Shape.from_vm(model_path(m)), n, z=z, pixel_perfect=pp, tile_sizes=F.HIP_TILES_2D)[0]
        assert same_bits_f32(outs[i].cpu().numpy(), b), f"2D frame {i} ({m} {n})"
    b = O.render3d(O.Shape.from_vm(model_path("bear.vm")), 128)[0]
    a = out3.cpu().numpy().view(np.uint32).reshape(128, 128, 4)
    assert (a[:, :, 3] == b["depth"]).all()
    del shapes, hip


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_regs,size", [("colonnade.vm", 255, 256), ("colonnade.vm", 6, 128), ("prospero.vm", 24, 256)])
def test_render_from_reference_bytecode(name, n_regs, size):
    """The words a Rust `fidget-hip` shim hands over (fidget_bytecode::Bytecode of a VmData<N>; N < 255 gives tapes with Mem
    load / store ops, which the import folds back into SSA form) rendered on the device: same image as the oracle's, 2D and 3D."""
    o = O.Shape.from_vm(model_path(name), n_regs=n_regs)
    words, regs, mem = o.bytecode()
    p = F.Shape.from_bytecode(words, axis_slots=[o.axis_index(a) for a in range(3)])
    a, b = F.render3d(p, size)[0], O.render3d(o, size)[0]
    assert (a["depth"] == b["depth"]).all() and same_bits_f32(a["normal"], b["normal"])
    a, b = F.render2d(p, size)[0], O.render2d(o, size, tile_sizes=F.HIP_TILES_2D)[0]
    assert same_bits_f32(a, b)


@pytest.mark.gpu
def test_render3d_bound_variables():
    """Var::V inputs bound at render time (ShapeVars, shape/mod.rs:372-400) through the whole 3D device path - tile stage,
    assembly leaf kernel, normals: a blend of two shapes steered by two variables, several bindings, rotated camera."""
    def build(be):
        ctx = be.Context()
        x, y, z = ctx.x(), ctx.y(), ctx.z()
        r, k = ctx.var(7), ctx.var(0x1234)
        sphere = ctx.sub(ctx.sqrt(ctx.add(ctx.add(ctx.square(x), ctx.square(y)), ctx.square(z))), r)
        box = ctx.max(ctx.max(ctx.sub(ctx.abs(x), 0.6), ctx.sub(ctx.abs(y), k)), ctx.sub(ctx.abs(z), 0.4))
        return be.Shape(ctx, ctx.min(sphere, ctx.add(box, ctx.mul(k, 0.1))))
    p, o = build(F), build(O)
    cam = bench_camera(0.2)
    for vars in ({7: 0.5, 0x1234: 0.3}, {7: 0.8, 0x1234: 0.7}, {7: 0.1, 0x1234: 0.05}):
        for w2m in (None, cam):
            a = F.render3d(p, 192, world_to_model=w2m, vars=vars)[0]
            b = O.render3d(o, 192, world_to_model=w2m, vars=vars)[0]
            assert b["depth"].max() > 0
            assert (a["depth"] == b["depth"]).all(), f"{vars}: {(a['depth'] != b['depth']).sum()} depths differ"
            same = (a["normal"] == b["normal"]) | (np.isnan(a["normal"]) & np.isnan(b["normal"]))
            assert same.all(), f"{vars}: {(~same).any(axis=2).sum()} normals differ"
    with pytest.raises(ValueError):
        F.render3d(p, 64, vars={7: 0.5})        # MissingVar, as the reference (shape/mod.rs:388-396)


@pytest.mark.gpu
@pytest.mark.parametrize("name,size", [("prospero.vm", 512), ("colonnade.vm", 256), ("colonnade.vm", 512), ("tanglecube.vm", 128)])
def test_render3d_column_invariant_parents(name, size, monkeypatch):
    """Tiles whose tape reads nothing that changes along z (an extrusion such as prospero.vm, the vertical shafts of
    colonnade.vm once pruned) repeat along z: the tile stage evaluates one z-layer of their children and hands the results to
    every instance (k_tape_flags, tsetup_body / tpush_body).  Same image as without the short cut, which is the oracle's;
    under a rotated camera nothing is invariant and nothing changes either."""
    p, o = both(name)
    ref = O.render3d(o, size)[0]
    hip = p.hip
    for var in (None, "no_zrep", "no_column_inv"):       # everything on; the tile stage's short cut off; all of them off
        with hip.options(**({var: 1} if var else {})):   # (switches are the context's: fhip_ctx_set_option, not the environment)
            a = F.render3d(p, size)[0]
        assert (a["depth"] == ref["depth"]).all(), f"{var}: {(a['depth'] != ref['depth']).sum()} depths differ"
        assert same_bits_f32(a["normal"], ref["normal"])
    assert hip.option("no_zrep") == 0 and hip.option("no_column_inv") == 0
    cam = bench_camera(0.0)
    a, b = F.render3d(p, size, world_to_model=cam)[0], O.render3d(o, size, world_to_model=cam)[0]
    assert (a["depth"] == b["depth"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_render3d_partly_column_invariant_shapes(kind, monkeypatch):
    """Shapes in which SOME tiles' tapes lose their z (an extruded profile joined with, cut by, or standing behind a body that
    depends on z), so that column-invariant stacks and ordinary tiles meet in one frame - in front of each other, occluding
    each other, sharing parents: depth and normals as the oracle's, cubic and not, plain and scaled (still axis-aligned) camera."""
    def build(be):
        c = be.Context()
        x, y, z = c.x(), c.y(), c.z()
        star = c.sub(c.add(c.abs(c.sub(x, 0.1)), c.mul(c.abs(c.add(y, 0.2)), 1.5)), 0.45)           # extruded diamond
        ring = c.sub(c.abs(c.sub(c.sqrt(c.add(c.square(c.add(x, 0.3)), c.square(c.sub(y, 0.3)))), 0.35)), 0.06)   # extruded ring
        ball = c.sub(c.sqrt(c.add(c.add(c.square(c.sub(x, 0.2)), c.square(y)), c.square(c.sub(z, 0.3)))), 0.5)
        if kind == 0:
            n = c.min(c.min(star, ring), ball)                      # union: stacks beside and behind a body with z
        elif kind == 1:
            n = c.max(c.min(star, ring), c.sub(c.abs(c.sub(z, 0.1)), 0.55))     # extrusions cut by two planes: z comes back near the cuts
        else:
            n = c.min(c.max(star, c.neg(ball)), c.max(ring, c.sub(z, -0.2)))    # a body carved out of one, the other cut off below
        return be.Shape(c, n)
    p, o = build(F), build(O)
    scaled = np.diag([1.3, 0.9, 1.1, 1.0]).astype(np.float32)
    for whd, cam in (((256, 256, 256), None), ((384, 256, 512), None), ((256, 256, 256), scaled)):
        ref = O.render3d(o, *whd, world_to_model=cam)[0]
        assert ref["depth"].max() > 0 and (ref["depth"] == 0).any()
        for var in (None, "no_column_inv"):
            with p.hip.options(**({var: 1} if var else {})):
                a = F.render3d(p, *whd, world_to_model=cam)[0]
            assert (a["depth"] == ref["depth"]).all(), f"kind {kind} {whd} {var}: {(a['depth'] != ref['depth']).sum()} depths differ"
            same = (a["normal"] == ref["normal"]) | (np.isnan(a["normal"]) & np.isnan(ref["normal"]))
            assert same.all(), f"kind {kind} {whd} {var}: {(~same).any(axis=2).sum()} normals differ"


@pytest.mark.gpu
def test_bulk_sqrt_min_max_bit_exact_over_the_float_range():
    """The assembly interpreters' sqrt (a short sequence, or the scaled one when a sample of the op is tiny, zero or negative) and
    their in-place min / max (one test and one select per sample unless a's samples sum to a NaN) through fhip_float_eval on
    4 M inputs covering every exponent, both signs, the denormals, zeros, infinities and NaNs: sqrtf is correctly rounded
    (numpy's is), min / max are dev_ops.hpp f_min / f_max - bit for bit, NaN for NaN (vm/mod.rs:885-896, 1004-1037)."""
    import fidget_amd as F
    hip = F.default_context()
    ctx = F.Context()
    x, y = ctx.x(), ctx.y()
    n = 1 << 22
    rng = np.random.default_rng(11)
    xs = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    xs[: 1 << 16] = (np.arange(1 << 16, dtype=np.uint32) << 16) | 0x8001            # every sign / exponent / top mantissa pattern
    xs[1 << 16: (1 << 16) + 8] = [0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 1, 0x007FFFFF, 0x00800000]
    ys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    ys[::7] = xs[::7]                                                                # equal operands, among them +0 / -0 pairs
    ys[3::1001] = 0x7FC00000
    xf, yf = xs.view(np.float32), ys.view(np.float32)
    zero = np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        for name, node, want in (
            ("sqrt", ctx.sqrt(x), np.sqrt(xf)),
            ("sqrt|x|", ctx.sqrt(ctx.abs(x)), np.sqrt(np.abs(xf))),                  # no negative sample: mostly the short sequence
            ("min", ctx.min(x, y), np.where(xf < yf, xf, np.where(yf < xf, yf, np.where(np.isnan(xf) | np.isnan(yf), np.float32(np.nan), yf)))),
            ("max", ctx.max(x, y), np.where(xf > yf, xf, np.where(yf > xf, yf, np.where(np.isnan(xf) | np.isnan(yf), np.float32(np.nan), yf)))),
        ):
            s = F.Shape(ctx, node, hip=hip)
            got = np.asarray(s.eval_float_slice(xf, yf, zero), np.float32)
            ok = (got.view(np.uint32) == want.astype(np.float32).view(np.uint32)) | (np.isnan(got) & np.isnan(want))
            assert ok.all(), f"{name}: {(~ok).sum()} of {n} differ, first at input {hex(int(xs[np.nonzero(~ok)[0][0]]))}"


@pytest.mark.gpu
@pytest.mark.parametrize("name,size", [("prospero.vm", 512), ("colonnade.vm", 256), ("bear.vm", 256), ("gyroid-sphere.vm", 128)])
def test_assembly_normals_are_the_hip_kernels(name, size):
    """fh_normals / fh_normals_t (gen_normals.py: the gradient interpreter in assembly, with the compiled transcendental routines for
    bear.vm and gyroid-sphere.vm) against k_normals3d, the HIP C++ kernel it replaces (option no_asm_normals): the same image, normals
    bit for bit - also under a perspective camera, where the input gradients go through the division by w."""
    import fidget_amd as F
    hip = F.HipContext(0)
    p = F.Shape.from_vm(model_path(name), hip=hip)
    for cam in (None, bench_camera(0.3)):
        a = F.render3d(p, size, world_to_model=cam)[0]
        with hip.options(no_asm_normals=1):
            b = F.render3d(p, size, world_to_model=cam)[0]
        assert (a["depth"] == b["depth"]).all() and (a["depth"] > 0).any()
        assert same_bits_f32(a["normal"], b["normal"]), f"{name}: {(a['normal'].view(np.uint32) != b['normal'].view(np.uint32)).any(axis=2).sum()} normals differ"


@pytest.mark.gpu
@pytest.mark.parametrize("name,size", [("bear.vm", 256), ("bear.vm", 512), ("gyroid-sphere.vm", 256)])
def test_assembly_tile_stage_of_transcendental_tapes(name, size):
    """fh_tiles_t / fh_tiles_v32_t / fh_tiles_v64_t (the tile kernels with interval sin cos tan asin acos atan exp ln: gen_tiles.py
    b_trans around the compiled routines) against the HIP C++ tile stage k_teval3d they replace for such tapes (option
    no_asm_tiles_t): the same image, and the same tapes for the tiles below the root level, word for word - also under a perspective
    camera.  The 2D renderer goes through the same kernels."""
    import fidget_amd as F
    hip = F.HipContext(0)
    p = F.Shape.from_vm(model_path(name), hip=hip)

    def tiles():
        g, _ = hip.groups(0, 1)
        return {(int(e["x"]), int(e["y"]), int(e["z"])): (hip.arena_ops(int(e["off"]), int(e["len"])).tobytes(), int(e["regs"]), int(e["choices"])) for e in g}

    for cam in (None, bench_camera(0.3)):
        a = F.render3d(p, size, world_to_model=cam)[0]
        ta = tiles()
        with hip.options(no_asm_tiles_t=1):
            b = F.render3d(p, size, world_to_model=cam)[0]
            tb = tiles()
        assert (a["depth"] == b["depth"]).all() and (a["depth"] > 0).any()
        assert same_bits_f32(a["normal"], b["normal"])
        assert ta.keys() == tb.keys() and len(ta) > 0
        assert all(ta[k] == tb[k] for k in ta), f"{sum(ta[k] != tb[k] for k in ta)} of {len(ta)} level-1 tapes differ"
    a2 = F.render2d(p, size)[0]
    with hip.options(no_asm_tiles_t=1):
        b2 = F.render2d(p, size)[0]
    assert (a2.view(np.uint32) == b2.view(np.uint32)).all() or same_bits_f32(a2, b2)


@pytest.mark.parametrize("size,camera", [(512, None), (256, None), (320, None), (384, "rot"), (512, "persp"), (1024, None)])
def test_render3d_root_tiles_of_32_and_root_column_invariance(size, camera):
    """Round 5: when the root level has few children the library renders with root tiles of 32^3 straight above the leaves (the linked
    prune of the ROOT tape per 32^3 tile, no level 1), and a root tape that reads nothing varying along a pixel column is evaluated for
    one layer of root tiles per z-slab - and, since nothing such a frame evaluates depends on z, for the FRONT slab only (capi_render.hpp root32_max, root_zrep, front_only; option no_zrep 3 / 2 / 1: every slab / not at the root / nowhere).  None of it may change a pixel: the oracle's image under
    every combination of the two - and with the column short cuts off (a tape with z everywhere), and under cameras that move x and y
    along a column (no invariance anywhere: rotated, perspective), and as the eight octants of the frame."""
    import torch
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    hip.set_option("frame_lanes", 0)
    p, o = F.Shape.from_vm(model_path("prospero.vm"), hip=hip), O.Shape.from_vm(model_path("prospero.vm"))
    m = None
    if camera == "rot":
        c, s_ = np.cos(0.4), np.sin(0.4)
        m = np.array([[c, 0, s_, 0.05], [0, 1, 0, -0.02], [-s_, 0, c, 0.1], [0, 0, 0, 1]], np.float32)
    elif camera == "persp":
        m = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0.3, 1]], np.float32)
    ref = O.render3d(o, size, world_to_model=m)[0]
    ref_words = np.concatenate([ref["normal"].view(np.uint32), ref["depth"][..., None]], axis=2)
    for root32_max, no_zrep, no_inv in ((4096, 0, 0), (0, 0, 0), (4096, 2, 0), (0, 2, 0), (4096, 1, 0), (4096, 0, 1), (1 << 20, 0, 0), (1 << 20, 0, 1),
                                        (4096, 3, 0), (0, 3, 0)):
        if size == 1024 and root32_max == (1 << 20) and no_inv:
            continue        # (32 768 children through the scalar sweep: right, and slow)
        with hip.options(root32_max=root32_max, no_zrep=no_zrep, no_column_inv=no_inv):
            out = torch.zeros((size, size, 4), dtype=torch.int32, device="cuda")
            F.render3d(p, size, world_to_model=m, out=out)
            hip.sync()
            got = out.cpu().numpy().view(np.uint32)
            assert (got[..., 3] == ref_words[..., 3]).all(), (root32_max, no_zrep, no_inv, int((got[..., 3] != ref_words[..., 3]).sum()))
            assert same_bits_f32(got[..., :3].view(np.float32), ref_words[..., :3].view(np.float32)), (root32_max, no_zrep, no_inv)
            if camera is None and size in (512, 1024):       # the frame as eight octants: each block's own tile choice, merged front to back
                img = None
                for ix in range(2):
                    for iy in range(2):
                        parts = []
                        for iz in (1, 0):
                            t = torch.zeros((size, size, 4), dtype=torch.int32, device="cuda")
                            F.render3d(p, size, out=t, block=(ix + 2 * iy + 4 * iz, (2, 2, 2)))
                            parts.append(t)
                        F.merge_depth(parts[0], parts[1], size, hip=hip)
                        img = parts[0] if img is None else img + parts[0]
                hip.sync()
                assert torch.equal(img, out), (root32_max, no_zrep, no_inv)
    del p, hip


def test_device_memory_of_a_context_follows_need_and_trim_gives_caches_back():
    """Round 5: a buffer set's tape arena starts at 128 MB and grows when a frame ran out (the frame is still right); until round 4 every set
    held 4 GiB - 18.6 GB per context for a peak use of 0.1.  A context that has rendered the headline frame a few times holds under 3 GB;
    fhip_ctx_trim gives the frame lanes and the mesher's leaf records back; a small arena cap still gives the oracle's image."""
    import torch
    # (free device memory is the DEVICE's: with other test processes on it - pytest -n - the readings mean nothing, and only the images are checked)
    alone = not os.environ.get("PYTEST_XDIST_WORKER")
    free0 = torch.cuda.mem_get_info()[0]
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    hip.set_option("frame_lanes", 0)
    p = F.Shape.from_vm(model_path("prospero.vm"), hip=hip)
    out = torch.zeros((1024, 1024, 4), dtype=torch.int32, device="cuda")
    for no_inv, bound in ((0, 3.0), (1, 6.5)):        # (GiB: four buffer sets of 0.33 GB + the arena: 128 MB, 1 GB when every tape has z - 65 M ops in flight per set)
        with hip.options(no_column_inv=no_inv):
            for _ in range(16):
                F.render3d(p, 1024, out=out)
            hip.sync()
        used = free0 - torch.cuda.mem_get_info()[0]
        assert used < bound * 2 ** 30 or not alone, (no_inv, used)
    ref = O.render3d(O.Shape.from_vm(model_path("prospero.vm")), 1024)[0]
    got = out.cpu().numpy().view(np.uint32)
    assert (got[..., 3] == ref["depth"]).all() and same_bits_f32(got[..., :3].view(np.float32), ref["normal"])
    hip.set_option("frame_lanes", 4)
    small = torch.zeros((256, 256, 4), dtype=torch.int32, device="cuda")
    b = F.Shape.from_vm(model_path("bear.vm"), hip=hip)
    for _ in range(40):
        F.render3d(b, 256, out=small)          # (a transcendental tape's queued frames take the lanes: child contexts)
    hip.sync()
    with_lanes = free0 - torch.cuda.mem_get_info()[0]
    hip.trim()
    after = free0 - torch.cuda.mem_get_info()[0]
    assert not alone or (after <= with_lanes and (F.lib().fhip_debug_lane_frames(hip._h) == 0 or after < with_lanes))
    del p, b, hip


def test_render3d_takes_every_tile_list_the_reference_takes():
    """TileSizes::new (fidget-core/src/render/mod.rs:181-251) accepts any descending list whose entries divide their predecessors; fidget-jit's
    hint is [64, 16, 8].  Until round 4 a list whose last entry is not 8 or whose fan-out exceeds 64 was refused; now it is rendered with the
    library's own list - the 3D image does not depend on the tile sizes - and counted.  Invalid lists are still refused."""
    import torch
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    p, o = F.Shape.from_vm(model_path("colonnade.vm"), hip=hip), O.Shape.from_vm(model_path("colonnade.vm"))
    ref = O.render3d(o, 192)[0]
    F.render3d(p, 192)
    before = hip.counters()["substituted_tile_lists"]
    for k, ts in enumerate(([64, 16, 8], [64, 16, 4], [128, 8], [256, 64, 16, 8, 2], [96, 32, 16], [8], [5])):
        a = F.render3d(p, 192, tile_sizes=ts)[0]
        assert (a["depth"] == ref["depth"]).all() and same_bits_f32(a["normal"], ref["normal"]), ts
    assert hip.counters()["substituted_tile_lists"] - before == 5        # ([64, 16, 8] and [8] are taken as given)
    for bad in ([8, 16], [64, 24, 8], [16, 16]):
        with pytest.raises(F.FidgetHipError):
            F.render3d(p, 192, tile_sizes=bad)


@pytest.mark.parametrize("name,size,ts", [("prospero.vm", 512, [128, 8]), ("prospero.vm", 700, [256, 16]), ("hi.vm", 256, [128, 4]), ("colonnade.vm", 300, [64, 2]),
                                          ("prospero.vm", 1024, [512, 8]), ("quarter.vm", 256, [256, 8])])
def test_render2d_takes_a_fan_out_above_64_in_two_steps(name, size, ts):
    """A step of the caller's 2D tile list with more than 64 children per parent (128 -> 8: 256) was refused until round 4.  It is taken in
    two now - a level in between that the caller does not see, whose fills carry the level of the caller's next one (pixel.rs:225-229) - and
    the image is the reference's for the CALLER's list, fill tags included: the oracle renders with exactly that list."""
    p, o = both(name)
    a = F.render2d(p, size, tile_sizes=ts)[0]
    b = O.render2d(o, size, tile_sizes=ts)[0]
    assert same_bits_f32(a, b), f"{ts}: {(a.view(np.uint32) != b.view(np.uint32)).sum()} pixels differ"
    assert (F.pixel_fill_depth(a) == O.pixel_fill_depth(b)).all()
    assert F.pixel_fill_depth(a).max() <= len(ts) - 1


@pytest.mark.parametrize("size,ts", [(64, None), (100, None), (256, None), (300, None), (512, None), (700, None), (256, [64, 8]), (384, [128, 32]), (200, [32, 8])])
def test_render2d_small_images_of_a_large_tape(size, ts):
    """Round 5: a small 2D image of a large tape (few root tiles, none of which prunes the tape much) is rendered as a one-level pass of the
    ROOT tape over the leaf tiles + a classify-only pass over the root tiles for the fills' level tags (capi_render.hpp render2d_frame).
    The image is the two-level recursion's, tags included: the oracle with the same list; the same with the short cut off; rectangular and
    pixel-perfect renders too."""
    import torch
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    p, o = F.Shape.from_vm(model_path("prospero.vm"), hip=hip), O.Shape.from_vm(model_path("prospero.vm"))
    b = O.render2d(o, size, tile_sizes=ts or F.HIP_TILES_2D)[0]
    for off in (0, 1):
        with hip.options(root32_max=0 if off else 4096):
            a = F.render2d(p, size, tile_sizes=ts)[0]
            assert same_bits_f32(a, b), f"{ts} off={off}: {(a.view(np.uint32) != b.view(np.uint32)).sum()} pixels differ"
            assert (F.pixel_fill_depth(a) == O.pixel_fill_depth(b)).all()
    a = F.render2d(p, size, size // 2 + 8, tile_sizes=ts)[0]
    b = O.render2d(o, size, size // 2 + 8, tile_sizes=ts or F.HIP_TILES_2D)[0]
    assert same_bits_f32(a, b)
    a = F.render2d(p, size, pixel_perfect=True, tile_sizes=ts)[0]
    b = O.render2d(o, size, pixel_perfect=True, tile_sizes=ts or F.HIP_TILES_2D)[0]
    assert same_bits_f32(a, b)
    del p, hip


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(1024, 1024, 768), (512, 384, 1280), (1024, 1024, 1024)])
def test_render3d_front_slab_only_for_frames_without_z(dims):
    """A frame whose tapes read nothing that changes along a pixel column renders its front z-slab only (round 5: a tile or a leaf
    further back repeats the front one's result with a smaller depth).  The oracle's image for volumes whose depth is not a multiple
    of the slab (a thin front slab), is deeper than wide, and with every slab rendered (no_zrep 3); queued frames alternate their
    root levels between two streams, so a run of them - different sizes in turn - is checked frame by frame."""
    import torch
    w, h, d = dims
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    hip.set_option("frame_lanes", 0)
    p, o = F.Shape.from_vm(model_path("prospero.vm"), hip=hip), O.Shape.from_vm(model_path("prospero.vm"))
    ref = O.render3d(o, w, h, d)[0]
    small = O.render3d(o, 256)[0]
    for no_zrep in (0, 3):
        with hip.options(no_zrep=no_zrep):
            outs = [torch.zeros((h, w, 4), dtype=torch.int32, device="cuda") for _ in range(6)]
            mids = [torch.zeros((256, 256, 4), dtype=torch.int32, device="cuda") for _ in range(6)]
            for a, b in zip(outs, mids):
                F.render3d(p, w, h, d, out=a)
                F.render3d(p, 256, out=b)
            hip.sync()
            for a, b in zip(outs, mids):
                got = a.cpu().numpy().view(np.uint32)
                assert (got[..., 3] == ref["depth"]).all(), (no_zrep, int((got[..., 3] != ref["depth"]).sum()))
                assert same_bits_f32(got[..., :3].view(np.float32), ref["normal"]), no_zrep
                gs = b.cpu().numpy().view(np.uint32)
                assert (gs[..., 3] == small["depth"]).all() and same_bits_f32(gs[..., :3].view(np.float32), small["normal"]), no_zrep


def test_rare_mode_takes_the_large_tapes_it_does_not_expect():
    """Rare mode (capi_render.hpp): after a frame that met no tape too large for the assembly kernels' register files, a context's next 3D
    frames fold the launches that exist for such tapes into three launches they make anyway.  A frame that then DOES have such tapes -
    prospero.vm at 128^3: leaves of more than 32 registers, per-slab parents outside the small list - is rendered by those folded blocks
    (C++, register files in HBM), bit for bit the oracle's; it tells the host, and the frames after it launch the kernels on their own
    again - the same image."""
    hip = F.HipContext(0)
    hip.set_option("frame_lanes", 0)
    for opt in ("no_asm", "no_split", "no_asm_tiles", "no_tiles_v", "no_asm_normals", "no_columns_t"):      # (rare mode is the assembly kernels' frames': whatever the environment says)
        hip.set_option(opt, 0)
    big, big_o = F.Shape.from_vm(model_path("prospero.vm"), hip=hip), O.Shape.from_vm(model_path("prospero.vm"))
    want = O.render3d(big_o, 128)[0]
    a = F.render3d(big, 128)[0]             # (a new context: the launches on their own)
    hip.sync()
    assert hip.rare_frames() == 0
    assert (a["depth"] == want["depth"]).all() and same_bits_f32(a["normal"], want["normal"])
    for _ in range(2):                      # 1024^3 has no such tape: the second frame knows
        F.render3d(big, 1024)
        hip.sync()
    n0 = hip.rare_frames()
    assert n0 >= 1, "the frame after one without large tapes is not in rare mode"
    b = F.render3d(big, 128)[0]             # ... and this one does not expect what it meets
    hip.sync()
    assert hip.rare_frames() == n0 + 1
    assert (b["depth"] == want["depth"]).all(), f"{(b['depth'] != want['depth']).sum()} depths differ in rare mode"
    assert same_bits_f32(b["normal"], want["normal"])
    c = F.render3d(big, 128)[0]             # told: on their own again
    hip.sync()
    assert hip.rare_frames() == n0 + 1
    assert (c["depth"] == want["depth"]).all() and same_bits_f32(c["normal"], want["normal"])
    # the same with bear.vm's transcendental tapes at a size where its leaves are beyond 32 registers too
    bear, bear_o = F.Shape.from_vm(model_path("bear.vm"), hip=hip), O.Shape.from_vm(model_path("bear.vm"))
    for _ in range(2):
        F.render3d(big, 1024)
        hip.sync()
    d = F.render3d(bear, 64)[0]
    hip.sync()
    w = O.render3d(bear_o, 64)[0]
    assert (d["depth"] == w["depth"]).all()


def test_bulk_division_by_an_immediate_bit_exact_over_the_float_range():
    """The assembly interpreters' division by an immediate (gen_interp.py f_div_imm: the reciprocal's refinement once per op, the quotient
    two samples per instruction, no v_div_scale_f32 while both operands lie within 2^-40 .. 2^40 - otherwise the general sequence for
    the op) through fhip_float_eval on 4 M numerators covering every exponent, both signs, denormals, zeros, infinities and NaNs, for
    divisors of every kind: IEEE division (numpy's), bit for bit."""
    hip = F.default_context()
    n = 1 << 22
    rng = np.random.default_rng(12)
    xs = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    xs[: 1 << 16] = (np.arange(1 << 16, dtype=np.uint32) << 16) | 0x8001
    xs[1 << 16: (1 << 16) + 8] = [0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 1, 0x007FFFFF, 0x00800000]
    xf = xs.view(np.float32)
    # (mostly ordinary numerators too: a block of values within the short sequence's range, so that whole ops take it)
    mid = (rng.standard_normal(n).astype(np.float32) * np.float32(1000.0))
    zero = np.zeros(n, np.float32)
    for c in (0.3, 3.0, -7.77, 1e-5, 123456.7, 2.0 ** -40, 1.5 * 2.0 ** -41, 2.0 ** 40, 2.0 ** 41, 1e-30, 1e30, 1.0, -0.5, float(np.float32(1.0000001))):
        ctx = F.Context()
        s = F.Shape(ctx, ctx.div(ctx.x(), float(np.float32(c))), hip=hip)
        for name, arg in (("every exponent", xf), ("ordinary", mid)):
            with np.errstate(all="ignore"):
                want = (arg / np.float32(c)).astype(np.float32)
            got = np.asarray(s.eval_float_slice(arg, zero, zero), np.float32)
            ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
            assert ok.all(), f"x / {c} ({name}): {(~ok).sum()} of {n} differ, first at input bits {hex(int(arg.view(np.uint32)[np.nonzero(~ok)[0][0]]))}"
