"""Events only where somebody waits (frame_schedule.hpp rec_fork / records_leaves, capi_render.hpp): a queued frame records no ev_leaves
for a slab context nobody takes again, no ev_fork where the tile chain runs on the fork's own stream, no event of its own for "the frame
before is still under way", and the pinned staging slot's guard at the end of the root level instead of behind k_frame_begin.  None of
that may show in an image, in any arrangement: stage pipeline, frame lanes, a lone frame, a host output, a profiled frame, a cancelled
frame in the middle of a queue.  Every test is an ordinary render against the CPU oracle, depth and normals bit for bit."""
import numpy as np
import pytest

import fidget_amd as F
import oracle as O
from conftest import model_path
from test_gpu_parity import same_bits_f32

pytestmark = pytest.mark.gpu

FHIP_ERR_CANCELLED = 8
_WANT = {}


def want(name, *whd):
    """the oracle's image, computed once per (model, size)"""
    key = (name,) + whd
    if key not in _WANT:
        _WANT[key] = O.render3d(O.Shape.from_vm(model_path(name)), *whd)[0]
    return _WANT[key]


def context(**options):
    import torch
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    for k, v in options.items():
        hip.set_option(k, v)
    return hip


def queue(shape, *whd):
    """one frame queued into a device image of its own (the call returns when the frame's kernels are queued)"""
    import torch
    w, h = whd[0], whd[1] if len(whd) > 1 else whd[0]
    out = torch.zeros((h, w, 4), dtype=torch.int32, device="cuda")
    F.render3d(shape, *whd, out=out)
    return out


def check(out, ref, what):
    a = out.cpu().numpy().view(np.uint32) if hasattr(out, "cpu") else None
    depth, normal = (a[..., 3], a[..., :3].copy().view(np.float32)) if a is not None else (out["depth"], out["normal"])
    assert (depth == ref["depth"]).all(), f"{what}: {(depth != ref['depth']).sum()} depths differ"
    assert same_bits_f32(normal, ref["normal"]), f"{what}: normals differ"


@pytest.mark.parametrize("lanes", [0, 4])
def test_staging_ring_comes_round_twice(lanes):
    """20 frames back to back on one context, 128^3 and 192^3 in turn: the state in a staging slot differs from frame to frame, the ring of
    eight comes round twice, and a slot overwritten before k_frame_begin has read it would give a frame the other size's state"""
    hip = context(frame_lanes=lanes)
    p = F.Shape.from_vm(model_path("prospero.vm"), hip=hip)
    sizes = [128 if i % 2 == 0 else 192 for i in range(20)]
    outs = [queue(p, n) for n in sizes]
    hip.sync()
    for i, (n, o) in enumerate(zip(sizes, outs)):
        check(o, want("prospero.vm", n), f"frame {i} ({n}^3)")
    del p, hip


@pytest.mark.parametrize("model,options,whd", [("colonnade.vm", {}, (256,)), ("prospero.vm", {"no_column_inv": 1}, (256,)),
                                               ("colonnade.vm", {}, (64, 64, 1024)), ("prospero.vm", {"no_column_inv": 1}, (64, 64, 1024))])
def test_ev_leaves_waits_that_remain(model, options, whd):
    """every slab rendered (colonnade.vm reads z; prospero.vm with the column short cuts off), slab_layers 1: slabs of 128 voxels, the
    most the option gives - two at 256^3, which is what that size has; the 64 x 64 x 1024 frames have eight slabs for the four slab
    contexts, so the tile chains of slabs 4 .. 7 wait for the events of slabs 0 .. 3 and the last slab's event is the image's.  Six
    frames queued; and one alone with a host output (normals on the tail stream)"""
    hip = context(frame_lanes=0, slab_layers=1, **options)
    s = F.Shape.from_vm(model_path(model), hip=hip)
    outs = [queue(s, *whd) for _ in range(6)]
    hip.sync()
    for i, o in enumerate(outs):
        check(o, want(model, *whd), f"{model} {whd} frame {i}")
    check(F.render3d(s, *whd)[0], want(model, *whd), f"{model} {whd} host image")
    del s, hip


@pytest.mark.parametrize("lanes", [0, 4])
@pytest.mark.parametrize("middle", ["cancelled", "host_output", "profiled"])
def test_early_exits_and_other_kinds_in_the_middle_of_a_queue(lanes, middle):
    """ten frames, the fifth of another kind: cancelled before the call (FHIP_ERR_CANCELLED; nothing of it is queued), with a host output,
    profiled.  The frames behind it take staging slots, buffer sets and the answer to "is the frame before under way?" from what it left"""
    hip = context(frame_lanes=lanes)
    p = F.Shape.from_vm(model_path("prospero.vm"), hip=hip)
    outs = [queue(p, 128 if i % 2 else 192) for i in range(4)]
    mid = None
    if middle == "cancelled":
        hip.cancel()
        with pytest.raises(F.FidgetHipError) as e:
            queue(p, 192)
        assert e.value.status == FHIP_ERR_CANCELLED
        hip.cancel_reset()
    elif middle == "host_output":
        mid = F.render3d(p, 192)[0]
    else:
        hip.profile(True)
        mid = queue(p, 192)
        hip.profile_read()
        hip.profile(False)
    outs += [queue(p, 128 if i % 2 else 192) for i in range(5)]
    hip.sync()
    for i, o in enumerate(outs):
        n = 128 if (i if i < 4 else i - 4) % 2 else 192
        check(o, want("prospero.vm", n), f"frame {i} around the {middle} one")
    if mid is not None:
        check(mid, want("prospero.vm", 192), f"the {middle} frame")
    del p, hip


def test_queue_status_reaches_a_verdict_and_the_lanes_give_the_same_image():
    """64 queued frames of one kind (1024^3, as the benchmark queues them: into one image): the tuner's windows (stage pipeline, lanes,
    stage pipeline) all see "the frame before is under way" - asked of the previous frame's own last event, whichever arrangement it
    took - and reach their verdict; under it, frame_lanes 4 and frame_lanes 0 give the same image, the oracle's at a size it renders quickly"""
    import torch
    hip = context(frame_lanes=4)
    p = F.Shape.from_vm(model_path("prospero.vm"), hip=hip)
    out = torch.zeros((1024, 1024, 4), dtype=torch.int32, device="cuda")
    hip.sync()
    for _ in range(64):
        F.render3d(p, 1024, out=out)
    hip.sync()
    print("lane_tune after 64 frames:", hip.lane_tune())
    assert hip.lane_tune()["phase"] == 4, hip.lane_tune()
    with_lanes = out.clone()
    hip.set_option("frame_lanes", 0)
    for _ in range(3):
        F.render3d(p, 1024, out=out)
    hip.sync()
    assert (with_lanes == out).all()
    assert int((out[..., 3] > 0).sum()) > 100000
    for lanes in (4, 0):
        hip.set_option("frame_lanes", lanes)
        outs = [queue(p, 256) for _ in range(4)]
        hip.sync()
        for o in outs:
            check(o, want("prospero.vm", 256), f"256^3 with frame_lanes {lanes}")
    del p, hip


# ---- rare mode of a frame whose leaf stage goes by the list: one launch for the large leaves' points and normals ---------------
def rare_context():
    hip = F.HipContext(0)
    hip.set_option("frame_lanes", 0)
    for opt in ("no_asm", "no_split", "no_asm_tiles", "no_tiles_v", "no_asm_normals", "no_columns_t"):      # (rare mode is the assembly kernels' frames': whatever the environment says)
        hip.set_option(opt, 0)
    return hip


_QUIET = []


def quiet_size():
    """the smallest size of prospero.vm whose frames meet no tape beyond the assembly kernels' files: after two of them the next frame is
    in rare mode (rare_frames() goes up).  Found once, on a context of its own."""
    if not _QUIET:
        for n in (256, 512, 1024):
            hip = rare_context()
            p = F.Shape.from_vm(model_path("prospero.vm"), hip=hip)
            for _ in range(3):
                F.render3d(p, n)
                hip.sync()
            up = hip.rare_frames() > 0
            del p, hip
            if up:
                _QUIET.append(n)
                break
    assert _QUIET, "no size of prospero.vm up to 1024^3 enters rare mode"
    return _QUIET[0]


def into_rare_mode(hip, shape):
    """two frames without large tapes: the second knows, and so does the frame after them"""
    n = quiet_size()
    for _ in range(2):
        F.render3d(shape, n)
        hip.sync()


def test_rare_mode_renders_unexpected_large_leaves_in_one_launch():
    """The situation of test_gpu_parity.py test_rare_mode_takes_the_large_tapes_it_does_not_expect: prospero.vm at 128^3 - its leaves are beyond
    the leaf kernel's file, its frame goes by the list - rendered by a frame in rare mode that does not expect them: the oracle's image, depth and
    normals bit for bit, from ONE launch of rare blocks (k_rare_leaves3d: the leaves' points, then the gradients of their own hits) where
    there were two; the frame after it, told, has the launches on their own again: the same image.  The same frame by the table (column_walk 3:
    the blocks behind k_classify3d's and k_hits3d's, as before), and bear.vm at 64^3 for depth."""
    hip = rare_context()
    big = F.Shape.from_vm(model_path("prospero.vm"), hip=hip)
    ref = want("prospero.vm", 128)
    check(F.render3d(big, 128)[0], ref, "a new context: the launches on their own")
    hip.sync()
    assert hip.rare_frames() == 0 and hip.rare_launches() == 0
    into_rare_mode(hip, big)
    n0, l0 = hip.rare_frames(), hip.rare_launches()
    assert n0 >= 1, "the frame after one without large tapes is not in rare mode"
    assert l0 == n0, f"{l0} launches of rare blocks in {n0} by-list frames in rare mode of one slab each: one per frame"
    b = F.render3d(big, 128)[0]             # ... and this one does not expect what it meets
    hip.sync()
    assert hip.rare_frames() == n0 + 1
    assert hip.rare_launches() == l0 + 1, "a by-list frame in rare mode makes one launch for its rare leaves"
    check(b, ref, "rare mode, by the list")
    c = F.render3d(big, 128)[0]             # told: on their own again
    hip.sync()
    assert hip.rare_frames() == n0 + 1 and hip.rare_launches() == l0 + 1
    check(c, ref, "the frame after")
    # by the table: the old path
    into_rare_mode(hip, big)
    n1, l1 = hip.rare_frames(), hip.rare_launches()
    with hip.options(column_walk=3):
        d = F.render3d(big, 128)[0]
        hip.sync()
    assert hip.rare_frames() == n1 + 1 and hip.rare_launches() == l1      # (not a by-list frame: no launch of rare blocks alone)
    check(d, ref, "rare mode, by the table")
    # queued, into device images: the frame in rare mode between frames that are told
    into_rare_mode(hip, big)
    outs = [queue(big, 128) for _ in range(4)]
    hip.sync()
    for i, o in enumerate(outs):
        check(o, ref, f"queued frame {i} behind rare mode")
    # bear.vm's transcendental tapes at a size where its leaves are beyond the leaf kernel's file too: depth
    bear = F.Shape.from_vm(model_path("bear.vm"), hip=hip)
    into_rare_mode(hip, big)
    e = F.render3d(bear, 64)[0]             # (44 registers for its points, 40 for its normals: the two launches as they were)
    hip.sync()
    assert (e["depth"] == want("bear.vm", 64)["depth"]).all()
    del big, bear, hip
