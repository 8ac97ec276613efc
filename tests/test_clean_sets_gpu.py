"""Clean buffer sets and the head of the tile chain (capi_render.hpp, frame_plan.hpp): a finished 3D frame hands z-buffer, normals and
min-depth pyramid back zeroed, so the next frame of the set skips its clears when it is of the same size; and in a frame of one coarse
level the parked parents' flags, the frame mark, the fork of the slab contexts and the first slab's reset ride on the tile chain's first
kernel.  Nothing of that may show in an image: frames that reuse a set after a frame of another shape, size or kind, after a cancelled
frame, after a frame whose image went to the host - every one the CPU oracle's, depth and normals bit for bit.  Every test is an ordinary
render."""
import numpy as np
import pytest

import fidget_amd as F
import oracle as O
from conftest import model_path
from test_gpu_parity import same_bits_f32

pytestmark = pytest.mark.gpu

RAGGED = (200, 136, 96)      # root blocks with inactive children, an image that is no multiple of a root tile
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


@pytest.mark.parametrize("whd", [(256,), RAGGED])
@pytest.mark.parametrize("no_pipeline", [0, 1])
def test_ten_frames_back_to_back(whd, no_pipeline):
    """256^3: one full block of 64 root children; ten frames on one context, so each of its four sets is taken at least twice (no_pipeline:
    the one set ten times) and all but a set's first frame skip their clears"""
    hip = context(no_pipeline=no_pipeline)
    p = F.Shape.from_vm(model_path("prospero.vm"), hip=hip)
    outs = [queue(p, *whd) for _ in range(10)]
    hip.sync()
    assert want("prospero.vm", *whd)["depth"].max() > 0
    for i, o in enumerate(outs):
        check(o, want("prospero.vm", *whd), f"frame {i}")
    del p, hip


def test_no_ambiguous_child():
    """far from the surface in the whole view: empty everywhere, full everywhere - the root push parks nothing, the head of the tile chain
    finds an empty queue; and a frame with a surface on the same sets before and after"""
    def build(be, off, **kw):
        c = be.Context()
        return be.Shape(c, c.add(c.add(c.abs(c.x()), c.abs(c.y())), off), **kw)
    hip = context()
    p = F.Shape.from_vm(model_path("prospero.vm"), hip=hip)
    for off in (2.5, -5.0):
        s, ref = build(F, off, hip=hip), O.render3d(build(O, off), 256)[0]
        outs = [queue(p, 256)] + [queue(s, 256) for _ in range(5)] + [queue(p, 256) for _ in range(4)]
        hip.sync()
        for i, o in enumerate(outs):
            check(o, want("prospero.vm", 256) if i == 0 or i > 5 else ref, f"offset {off} frame {i}")
    del p, hip


@pytest.mark.parametrize("no_pipeline", [0, 1])
def test_sizes_and_kinds_in_turn(no_pipeline):
    """256^3, 128^3, 256^3, a frame with the column short cuts off (another tile hierarchy: another pyramid), 256^3 - three times round, so
    every set meets every change of size and kind: a record that does not match means the full clears"""
    hip = context(no_pipeline=no_pipeline)
    p = F.Shape.from_vm(model_path("prospero.vm"), hip=hip)
    outs = []
    for _ in range(3):
        for n, nci in ((256, 0), (128, 0), (256, 0), (256, 1), (256, 0)):
            with hip.options(no_column_inv=nci):
                outs.append((n, nci, queue(p, n)))
    hip.sync()
    for i, (n, nci, o) in enumerate(outs):
        check(o, want("prospero.vm", n), f"frame {i} ({n}^3, no_column_inv {nci})")
    del p, hip


@pytest.mark.parametrize("no_pipeline", [0, 1])
def test_after_a_cancelled_frame_and_after_a_host_image(no_pipeline):
    hip = context(no_pipeline=no_pipeline)
    p, h = F.Shape.from_vm(model_path("prospero.vm"), hip=hip), F.Shape.from_vm(model_path("hi.vm"), hip=hip)
    outs = [queue(h, 256) for _ in range(5)]
    hip.cancel()
    with pytest.raises(F.FidgetHipError):
        queue(p, 256)
    hip.cancel_reset()
    outs2 = [queue(p, 256) for _ in range(5)]
    host = F.render3d(h, 256)[0]       # the image goes to the host: such a frame leaves no record
    outs3 = [queue(p, 256) for _ in range(5)]
    host2 = F.render3d(p, 256)[0]
    hip.sync()
    for i, o in enumerate(outs):
        check(o, want("hi.vm", 256), f"frame {i} before the cancelled one")
    for i, o in enumerate(outs2):
        check(o, want("prospero.vm", 256), f"frame {i} after the cancelled one")
    check(host, want("hi.vm", 256), "host image")
    for i, o in enumerate(outs3):
        check(o, want("prospero.vm", 256), f"frame {i} after the host image")
    check(host2, want("prospero.vm", 256), "second host image")
    del p, h, hip


@pytest.mark.parametrize("lanes", [4, 0])
def test_two_shapes_of_one_size_in_turn(lanes):
    """the record matches every time, the shapes do not: whatever a frame left behind would show in the other shape's image.  Long enough
    for the tuner's windows (stage pipeline, frame lanes - child contexts with a set each -, stage pipeline again)"""
    hip = context(frame_lanes=lanes)
    shapes = [F.Shape.from_vm(model_path(m), hip=hip) for m in ("prospero.vm", "hi.vm")]
    outs = [queue(shapes[i % 2], 256) for i in range(60)]
    hip.sync()
    for i, o in enumerate(outs):
        check(o, want(("prospero.vm", "hi.vm")[i % 2], 256), f"frame {i}")
    del shapes, hip


@pytest.mark.parametrize("whd", [(256,), RAGGED])
def test_equal_to_the_short_cuts_off(whd):
    """the flags of the parked parents are the entry's own wave's now: the same image with no sharing of tiles along z at all (no_zrep 1) and
    with column invariance off everywhere"""
    hip = context()
    p = F.Shape.from_vm(model_path("prospero.vm"), hip=hip)
    for opts in ({}, {"no_zrep": 1}, {"no_column_inv": 1}):
        with hip.options(**opts):
            outs = [queue(p, *whd) for _ in range(3)] + [F.render3d(p, *whd)[0]]
            hip.sync()
        for i, o in enumerate(outs):
            check(o, want("prospero.vm", *whd), f"{opts} frame {i}")
    del p, hip
