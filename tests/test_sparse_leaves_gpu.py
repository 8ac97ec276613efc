"""The leaf stage by the slab's list of leaves (option column_walk = 1 in frames whose tapes guarantee sparse columns: capi_render.hpp
by_list) against the same frames by the leaf table (3), by blocks (0) and the CPU oracle: depth and normals equal, bit for bit; frames
of other kinds in between on the same context; the large-tape routes; queued frames under both arrangements.  Every test is an
ordinary render."""
import numpy as np
import pytest

import fidget_amd as F
import oracle as O
from conftest import model_path
from test_gpu_parity import bench_camera, same_bits_f32

pytestmark = pytest.mark.gpu


def equal(a, b):
    return (a["depth"] == b["depth"]).all() and same_bits_f32(a["normal"], b["normal"])


def by_walks(shape, *whd, walks=(1, 3, 0), **kw):
    out = {}
    for cw in walks:
        with shape.hip.options(column_walk=cw):
            out[cw] = [F.render3d(shape, *whd, **kw)[0] for _ in range(2)]      # (the second frame's launches follow the first one's leaf count)
    return out


@pytest.mark.parametrize("name,whd", [("prospero.vm", (256,)), ("prospero.vm", (1024,)), ("prospero.vm", (200, 120, 300)), ("hi.vm", (256,))])
def test_list_table_blocks_and_oracle_agree(name, whd):
    p, o = F.Shape.from_vm(model_path(name)), O.Shape.from_vm(model_path(name))
    want = O.render3d(o, *whd)[0]
    assert want["depth"].max() > 0
    for cw, imgs in by_walks(p, *whd).items():
        for k, a in enumerate(imgs):
            assert (a["depth"] == want["depth"]).all(), f"column_walk {cw} frame {k}: {(a['depth'] != want['depth']).sum()} depths differ"
            assert same_bits_f32(a["normal"], want["normal"]), f"column_walk {cw} frame {k}: normals differ"


@pytest.mark.parametrize("part", [{"shard": 1, "n_shards": 4}, {"block": (5, (2, 2, 2))}, {"block": (1, (2, 2, 2))}])
def test_parts_of_a_frame(part):
    p = F.Shape.from_vm(model_path("prospero.vm"))
    got = by_walks(p, 512, **part)
    assert got[3][0]["depth"].max() > 0 or part.get("block", (5,))[0] == 1
    for cw in (1, 0):
        for a in got[cw]:
            assert equal(a, got[3][0]), f"column_walk {cw} against 3: {part}"


def test_a_front_slab_without_leaves():
    """nothing anywhere near the surface: the list is empty (count 0), the launches find no leaf, the image is the oracle's"""
    def build(be, off):
        c = be.Context()
        return be.Shape(c, c.add(c.add(c.abs(c.x()), c.abs(c.y())), off))
    for off in (2.5, -5.0):        # empty everywhere; full everywhere (every tile decided by its interval)
        p, o = build(F, off), build(O, off)
        want = O.render3d(o, 256)[0]
        for cw, imgs in by_walks(p, 256).items():
            for a in imgs:
                assert equal(a, want), f"offset {off} column_walk {cw}"
    # ... and a frame WITH leaves before and after on the same context: the count it left behind sizes nothing wrongly
    big = F.Shape.from_vm(model_path("prospero.vm"))
    ref = O.render3d(O.Shape.from_vm(model_path("prospero.vm")), 512)[0]
    none = build(F, 2.5)
    for s, n, w in ((big, 512, ref), (none, 512, None), (big, 512, ref), (big, 512, ref)):
        a = F.render3d(s, n)[0]
        if w is not None:
            assert equal(a, w)


def test_frames_of_other_kinds_in_between():
    """one context, queued frames: sparse frames (two sizes) switching with bear.vm, colonnade.vm and a rotated camera - buffer sets and the
    carried-back leaf count must not leak from one kind to the next"""
    import torch
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    cam = bench_camera(0.0)
    jobs = [("prospero.vm", 1024, None), ("bear.vm", 128, None), ("prospero.vm", 256, None), ("colonnade.vm", 256, None), ("prospero.vm", 1024, None),
            ("prospero.vm", 256, cam), ("prospero.vm", 256, None), ("prospero.vm", 1024, None), ("colonnade.vm", 512, None), ("prospero.vm", 1024, None)]
    shapes = {m: F.Shape.from_vm(model_path(m), hip=hip) for m, _, _ in jobs}
    outs = [torch.zeros((n, n, 4), dtype=torch.int32, device="cuda") for _, n, _ in jobs]
    for rep in range(3):
        for i, (m, n, c) in enumerate(jobs):
            F.render3d(shapes[m], n, world_to_model=c, out=outs[i])
    hip.sync()
    osh = {m: O.Shape.from_vm(model_path(m)) for m in shapes}
    seen = {}
    for i, (m, n, c) in enumerate(jobs):
        key = (m, n, c is not None)
        if key not in seen:
            seen[key] = O.render3d(osh[m], n, world_to_model=c)[0]
        b = seen[key]
        a = outs[i].cpu().numpy().view(np.uint32).reshape(n, n, 4)
        assert (a[:, :, 3] == b["depth"]).all(), f"frame {i} ({m} {n}): {(a[:, :, 3] != b['depth']).sum()} depths differ"
        an = a[:, :, :3].copy().view(np.float32)
        if m != "bear.vm":       # (transcendental tape: values within the library's bound of the oracle's - tests/test_gpu_parity.py test_render3d_bear)
            assert same_bits_f32(an, b["normal"]), f"frame {i} ({m} {n}): normals differ"
    del shapes, hip


@pytest.mark.parametrize("walk", [1, 3])
def test_large_leaves_in_and_out_of_rare_mode(walk):
    """leaves beyond the assembly kernels' register files (prospero.vm at 128^3 and 64^3) in a sparse frame: met unexpectedly in rare mode
    (the blocks left of k_classify3d and k_hits3d take them; the push itself lists their footprints for the normals), and in the frames
    after, when the launches for them are made on their own again"""
    hip = F.HipContext(0)
    hip.set_option("frame_lanes", 0)
    hip.set_option("column_walk", walk)
    for opt in ("no_asm", "no_split", "no_asm_tiles", "no_tiles_v", "no_asm_normals", "no_columns_t"):
        hip.set_option(opt, 0)
    p, o = F.Shape.from_vm(model_path("prospero.vm"), hip=hip), O.Shape.from_vm(model_path("prospero.vm"))
    for n in (128, 64):
        want = O.render3d(o, n)[0]
        for _ in range(2):
            F.render3d(p, 1024)
            hip.sync()
        n0 = hip.rare_frames()
        assert n0 >= 1
        a = F.render3d(p, n)[0]           # rare mode on, and the frame meets what it does not expect
        hip.sync()
        assert hip.rare_frames() == n0 + 1
        assert equal(a, want), f"{n}^3 in rare mode: {(a['depth'] != want['depth']).sum()} depths differ"
        for _ in range(2):                # flipped off: the kernels for the large tapes on their own
            b = F.render3d(p, n)[0]
            hip.sync()
            assert hip.rare_frames() == n0 + 1
            assert equal(b, want), f"{n}^3 after rare mode"
    del p, hip


@pytest.mark.parametrize("lanes", [4, 0])
def test_queued_frames_under_both_arrangements(lanes):
    """frames queued back to back through the tuner's windows (stage pipeline, frame lanes, stage pipeline again) and beyond: every image the
    oracle's, with the lanes and without them"""
    import torch
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    hip.set_option("frame_lanes", lanes)
    n = 512
    shape = F.Shape.from_vm(model_path("prospero.vm"), hip=hip)
    outs = [torch.zeros((n, n, 4), dtype=torch.int32, device="cuda") for _ in range(7)]
    for i in range(100):
        F.render3d(shape, n, out=outs[i % 7])
    hip.sync()
    b = O.render3d(O.Shape.from_vm(model_path("prospero.vm")), n)[0]
    for o in outs:
        a = o.cpu().numpy().view(np.uint32).reshape(n, n, 4)
        assert (a[:, :, 3] == b["depth"]).all() and same_bits_f32(a[:, :, :3].copy().view(np.float32), b["normal"])
    if lanes:
        assert F.lib().fhip_debug_lane_frames(hip._h) >= 10
    del shape, hip


def test_column_walk_0_and_2_still_honoured():
    """0: never by columns; 2: always by the table's columns, also where a column holds many leaves (bear.vm, a rotated camera) - same images"""
    for name, n, cam in (("bear.vm", 128, None), ("prospero.vm", 256, bench_camera(0.0)), ("prospero.vm", 256, None)):
        p = F.Shape.from_vm(model_path(name))
        got = by_walks(p, n, walks=(0, 2, 1, 3), world_to_model=cam)
        for cw in (2, 1, 3):
            for a in got[cw]:
                assert (a["depth"] == got[0][0]["depth"]).all() and same_bits_f32(a["normal"], got[0][0]["normal"]), f"{name} column_walk {cw}"
