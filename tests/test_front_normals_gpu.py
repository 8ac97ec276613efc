"""Whole front-slab-only frames make no normals launches (frame_schedule.hpp normals_on; capi_render.hpp render_slabs): every hit of such a
frame is clamped to (0, 0, 1, depth) by k_finish3d, so nothing may show in an image.  Every test is an ordinary render compared word for word -
depth and normals - with the CPU oracle's image, or, for parts of a frame (which the oracle does not render), with the same part rendered
with the column short cuts off; the frames that keep their normals - a tilted camera, a back z-block - are held to the same references."""
import numpy as np
import pytest

import fidget_amd as F
import oracle as O
from conftest import model_path
from test_gpu_parity import same_bits_f32

pytestmark = pytest.mark.gpu


def dots_text(n=20, r=0.03):
    """400 discs in x and y, no z: 1 282 ops, 24 registers, a root min over 400 terms - long enough for the root level by term groups, so small
    images get root tiles of 32^3 straight above the leaves as prospero.vm's do, with no tape beyond the leaf kernel's register file"""
    lines, k, acc = ["_x var-x", "_y var-y"], 0, None
    for i in range(n):
        for j in range(n):
            cx, cy = -0.875 + 1.75 * i / (n - 1), -0.875 + 1.75 * j / (n - 1)
            p = f"_{k}"
            lines += [f"{p}a const {cx}", f"{p}b sub _x {p}a", f"{p}c mul {p}b {p}b", f"{p}d const {cy}", f"{p}e sub _y {p}d", f"{p}f mul {p}e {p}e",
                      f"{p}g add {p}c {p}f", f"{p}h const {r * r * (1 + 0.3 * ((i + j) % 3))}", f"{p}i sub {p}g {p}h"]
            if acc is not None:
                lines.append(f"{p}m min {acc} {p}i")
            acc = f"{p}m" if acc is not None else f"{p}i"
            k += 1
    return "\n".join(lines) + "\n"


_SHAPES = {}


def shapes(name, hip=None):
    """(device shape on `hip` or the default context, oracle shape); the oracle's is made once per model"""
    text = dots_text() if name == "dots" else model_path(name)
    if name not in _SHAPES:
        _SHAPES[name] = O.Shape.from_vm(text)
    return F.Shape.from_vm(text, hip=hip), _SHAPES[name]


_WANT = {}


def want(name, whd, cam=None):
    key = (name, whd, None if cam is None else cam.tobytes())
    if key not in _WANT:
        _WANT[key] = O.render3d(shapes(name)[1], *whd, world_to_model=cam)[0]
    return _WANT[key]


def check(got, ref, what):
    if hasattr(got, "cpu"):
        a = got.cpu().numpy().view(np.uint32)
        got = {"depth": a[..., 3], "normal": a[..., :3].copy().view(np.float32)}
    assert (got["depth"] == ref["depth"]).all(), f"{what}: {(got['depth'] != ref['depth']).sum()} depths differ"
    assert same_bits_f32(got["normal"], ref["normal"]), f"{what}: normals differ"


def rot(axis, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    m = np.eye(4, dtype=np.float32)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def shift_x(dx):
    m = np.eye(4, dtype=np.float32)
    m[0, 3] = dx
    return m


@pytest.mark.parametrize("name", ["dots", "prospero.vm"])
@pytest.mark.parametrize("whd", [(64, 64, 64), (96, 64, 40)])
def test_a_shape_without_z_blocking(name, whd):
    """64^3 (two coarse levels), and 96 x 64 x 40: root tiles of 32^3 above the leaves, a width that is no multiple of 32, a depth that is no
    multiple of 32, root tiles and footprints hanging over the image's edge and its top.  Two blocking frames (the second one's launches
    follow the first one's report), by the list of leaves, by the table and by blocks"""
    s, _ = shapes(name)
    ref = want(name, whd)
    assert ref["depth"].max() == whd[2] and (ref["depth"] > 0).sum() > 100
    inside = ref["depth"] > 0
    assert (ref["normal"][inside] == np.array([0, 0, 1], np.float32)).all()      # (what the rule rests on: every hit of such a frame is clamped)
    for walk in (1, 3, 0):
        with s.hip.options(column_walk=walk):
            for k in range(2):
                check(F.render3d(s, *whd)[0], ref, f"{name} {whd} column_walk {walk} frame {k}")


def test_twelve_queued_frames_with_a_moving_camera():
    """prospero.vm at 256^3, the camera one step further in x every frame (four positions in turn, so the root children differ from frame to
    frame), queued back to back into images of their own: the root levels' turns wrap and the four buffer sets come round three times"""
    import torch
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    hip.set_option("frame_lanes", 0)
    s, _ = shapes("prospero.vm", hip)
    cams = [shift_x(0.07 * k) for k in range(4)]
    outs = [torch.zeros((256, 256, 4), dtype=torch.int32, device="cuda") for _ in range(12)]
    for i, o in enumerate(outs):
        F.render3d(s, 256, world_to_model=cams[i % 4], out=o)
    hip.sync()
    for i, o in enumerate(outs):
        check(o, want("prospero.vm", (256, 256, 256), cams[i % 4]), f"queued frame {i}")
    del s, hip


@pytest.mark.parametrize("name,n", [("dots", 128), ("prospero.vm", 128)])
def test_a_camera_rotated_about_z_and_one_tilted_about_x(name, n):
    """rotated about z the frame still reads nothing that changes along a pixel column: front slab only, no normals launch; tilted about x it
    does: every slab, and its normals are the oracle's gradients"""
    s, _ = shapes(name)
    flat, tilted = rot(2, 30.0), rot(0, 25.0)
    ref = want(name, (n, n, n), tilted)
    hit = (ref["depth"] > 0) & (ref["depth"] < n - 1)
    assert hit.sum() > 100 and (ref["normal"][hit] != np.array([0, 0, 1], np.float32)).any()      # (this frame has normals to get right)
    for k in range(2):
        check(F.render3d(s, n, world_to_model=flat)[0], want(name, (n, n, n), flat), f"{name} rotated about z, frame {k}")
        check(F.render3d(s, n, world_to_model=tilted)[0], ref, f"{name} tilted about x, frame {k}")


def test_frames_with_and_without_normals_in_turn_on_one_buffer_set():
    """a host image takes the context's one set every time: a frame whose hits keep their leaf's number in the z-buffer (no normals kernel
    took it out) hands the set to a frame that computes normals, and back"""
    s, _ = shapes("dots")
    tilted = rot(0, 25.0)
    for k in range(3):
        check(F.render3d(s, 128)[0], want("dots", (128, 128, 128)), f"whole frame {k}")
        check(F.render3d(s, 128, world_to_model=tilted)[0], want("dots", (128, 128, 128), tilted), f"tilted frame {k}")


@pytest.mark.parametrize("part", [{"shard": 1, "n_shards": 2}, {"block": (1, (2, 1, 1))}, {"block": (1, (1, 1, 2))}, {"block": (0, (1, 1, 2))}])
def test_parts_of_a_frame_keep_their_normals(part):
    """a shard, a block of columns, the front z-block and the BACK z-block (whose hits lie below the volume's top: real gradients) of
    prospero.vm at 256^3: word for word the same part rendered with the column short cuts off, which renders every slab and always computed
    its normals; the back block has gradients other than (0, 0, 1)"""
    s, _ = shapes("prospero.vm")
    with s.hip.options(no_column_inv=1):
        ref = F.render3d(s, 256, **part)[0]
    assert ref["depth"].max() > 0
    if part.get("block") == (0, (1, 1, 2)):
        hit = ref["depth"] > 0
        assert ref["depth"].max() < 255 and (ref["normal"][hit] != np.array([0, 0, 1], np.float32)).any()
    for k in range(2):
        check(F.render3d(s, 256, **part)[0], ref, f"{part} frame {k}")


def test_the_shards_of_a_frame_make_the_oracles_image():
    s, _ = shapes("prospero.vm")
    ref = want("prospero.vm", (256, 256, 256))
    parts = [F.render3d(s, 256, shard=k, n_shards=2)[0] for k in range(2)]
    depth = np.maximum(parts[0]["depth"], parts[1]["depth"])
    assert (depth == ref["depth"]).all()
    normal = np.where((parts[0]["depth"] >= parts[1]["depth"])[..., None], parts[0]["normal"], parts[1]["normal"])
    assert same_bits_f32(normal, ref["normal"])
