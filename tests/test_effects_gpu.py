"""The image-effects kernels (fidget_amd/csrc/effects.hip) and k_merge_depth against tests/effects_ref.py - a restatement of effects.rs
that shares no text with the kernels or the oracle - on inputs that reach the rules rendered cubic frames leave alone: non-square images,
tied window scores, zero / NaN / infinite normals, images smaller than a window, device-resident inputs, the error returns.

Every comparison is bit for bit (NaN equal to NaN), to_rgba_distance included: each operation is IEEE f32 with contraction off, divide and
sqrt correctly rounded, and exp / cos are the routines tests/test_gpu_math.py holds to the host's libm.  tests/test_effects_ref.py shows
that each single-rule mutant of the reference changes 3 pixels or more of some input used here."""
import ctypes as C

import numpy as np
import pytest

import effects_ref as R
from conftest import model_path

pytestmark = pytest.mark.gpu

UNSUPPORTED = 6
GEOMETRY = [c[0] for c in R.geometry_cases()]


def case(name):
    return next(c for c in R.geometry_cases() if c[0] == name)


def host_chain(F, name, hip=None):
    """every F.* effect of one geometry case through host buffers, against the reference"""
    _, img, d, k, nz = case(name)
    dn, s, b, rgb, rgb0 = R.chain(name)
    assert R.same(F.denoise_normals(img, hip=hip), dn), name
    assert R.same(F.compute_ssao(dn, d, k, nz, hip=hip), s), name
    assert R.same(F.blur_ssao(s, hip=hip), b), name
    assert R.same(F.apply_shading(dn, d, b, hip=hip), rgb), name
    assert R.same(F.apply_shading(dn, d, hip=hip), rgb0), name


@pytest.mark.parametrize("name", GEOMETRY)
def test_host_path_equals_reference(name):
    import fidget_amd as F
    host_chain(F, name)
    _, img, d, k, nz = case(name)
    s = R.chain(name)[1]
    assert R.same(F.compute_ssao(img, d, k, nz), R.compute_ssao(img, d, k, nz))            # zero, NaN and infinite normals in SSAO
    assert R.same(F.apply_shading(img, d, s), R.apply_shading(img, d, s))                  # ... and through the shading's cast


def test_host_blur_of_ssao_maps():
    import fidget_amd as F
    for name, s in R.ssao_maps():
        assert R.same(F.blur_ssao(s), R.blur_ssao(s)), name


def test_host_colour_maps_are_exact():
    import fidget_amd as F
    img = R.distance_image()
    assert R.same(F.to_rgba_bitmap(img), R.to_rgba_bitmap(img))
    assert R.same(F.to_rgba_bitmap(img, True), R.to_rgba_bitmap(img, True))
    assert R.same(F.to_debug_bitmap(img), R.to_debug_bitmap(img))
    got, want = F.to_rgba_distance(img), R.to_rgba_distance(img)
    bad = np.argwhere((got != want).any(axis=-1))
    assert not len(bad), [(hex(int(img.view(np.uint32)[tuple(p)])), got[tuple(p)].tolist(), want[tuple(p)].tolist()) for p in bad[:8]]


# ---- device-resident images: on_device = 1, asynchronous on the context's stream ----------------------------------------------
def ptr(t):
    return C.c_void_p(t.data_ptr())


def to_device(a):
    import torch
    a = np.array(a)                  # (a writable copy: the inputs are shared and read-only)
    if a.dtype == R.GEOMETRY_PIXEL:
        a = a.view(np.int32).reshape(a.shape + (4,))
    return torch.from_numpy(a).cuda()


def geometry_of(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(R.GEOMETRY_PIXEL)[..., 0]


def device_chain(F, hip, image, w, h, d, kernel, noise):
    """denoise -> ssao -> blur -> shade (with and without the occlusion map) on device tensors, nothing waited for in between;
    -> the five output tensors, not yet synchronised"""
    import torch
    L = F.lib()
    k, nz = to_device(np.ascontiguousarray(kernel.T)), to_device(np.ascontiguousarray(noise.T))       # [n][3], [m][2]
    dn = torch.zeros((h, w, 4), dtype=torch.int32, device="cuda")
    s, b = (torch.zeros((h, w), dtype=torch.float32, device="cuda") for _ in range(2))
    rgb, rgb0 = (torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    hip.check(L.fhip_denoise_normals(hip._h, ptr(image), w, h, ptr(dn), 1))
    hip.check(L.fhip_compute_ssao(hip._h, ptr(dn), w, h, d, ptr(k), k.shape[0], ptr(nz), nz.shape[0], ptr(s), 1))
    hip.check(L.fhip_blur_ssao(hip._h, ptr(s), w, h, ptr(b), 1))
    hip.check(L.fhip_apply_shading(hip._h, ptr(dn), w, h, d, ptr(b), ptr(rgb), 1))
    hip.check(L.fhip_apply_shading(hip._h, ptr(dn), w, h, d, None, ptr(rgb0), 1))
    return dn, s, b, rgb, rgb0, (k, nz)


def test_device_path_equals_reference_and_host_path():
    import torch
    import fidget_amd as F
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    runs = []
    for name, img, d, k, nz in R.geometry_cases():
        h, w = img.shape
        t = to_device(img)
        runs.append((name, t, device_chain(F, hip, t, w, h, d, k, nz)))
    dist = R.distance_image()
    dt = to_device(dist)
    maps = [torch.zeros(dist.shape + (4,), dtype=torch.uint8, device="cuda") for _ in range(4)]
    for mode, o in enumerate(maps):
        hip.check(F.lib().fhip_to_rgba(hip._h, ptr(dt), dist.shape[1], dist.shape[0], mode, ptr(o), 1))
    hip.sync()
    for name, _, (dn, s, b, rgb, rgb0, _) in runs:
        want = R.chain(name)
        got = (geometry_of(dn), s.cpu().numpy(), b.cpu().numpy(), rgb.cpu().numpy(), rgb0.cpu().numpy())
        _, img, d, k, nz = case(name)
        host = (F.denoise_normals(img), F.compute_ssao(want[0], d, k, nz), F.blur_ssao(want[1]), F.apply_shading(want[0], d, want[2]),
                F.apply_shading(want[0], d))
        for stage, g, r, hst in zip(("denoise", "ssao", "blur", "shade", "shade without ssao"), got, want, host):
            assert R.same(g, r), (name, stage, R.differing(g, r))
            assert R.same(g, hst), (name, stage, "host path")
    want = (R.to_rgba_bitmap(dist), R.to_rgba_bitmap(dist, True), R.to_debug_bitmap(dist), R.to_rgba_distance(dist))
    host = (F.to_rgba_bitmap(dist), F.to_rgba_bitmap(dist, True), F.to_debug_bitmap(dist), F.to_rgba_distance(dist))
    for mode, o in enumerate(maps):
        assert R.same(o.cpu().numpy(), want[mode]) and R.same(o.cpu().numpy(), host[mode]), mode
    del hip


def test_rendered_non_cubic_frame_through_the_device_chain():
    """a frame rendered into device memory at 120 x 88 x 72 - neither side a multiple of the 16 x 16 block - with a rotated camera, consumed
    where it lies; every stage against the reference applied to the downloaded frame"""
    import torch
    import fidget_amd as F
    w, h, d = 120, 88, 72
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    shape = F.Shape.from_vm(model_path("colonnade.vm"), hip=hip)
    ca, sa, cb, sb = np.cos(0.7), np.sin(0.7), np.cos(0.4), np.sin(0.4)
    cam = (np.array([[cb, -sb, 0, 0], [sb, cb, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]) @ np.array([[1, 0, 0, 0], [0, ca, -sa, 0], [0, sa, ca, 0], [0, 0, 0, 1]])
           @ np.diag([1.25, 1.25, 1.25, 1.0])).astype(np.float32)
    k, nz = R.ssao_matrices(64, 256)
    frame = torch.zeros((h, w, 4), dtype=torch.int32, device="cuda")
    F.render3d(shape, w, h, d, world_to_model=cam, out=frame)
    dn, s, b, rgb, rgb0, _ = device_chain(F, hip, frame, w, h, d, k, nz)
    hip.sync()
    img = geometry_of(frame)
    filled = img["depth"] != 0
    assert 0.1 < filled.mean() < 0.95 and (filled & (img["normal"][..., 2] <= 0)).sum() >= 3       # a frame with back-facing pixels to denoise
    r_dn = R.denoise_normals(img)
    assert R.same(geometry_of(dn), r_dn), R.differing(geometry_of(dn), r_dn)
    r_s = R.compute_ssao(r_dn, d, k, nz)
    assert R.same(s.cpu().numpy(), r_s), R.differing(s.cpu().numpy(), r_s)
    r_b = R.blur_ssao(r_s)
    assert R.same(b.cpu().numpy(), r_b), R.differing(b.cpu().numpy(), r_b)
    assert R.same(rgb.cpu().numpy(), R.apply_shading(r_dn, d, r_b))
    assert R.same(rgb0.cpu().numpy(), R.apply_shading(r_dn, d))
    del shape, hip


def test_interleaved_sizes_on_one_context():
    """the host path stages through the context's io_a..io_d: a 1 x 1 image between two large ones must find them as good as new"""
    import fidget_amd as F
    hip = F.HipContext(0)
    for name in ("geom19x37x50", "geom1x1x1", "geom37x19x11", "geom1x1x1", "geom19x37x50"):
        host_chain(F, name, hip=hip)
    del hip


def test_error_returns():
    import fidget_amd as F
    L, hip = F.lib(), F.HipContext(0)
    _, img, d, k, nz = case("geom33x17x17")
    h, w = img.shape
    img = np.array(img)
    kt, nt = np.ascontiguousarray(k.T), np.ascontiguousarray(nz.T)
    p = lambda a: a.ctypes.data_as(C.c_void_p)           # noqa: E731
    mark = 0xAB
    geo, f32, rgb, rgba = (np.full((h, w, n), mark, np.uint8) for n in (16, 4, 3, 4))
    s = np.array(R.chain("geom33x17x17")[1])
    dist = np.array(R.distance_image())
    ssao = lambda wd, ht, dp, n_k, n_n: L.fhip_compute_ssao(hip._h, p(img), wd, ht, dp, p(kt), n_k, p(nt), n_n, p(f32), 0)      # noqa: E731
    assert ssao(w, h, d, 0, len(nt)) == UNSUPPORTED                      # empty kernel
    assert ssao(w, h, d, len(kt), 0) == UNSUPPORTED                      # empty noise
    assert ssao(w, h, 0, len(kt), len(nt)) == UNSUPPORTED                # zero depth
    assert L.fhip_apply_shading(hip._h, p(img), w, h, 0, None, p(rgb), 0) == UNSUPPORTED
    for mode in (-1, 4):
        assert L.fhip_to_rgba(hip._h, p(dist), dist.shape[1], dist.shape[0], mode, p(rgba), 0) == UNSUPPORTED
    for wd, ht in ((0, h), (w, 0), (0, 0)):                              # nothing to do: OK, and nothing written
        assert L.fhip_denoise_normals(hip._h, p(img), wd, ht, p(geo), 0) == 0
        assert ssao(wd, ht, d, len(kt), len(nt)) == 0
        assert L.fhip_blur_ssao(hip._h, p(s), wd, ht, p(f32), 0) == 0
        assert L.fhip_apply_shading(hip._h, p(img), wd, ht, d, None, p(rgb), 0) == 0
        assert L.fhip_to_rgba(hip._h, p(dist), wd, ht, 3, p(rgba), 0) == 0
    for out in (geo, f32, rgb, rgba):
        assert (out == mark).all()
    assert R.same(F.denoise_normals(img, hip=hip), R.chain("geom33x17x17")[0])          # the context still works after the refusals
    del hip


@pytest.mark.parametrize("n", [1, 257, 4099])
def test_merge_depth_on_constructed_pixels(n):
    """k_merge_depth on pixels built for its rule: back deeper, front deeper, ties with different normals (front stays), either side at
    D - 1 and at D, both empty; and image_depth 0, which switches the clamp off"""
    import torch
    import fidget_amd as F
    hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
    front, back = R.merge_case(n)
    for image_depth in (64, 0):
        f, b = to_device(front), to_device(back)
        F.merge_depth(f, b, image_depth, hip=hip)
        hip.sync()
        want = R.merge_depth(front, back, image_depth)
        got = geometry_of(f)
        assert R.same(got, want), (image_depth, R.differing(got, want, 1))
        assert R.same(geometry_of(b), back)
    del hip
