"""The renders and what is made of their images: `render2d`, `render3d`, `merge_depth`, the RawDistancePixel helpers, the image effects
(fidget_raster::effects) and the `to_*` bitmaps.  `_var_arrays` and `_dev_ptr` are shared with the later subjects."""
import ctypes as C

import numpy as np

from ._abi import GEOMETRY_PIXEL, _Cfg2D, _Cfg3D, _p, lib
from .context import default_context


def _var_arrays(shape, vars_):
    vars_ = vars_ or {}
    k = np.array(list(vars_.keys()), dtype=np.uint64)
    v = np.array(list(vars_.values()), dtype=np.float32)
    return k, v


def _dev_ptr(out):
    """Accept a torch CUDA tensor (device pointer) or None."""
    if out is None:
        return None
    return C.c_void_p(out.data_ptr())


def render2d(shape, width, height=None, z=0.0, pixel_perfect=False, world_to_model=None, tile_sizes=None,
             vars=None, out=None, mode=None, threads=None):
    """fidget_raster::pixel::render on the GPU.  Returns (float32 [h,w] RawDistancePixel image, stats, seconds);
    with `out` (a torch CUDA float32 tensor) the call is asynchronous and returns (out, None, None)."""
    height = width if height is None else height
    hip = shape.hip
    ts = np.array(tile_sizes, dtype=np.uint32) if tile_sizes else None
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    vk, vv = _var_arrays(shape, vars)
    ax = None
    if shape._vars is not None:
        ax = np.array(shape._vars, dtype=np.int32)
        vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
    cfg = _Cfg2D(width, height, _p(w2m), z, int(pixel_perfect), _p(ts), 0 if ts is None else len(ts), _p(vk), _p(vv),
                 len(vk), _p(ax))
    if out is not None:
        st = lib().fhip_render2d(hip._h, shape._h, C.byref(cfg), _dev_ptr(out), 1)
        if st == 4:
            raise ValueError("MissingVar")
        hip.check(st)
        return out, None, None
    img = np.zeros((height, width), dtype=np.float32)
    import time
    t0 = time.perf_counter()
    st = lib().fhip_render2d(hip._h, shape._h, C.byref(cfg), _p(img), 0)
    dt = time.perf_counter() - t0
    if st == 4:
        raise ValueError("MissingVar")
    hip.check(st)
    return img, {}, dt


def render3d(shape, width, height=None, depth=None, world_to_model=None, tile_sizes=None, vars=None, out=None,
             shard=0, n_shards=1, mode=None, threads=None, block=None, host_out=None):
    """fidget_raster::voxel::render on the GPU.  Returns (GeometryPixel [h,w] image, stats, seconds).
    Multi-GPU parts: (shard, n_shards) = root-tile columns round robin; block = (index, (nx, ny, nz)) = one block of an
    nx x ny x nz split of the volume (fhip_render3d_block)."""
    height = width if height is None else height
    depth = width if depth is None else depth
    hip = shape.hip
    if out is not None and world_to_model is None and not tile_sizes and not vars and shape._vars is None:
        # (the same frame again - what a caller that holds its RenderConfig does: the configuration struct is kept with the shape, the call
        # is the C call and nothing else; queued frames are bound by the thread that queues them)
        key = (width, height, depth, shard, n_shards, None if block is None else (int(block[0]), tuple(int(b) for b in block[1])))
        frames = shape.__dict__.setdefault("_frames", {})
        ent = frames.get(key)
        if ent is None:
            cfg = _Cfg3D(width, height, depth, None, None, 0, None, None, 0, None)
            split = None if block is None else np.array(block[1], dtype=np.uint32)
            ent = frames[key] = (cfg, C.byref(cfg), split, _p(split))
        if block is not None:
            st = lib().fhip_render3d_block(hip._h, shape._h, ent[1], C.c_void_p(out.data_ptr()), 1, key[5][0], ent[3])
        else:
            st = lib().fhip_render3d_shard(hip._h, shape._h, ent[1], C.c_void_p(out.data_ptr()), 1, shard, n_shards)
        if st:
            if st == 4:
                raise ValueError("MissingVar")
            hip.check(st)
        return out, None, None
    ts = np.array(tile_sizes, dtype=np.uint32) if tile_sizes else None
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    vk, vv = _var_arrays(shape, vars)
    ax = None
    if shape._vars is not None:
        ax = np.array(shape._vars, dtype=np.int32)
        vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
    cfg = _Cfg3D(width, height, depth, _p(w2m), _p(ts), 0 if ts is None else len(ts), _p(vk), _p(vv), len(vk), _p(ax))
    def call(ptr, dev):
        if block is not None:
            split = np.array(block[1], dtype=np.uint32)
            return lib().fhip_render3d_block(hip._h, shape._h, C.byref(cfg), ptr, dev, int(block[0]), _p(split))
        return lib().fhip_render3d_shard(hip._h, shape._h, C.byref(cfg), ptr, dev, shard, n_shards)
    if out is not None:
        st = call(_dev_ptr(out), 1)
        if st == 4:
            raise ValueError("MissingVar")
        hip.check(st)
        return out, None, None
    # (host_out: a caller's own [height, width] GEOMETRY_PIXEL array to land in - pinned memory, say)
    img = np.zeros((height, width), dtype=GEOMETRY_PIXEL) if host_out is None else host_out
    assert img.dtype == GEOMETRY_PIXEL and img.shape == (height, width) and img.flags.c_contiguous
    import time
    t0 = time.perf_counter()
    st = call(_p(img), 0)
    dt = time.perf_counter() - t0
    if st == 4:
        raise ValueError("MissingVar")
    hip.check(st)
    return img, {}, dt


def merge_depth(front, back, image_depth, hip=None):
    """fhip_merge_depth on torch CUDA tensors ([h, w, 4] int32 GeometryPixel words), in place on `front`."""
    hip = hip or default_context()
    hip.check(lib().fhip_merge_depth(hip._h, _dev_ptr(front), _dev_ptr(back), front.numel() // 4, int(image_depth)))
    return front


def pixel_inside(img):
    """RawDistancePixel::inside (fidget-raster/src/pixel.rs:187-193)."""
    img = np.asarray(img, np.float32)
    bits = img.view(np.uint32)
    is_fill = np.isnan(img) & ((bits & (0xFF << 9)) == (0xF6 << 9))
    return np.where(is_fill, (bits & 1) == 1, img < 0.0)


def pixel_fill_depth(img):
    img = np.asarray(img, np.float32)
    bits = img.view(np.uint32)
    is_fill = np.isnan(img) & ((bits & (0xFF << 9)) == (0xF6 << 9))
    return np.where(is_fill, ((bits >> 1) & 0xFF).astype(np.int32), -1)


# ---- fidget_raster::effects (fidget-raster/src/effects.rs), host arrays in / out -----------------------
def denoise_normals(image, hip=None):
    hip = hip or default_context()
    image = np.ascontiguousarray(image, GEOMETRY_PIXEL)
    out = np.zeros_like(image)
    hip.check(lib().fhip_denoise_normals(hip._h, _p(image), image.shape[1], image.shape[0], _p(out), 0))
    return out


def compute_ssao(image, depth, kernel, noise, hip=None):
    """kernel: 3 x n, noise: 2 x m (the matrices effects::ssao_kernel / ssao_noise return)"""
    hip = hip or default_context()
    image = np.ascontiguousarray(image, GEOMETRY_PIXEL)
    k = np.ascontiguousarray(np.asarray(kernel, np.float32).T)
    nz = np.ascontiguousarray(np.asarray(noise, np.float32).T)
    out = np.zeros(image.shape, np.float32)
    hip.check(lib().fhip_compute_ssao(hip._h, _p(image), image.shape[1], image.shape[0], depth, _p(k), len(k), _p(nz), len(nz), _p(out), 0))
    return out


def blur_ssao(ssao, hip=None):
    hip = hip or default_context()
    ssao = np.ascontiguousarray(ssao, np.float32)
    out = np.zeros_like(ssao)
    hip.check(lib().fhip_blur_ssao(hip._h, _p(ssao), ssao.shape[1], ssao.shape[0], _p(out), 0))
    return out


def apply_shading(image, depth, ssao=None, hip=None):
    hip = hip or default_context()
    image = np.ascontiguousarray(image, GEOMETRY_PIXEL)
    s = None if ssao is None else np.ascontiguousarray(ssao, np.float32)
    out = np.zeros(image.shape + (3,), np.uint8)
    hip.check(lib().fhip_apply_shading(hip._h, _p(image), image.shape[1], image.shape[0], depth, _p(s), _p(out), 0))
    return out


def _to_rgba(image, mode, hip=None):
    hip = hip or default_context()
    image = np.ascontiguousarray(image, np.float32)
    out = np.zeros(image.shape + (4,), np.uint8)
    hip.check(lib().fhip_to_rgba(hip._h, _p(image), image.shape[1], image.shape[0], mode, _p(out), 0))
    return out


def to_rgba_bitmap(image, transparent=False, hip=None):
    return _to_rgba(image, 1 if transparent else 0, hip)


def to_debug_bitmap(image, hip=None):
    return _to_rgba(image, 2, hip)


def to_rgba_distance(image, hip=None):
    return _to_rgba(image, 3, hip)
