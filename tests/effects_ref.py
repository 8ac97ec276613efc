"""fidget_raster::effects (fidget-raster/src/effects.rs), RawDistancePixel (pixel.rs:179-217), fidget_core::rng::hash / mix and the
stitch rule of fhip_merge_depth (voxel.rs:527-550 across z ranges, include/fidget_hip.h), restated in numpy from the Rust text - not
from effects.hip and not from oracle/src/effects.hpp, which are one text twice - so that a shared misreading shows.

The structure differs from the kernels on purpose: every function works on the whole image at once; a neighbour is a shifted view of a
padded copy, an SSAO sample a clipped gather; there is no per-pixel loop except in to_rgba_distance, which calls the host's expf and cosf
through ctypes.  The per-pixel f32 operation ORDER is the reference's.  Every value is np.float32: _f() asserts it where a silent upcast
could creep in.

Semantics followed (each named again at the line that relies on it):
  nalgebra Vector3 dot      (a0*b0 + a1*b1) + a2*b2
  norm                      sqrt(0 + dot(v, v))
  normalize                 each component / norm
  Matrix3 * v               by columns: col0*v0, then col_j*v_j + acc
  cross                     (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx)
  OrderedFloat              NaN above everything and equal to itself
  max_by_key / min_by_key   the LAST of equal maxima / the FIRST of equal minima
  f32::max                  ignores a NaN operand
  f32::clamp                keeps NaN
  `as u8`                   saturates, NaN -> 0, truncates toward zero
  powi(2)                   x*x

Every function takes mutant=NAME: exactly one rule switched to a plausible wrong one (MUTANTS lists them).  tests/test_effects_ref.py shows
that each mutant changes 3 pixels or more of some input below - the condition under which a device test that compares with this reference
on those inputs can claim to notice that fault.  Two rules have no mutant, because the inputs cannot tell the variants apart:
  - the `dz < 2 RADIUS` falloff arm of compute_pixel_ssao is unreachable: dz = sample_pos.z - actual_z >= RADIUS > 0 means
    sample_pos.z > actual_z (a NaN dz fails both tests), and the arm asks for sample_pos.z <= actual_z.  It is restated all the same;
  - `px > 0.0` against `px >= 0.0`: they part only for a sample at px = 0.0 exactly, that is offset + p rounding to -1.0 exactly, where
    p is at least 1 / W inside; a seeded kernel does not put a sample there, and one tuned to would pin a rounding accident, not a rule."""
import ctypes
import ctypes.util
import functools

import numpy as np

F32 = np.float32
GEOMETRY_PIXEL = np.dtype([("normal", np.float32, 3), ("depth", np.uint32)])     # voxel.rs:122-134

MUTANTS = {
    # tie_first: max_by_key keeps the first of equal maxima; nan_low: a NaN score ordered below everything; j_outer: the window summed
    # row by row (`for j { for i {`), which rounds the f32 sums differently
    "denoise_normals": ("tie_first", "nan_low", "j_outer"),
    # tie_last: min_by_key keeps the last of equal minima
    "blur_ssao": ("tie_last",),
    # sxsy_swapped: the aspect compensation of x and y exchanged; sz_ignored: none in z; x_by_height: the sample's x scaled to pixels by
    # the height; mix_xy: mix(x, y) for mix(pos.0 = y, pos.1 = x); strict_less: `sample_pos.z < actual_z`
    "compute_ssao": ("sxsy_swapped", "sz_ignored", "x_by_height", "mix_xy", "strict_less"),
    # xy_norm_swapped: x / height and y / width; half_pixel: the (x + 0.5) offset of compute_pixel_ssao, which shade_pixel does not have
    "apply_shading": ("xy_norm_swapped", "half_pixel"),
    # key_bits_10_17: the fill key tested where the struct's comment puts it, not at bits 9..16; depth_wide: see _unpack
    "colour_maps": ("key_bits_10_17", "depth_wide"),
    # tie_back: equal depths take the back pixel; clamp_at_depth: the clamp at depth >= D, not D - 1
    "merge_depth": ("tie_back", "clamp_at_depth"),
}


def _mut(fn, mutant):
    assert mutant is None or mutant in MUTANTS[fn], (fn, mutant)
    return mutant


def _f(a):
    assert np.asarray(a).dtype == np.float32, np.asarray(a).dtype
    return a


def same(a, b):
    """bit-for-bit up to the NaN payload: NaN equals NaN (+0 equals -0 nowhere: the bits are compared)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.names:
        return all(same(a[k], b[k]) for k in a.dtype.names)
    if a.dtype.kind != "f":
        return a.shape == b.shape and bool((a == b).all())
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def differing(a, b, pixel_axes=2):
    """the number of pixels (the first `pixel_axes` axes) at which two results differ, NaN equal to NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.names:
        a, b = a.view(np.uint32).reshape(a.shape + (4,)), b.view(np.uint32).reshape(b.shape + (4,))
        a = np.where(np.isnan(a.view(np.float32)) & (np.arange(4) < 3), np.uint32(0x7FC00000), a)
        b = np.where(np.isnan(b.view(np.float32)) & (np.arange(4) < 3), np.uint32(0x7FC00000), b)
    with np.errstate(invalid="ignore"):
        ne = ~((a == b) | (np.isnan(a) & np.isnan(b))) if a.dtype.kind == "f" else a != b
    return int(ne.reshape(ne.shape[:pixel_axes] + (-1,)).any(axis=-1).sum())


# ---- fidget_core::rng (rng/mod.rs) ----------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def rng_hash(v):
    """rng::hash (the PCG hash of Jarzynski & Olano): u32 wrapping arithmetic, done in u64 and masked"""
    v = np.asarray(v).astype(np.uint64) & _M32
    state = (v * np.uint64(747796405) + np.uint64(2891336453)) & _M32
    word = (((state >> ((state >> np.uint64(28)) + np.uint64(4))) ^ state) * np.uint64(277803737)) & _M32
    return ((word >> np.uint64(22)) ^ word).astype(np.uint32)


def rng_mix(a, b):
    """rng::mix(a, b) = hash(a + hash(b)), the sum wrapping"""
    return rng_hash((np.asarray(a).astype(np.uint64) + rng_hash(b).astype(np.uint64)) & _M32)


# ---- small-vector code of nalgebra, on [..., 3] arrays held as three planes -----------------------------------------------------
def _dot(a, b):
    return _f((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])             # dot: (a0*b0 + a1*b1) + a2*b2


def _normalize(a):
    norm = np.sqrt(F32(0.0) + _dot(a, a))                            # norm: sqrt(0 + dot)
    return [_f(a[0] / norm), _f(a[1] / norm), _f(a[2] / norm)]       # normalize: componentwise division


def _planes(img):
    n = np.ascontiguousarray(img["normal"], np.float32)
    return [n[..., 0], n[..., 1], n[..., 2]]


def _shifted(a, dy, dx, r=2):
    """b[y, x] = a[y + dy, x + dx], zero where that is outside the image (|dy|, |dx| <= r)"""
    h, w = a.shape
    return np.pad(a, r)[r + dy:r + dy + h, r + dx:r + dx + w]


def _of_ge(a, b):
    """OrderedFloat: a >= b with NaN above everything and equal to itself"""
    return np.isnan(a) | (~np.isnan(b) & (a >= b))


def _of_lt(a, b):
    return ~_of_ge(a, b)


def _as_u8(v):
    """`as u8`: NaN -> 0, saturating, toward zero"""
    v = _f(np.asarray(v))
    return np.where(np.isnan(v), F32(0.0), np.clip(v, F32(0.0), F32(255.0))).astype(np.uint8)


_WINDOWS = ((0, 0), (-2, 0), (0, -2), (-2, -2))          # (xmin, ymin) of effects.rs:260-265 and 326-331, radius 2


def _window_cells(order):
    """(i, j) in the order of the reference's loops: `for i { for j {` - i moves x, j moves y"""
    if order == "j_outer":
        return [(i, j) for j in range(3) for i in range(3)]
    return [(i, j) for i in range(3) for j in range(3)]


# ---- denoise_normals (effects.rs:17-36) + denoise_pixel (247-315) ------------------------------------------------------------
def denoise_normals(image, mutant=None):
    m = _mut("denoise_normals", mutant)
    image = np.ascontiguousarray(image, GEOMETRY_PIXEL)
    depth = image["depth"]
    n = _planes(image)
    filled = depth != 0
    front = filled & (n[2] > F32(0.0))                   # `depth != 0 && normal[2] > 0.0`: contributes to a window's mean
    best = [c.copy() for c in n]                        # unwrap_or((0.0, n)): no window with a front-facing pixel keeps n
    best_score = np.zeros(depth.shape, np.float32)
    have = np.zeros(depth.shape, bool)
    with np.errstate(all="ignore"):
        for xmin, ymin in _WINDOWS:
            total = [np.zeros(depth.shape, np.float32) for _ in range(3)]
            count = np.zeros(depth.shape, np.int32)
            for i, j in _window_cells(m):
                use = _shifted(front, ymin + j, xmin + i)            # False outside the image
                for c in range(3):
                    total[c] = np.where(use, total[c] + _shifted(n[c], ymin + j, xmin + i), total[c])     # sum += n
                count += use
            mean = [_f(t / count.astype(np.float32)) for t in total]             # sum / count as f32
            score = np.zeros(depth.shape, np.float32)
            for i, j in _window_cells(m):
                use = _shifted(filled, ymin + j, xmin + i)           # `depth != 0`, back-facing pixels included
                q = [_shifted(n[c], ymin + j, xmin + i) for c in range(3)]
                score = np.where(use, score + _dot(q, mean), score)              # score += n.dot(&mean)
            if m == "tie_first":
                better = score > best_score
                better |= np.isnan(score) & ~np.isnan(best_score)
            elif m == "nan_low":
                better = np.isnan(best_score) | (~np.isnan(score) & (score >= best_score))
            else:
                better = _of_ge(score, best_score)                               # max_by_key: the last maximum wins
            take = (count > 0) & (~have | better)                                # count == 0: the window yields None
            for c in range(3):
                best[c] = np.where(take, mean[c], best[c])
            best_score = np.where(take, score, best_score)
            have |= count > 0
    out = np.zeros(image.shape, GEOMETRY_PIXEL)
    out["depth"] = depth
    keep = n[2] > F32(0.0)                                                       # `if n[2] > 0.0 { return n; }`
    for c in range(3):
        out["normal"][..., c] = np.where(filled, np.where(keep, n[c], best[c]), F32(0.0))      # depth 0 -> [0.0; 3]
    return out


# ---- compute_ssao (effects.rs:73-95) + compute_pixel_ssao (157-245) ----------------------------------------------------------
def compute_ssao(image, depth, kernel, noise, mutant=None):
    """kernel: 3 x n, noise: 2 x m (the matrices ssao_kernel / ssao_noise return; the reference draws them from rand::rng())"""
    m = _mut("compute_ssao", mutant)
    image = np.ascontiguousarray(image, GEOMETRY_PIXEL)
    kernel, noise = np.asarray(kernel, np.float32), np.asarray(noise, np.float32)
    H, W = image.shape
    D = int(depth)
    d = image["depth"]
    fW, fH, fD = F32(W), F32(H), F32(D)
    scale_min = F32(min(W, H, D))
    sx, sy, sz = scale_min / fW, scale_min / fH, scale_min / fD
    if m == "sxsy_swapped":
        sx, sy = sy, sx
    if m == "sz_ignored":
        sz = F32(1.0)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    RADIUS = F32(0.1)
    with np.errstate(all="ignore"):
        p = [_f((((xs.astype(np.float32) + F32(0.5)) / fW) - F32(0.5)) * F32(2.0)),
             _f((((ys.astype(np.float32) + F32(0.5)) / fH) - F32(0.5)) * F32(2.0)),
             _f(((d.astype(np.float32) / fD) - F32(0.5)) * F32(2.0))]
        n = _normalize(_planes(image))
        # pos = (y, x); mix(pos.0, pos.1)
        ri = (rng_mix(xs, ys) if m == "mix_xy" else rng_mix(ys, xs)).astype(np.int64) % noise.shape[1]
        rvec = [noise[0][ri], noise[1][ri], np.zeros((H, W), np.float32)]
        rn = _dot(rvec, n)
        tangent = _normalize([_f(rvec[c] - n[c] * rn) for c in range(3)])        # (rvec - n * rvec.dot(&n)).normalize()
        bitangent = [_f(n[1] * tangent[2] - n[2] * tangent[1]),                 # n.cross(&tangent)
                     _f(n[2] * tangent[0] - n[0] * tangent[2]),
                     _f(n[0] * tangent[1] - n[1] * tangent[0])]
        occlusion = np.zeros((H, W), np.float32)
        for i in range(kernel.shape[1]):
            k = kernel[:, i]
            off = [tangent[c] * k[0] for c in range(3)]                          # tbn * k by columns: tangent, bitangent, n
            off = [bitangent[c] * k[1] + off[c] for c in range(3)]
            off = [n[c] * k[2] + off[c] for c in range(3)]
            off = [_f(o * RADIUS) for o in off]
            off = [off[0] * sx, off[1] * sy, off[2] * sz]
            sp = [_f(off[c] + p[c]) for c in range(3)]                           # offset + p
            px = _f(((sp[0] / F32(2.0)) + F32(0.5)) * (fH if m == "x_by_height" else fW))
            py = _f(((sp[1] / F32(2.0)) + F32(0.5)) * fH)
            inside = (px < fW) & (py < fH) & (px > F32(0.0)) & (py > F32(0.0))
            gx = np.clip(np.where(inside, px, F32(0.0)), 0, W - 1).astype(np.int64)       # `px as usize`: toward zero
            gy = np.clip(np.where(inside, py, F32(0.0)), 0, H - 1).astype(np.int64)
            actual_h = np.where(inside, d[gy, gx], np.uint32(0))
            actual_z = _f(((actual_h.astype(np.float32) / fD) - F32(0.5)) * F32(2.0))
            dz = _f(sp[2] - actual_z)
            below = (sp[2] < actual_z) if m == "strict_less" else (sp[2] <= actual_z)
            near = dz < RADIUS
            occlusion = np.where(near, occlusion + below.astype(np.float32), occlusion)
            fall = ~near & (dz < RADIUS * F32(2.0)) & below                      # (unreachable: see the module text)
            t = _f((RADIUS - (dz - RADIUS)) / RADIUS)
            occlusion = _f(np.where(fall, occlusion + t * t, occlusion))         # powi(2)
        res = _f(F32(1.0) - (occlusion / F32(kernel.shape[1])))
    return np.where(d != 0, res, F32(np.nan)).astype(np.float32)


# ---- blur_ssao (effects.rs:98-115) + compute_pixel_blur (318-379) ------------------------------------------------------------
def blur_ssao(ssao, mutant=None):
    m = _mut("blur_ssao", mutant)
    s0 = np.ascontiguousarray(ssao, np.float32)
    valid = ~np.isnan(s0)
    sz = np.where(valid, s0, F32(0.0))                   # a NaN is skipped; the zero is never added
    best = s0.copy()                                     # unwrap_or_else(|| (0.0, ssao[(y, x)]))
    best_dev = np.zeros(s0.shape, np.float32)
    have = np.zeros(s0.shape, bool)
    with np.errstate(all="ignore"):
        for xmin, ymin in _WINDOWS:
            total = np.zeros(s0.shape, np.float32)
            count = np.zeros(s0.shape, np.int32)
            for i, j in _window_cells(None):
                use = _shifted(valid, ymin + j, xmin + i)
                total = np.where(use, total + _shifted(sz, ymin + j, xmin + i), total)
                count += use
            mean = _f(total / count.astype(np.float32))
            stdev = np.zeros(s0.shape, np.float32)
            for i, j in _window_cells(None):
                use = _shifted(valid, ymin + j, xmin + i)
                e = _f(mean - _shifted(sz, ymin + j, xmin + i))
                stdev = np.where(use, stdev + e * e, stdev)                      # (mean - s).powi(2)
            dev = _f(stdev / count.astype(np.float32))
            if m == "tie_last":
                better = ~_of_lt(best_dev, dev)
            else:
                better = _of_lt(dev, best_dev)                                   # min_by_key: the first minimum stays
            take = (count > 0) & (~have | better)
            best = np.where(take, mean, best)
            best_dev = np.where(take, dev, best_dev)
            have |= count > 0
    return np.where(valid, best, F32(np.nan)).astype(np.float32)             # `if ssao[(y, x)].is_nan() { f32::NAN }`


# ---- apply_shading (effects.rs:42-67) + shade_pixel (118-152) ------------------------------------------------------------------
_LIGHTS = ((5.0, -5.0, 10.0, 0.5), (-5.0, 0.0, 10.0, 0.15), (0.0, -5.0, 10.0, 0.15))


def apply_shading(image, depth, ssao=None, mutant=None):
    """ssao = the blurred occlusion map or None; returns uint8 [h, w, 3]"""
    m = _mut("apply_shading", mutant)
    image = np.ascontiguousarray(image, GEOMETRY_PIXEL)
    H, W = image.shape
    d = image["depth"]
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    fW, fH, fD = F32(W), F32(H), F32(int(depth))
    if m == "half_pixel":
        xs, ys = xs + F32(0.5), ys + F32(0.5)
    if m == "xy_norm_swapped":
        fW, fH = fH, fW
    with np.errstate(all="ignore"):
        n = _normalize(_planes(image))
        p = [_f(F32(2.0) * (xs / fW - F32(0.5))), _f(F32(2.0) * (ys / fH - F32(0.5))), _f(F32(2.0) * (d.astype(np.float32) / fD - F32(0.5)))]
        accum = np.full((H, W), F32(0.2), np.float32)                            # ambient
        for lx, ly, lz, lw in _LIGHTS:
            ldir = _normalize([_f(F32(lx) - p[0]), _f(F32(ly) - p[1]), _f(F32(lz) - p[2])])
            accum = _f(accum + np.fmax(_dot(ldir, n), F32(0.0)) * F32(lw))       # f32::max ignores NaN: fmax
        if ssao is not None:
            accum = _f(accum * (np.ascontiguousarray(ssao, np.float32) * F32(0.6) + F32(0.4)))
        accum = np.where(accum < F32(0.0), F32(0.0), np.where(accum > F32(1.0), F32(1.0), accum))      # clamp keeps NaN
        c = _as_u8(_f(accum * F32(255.0)))
    c = np.where(d > 0, c, np.uint8(0))
    return np.repeat(c[..., None], 3, axis=-1).astype(np.uint8)


# ---- RawDistancePixel (pixel.rs:179-217) and its colour maps (effects.rs:443-547) -------------------------------------------
_KEY, _KEY_MASK = 0b1111_0110 << 9, 0b1111_1111 << 9


def _unpack(image, m):
    """-> (f, is_distance, fill inside, fill depth)"""
    f = np.ascontiguousarray(image, np.float32)
    bits = f.view(np.uint32)
    mask, key = _KEY_MASK, _KEY
    if m == "key_bits_10_17":                            # the struct's comment says "bits 10-17"; the constants sit at 9..16
        mask = 0xFF << 10
        key = _KEY & mask
    is_distance = ~np.isnan(f) | ((bits & np.uint32(mask)) != np.uint32(key))
    inside = (bits & np.uint32(1)) == 1
    depth = (bits >> np.uint32(1)).astype(np.uint8).astype(np.uint32)            # `(bits >> 1) as u8`
    if m == "depth_wide":
        # the truncation forgotten: bit 9 and the key above it stay in the depth.  (Keeping bit 9 alone - "bits 1-9" in the struct's
        # comment - changes nothing on any input, since a fill pixel's bit 9 is the key's lowest bit, 0; so the mutant is this one.)
        depth = bits >> np.uint32(1)
    return f, is_distance, inside, depth


def _rgba(shape):
    out = np.zeros(shape + (4,), np.uint8)
    out[..., 3] = 255
    return out


def to_rgba_bitmap(image, transparent=False, mutant=None):
    f, is_distance, fill_inside, _ = _unpack(image, _mut("colour_maps", mutant))
    with np.errstate(invalid="ignore"):
        inside = np.where(is_distance, f < F32(0.0), fill_inside)                # RawDistancePixel::inside
    out = _rgba(f.shape)
    out[inside] = 255
    if transparent:
        out[~inside] = 0
    return out


def to_debug_bitmap(image, mutant=None):
    f, is_distance, inside, depth = _unpack(image, _mut("colour_maps", mutant))
    out = _rgba(f.shape)
    with np.errstate(invalid="ignore"):
        out[is_distance & (f < F32(0.0)), :3] = 255
    level = np.where(inside, 255, 50).astype(np.uint8)
    fill = ~is_distance
    for channel, which in ((0, depth == 0), (1, depth == 1), (2, depth == 2)):
        out[..., channel] = np.where(fill & which, level, out[..., channel])
    rest = fill & (depth > 2)
    out[..., 0] = np.where(rest, level, out[..., 0])
    out[..., 1] = np.where(rest, level, out[..., 1])
    return out


@functools.lru_cache(None)
def _libm():
    lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for name in ("expf", "cosf"):
        getattr(lib, name).restype = ctypes.c_float
        getattr(lib, name).argtypes = [ctypes.c_float]
    return lib


def _distance_colour(f):
    """one DistancePixel::Value that is no NaN -> [r, g, b] (effects.rs:512-534), in np.float32 scalars"""
    libm = _libm()
    one, zero = F32(1.0), F32(0.0)
    af = _f(np.abs(f))
    dim = _f(one - F32(libm.expf(float(_f(F32(-4.0) * af)))))                    # dimming near 0
    bands = _f(F32(0.8) + F32(0.2) * F32(libm.cosf(float(_f(F32(140.0) * f)))))  # banding

    def clamp01(v):
        return zero if v < zero else (one if v > one else v)                     # keeps NaN

    def smoothstep(edge0, edge1, x):
        t = clamp01(_f((x - edge0) / (edge1 - edge0)))
        return _f(t * t * (F32(3.0) - F32(2.0) * t))

    def mix(x, y, a):
        return _f(x * (one - a) + y * a)

    rgb = []
    for base in (0.1, 0.4, 0.7):
        v = _f(_f(one - np.copysign(F32(base), f)) * dim * bands)
        v = mix(v, one, one - smoothstep(zero, F32(0.015), af))
        v = mix(v, one, one - smoothstep(zero, F32(0.005), af))
        rgb.append(int(_as_u8(_f(clamp01(v) * F32(255.0)))))
    return rgb


def to_rgba_distance(image, mutant=None):
    f, is_distance, inside, _ = _unpack(image, _mut("colour_maps", mutant))
    out = _rgba(f.shape)
    flat, o = f.reshape(-1), out.reshape(-1, 4)
    with np.errstate(all="ignore"):
        for i in range(flat.size):
            if not is_distance.reshape(-1)[i]:
                o[i, :3] = (184, 235, 255) if inside.reshape(-1)[i] else (217, 144, 72)
            elif np.isnan(flat[i]):
                o[i, :3] = (255, 0, 0)
            else:
                o[i, :3] = _distance_colour(flat[i])
    return out


# ---- fhip_merge_depth: the stitch rule of voxel.rs:527-550 across two z ranges ------------------------------------------------
def merge_depth(front, back, image_depth, mutant=None):
    """front, back: GEOMETRY_PIXEL arrays of the same pixels, `front` from the range nearer the camera.  The larger depth wins, a tie
    keeps `front` (a hit there carries the normal); then depth >= image_depth - 1 becomes (image_depth, [0, 0, 1]) as the reference
    clamps (`d = depth - 1; if out.depth >= d { depth: d + 1, normal: [0, 0, 1] }`); image_depth 0 means no clamp.  Returns the merged
    array."""
    m = _mut("merge_depth", mutant)
    front, back = np.ascontiguousarray(front, GEOMETRY_PIXEL), np.ascontiguousarray(back, GEOMETRY_PIXEL)
    take = (back["depth"] >= front["depth"]) if m == "tie_back" else (back["depth"] > front["depth"])
    out = np.where(take, back, front)
    D = int(image_depth)
    if D:
        sat = out["depth"].astype(np.int64) >= (D if m == "clamp_at_depth" else D - 1)
        out["depth"][sat] = D
        out["normal"][sat] = (0.0, 0.0, 1.0)
    return out


# ---- inputs: small, seeded, adversarial ------------------------------------------------------------------------------------------
GEOMETRY_SIZES = ((19, 37, 50), (37, 19, 11), (33, 17, 17), (2, 40, 300), (1, 1, 1))       # (H, W, D)
SMOOTH_SIZES = ((19, 37, 50), (37, 19, 11))


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def ssao_matrices(nk=24, nn=16, seed=11):
    """a hemisphere kernel (3 x nk) and unit rotation noise (2 x nn) in the manner of ssao_kernel / ssao_noise, seeded"""
    rng = np.random.default_rng(seed)
    k = rng.uniform(-1, 1, (3, nk)).astype(np.float32)
    k[2] = np.abs(k[2])
    k = (k / np.sqrt((k * k).sum(axis=0)) * rng.uniform(0.1, 1.0, nk)).astype(np.float32)
    nz = rng.uniform(-1, 1, (2, nn)).astype(np.float32)
    nz = (nz / np.sqrt((nz * nz).sum(axis=0))).astype(np.float32)
    return _frozen(k), _frozen(nz)


@functools.lru_cache(None)
def geometry_image(h, w, d, seed=5):
    """about a quarter empty; of the filled about a tenth with a zero normal, about 40 % with small integer normals (window scores tie),
    most of the rest back-facing; NaN and infinite components in the corners and in the interior"""
    rng = np.random.default_rng(seed + 1000 * h + w)
    img = np.zeros((h, w), GEOMETRY_PIXEL)
    img["depth"] = rng.integers(1, d + 1, (h, w))
    n = rng.normal(size=(h, w, 3)).astype(np.float32)
    n[..., 2] = np.where(rng.random((h, w)) < 0.65, -np.abs(n[..., 2]), np.abs(n[..., 2]))
    u = rng.random((h, w))
    whole = rng.integers(-1, 2, (h, w, 3)).astype(np.float32)
    n = np.where((u < 0.5)[..., None], whole, n)
    n = np.where((u < 0.1)[..., None], np.float32(0.0), n)
    img["normal"] = n
    img["depth"][rng.random((h, w)) < 0.25] = 0
    odd = ((0, 0, (np.nan, 0.5, 1.0)), (h - 1, w - 1, (np.inf, 0.0, -1.0)), (0, w - 1, (0.25, -np.inf, 0.5)), (h - 1, 0, (1.0, 2.0, np.nan)),
           (h // 2, w // 2, (0.5, np.nan, -1.0)), (h // 3, (2 * w) // 3, (-np.inf, 1.0, 2.0)), ((2 * h) // 3, w // 3, (0.0, 0.0, np.inf)))
    if h * w > 1:
        for y, x, v in odd:
            img["normal"][y, x] = v
            img["depth"][y, x] = max(1, d // 2)
    else:
        img["depth"], img["normal"] = 1, (0.5, -0.25, -1.0)
    return _frozen(img)


@functools.lru_cache(None)
def smooth_image(h, w, d):
    """a sinusoidal height field, every pixel filled and front-facing: SSAO samples land on neighbours of nearby depth"""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    z = 0.5 + 0.3 * np.sin(x * 0.45) * np.cos(y * 0.35)
    img = np.zeros((h, w), GEOMETRY_PIXEL)
    img["depth"] = np.clip(np.rint(z * d), 1, d - 1).astype(np.uint32)
    gx, gy = 0.3 * 0.45 * np.cos(x * 0.45) * np.cos(y * 0.35), -0.3 * 0.35 * np.sin(x * 0.45) * np.sin(y * 0.35)
    img["normal"] = np.stack([-gx * 4, -gy * 4, np.ones((h, w))], axis=-1).astype(np.float32)
    return _frozen(img)


@functools.lru_cache(None)
def plane_case(h=21, w=34, d=40):
    """a flat plane facing the camera and a kernel with columns of z exactly 0: there sample_pos.z == actual_z, which `<=` counts
    and `<` does not.  -> (image, depth, kernel, noise)"""
    img = np.zeros((h, w), GEOMETRY_PIXEL)
    img["depth"] = d // 2
    img["normal"] = (0.0, 0.0, 1.0)
    k, nz = ssao_matrices()
    k = k.copy()
    k[2, ::2] = 0.0
    return _frozen(img), d, _frozen(k), nz


@functools.lru_cache(None)
def ssao_map(h, w, seed=3):
    """values on the grid k / 4 (window deviations tie), a constant plateau, 15 % NaN, one +inf"""
    rng = np.random.default_rng(seed + 1000 * h + w)
    s = (rng.integers(0, 5, (h, w)) / 4).astype(np.float32)
    s[h // 4:h // 4 + 7, w // 4:w // 4 + 7] = 0.75
    s[rng.random((h, w)) < 0.15] = np.nan
    if h * w > 1:
        s[h // 2, w // 3] = np.inf
    return _frozen(s)


def fill_pixel(depth, inside, sign=0):
    """RawDistancePixel::from(DistancePixel::Fill) (pixel.rs:224-229), the sign bit as asked"""
    return 0x7FC00000 | (depth << 1) | int(inside) | _KEY | (sign << 31)


@functools.lru_cache(None)
def distance_image(seed=9, width=24):
    rng = np.random.default_rng(seed)
    f = np.float32
    edges = []
    for e in (f(0.005), f(0.015)):
        edges += [np.nextafter(e, f(0)), e, np.nextafter(e, f(1))]
    special = [0.0, -0.0, np.inf, -np.inf, 1e-30, -1e-30, 3e38, -3e38] + edges + [-e for e in edges]
    vals = np.concatenate([(rng.normal(size=300) * 0.3).astype(np.float32), (rng.normal(size=300) * 0.01).astype(np.float32),
                           np.array(special, np.float32)]).view(np.uint32).tolist()
    vals += [0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF]                     # plain NaNs
    fills = [fill_pixel(dp, ins, sg) for dp in (0, 1, 2, 3, 255) for ins in (0, 1) for sg in (0, 1)]
    vals += fills
    for b in range(9, 18):                                                       # the key field, and bit 17 above it, one bit off
        vals += [v ^ (1 << b) for v in fills[::3]]
    vals += (rng.normal(size=(-len(vals)) % width) * 0.05).astype(np.float32).view(np.uint32).tolist()
    img = np.array(vals, np.uint32)[rng.permutation(len(vals))].view(np.float32).reshape(-1, width)
    return _frozen(img)


@functools.lru_cache(None)
def merge_case(n, image_depth=64, seed=13):
    """-> (front, back): back deeper, front deeper, equal depths with different normals, either side at D - 1 and at D, both empty, in turn"""
    rng = np.random.default_rng(seed + n)
    D = image_depth
    rows = [(10, 30), (40, 5), (22, 22), (D - 1, 7), (7, D - 1), (D, 3), (3, D), (0, 0), (D - 2, D - 2), (D - 1, D - 1), (0, 9), (9, 0)]
    pick = rng.permutation(np.arange(n) + 2) % len(rows)
    front, back = np.zeros(n, GEOMETRY_PIXEL), np.zeros(n, GEOMETRY_PIXEL)
    front["depth"], back["depth"] = np.array(rows, np.uint32)[pick].T
    front["normal"], back["normal"] = rng.normal(size=(2, n, 3)).astype(np.float32)
    front["normal"][front["depth"] == 0] = 0
    back["normal"][back["depth"] == 0] = 0
    return _frozen(front), _frozen(back)


@functools.lru_cache(None)
def geometry_cases():
    """[(name, image, depth, kernel, noise)]: the adversarial images, the smooth height fields and the engineered equality case"""
    k, nz = ssao_matrices()
    out = [("geom%dx%dx%d" % s, geometry_image(*s), s[2], k, nz) for s in GEOMETRY_SIZES]
    out += [("smooth%dx%dx%d" % s, smooth_image(*s), s[2], k, nz) for s in SMOOTH_SIZES]
    out.append(("plane",) + plane_case())
    return tuple(out)


@functools.lru_cache(None)
def ssao_maps():
    return tuple(("map%dx%d" % s[:2], ssao_map(*s[:2])) for s in GEOMETRY_SIZES)


@functools.lru_cache(None)
def chain(name):
    """denoise -> ssao -> blur -> shade of one geometry case by the reference, computed once: (denoised, ssao, blurred, rgb, rgb without ssao)"""
    _, img, d, k, nz = next(c for c in geometry_cases() if c[0] == name)
    dn = denoise_normals(img)
    s = compute_ssao(dn, d, k, nz)
    b = blur_ssao(s)
    return tuple(_frozen(a) for a in (dn, s, b, apply_shading(dn, d, b), apply_shading(dn, d)))
