"""Contours of a shape's 2D slice: `contour` and its `Contours`, `contour_loops`, `slice_stack`."""
import ctypes as C

import numpy as np

from ._abi import FidgetHipError, _Cfg2D, _DeviceArray, _Handle, _p, lib
from .render import _var_arrays
from .shape import screen_to_world


# ---- contours of a 2D slice: vertices on the crossing lattice edges, directed segments, loops, SVG (fhip_contour2d) -----------
def contour_loops(next):
    """fhip_contour_loops (host only): the chains of a link array as [(ids uint32 array, closed bool)] - open chains first, from the
    vertices no segment arrives at in ascending order, then the closed loops, each from its smallest id, in ascending order of that"""
    nxt = np.ascontiguousarray(next, np.uint32)
    n = len(nxt)
    order, start, closed, count = np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64), np.zeros(n, np.uint8), C.c_uint64(0)
    st = lib().fhip_contour_loops(_p(nxt), n, _p(order), _p(start), _p(closed), C.byref(count))
    if st:
        raise ValueError("not the link array of a contour")
    return [(order[int(start[k]):int(start[k + 1])].copy(), bool(closed[k])) for k in range(count.value)]


class Contours:
    """The outlines of `contour`: `.vertices` [n, 2] float32 in pixel units (the centre of pixel (i, j) is (i, j)), `.segments` [m, 2]
    uint32 {from, to} with the inside on their left, `.next` [n] uint32 (0xFFFFFFFF: no segment leaves the vertex) - host copies, made
    on first use - `.width`, `.height`, `.z`, `.n_vertices`, `.n_segments`.  The arrays themselves stay in device memory."""

    def __init__(self, owner, width, height, z, n_vertices, n_segments):
        self._owner, self.width, self.height, self.z = owner, int(width), int(height), float(z)
        self.n_vertices, self.n_segments = int(n_vertices), int(n_segments)
        self._host = {}

    def _copy(self, name, shape, dtype):
        if name not in self._host:
            a = np.zeros(shape, dtype)
            if getattr(lib(), "fhip_contours_" + name)(self._owner.h, _p(a)):
                raise FidgetHipError("fhip_contours_" + name)
            self._host[name] = a
        return self._host[name]

    @property
    def vertices(self):
        return self._copy("vertices", (self.n_vertices, 2), np.float32)

    @property
    def segments(self):
        return self._copy("segments", (self.n_segments, 2), np.uint32)

    @property
    def next(self):
        return self._copy("next", (self.n_vertices,), np.uint32)

    def vertices_device(self):
        """The vertices in device memory ([n, 2] float32) as an object carrying `__cuda_array_interface__` that keeps the result alive -
        `torch.as_tensor(obj, device="cuda")` views it; None when there are none."""
        ptr = lib().fhip_contours_vertices_dev(self._owner.h)
        return _DeviceArray(self._owner, ptr, (self.n_vertices, 2), "<f4") if ptr else None

    def segments_device(self):
        """... and the segments ([m, 2] vertex ids; "<i4" - torch has no unsigned 32-bit views before 2.3 and the ids are below 2^31
        for every image that fits device memory twice over)"""
        ptr = lib().fhip_contours_segments_dev(self._owner.h)
        return _DeviceArray(self._owner, ptr, (self.n_segments, 2), "<i4") if ptr else None

    def loops(self):
        """[(ids, closed)]: `contour_loops` of `.next`"""
        return contour_loops(self.next)

    def areas(self):
        """the signed area of every chain of `.loops()` in pixel units (shoelace sum in float64, an open chain closed by its chord):
        positive for an outer boundary, negative for a hole"""
        v = self.vertices.astype(np.float64)
        out = []
        for ids, _ in self.loops():
            x, y = v[ids, 0], v[ids, 1]
            out.append(0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)))
        return out

    def world(self):
        """the vertices through screen_to_world((W, H)) - [n, 2] float32 in the region the image spans ([-1, 1] along its shorter side, y upward: row 0
        has the largest y), before world_to_model - in the driver's f32 operation order: (m00 x + m01 y) + m02"""
        m = screen_to_world((self.width, self.height))
        v = self.vertices
        x, y = v[:, 0], v[:, 1]
        out = np.empty_like(v)
        for r in range(2):
            out[:, r] = (m[r, 0] * x + m[r, 1] * y) + m[r, 2]
        return out

    def svg(self, path=None):
        """One <path fill-rule="evenodd"> of all chains, `M x y L x y ... Z` per closed loop (no Z for an open chain).  Coordinates are
        `.world()`'s with y negated: screen_to_world puts row 0 at the largest y, SVG's y grows downward, so row 0 comes out on top
        and the drawing is the image as displayed (and the model with y up), not its mirror.  The viewBox is the image's pixel lattice
        - the corners (-0.5, -0.5) and (W - 0.5, H - 0.5) through the same transform - whatever W : H is.  Returns the text; written to
        `path` when one is given."""
        w = self.world()
        d = []
        for ids, closed in self.loops():
            pts = " L ".join(f"{float(w[k, 0]):.9g} {-float(w[k, 1]):.9g}" for k in ids)
            d.append("M " + pts + (" Z" if closed else ""))
        m = screen_to_world((self.width, self.height)).astype(np.float64)
        cx = [m[0, 0] * px + m[0, 1] * py + m[0, 2] for px in (-0.5, self.width - 0.5) for py in (-0.5, self.height - 0.5)]
        cy = [-(m[1, 0] * px + m[1, 1] * py + m[1, 2]) for px in (-0.5, self.width - 0.5) for py in (-0.5, self.height - 0.5)]
        box = f"{min(cx):.9g} {min(cy):.9g} {max(cx) - min(cx):.9g} {max(cy) - min(cy):.9g}"
        text = (f'<svg xmlns="http://www.w3.org/2000/svg" viewBox="{box}">\n'
                f'<path fill-rule="evenodd" d="{" ".join(d)}"/>\n</svg>\n')
        if path is not None:
            with open(path, "w") as f:
                f.write(text)
        return text

    def __repr__(self):
        return f"Contours({self.width}x{self.height}, z={self.z}, vertices={self.n_vertices}, segments={self.n_segments})"


def contour(shape, width, height=None, z=0.0, world_to_model=None, vars=None):
    """fhip_contour2d: the outlines of `shape < 0` in the pixel-perfect render2d image of this configuration -> Contours.  One blocking
    call; only the two totals come back from the device before the arrays are asked for."""
    height = width if height is None else height
    hip = shape.hip
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    vk, vv = _var_arrays(shape, vars)
    ax = None
    if shape._vars is not None:
        ax = np.array(shape._vars, dtype=np.int32)
        vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
    cfg = _Cfg2D(width, height, _p(w2m), z, 1, None, 0, _p(vk), _p(vv), len(vk), _p(ax))
    h = C.c_void_p()
    st = lib().fhip_contour2d(hip._h, shape._h, C.byref(cfg), C.byref(h))
    if st == 4:
        raise ValueError("MissingVar")
    hip.check(st)
    counts = np.zeros(4, np.uint64)
    owner = _Handle(h.value, lib().fhip_contours_free)
    lib().fhip_contours_counts(owner.h, _p(counts))
    return Contours(owner, width, height, z, counts[0], counts[1])


def slice_stack(shape, size, zs, world_to_model=None, vars=None):
    """One `contour` per z of `zs` (size: W, or (W, H)) -> [Contours]: what a slicer asks for, layer by layer; a layer waits for its
    two totals and nothing else"""
    w, h = (size, size) if np.isscalar(size) else size
    return [contour(shape, int(w), int(h), float(z), world_to_model, vars) for z in zs]
