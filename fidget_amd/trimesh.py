"""The triangle-mesh family - a mesh given as triangles back into the library: `read_stl`, `voxelize_mesh`, `mesh_topology` and its
`Topology`, `mesh_slices` and its `MeshSlices`, whose `nesting()` gives a `SliceNesting`."""
import ctypes as C
import os

import numpy as np

from ._abi import _DeviceArray, _Handle, _p, lib
from .context import default_context
from .mesher import Mesh
from .render import _dev_ptr
from .voxels import _bitmap_of, _bitmap_out


# ---- a triangle mesh back into the library: binary STL in, voxel bitmap out (fhip_triangles_voxels, fhip_mesh_voxels) ------------
def read_stl(path_or_bytes):
    """A binary STL file -> its triangles, float32 [T, 3, 3] (triangle, corner, xyz), read on the host; the file's normals and
    attribute words are ignored.  `path_or_bytes`: a path, or the file's bytes (bytes, bytearray, memoryview, a numpy uint8 array such
    as `Mesh.stl()` returns).  ASCII STL is refused with a ValueError."""
    if isinstance(path_or_bytes, (str, os.PathLike)):
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    elif isinstance(path_or_bytes, np.ndarray):
        data = np.ascontiguousarray(path_or_bytes).view(np.uint8).tobytes()
    else:
        data = bytes(path_or_bytes)
    n = int.from_bytes(data[80:84], "little") if len(data) >= 84 else -1
    if n < 0 or len(data) != 84 + 50 * n:
        if data.lstrip()[:5].lower() == b"solid":
            raise ValueError("read_stl: this is an ASCII STL file; only binary STL is read")
        raise ValueError(f"read_stl: not a binary STL file: {len(data)} bytes, but its header counts {n} triangles" if n >= 0 else "read_stl: not a binary STL file: shorter than its header")
    rec = np.frombuffer(data, np.uint8, 50 * n, 84).reshape(n, 50)
    return np.ascontiguousarray(rec[:, 12:48]).view("<f4").astype(np.float32).reshape(n, 3, 3)


MESH_INFO = ("triangles", "rejected", "flat", "crossings", "clipped", "open_rows", "set_voxels", "W")


def voxelize_mesh(mesh, depth, mesh_to_world=None, out=None, hip=None):
    """fhip_triangles_voxels / fhip_mesh_voxels: the solid a closed triangle mesh encloses, on the grid of 4 << depth voxels per axis
    over [-1, 1]^3, by parity counting along +x (even-odd: nested sheets make cavities) -> Voxels; the definition, exact in integers
    after the vertices are snapped to 1/256 voxel, stands in include/fidget_hip.h.  `mesh`: a `Mesh` (its resident device arrays are
    read where they are); float32 [T, 3, 3] triangles as `read_stl` returns them, a numpy array or a torch CUDA tensor; or a pair
    (vertices [V, 3] float32, triangles [T, 3] indices), both numpy or both torch CUDA (indices int64).  `mesh_to_world`: a 3 x 4
    matrix (or 4 x 4, whose first three rows are used), applied in float64 before the snap.  `out` as for `voxelize`.  `hip`: the context for
    arrays (default: `default_context()`; a `Mesh` brings its own).  A pair may be a tuple or a list of the two arrays.  The result's
    `.cells` are all zeros and `.mesh_info` = {triangles, rejected, flat, crossings, clipped, open_rows, set_voxels, W}: open_rows > 0 shows
    a mesh that is not closed.  ValueError when triangles were rejected: a vertex not finite or outside [-1.5, 1.5], or an index
    beyond the vertices."""
    depth = int(depth)
    m2w = None
    if mesh_to_world is not None:
        m2w = np.ascontiguousarray(np.asarray(mesh_to_world, np.float64).reshape(-1)[:12])
        assert m2w.size == 12, "mesh_to_world: 3 x 4 or 4 x 4"
    keep = None          # what the pointers point into, until the call returns
    if isinstance(mesh, Mesh):
        hip = mesh._hip
    else:
        hip = hip or default_context()
        # a pair is a tuple or a list of two arrays; a nested list of numbers is the [T, 3, 3] form
        pair = isinstance(mesh, (tuple, list)) and len(mesh) == 2 and all(hasattr(a, "shape") for a in mesh)
        if isinstance(mesh, (tuple, list)) and not pair and any(hasattr(a, "shape") for a in mesh):
            raise TypeError("voxelize_mesh: a mesh is a Mesh, [T, 3, 3] triangles, or a pair (vertices [V, 3], triangles [T, 3]) of two arrays")
        verts, tris = mesh if pair else (mesh, None)
        if isinstance(verts, np.ndarray) or not hasattr(verts, "is_cuda"):
            verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
            vp, dev = _p(verts), 0
            if tris is not None:
                tris = np.ascontiguousarray(tris, np.uint64).reshape(-1, 3)
            tp = _p(tris)
        else:
            assert verts.is_cuda and verts.element_size() == 4 and verts.is_floating_point(), "vertices on the device: a float32 CUDA tensor"
            verts = verts.contiguous().reshape(-1, 3)
            vp, dev = _dev_ptr(verts), 1
            if tris is not None:
                assert tris.is_cuda and tris.element_size() == 8 and not tris.is_floating_point(), "triangles on the device: an int64 CUDA tensor"
                tris = tris.contiguous().reshape(-1, 3)
            tp = _dev_ptr(tris)
        n_verts = int(verts.shape[0])
        n_tris = int(tris.shape[0]) if tris is not None else n_verts // 3
        keep = (verts, tris)
    out, ptr, out_dev = _bitmap_out(depth, out, aligned=True)
    info = np.zeros(8, np.uint64)
    if isinstance(mesh, Mesh):
        st = lib().fhip_mesh_voxels(hip._h, mesh._owner.h, _p(m2w), depth, ptr, out_dev, _p(info))
    else:
        st = lib().fhip_triangles_voxels(hip._h, vp, n_verts, tp, n_tris, dev, _p(m2w), depth, ptr, out_dev, _p(info))
    del keep
    hip.check(st)
    res = _bitmap_of(hip, out, out_dev, depth, {"cells": 0, "full": 0, "empty": 0, "leaf_cells": 0})
    res.mesh_info = dict(zip(MESH_INFO, (int(v) for v in info)))
    res._n = res.mesh_info["set_voxels"]
    if res.mesh_info["rejected"]:
        raise ValueError(f"voxelize_mesh: {res.mesh_info['rejected']} of {res.mesh_info['triangles']} triangles rejected: a vertex that is not finite or "
                         "lies outside [-1.5, 1.5] after mesh_to_world, or an index beyond the vertices")
    return res


# ---- the check of a triangle mesh: weld, edges, shells, volume (fhip_triangles_topology, fhip_mesh_topology) ----------------------
TOPOLOGY_COUNTS = ("triangles", "rejected", "degenerate", "vertices", "edges", "boundary", "flipped", "nonmanifold", "unbalanced", "shells", "vertex_slots", "edge_slots")
EDGE_KINDS = ("boundary", "flipped", "nonmanifold", "unbalanced")


class Topology:
    """What `mesh_topology` found.  `.counts`: {triangles, rejected, degenerate, vertices, edges, boundary, flipped, nonmanifold,
    unbalanced, shells, vertex_slots, edge_slots}; `.closed`: no unbalanced edge - what parity filling needs; `.manifold`: no boundary,
    flipped or nonmanifold edge; `.euler` = vertices - edges + (triangles - degenerate).  `.vertices` [V, 3] float32 and `.triangles`
    [T, 3] uint64: the indexed mesh - welded, or as given - which goes straight into `voxelize_mesh` as the pair
    `(t.vertices, t.triangles)`; `.triangle_shell` [T] uint32, 0xFFFFFFFF for a degenerate triangle; `.shells`: a dict of arrays, one
    row per shell in the order of their first triangles - triangles, first, unbalanced, lo, hi, volume6, area2; a shell with volume6 < 0
    is an inward-facing cavity.  `.volume` = sum(volume6) / 6 and `.area` = sum(area2) / 2, added on the host in shell order.  The
    host arrays are copied from the device when first asked for.  Every integer is the same from run to run; volume6 and area2 are
    float64 sums of the same terms in an order of arrival that may differ from run to run, and they alone."""
    def __init__(self, owner, hip):
        self._owner, self._hip = owner, hip
        c = np.zeros(16, np.uint64)
        lib().fhip_topology_counts(owner.h, _p(c))
        self.counts = dict(zip(TOPOLOGY_COUNTS, (int(v) for v in c)))
        n = self.counts["shells"]
        self.shells = {"triangles": np.zeros(n, np.uint64), "first": np.zeros(n, np.uint32), "unbalanced": np.zeros(n, np.uint64), "lo": np.zeros((n, 3), np.float32),
                       "hi": np.zeros((n, 3), np.float32), "volume6": np.zeros(n, np.float64), "area2": np.zeros(n, np.float64)}
        hip.check(lib().fhip_topology_shells(owner.h, *(_p(self.shells[k]) for k in ("triangles", "first", "unbalanced", "lo", "hi", "volume6", "area2"))))
        self._host = {}

    closed = property(lambda self: self.counts["unbalanced"] == 0)
    manifold = property(lambda self: self.counts["boundary"] == self.counts["flipped"] == self.counts["nonmanifold"] == 0)
    euler = property(lambda self: self.counts["vertices"] - self.counts["edges"] + self.counts["triangles"] - self.counts["degenerate"])
    volume = property(lambda self: float(sum(float(v) for v in self.shells["volume6"])) / 6.0)
    area = property(lambda self: float(sum(float(v) for v in self.shells["area2"])) / 2.0)

    def _shape(self, what):
        T = self.counts["triangles"]
        return {"vertices": ((int(lib().fhip_topology_vertex_rows(self._owner.h)), 3), np.float32, "<f4"), "triangles": ((T, 3), np.uint64, "<u8"),
                "triangle_shells": ((T,), np.uint32, "<u4")}[what]

    def _array(self, what):
        if what not in self._host:
            shape, dtype, _ = self._shape(what)
            a = np.zeros(shape, dtype)
            self._hip.check(getattr(lib(), "fhip_topology_" + what)(self._owner.h, _p(a)))
            self._host[what] = a
        return self._host[what]

    def _device(self, what):
        ptr = getattr(lib(), f"fhip_topology_{what}_dev")(self._owner.h)
        shape, _, typestr = self._shape(what)
        return _DeviceArray(self._owner, ptr, shape, typestr) if ptr else None

    vertices = property(lambda self: self._array("vertices"))
    triangles = property(lambda self: self._array("triangles"))
    triangle_shell = property(lambda self: self._array("triangle_shells"))

    def vertices_device(self):
        """`.vertices` where they are in device memory, as `Mesh.vertices_device` gives a mesh's; None for a mesh without triangles"""
        return self._device("vertices")

    def triangles_device(self):
        """... `.triangles` ("<u8": see `Mesh.triangles_device`)"""
        return self._device("triangles")

    def triangle_shell_device(self):
        """... and `.triangle_shell` ("<u4")"""
        return self._device("triangle_shells")

    def slices(self, zs, table_log2=0):
        """fhip_topology_slices: this indexed mesh cut by the planes z = zs[p] (float32, finite, strictly ascending) -> MeshSlices: per
        plane the closed polygons whose vertices lie on the mesh's edges.  `table_log2`: 0, or the size of the crossing edges' hash table
        as a power of two (tests; a table too small raises FidgetHipError Overflow)."""
        zs = np.ascontiguousarray(zs, np.float32).reshape(-1)
        h = C.c_void_p()
        self._hip.check(lib().fhip_topology_slices(self._hip._h, self._owner.h, _p(zs), len(zs), int(table_log2), C.byref(h)))
        return MeshSlices(_Handle(h.value, lib().fhip_slices_free), self._hip, self)

    def edges(self, kind, device=False):
        """fhip_topology_edges: the edges of one class - "boundary" (where the holes are), "flipped", "nonmanifold", "unbalanced" - as
        [n, 2] uint32 vertex pairs (a, b), a < b, in the order of the first corners that use them: a numpy array, or with `device` a
        torch CUDA tensor (int32: the bits of the uint32 pairs)."""
        k = EDGE_KINDS.index(kind)
        n = self.counts[kind]
        if device:
            import torch
            out = torch.empty((n, 2), dtype=torch.int32, device="cuda")
            self._hip.check(lib().fhip_topology_edges(self._hip._h, self._owner.h, k, _dev_ptr(out) if n else None, 1))
            self._hip.sync()
            return out
        out = np.zeros((n, 2), np.uint32)
        self._hip.check(lib().fhip_topology_edges(self._hip._h, self._owner.h, k, _p(out), 0))
        return out


def mesh_topology(mesh, weld=None, hip=None, table_log2=0):
    """fhip_triangles_topology / fhip_mesh_topology: what kind of triangle mesh this is -> Topology: the welded indexed mesh, the class
    of every edge (boundary, flipped, nonmanifold, unbalanced), the shells - edge-connected parts - with their triangles, bounds, volume
    and area; the definitions stand in include/fidget_hip.h.  `mesh`: as for `voxelize_mesh` - a `Mesh` (its resident device arrays are
    read where they are), float32 [T, 3, 3] triangles (numpy or a torch CUDA tensor), or a pair (vertices [V, 3] float32, triangles
    [T, 3] indices), both numpy or both torch CUDA.  `weld`: make one vertex of all corners with equal coordinates (-0 equals +0);
    default on for a soup, where it cannot be turned off, and off for a pair or a `Mesh`, whose indices then are the vertices.
    `table_log2`: 0, or the size of both hash tables as a power of two (tests; a table too small raises FidgetHipError Overflow).
    ValueError when triangles were rejected: a coordinate that is not finite, or an index beyond the vertices.  All integer results
    are the same from run to run; the shells' volume6 and area2 - float64 sums in an order of arrival - alone may differ in their last
    bits."""
    keep = None          # what the pointers point into, until the call returns
    h = C.c_void_p()
    if isinstance(mesh, Mesh):
        hip = mesh._hip
        st = lib().fhip_mesh_topology(hip._h, mesh._owner.h, int(bool(weld)), int(table_log2), C.byref(h))
    else:
        hip = hip or default_context()
        pair = isinstance(mesh, (tuple, list)) and len(mesh) == 2 and all(hasattr(a, "shape") for a in mesh)
        if isinstance(mesh, (tuple, list)) and not pair and any(hasattr(a, "shape") for a in mesh):
            raise TypeError("mesh_topology: a mesh is a Mesh, [T, 3, 3] triangles, or a pair (vertices [V, 3], triangles [T, 3]) of two arrays")
        verts, tris = mesh if pair else (mesh, None)
        if tris is None and weld is not None and not weld:
            raise ValueError("mesh_topology: a soup of triangles has no vertices until it is welded: weld=False needs a pair or a Mesh")
        if isinstance(verts, np.ndarray) or not hasattr(verts, "is_cuda"):
            verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
            vp, dev = _p(verts), 0
            if tris is not None:
                tris = np.ascontiguousarray(tris, np.uint64).reshape(-1, 3)
            tp = _p(tris)
        else:
            assert verts.is_cuda and verts.element_size() == 4 and verts.is_floating_point(), "vertices on the device: a float32 CUDA tensor"
            verts = verts.contiguous().reshape(-1, 3)
            vp, dev = _dev_ptr(verts), 1
            if tris is not None:
                assert tris.is_cuda and tris.element_size() == 8 and not tris.is_floating_point(), "triangles on the device: an int64 CUDA tensor"
                tris = tris.contiguous().reshape(-1, 3)
            tp = _dev_ptr(tris)
        n_verts = int(verts.shape[0])
        n_tris = int(tris.shape[0]) if tris is not None else n_verts // 3
        keep = (verts, tris)
        st = lib().fhip_triangles_topology(hip._h, vp, n_verts, tp, n_tris, dev, int(tris is None if weld is None else bool(weld)), int(table_log2), C.byref(h))
    del keep
    hip.check(st)
    res = Topology(_Handle(h.value, lib().fhip_topology_free), hip)
    if res.counts["rejected"]:
        raise ValueError(f"mesh_topology: {res.counts['rejected']} of {res.counts['triangles']} triangles rejected: a coordinate that is not finite, or an index beyond the vertices")
    return res


# ---- the slices of a triangle mesh: contour loops per plane (fhip_topology_slices) -------------------------------------------------
SLICES_COUNTS = ("planes", "vertices", "segments", "loops", "irregular", "edge_slots")


class MeshSlices:
    """What `mesh_slices` found: the mesh of a `Topology` cut by planes z = const; the definitions stand in include/fidget_hip.h.
    `.counts`: {planes, vertices, segments, loops, irregular, edge_slots}; `.zs` float32 [P]; `.per_plane`: {crossings, segments, loops}
    uint64 [P]; `.topology`: the mesh that was cut.  Per crossing - a vertex of the slice on a mesh edge, ids in the order of the edges'
    first corners and then by plane: `.xy` float32 [n, 2], `.plane` uint32 [n], `.edge` uint32 [n, 2] (u < v), `.next` uint32 [n]
    (0xFFFFFFFF: no segment leaves), `.loop_of` uint32 [n], `.degree` uint8 [n] (out | in << 4, each at most 15).  `.loops`: a dict of
    arrays, a row per loop in ascending order of leader - leader, plane, crossings, segments, irregular, area2 (float64: > 0 an outer
    boundary, < 0 a hole), lo, hi [., 2].  The crossings' arrays stay in device memory (`.xy_device()` ...); host copies are made when
    first asked for.  Everything is the same from run to run but area2, a float64 sum in an order of arrival."""

    def __init__(self, owner, hip, topology=None):
        self._owner, self._hip, self.topology = owner, hip, topology
        c = np.zeros(8, np.uint64)
        lib().fhip_slices_counts(owner.h, _p(c))
        self.counts = dict(zip(SLICES_COUNTS, (int(v) for v in c)))
        P, L = self.counts["planes"], self.counts["loops"]
        self.zs = np.zeros(P, np.float32)
        self.per_plane = {"crossings": np.zeros(P, np.uint64), "segments": np.zeros(P, np.uint64), "loops": np.zeros(P, np.uint64)}
        hip.check(lib().fhip_slices_planes(owner.h, _p(self.zs), *(_p(self.per_plane[k]) for k in ("crossings", "segments", "loops"))))
        self._loops = {"leader": np.zeros(L, np.uint32), "plane": np.zeros(L, np.uint32), "crossings": np.zeros(L, np.uint32), "segments": np.zeros(L, np.uint32),
                       "irregular": np.zeros(L, np.uint32), "area2": np.zeros(L, np.float64), "lo": np.zeros((L, 2), np.float32), "hi": np.zeros((L, 2), np.float32)}
        hip.check(lib().fhip_slices_loops(owner.h, *(_p(a) for a in self._loops.values())))
        self._host = None

    def _vertices(self):
        if self._host is None:
            n = self.counts["vertices"]
            a = {"xy": np.zeros((n, 2), np.float32), "plane": np.zeros(n, np.uint32), "edge": np.zeros((n, 2), np.uint32), "next": np.zeros(n, np.uint32),
                 "loop_of": np.zeros(n, np.uint32), "degree": np.zeros(n, np.uint8)}
            self._hip.check(lib().fhip_slices_vertices(self._owner.h, *(_p(v) for v in a.values())))
            self._host = a
        return self._host

    xy = property(lambda self: self._vertices()["xy"])
    plane = property(lambda self: self._vertices()["plane"])
    edge = property(lambda self: self._vertices()["edge"])
    next = property(lambda self: self._vertices()["next"])
    loop_of = property(lambda self: self._vertices()["loop_of"])
    degree = property(lambda self: self._vertices()["degree"])
    loops = property(lambda self: self._loops)

    def _plane(self, p):
        p = int(p)
        if not 0 <= p < self.counts["planes"]:
            raise IndexError(f"plane {p} is not among 0 .. {self.counts['planes'] - 1}")
        return p

    def loops_of(self, p):
        """the ids of plane p's loops, ascending"""
        return np.flatnonzero(self._loops["plane"] == self._plane(p))

    def polygons(self, p):
        """-> (the closed loops of plane p as float32 [n, 2] arrays, each from its leader on along `next`: walked on the host; the number
        of plane p's loops left out because they hold an irregular crossing)"""
        out, skipped = [], 0
        for q in self.loops_of(p):
            if self._loops["irregular"][q]:
                skipped += 1
                continue
            m = int(self._loops["crossings"][q])
            ids, v = np.zeros(m, np.int64), int(self._loops["leader"][q])
            for k in range(m):
                ids[k] = v
                v = int(self.next[v])
            out.append(self.xy[ids])
        return out, skipped

    def svg(self, p, path=None):
        """Plane p's closed loops as one <path fill-rule="evenodd"> each, `M x y L x y ... Z`, with y negated - SVG's y grows downward -
        and the bounds of the plane's loops as the viewBox.  Returns the text; written to `path` when given."""
        polys, _ = self.polygons(p)
        ids = self.loops_of(p)
        lo = self._loops["lo"][ids].min(axis=0) if len(ids) else np.array([-1.0, -1.0])
        hi = self._loops["hi"][ids].max(axis=0) if len(ids) else np.array([1.0, 1.0])
        paths = "".join('<path fill-rule="evenodd" d="M ' + " L ".join(f"{float(x):.9g} {-float(y):.9g}" for x, y in q) + ' Z"/>\n' for q in polys)
        text = (f'<svg xmlns="http://www.w3.org/2000/svg" viewBox="{float(lo[0]):.9g} {-float(hi[1]):.9g} {float(hi[0] - lo[0]):.9g} {float(hi[1] - lo[1]):.9g}">\n'
                f'{paths}</svg>\n')
        if path is not None:
            with open(path, "w") as f:
                f.write(text)
        return text

    def _device(self, what, shape, typestr):
        ptr = getattr(lib(), f"fhip_slices_{what}_dev")(self._owner.h)
        return _DeviceArray(self._owner, ptr, shape, typestr) if ptr else None

    def xy_device(self):
        """`.xy` where it is in device memory ([n, 2] "<f4") as an object carrying `__cuda_array_interface__` that keeps the result
        alive; None when nothing crosses"""
        return self._device("xy", (self.counts["vertices"], 2), "<f4")

    def next_device(self):
        """... `.next` ("<i4": the bits of the uint32 ids, as `Outlines.next_device` gives its)"""
        return self._device("next", (self.counts["vertices"],), "<i4")

    def loop_of_device(self):
        """... `.loop_of` ("<i4")"""
        return self._device("loop", (self.counts["vertices"],), "<i4")

    def plane_device(self):
        """... and `.plane` ("<i4")"""
        return self._device("plane", (self.counts["vertices"],), "<i4")

    def nesting(self, bands=0):
        """fhip_slices_nesting: which regular loop of a plane contains which, on the device from the arrays this call left there ->
        SliceNesting: polygons with holes per plane.  `bands`: 0, or the number of y-bands of every plane's segment index (tests; no
        result depends on it)."""
        h = C.c_void_p()
        self._hip.check(lib().fhip_slices_nesting(self._hip._h, self._owner.h, int(bands), C.byref(h)))
        return SliceNesting(self, _Handle(h.value, lib().fhip_slice_nesting_free))

    def __repr__(self):
        return f"MeshSlices({', '.join(f'{k}={v}' for k, v in self.counts.items())})"


SLICE_NESTING_PLANES = ("regular", "outer", "top", "max_depth", "improper", "misoriented")


class SliceNesting:
    """The containment tree of the regular loops of a `MeshSlices` (`MeshSlices.nesting()`), per plane; the definitions stand in
    include/fidget_hip.h.  `.slices`; `.n_loops`, `.n_regular`, `.n_outer` (even depth), `.n_top` (no parent), `.max_depth`,
    `.n_improper` (loops whose parent is not one level up: loops cross), `.n_misoriented` (orientation against depth); `.per_plane`:
    {regular, outer, top, max_depth, improper, misoriented} uint64 [P], also as `.regular`, `.outer` ...; `.bands` uint32 [P] and
    `.index` = {bands, entries, hits}: the segment index that was used.  Per loop, [n_loops] with `NONE` = 0xFFFFFFFF for none and for
    irregular loops, copied when first asked for: `.parent`, `.depth`, `.n_children` uint32, `.region_area2` float64 - area2 of the
    loop and of its children.  parent and depth also stay in device memory (`.parent_device()`, `.depth_device()`)."""
    NONE = 0xFFFFFFFF

    def __init__(self, slices, owner):
        self.slices, self._owner, self._hip = slices, owner, slices._hip
        c = np.zeros(16, np.uint64)
        lib().fhip_slice_nesting_counts(owner.h, _p(c))
        self.n_loops, self.n_regular, self.n_outer, self.n_top, self.max_depth, self.n_improper, self.n_misoriented, self.n_planes = (int(v) for v in c[:8])
        self.index = {"bands": int(c[8]), "entries": int(c[9]), "hits": int(c[10])}
        P = self.n_planes
        self.per_plane = {k: np.zeros(P, np.uint64) for k in SLICE_NESTING_PLANES}
        self.bands = np.zeros(P, np.uint32)
        self._hip.check(lib().fhip_slice_nesting_planes(owner.h, *(_p(a) for a in self.per_plane.values()), _p(self.bands)))
        self._loops = None
        self._children = None

    regular = property(lambda self: self.per_plane["regular"])
    outer = property(lambda self: self.per_plane["outer"])
    top = property(lambda self: self.per_plane["top"])
    plane_max_depth = property(lambda self: self.per_plane["max_depth"])
    improper = property(lambda self: self.per_plane["improper"])
    misoriented = property(lambda self: self.per_plane["misoriented"])

    def _table(self):
        if self._loops is None:
            n = self.n_loops
            t = {key: np.zeros(n, np.float64 if key == "region_area2" else np.uint32) for key in ("parent", "depth", "n_children", "region_area2")}
            self._hip.check(lib().fhip_slice_nesting_loops(self._owner.h, *(_p(a) for a in t.values())))
            self._loops = t
        return self._loops

    parent = property(lambda self: self._table()["parent"])
    depth = property(lambda self: self._table()["depth"])
    n_children = property(lambda self: self._table()["n_children"])
    region_area2 = property(lambda self: self._table()["region_area2"])

    def children(self):
        """fhip_nesting_children -> (child_start uint64 [n_loops + 1], children uint32): the children of loop l, ascending, are
        children[child_start[l]:child_start[l + 1]]; loops without a parent are in no list"""
        if self._children is None:
            n = self.n_loops
            start, kids = np.zeros(n + 1, np.uint64), np.zeros(n, np.uint32)
            self._hip.check(lib().fhip_nesting_children(_p(self.parent), n, _p(start), _p(kids)))
            self._children = (start, kids[:int(start[n])])
        return self._children

    def regions(self, p):
        """plane p's polygons with holes as [(outer loop id, [hole ids])]: every regular loop of even depth of the plane, ascending,
        with its children - even-odd filling; every regular loop of the plane is in exactly one region where no loops cross"""
        start, kids = self.children()
        depth = self.depth
        return [(int(l), [int(c) for c in kids[int(start[l]):int(start[l + 1])]]) for l in self.slices.loops_of(p) if depth[l] != self.NONE and depth[l] % 2 == 0]

    def _walk(self, l):
        s = self.slices
        m, v = int(s.loops["crossings"][l]), int(s.loops["leader"][l])
        ids = np.zeros(m, np.int64)
        for k in range(m):
            ids[k] = v
            v = int(s.next[v])
        return s.xy[ids]

    def polygons(self, p):
        """the same regions as [(outer float32 [m, 2], [holes float32 [m, 2]])], each loop walked from its leader as
        `MeshSlices.polygons(p)` walks it"""
        return [(self._walk(l), [self._walk(c) for c in holes]) for l, holes in self.regions(p)]

    def svg(self, p, path=None):
        """Plane p as one <path fill-rule="evenodd"> per region, the outer boundary and its holes as its subpaths `M x y L x y ... Z`:
        holes render empty and islands as regions of their own.  Coordinates and viewBox as in `MeshSlices.svg`.  Returns the text;
        written to `path` when given."""
        s = self.slices
        ids = s.loops_of(p)
        lo = s.loops["lo"][ids].min(axis=0) if len(ids) else np.array([-1.0, -1.0])
        hi = s.loops["hi"][ids].max(axis=0) if len(ids) else np.array([1.0, 1.0])
        sub = lambda q: "M " + " L ".join(f"{float(x):.9g} {-float(y):.9g}" for x, y in q) + " Z"          # noqa: E731
        paths = "".join('<path fill-rule="evenodd" d="' + " ".join(sub(q) for q in [outer] + holes) + '"/>\n' for outer, holes in self.polygons(p))
        text = (f'<svg xmlns="http://www.w3.org/2000/svg" viewBox="{float(lo[0]):.9g} {-float(hi[1]):.9g} {float(hi[0] - lo[0]):.9g} {float(hi[1] - lo[1]):.9g}">\n'
                f'{paths}</svg>\n')
        if path is not None:
            with open(path, "w") as f:
                f.write(text)
        return text

    def _device(self, what):
        ptr = getattr(lib(), f"fhip_slice_nesting_{what}_dev")(self._owner.h)
        return _DeviceArray(self._owner, ptr, (self.n_loops,), "<i4") if ptr else None

    def parent_device(self):
        """`.parent` where it is in device memory ([n_loops] "<i4": the bits of the uint32 ids, NONE as -1) as an object carrying
        `__cuda_array_interface__` that keeps the result alive; None for an empty result"""
        return self._device("parent")

    def depth_device(self):
        """... and `.depth` ("<i4")"""
        return self._device("depth")

    def __repr__(self):
        return (f"SliceNesting(planes={self.n_planes}, loops={self.n_loops}, regular={self.n_regular}, outer={self.n_outer}, top={self.n_top}, "
                f"max_depth={self.max_depth}, improper={self.n_improper}, misoriented={self.n_misoriented})")


def mesh_slices(mesh, zs, weld=None, hip=None, table_log2=0):
    """fhip_topology_slices: the step a slicer performs on an STL - the triangles cut by the planes z = zs[p] -> MeshSlices.  `mesh`:
    anything `mesh_topology` takes - a `Mesh`, [T, 3, 3] triangles, a pair (vertices, triangles), numpy or torch CUDA - which is run
    first with `weld`, or a `Topology`, which is cut as it is.  `zs`: float32, finite and strictly ascending, else FidgetHipError
    Unsupported."""
    topo = mesh if isinstance(mesh, Topology) else mesh_topology(mesh, weld, hip)
    return topo.slices(zs, table_log2)
