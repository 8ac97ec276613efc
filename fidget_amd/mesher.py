"""The mesher and what counts down its octree: `mesh`, `Mesh`, `build_mesh`, the parts and their merge for several GPUs, `mesh_sample`,
and `occupancy`.

Late imports (inside the methods, `trimesh` comes after this module): `Mesh.voxelize` -> `trimesh.voxelize_mesh`, `Mesh.topology` ->
`trimesh.mesh_topology`, `Mesh.slices` -> `trimesh.mesh_slices`."""
import ctypes as C

import numpy as np

from ._abi import _DeviceArray, _Handle, _p, lib
from .render import _dev_ptr, _var_arrays


# ---- fidget_mesh: leaf sampling on the device -----------------------------------------------------------------------
MESH_LEAF = np.dtype([("bounds", np.float32, 6), ("path", np.uint64), ("mask", np.uint32), ("n_edges", np.uint32), ("n_verts", np.uint32),
                      ("pad", np.uint32), ("inter", np.uint16, (12, 3)), ("pad2", np.uint16, 4), ("pos", np.float32, (12, 3)),
                      ("grad", np.float32, (12, 4)), ("vert", np.float32, (4, 3)), ("qef_err", np.float32, 4)])


def debug_walk_dual(cells, root, verts, parallel):
    """Octree::walk_dual of the library's host side on a given octree (fhip_debug_walk_dual): (triangles, vertices)"""
    cells = np.ascontiguousarray(cells, np.uint32)
    root = np.ascontiguousarray(root, np.uint32)
    verts = np.ascontiguousarray(verts, np.float32)
    c = np.zeros(2, np.uint64)
    lib().fhip_debug_walk_dual(_p(cells), len(cells), _p(root), _p(verts), len(verts), int(parallel), _p(c), None, None)
    tris = np.zeros((int(c[0]), 3), np.uint64)
    out = np.zeros((int(c[1]), 3), np.float32)
    lib().fhip_debug_walk_dual(_p(cells), len(cells), _p(root), _p(verts), len(verts), int(parallel), _p(c), _p(tris), _p(out))
    return tris, out


class _MeshHandle(_Handle):
    """owner of an fhip_mesh whose arrays numpy views borrow"""
    def view(self, ptr, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if not n or not ptr:
            return np.zeros(shape, dtype)
        buf = (C.c_uint8 * n).from_address(ptr)
        buf._owner = self           # (numpy keeps `buf` as the view's base, `buf` keeps the handle)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)


def mesh(shape, depth, world_to_model=None, vars=None):
    """fidget_mesh::Octree::build(...).walk_dual(): (triangles [n, 3] uint64, vertices [m, 3] float32, counts)"""
    return mesh_sample(shape, depth, world_to_model, vars, _build=True)


class Mesh:
    """A mesh of `build_mesh`: fidget_mesh::Mesh { vertices, triangles } (fidget-mesh/src/lib.rs:64-69), with what a caller does with
    one on the device.  `.triangles` [n, 3] uint64, `.vertices` [m, 3] float32, `.counts`: the views `mesh()` returns, borrowed from the handle."""
    def __init__(self, owner, hip, triangles, vertices, counts):
        self._owner, self._hip = owner, hip
        self.triangles, self.vertices, self.counts = triangles, vertices, counts

    def stl(self, out=None):
        """Mesh::write_stl's bytes (fhip_mesh_stl) as a numpy uint8 array; with `out` (a torch CUDA uint8 tensor of at least that many
        bytes) the call is asynchronous on the context's stream and returns `out`."""
        n = int(lib().fhip_mesh_stl_bytes(self._owner.h))
        if out is not None:
            assert out.is_cuda and out.is_contiguous() and out.element_size() == 1 and out.numel() >= n
            self._hip.check(lib().fhip_mesh_stl(self._hip._h, self._owner.h, _dev_ptr(out), 1))
            return out
        buf = np.zeros(n, np.uint8)
        self._hip.check(lib().fhip_mesh_stl(self._hip._h, self._owner.h, _p(buf), 0))
        return buf

    def write_stl(self, path):
        """Mesh::write_stl (fidget-mesh/src/output.rs:5-38) to a file"""
        with open(path, "wb") as f:
            f.write(self.stl().tobytes())

    def vertex_grads(self, shape, vars=None, out=None):
        """fhip_mesh_vertex_grads: [m, 4] float32 {v, dx, dy, dz} of `shape` at the mesh's vertices (model space, unnormalised); with
        `out` (a torch CUDA float32 tensor [m, 4]) the result stays on the device and `out` is returned."""
        n = len(self.vertices)
        vk, vv = _var_arrays(shape, vars)
        ax = None
        if shape._vars is not None:
            ax = np.array(shape._vars, dtype=np.int32)
            vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
        if out is not None:
            assert out.is_cuda and out.is_contiguous() and out.element_size() == 4 and out.numel() == 4 * n
            ptr, dev, res = _dev_ptr(out), 1, out
        else:
            res = np.zeros((n, 4), np.float32)
            ptr, dev = _p(res), 0
        st = lib().fhip_mesh_vertex_grads(self._hip._h, shape._h, self._owner.h, _p(ax), _p(vk), _p(vv), len(vk), ptr, dev)
        if st == 4:
            raise ValueError("MissingVar")
        self._hip.check(st)
        return res

    def voxelize(self, depth, out=None):
        """`voxelize_mesh(self, depth, out=out)`: the solid this mesh encloses as a Voxels, from the resident arrays where there are any"""
        from .trimesh import voxelize_mesh
        return voxelize_mesh(self, depth, out=out)

    def topology(self, weld=None):
        """`mesh_topology(self, weld)`: what kind of mesh this is - edges, shells, volume - from the resident arrays where there are any"""
        from .trimesh import mesh_topology
        return mesh_topology(self, weld)

    def slices(self, zs):
        """`mesh_slices(self, zs)`: the contour loops in which the planes z = zs[p] cut this mesh, from the resident arrays where there are any"""
        from .trimesh import mesh_slices
        return mesh_slices(self, zs)

    def vertices_device(self):
        """The vertices where the dual walk left them in device memory ([m, 3] float32), as an object carrying
        `__cuda_array_interface__` that keeps the mesh alive - `torch.as_tensor(obj, device="cuda")` views it; None when the
        arrays are not resident (built with keep_device off, by the host's walk, or empty)."""
        ptr = lib().fhip_mesh_vertices_dev(self._owner.h)
        return _DeviceArray(self._owner, ptr, (len(self.vertices), 3), "<f4") if ptr else None

    def triangles_device(self):
        """... and the triangles ([n, 3] vertex indices; "<u8", which torch takes from version 2.3 on - older ones want
        `torch.as_tensor(obj, device="cuda")` of a copy of the interface with typestr "<i8": the indices are below 2^63)"""
        ptr = lib().fhip_mesh_triangles_dev(self._owner.h)
        return _DeviceArray(self._owner, ptr, (len(self.triangles), 3), "<u8") if ptr else None


def build_mesh(shape, depth, world_to_model=None, vars=None, keep_device=True):
    """fidget_mesh::Octree::build(...).walk_dual() as a `Mesh` object.  keep_device: context option mesh_keep_device for this build (the
    option is restored afterwards) - the device walk's arrays stay resident for .stl(), .vertex_grads() and the *_device() views."""
    hip = shape.hip
    with hip.options(mesh_keep_device=1 if keep_device else 0):
        owner, tris, verts, counts = mesh_sample(shape, depth, world_to_model, vars, _build=True, _owner=True)
    return Mesh(owner, hip, tris, verts, counts)


def mesh_part(shape, depth, part, n_parts, world_to_model=None, vars=None, alloc=None):
    """The device side of a mesh build for part `part` of `n_parts` (the root's octants o with o * n_parts // 8 == part;
    fhip_mesh_sample_part), as the flat uint8 buffer fhip_mesh_part_export writes: what a rank sends to the merging rank.
    `alloc(nbytes)` -> writable uint8 array to export into (shared memory, say); default: a fresh numpy array."""
    hip = shape.hip
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    vk, vv = _var_arrays(shape, vars)
    ax = None
    if shape._vars is not None:
        ax = np.array(shape._vars, dtype=np.int32)
        vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
    h = C.c_void_p()
    st = lib().fhip_mesh_sample_part(hip._h, shape._h, depth, _p(w2m), _p(ax), _p(vk), _p(vv), len(vk), part, n_parts, C.byref(h))
    if st == 4:
        raise ValueError("MissingVar")
    hip.check(st)
    try:
        n = int(lib().fhip_mesh_part_bytes(h))
        buf = np.zeros(n, np.uint8) if alloc is None else alloc(n)
        assert buf.dtype == np.uint8 and buf.size == n and buf.flags.c_contiguous
        lib().fhip_mesh_part_export(h, buf.ctypes.data_as(C.c_void_p))
    finally:
        lib().fhip_mesh_free(h)
    return buf


def mesh_merge(parts, world_to_model=None, hip=None):
    """fhip_mesh_merge: the buffers of all parts (parts[k] = mesh_part(.., k, len(parts))) -> (triangles, vertices, counts),
    the mesh of `mesh()` on one GPU.  `hip`: a context for the error text only (no device work)."""
    parts = [np.ascontiguousarray(b, np.uint8) for b in parts]
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    ptrs = (C.c_void_p * len(parts))(*[b.ctypes.data for b in parts])
    sizes = np.array([b.size for b in parts], np.uint64)
    h = C.c_void_p()
    st = lib().fhip_mesh_merge(hip._h if hip is not None else None, ptrs, _p(sizes), len(parts), _p(w2m), C.byref(h))
    if st:
        if hip is not None:
            hip.check(st)
        raise RuntimeError(f"fhip_mesh_merge: status {st}")
    try:
        c = np.zeros(8, np.uint64)
        lib().fhip_mesh_counts(h, _p(c))
        verts = np.zeros((int(c[6]), 3), np.float32)
        tris = np.zeros((int(c[7]), 3), np.uint64)
        if len(verts):
            lib().fhip_mesh_vertices(h, _p(verts))
        if len(tris):
            lib().fhip_mesh_triangles(h, _p(tris))
    finally:
        lib().fhip_mesh_free(h)
    return tris, verts, {"cells": int(c[0]), "full": int(c[1]), "empty": int(c[2]), "leaf_cells": int(c[3]), "levels": int(c[5])}


def mesh_sample(shape, depth, world_to_model=None, vars=None, _build=False, _owner=False):
    """The evaluation side of fidget_mesh::Octree::build on the device (fhip_mesh_sample): returns (leaf records as a
    MESH_LEAF array, counts dict)."""
    hip = shape.hip
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    vk, vv = _var_arrays(shape, vars)
    ax = None
    if shape._vars is not None:
        ax = np.array(shape._vars, dtype=np.int32)
        vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
    h = C.c_void_p()
    fn = lib().fhip_mesh_build if _build else lib().fhip_mesh_sample
    st = fn(hip._h, shape._h, depth, _p(w2m), _p(ax), _p(vk), _p(vv), len(vk), C.byref(h))
    if st == 4:
        raise ValueError("MissingVar")
    hip.check(st)
    try:
        c = np.zeros(8, np.uint64)
        lib().fhip_mesh_counts(h, _p(c))
        assert int(c[4]) == MESH_LEAF.itemsize, (int(c[4]), MESH_LEAF.itemsize)
        counts = {"cells": int(c[0]), "full": int(c[1]), "empty": int(c[2]), "leaf_cells": int(c[3]), "levels": int(c[5])}
        if _build:
            # the arrays where the mesh holds them, no copy: numpy views whose base keeps the handle (freed with the last of them)
            owner = _MeshHandle(h, lib().fhip_mesh_free)
            h = None
            verts = owner.view(lib().fhip_mesh_vertices_ptr(owner.h), (int(c[6]), 3), np.float32)
            tris = owner.view(lib().fhip_mesh_triangles_ptr(owner.h), (int(c[7]), 3), np.uint64)
            return (owner, tris, verts, counts) if _owner else (tris, verts, counts)
        leaves = np.zeros(int(c[3]), MESH_LEAF)
        if len(leaves):
            lib().fhip_mesh_leaves(h, _p(leaves))
    finally:
        lib().fhip_mesh_free(h)
    return leaves, {"cells": int(c[0]), "full": int(c[1]), "empty": int(c[2]), "leaf_cells": int(c[3]), "levels": int(c[5])}


# ---- shape occupancy: volume, centroid, second moments, bounds (fhip_shape_occupancy) ------------------------------------
class OccupancyStruct(C.Structure):
    """fhip_occupancy (include/fidget_hip.h)"""
    _fields_ = [("n", C.c_uint64), ("s1", C.c_uint64 * 3), ("s2", C.c_uint64 * 6), ("lo", C.c_uint32 * 3), ("hi", C.c_uint32 * 3),
                ("grid", C.c_uint32), ("pad", C.c_uint32), ("cells", C.c_uint64 * 4)]


class Occupancy:
    """The inside voxels of the grid of N = 4 << depth per axis over [-1, 1]^3, as the integers fhip_shape_occupancy returns (Python
    ints: n, s1 (sum of i, j, k), s2 (sum of i^2, j^2, k^2, ij, ik, jk), lo / hi (inclusive, lo = N and hi = 0 when empty), grid,
    cells = {"cells", "full", "empty", "leaf_cells"} as mesh_sample counts them) and what follows from them in float64, in the region's
    own coordinates, with h = 2 / N."""

    def __init__(self, raw):
        self.n = int(raw.n)
        self.s1 = tuple(int(v) for v in raw.s1)
        self.s2 = tuple(int(v) for v in raw.s2)
        self.lo = tuple(int(v) for v in raw.lo)
        self.hi = tuple(int(v) for v in raw.hi)
        self.grid = int(raw.grid)
        self.cells = dict(zip(("cells", "full", "empty", "leaf_cells"), (int(v) for v in raw.cells)))

    @property
    def h(self):
        return 2.0 / self.grid

    @property
    def volume(self):
        return self.n * self.h ** 3

    @property
    def centroid(self):
        """mean of the inside voxels' centres, -1 + (i + 1/2) h per axis; NaN for an empty shape"""
        if self.n == 0:
            return np.full(3, np.nan)
        # (the quotient of the integers first: exact to the last place)
        return np.array([-1.0 + (s / self.n + 0.5) * self.h for s in self.s1], np.float64)

    @property
    def covariance(self):
        """second moments of the inside voxels' centres about the centroid, [3, 3]: h^2 (sum ab / n - (sum a / n)(sum b / n)), the
        numerator n sum ab - sum a sum b taken in integers, so nothing cancels in floating point"""
        if self.n == 0:
            return np.full((3, 3), np.nan)
        pair = {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (0, 2): 4, (1, 2): 5}
        out = np.zeros((3, 3), np.float64)
        for a in range(3):
            for b in range(3):
                num = self.n * self.s2[pair[(min(a, b), max(a, b))]] - self.s1[a] * self.s1[b]
                out[a, b] = num / (self.n * self.n) * self.h * self.h
        return out

    @property
    def bounds(self):
        """the faces of the outermost inside voxels: ([x0, y0, z0], [x1, y1, z1]); NaN for an empty shape"""
        if self.n == 0:
            return np.full(3, np.nan), np.full(3, np.nan)
        return (np.array([-1.0 + l * self.h for l in self.lo], np.float64), np.array([-1.0 + (u + 1) * self.h for u in self.hi], np.float64))

    def __repr__(self):
        return f"Occupancy(grid={self.grid}, n={self.n}, s1={self.s1}, s2={self.s2}, lo={self.lo}, hi={self.hi}, cells={self.cells})"


def occupancy(shape, depth, world_to_model=None, vars=None):
    """fhip_shape_occupancy: the solid `shape < 0` on the grid of 4 << depth voxels per axis over [-1, 1]^3 (world_to_model as for
    `mesh`), counted down the mesher's octree -> Occupancy"""
    hip = shape.hip
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    vk, vv = _var_arrays(shape, vars)
    ax = None
    if shape._vars is not None:
        ax = np.array(shape._vars, dtype=np.int32)
        vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
    raw = OccupancyStruct()
    st = lib().fhip_shape_occupancy(hip._h, shape._h, depth, _p(w2m), _p(ax), _p(vk), _p(vv), len(vk), C.byref(raw))
    if st == 4:
        raise ValueError("MissingVar")
    hip.check(st)
    return Occupancy(raw)
