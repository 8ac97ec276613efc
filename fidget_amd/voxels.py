"""The voxel family: `voxelize` and its `Voxels` bitmap, and what is made of one - `Outlines` and their `Nesting`, `Surface`, `DistanceField`,
`ThicknessField`, `Components`."""
import ctypes as C
import math

import numpy as np

from ._abi import FidgetHipError, _DeviceArray, _Handle, _p, lib
from .mesher import Mesh, _MeshHandle
from .render import _dev_ptr, _var_arrays


# ---- shape voxels: the inside voxels as a packed bitmap, layer images, voxels per layer (fhip_shape_voxels) ---------------
def voxels_unpack(bricks):
    """bricks uint64 [B, B, B] (indexed [bz, by, bx]; bit lx + 4 ly + 16 lz of a word: voxel (4 bx + lx, 4 by + ly, 4 bz + lz)) ->
    bool [N, N, N], N = 4 B, indexed [i, j, k]"""
    b = np.ascontiguousarray(bricks, "<u8")
    B = b.shape[0]
    bits = np.unpackbits(b.view(np.uint8).reshape(B, B, B, 8), axis=-1, bitorder="little")       # [bz, by, bx, 16 lz + 4 ly + lx]
    return bits.reshape(B, B, B, 4, 4, 4).transpose(2, 5, 1, 4, 0, 3).reshape(4 * B, 4 * B, 4 * B).astype(bool)


def _bitmap_out(depth, out, device=None, aligned=False):
    """Where a call writes a result bitmap of this depth -> (out, pointer, on the device?).  `out`: a contiguous torch CUDA tensor of at
    least 8 B^3 bytes, B = 1 << depth, or a contiguous writeable numpy array of that size; without it a new one - a torch int64
    [B, B, B] on `device`, or with no device a numpy uint64 [B, B, B].  `aligned`: a tensor that is not 8-byte aligned fails the
    assertion here; otherwise it is left to the library's error."""
    B = 1 << depth
    words = int(lib().fhip_voxels_words(depth))       # (0 beyond depth 10: the call refuses before it touches `out`)
    if out is None and device is not None:
        import torch
        out = torch.empty((B, B, B), dtype=torch.int64, device=device)
    if out is not None and not isinstance(out, np.ndarray):
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() >= 8 * words and (not aligned or out.data_ptr() % 8 == 0)
        return out, _dev_ptr(out), 1
    if out is None:
        out = np.zeros((B, B, B) if words else 0, np.uint64)
    assert out.flags.c_contiguous and out.flags.writeable and out.nbytes >= 8 * words
    return out, _p(out), 0


def _bitmap_of(hip, out, dev, depth, cells=None):
    """the bitmap a call wrote into `out` (`_bitmap_out`) -> Voxels: the first 8 B^3 bytes as [B, B, B] bricks"""
    B = 1 << depth
    if dev:
        import torch
        bricks = out.reshape(-1).view(torch.uint8)[:8 * B ** 3].view(torch.int64).view(B, B, B)
    else:
        bricks = out.reshape(-1).view(np.uint8)[:8 * B ** 3].view(np.uint64).reshape(B, B, B)
    return Voxels(hip, bricks, depth, cells)


class Voxels:
    """The bitmap of `voxelize`: `.bricks` [B, B, B] (numpy uint64, or a view of the caller's torch CUDA tensor as int64), `.depth`,
    `.grid` = N = 4 B, `.cells` = {"cells", "full", "empty", "leaf_cells"} as Occupancy's, `.n` = the number of inside voxels.  What is
    made of it runs where the bricks are: on the host's arrays through the library's staging buffers, or on the device in place and
    asynchronous on the context's stream."""

    def __init__(self, hip, bricks, depth, cells):
        self._hip, self.bricks, self.depth, self.grid, self.cells = hip, bricks, int(depth), 4 << int(depth), cells
        self._n = None

    @property
    def on_device(self):
        return not isinstance(self.bricks, np.ndarray)

    def _ptr(self):
        return _dev_ptr(self.bricks) if self.on_device else _p(self.bricks)

    def slices(self, k0, k1, out=None):
        """fhip_voxels_slices: uint8 [k1 - k0, N, N], [k - k0, j, i] = 255 where voxel (i, j, k) is inside, 0 where not: numpy for bricks
        on the host; for bricks on the device a torch CUDA tensor (`out`, contiguous uint8 of that size, or a new one)"""
        N = self.grid
        k0, k1 = int(k0), int(k1)
        n = max(k1 - k0, 0) * N * N
        if self.on_device:
            if out is None:
                import torch
                out = torch.empty((max(k1 - k0, 0), N, N), dtype=torch.uint8, device=self.bricks.device)
            assert out.is_cuda and out.is_contiguous() and out.element_size() == 1 and out.numel() >= n
            self._hip.check(lib().fhip_voxels_slices(self._hip._h, self._ptr(), self.depth, k0, k1, _dev_ptr(out), 1))
            return out
        assert out is None, "bricks on the host: the images are returned as a numpy array"
        img = np.zeros((max(k1 - k0, 0), N, N), np.uint8)
        self._hip.check(lib().fhip_voxels_slices(self._hip._h, self._ptr(), self.depth, k0, k1, _p(img), 0))
        return img

    def layer_counts(self):
        """fhip_voxels_layer_counts: [N] inside voxels per third index k: numpy uint64, or a torch CUDA int64 tensor for bricks on the device"""
        if self.on_device:
            import torch
            out = torch.empty(self.grid, dtype=torch.int64, device=self.bricks.device)
            self._hip.check(lib().fhip_voxels_layer_counts(self._hip._h, self._ptr(), self.depth, _dev_ptr(out), 1))
            return out
        out = np.zeros(self.grid, np.uint64)
        self._hip.check(lib().fhip_voxels_layer_counts(self._hip._h, self._ptr(), self.depth, _p(out), 0))
        return out

    @property
    def n(self):
        """the number of set bits (Occupancy.n at the same depth)"""
        if self._n is None:
            self._n = int(self.layer_counts().sum())
        return self._n

    def inside(self):
        """bool [N, N, N] indexed [i, j, k], unpacked on the host (bricks on the device are copied there first)"""
        b = self.bricks.cpu().numpy().view(np.uint64) if self.on_device else self.bricks
        return voxels_unpack(b)

    def components(self, connectivity=6, complement=False):
        """fhip_voxels_components: the connected parts of the set bits - with `complement` of the clear bits, whose parts away from the
        grid's border are the enclosed voids - under connectivity 6 (faces) or 26 (faces, edges, corners) -> Components"""
        h = C.c_void_p()
        self._hip.check(lib().fhip_voxels_components(self._hip._h, self._ptr(), self.depth, int(self.on_device), int(connectivity), int(bool(complement)), C.byref(h)))
        return Components(self, _Handle(h.value, lib().fhip_components_free), int(connectivity), bool(complement))

    def distance(self, complement=False):
        """fhip_voxels_distance: the exact squared Euclidean distance, in voxels, from every voxel to the nearest set bit - with
        `complement` to the nearest clear bit -> DistanceField"""
        h = C.c_void_p()
        self._hip.check(lib().fhip_voxels_distance(self._hip._h, self._ptr(), self.depth, int(self.on_device), int(bool(complement)), C.byref(h)))
        return DistanceField(self, _Handle(h.value, lib().fhip_distance_free), bool(complement))

    def thickness(self, complement=False):
        """the local thickness of the solid's walls - `distance(complement=True).thickness()` - or with `complement` the local width of
        the empty space - `distance().thickness()` -> ThicknessField"""
        return self.distance(complement=not complement).thickness()

    def mesh(self):
        """fhip_voxels_mesh: the boundary of the set voxels -> Mesh.  Every exposed face of a voxel is two triangles, counter-clockwise
        seen from outside, in the order (brick word, direction -x +x -y +y -z +z, bit); the vertices are the lattice corners the faces
        use, one each, at float(2 a - N) / N in the cube [-1, 1]^3 the bitmap was sampled in.  The arrays are resident on the device
        (`.stl()`, `.vertex_grads()`, `.vertices_device()`, `.triangles_device()`) and copied to the host (`.triangles`, `.vertices`);
        `.counts` holds the octree's counters, all 0 here.  Overflow: 2^32 triangles or vertices and more."""
        h = C.c_void_p()
        self._hip.check(lib().fhip_voxels_mesh(self._hip._h, self._ptr(), self.depth, int(self.on_device), C.byref(h)))
        owner = _MeshHandle(h.value, lib().fhip_mesh_free)
        c = np.zeros(8, np.uint64)
        lib().fhip_mesh_counts(owner.h, _p(c))
        counts = {"cells": int(c[0]), "full": int(c[1]), "empty": int(c[2]), "leaf_cells": int(c[3]), "levels": int(c[5])}
        verts = owner.view(lib().fhip_mesh_vertices_ptr(owner.h), (int(c[6]), 3), np.float32)
        tris = owner.view(lib().fhip_mesh_triangles_ptr(owner.h), (int(c[7]), 3), np.uint64)
        return Mesh(owner, self._hip, tris, verts, counts)

    def surface(self):
        """fhip_voxels_surface: the counting pass of `mesh()` alone -> Surface: exposed faces per direction, used lattice corners and
        edges, and from them the area and the Euler number"""
        out = np.zeros(10, np.uint64)
        self._hip.check(lib().fhip_voxels_surface(self._hip._h, self._ptr(), self.depth, int(self.on_device), _p(out)))
        return Surface(self.grid, out)

    def offset(self, r, out=None):
        """the solid grown by a ball of radius r >= 0 - `distance().within(r)` - or shrunk by one of radius -r -
        `distance(complement=True).beyond(-r)`: what stays is farther than |r| from the nearest clear voxel, so offset(-1) keeps the
        voxels at distance 1 and removes nothing; to take the surface layer off, use beyond(squared=1) -> Voxels (`out` as for `within`)"""
        if r >= 0:
            return self.distance().within(r, out=out)
        return self.distance(complement=True).beyond(-r, out=out)

    def opened(self, r):
        """shrunk by r, then grown by r: drops what no ball of that radius fits into (specks, thin walls)"""
        return self.offset(-r).offset(r)

    def closed(self, r):
        """grown by r, then shrunk by r: fills what no ball of that radius fits into (pinholes, thin gaps)"""
        return self.offset(r).offset(-r)

    # ---- along a direction: d = 0 .. 5 = -x, +x, -y, +y, -z, +z, e(d) its unit vector, d ^ 1 its opposite --------------------------
    def _out_device(self):
        """where a new result bitmap goes (`_bitmap_out`): the bricks' device, or None for the host"""
        return self.bricks.device if self.on_device else None

    def flow(self, dir, blockers=None, with_seeds=False, out=None):
        """fhip_voxels_flow: these voxels as seeds S flowing towards direction `dir` past the blockers K (a Voxels of the same depth, in
        the same place as these; None: none) -> Voxels R (`.cells` None) with R(p) = (R(p - e) | S(p - e)) & ~K(p), R and S false
        outside the grid: R(p) holds iff there is t >= 1 with S(p - t e) and no blocker at p - s e for all 0 <= s < t.  A seed that is
        itself blocked still emits; a blocked voxel is never in R.  `with_seeds`: R | S.  `out` as for `DistanceField.within`, not
        the seeds' or the blockers' own array.  The space trapped along an axis - reachable from neither side, an undercut of a
        two-part mould - is the AND of the two opposite shadows: `a.shadow(4).bricks & a.shadow(5).bricks`."""
        if blockers is not None:
            if not isinstance(blockers, Voxels) or blockers.depth != self.depth:
                raise ValueError("blockers: a Voxels of the same depth")
            if blockers.on_device != self.on_device:
                raise ValueError("seeds and blockers live in the same place: both on the host or both on the device")
        out, ptr, dev = _bitmap_out(self.depth, out, self._out_device())
        self._hip.check(lib().fhip_voxels_flow(self._hip._h, self._ptr(), None if blockers is None else blockers._ptr(), self.depth, int(self.on_device),
                                               int(dir), 1 if with_seeds else 0, ptr, dev))
        return _bitmap_of(self._hip, out, dev, self.depth)

    def shadow(self, dir, out=None):
        """the clear voxels with a set voxel behind them, seen towards `dir`: `flow(dir, blockers=self)`"""
        return self.flow(dir, blockers=self, out=out)

    def swept(self, dir, out=None):
        """the solid swept towards `dir` to the grid's border - the shadow and the solid: `flow(dir, with_seeds=True)`"""
        return self.flow(dir, with_seeds=True, out=out)

    def overhangs(self, up=5, reach2=1, bed=True, out=None):
        """fhip_voxels_overhangs: the set voxels that are not supported when the part is built towards `up` -> Voxels.  p is supported iff
        there is a set q one layer below, (q - p) . e(up) = -1, whose squared perpendicular offset is at most `reach2` (0 .. 16): a
        Euclidean disc - 0 straight below only, 1 a plus of five, 2 the 3 x 3 square.  For p in the first layer every q counts as set
        iff `bed`, and as clear otherwise.  `out` as for `flow`."""
        out, ptr, dev = _bitmap_out(self.depth, out, self._out_device())
        self._hip.check(lib().fhip_voxels_overhangs(self._hip._h, self._ptr(), self.depth, int(self.on_device), int(up), int(reach2), int(bool(bed)), ptr, dev))
        return _bitmap_of(self._hip, out, dev, self.depth)

    def supports(self, up=5, reach2=1, bed=True, out=None):
        """the clear columns under every overhanging voxel, down to the next set voxel or the grid's border:
        `overhangs(up, reach2, bed).flow(up ^ 1, blockers=self)`.  On the device the calls are asynchronous on the context's stream: a
        bitmap handed to them must stay allocated until that stream has passed them - with a context on a stream other than torch's
        current one, keep the tensors (or synchronise) before dropping them."""
        over = self.overhangs(up, reach2, bed)
        res = over.flow(int(up) ^ 1, blockers=self, out=out)
        res._seeds = over          # (on the device the flow may still be reading them: they live as long as the result)
        return res

    def heights(self, axis=2, out=None):
        """fhip_voxels_heights: int32 [3, N, N] over the columns along `axis`, indexed by the two remaining coordinates, the lower axis
        fastest - axis 2 gives [j][i], 1 [k][i], 0 [k][j].  Plane 0: the smallest coordinate along the axis of a set voxel in the
        column, -1 in an empty column; plane 1: the largest, -1 likewise; plane 2: the number of set voxels.  numpy, or a torch CUDA
        int32 tensor for bricks on the device; `out`: a contiguous array of either kind with 4-byte elements and that size."""
        N = self.grid
        if out is None and self.on_device:
            import torch
            out = torch.empty((3, N, N), dtype=torch.int32, device=self.bricks.device)
        if out is not None and not isinstance(out, np.ndarray):
            assert out.is_cuda and out.is_contiguous() and out.element_size() == 4 and out.numel() >= 3 * N * N
            ptr, dev = _dev_ptr(out), 1
        else:
            if out is None:
                out = np.zeros((3, N, N), np.int32)
            assert out.flags.c_contiguous and out.flags.writeable and out.itemsize == 4 and out.size >= 3 * N * N
            ptr, dev = _p(out), 0
        self._hip.check(lib().fhip_voxels_heights(self._hip._h, self._ptr(), self.depth, int(self.on_device), int(axis), ptr, dev))
        return out

    def outlines(self, k0, k1, connectivity=4):
        """fhip_voxels_outlines: the boundary loops of every layer k0 <= k < k1 (layers along z, as for `slices`) -> Outlines.  The
        loops are closed rectilinear polygons over the corners (a, b), 0 <= a, b <= N, of the layer image P(i, j) = voxel (i, j, k),
        clear outside the grid; directed with the inside on the left, so an outer boundary runs counter-clockwise (area2 > 0) and a
        hole clockwise (area2 < 0); vertices only where the outline turns.  `connectivity` 4: pixels that touch at a corner alone
        are separate, 8: they are joined - it decides how the two vertices of a saddle corner pair up.  One blocking call, run where
        the bricks are; the vertices' arrays stay in device memory.  Integers throughout: the same bits from run to run."""
        h = C.c_void_p()
        self._hip.check(lib().fhip_voxels_outlines(self._hip._h, self._ptr(), self.depth, int(self.on_device), int(k0), int(k1), int(connectivity), C.byref(h)))
        return Outlines(_Handle(h.value, lib().fhip_outlines_free), self._hip, self)

    def outline(self, k, connectivity=4):
        """the loops of the one layer k: `outlines(k, k + 1)`"""
        return self.outlines(k, int(k) + 1, connectivity)

    def __repr__(self):
        return f"Voxels(depth={self.depth}, grid={self.grid}, cells={self.cells}, on_device={self.on_device})"


class Outlines:
    """The loops of `Voxels.outlines(k0, k1)`.  `.grid` = N, `.k0`, `.k1`, `.connectivity`, `.n_vertices`, `.n_loops`, `.n_layers`.
    Per layer (index k - k0): `.vertex_start` and `.loop_start` uint64 [K + 1], the ranges of the layer's vertices and loops - ids are
    global, layers ascending; `.layer_area2` int64 [K] = twice the layer's set voxels; `.layer_perimeter` uint64 [K] = its unit
    boundary edges.  Per vertex: `.xy()` uint16 [n, 2] the corner (a, b); `.next()` uint32 [n] the next vertex along the loop, a
    permutation inside each layer; `.loop_of()` uint32 [n].  Per loop (`.table()`): leader - its smallest vertex id; loops are numbered
    by ascending leader - n_vertices, area2 (int64 shoelace sum: > 0 an outer boundary, < 0 a hole), perimeter, lo and hi [., 2].
    The vertices' arrays stay in device memory (`.xy_device()` ...); host copies are made when first asked for.  `.voxels`: the
    bitmap that was outlined, which `nesting()` reads again."""

    def __init__(self, owner, hip, voxels=None):
        self._owner, self._hip, self.voxels = owner, hip, voxels
        c = np.zeros(8, np.uint64)
        lib().fhip_outlines_counts(owner.h, _p(c))
        self.n_vertices, self.n_loops, self.n_layers, self.grid, self.k0, self.connectivity = (int(v) for v in c[:6])
        self.k1 = self.k0 + self.n_layers
        K = self.n_layers
        self.vertex_start, self.loop_start = np.zeros(K + 1, np.uint64), np.zeros(K + 1, np.uint64)
        self.layer_area2, self.layer_perimeter = np.zeros(K, np.int64), np.zeros(K, np.uint64)
        hip.check(lib().fhip_outlines_layers(owner.h, _p(self.vertex_start), _p(self.loop_start), _p(self.layer_area2), _p(self.layer_perimeter)))
        self._host = None
        self._table = None

    def _layer(self, k, start):
        """the range of layer k in `start`, or everything"""
        if k is None:
            return 0, int(start[-1])
        k = int(k)
        if not self.k0 <= k < self.k1:
            raise IndexError(f"layer {k} is not among {self.k0} .. {self.k1 - 1}")
        return int(start[k - self.k0]), int(start[k - self.k0 + 1])

    def _vertices(self):
        if self._host is None:
            n = self.n_vertices
            xy, nxt, loop = np.zeros((n, 2), np.uint16), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
            self._hip.check(lib().fhip_outlines_vertices(self._owner.h, 0, n, _p(xy), _p(nxt), _p(loop)))
            self._host = (xy, nxt, loop)
        return self._host

    def xy(self, k=None):
        """uint16 [n, 2]: the corners (a, b) of all vertices, or of layer k's"""
        lo, hi = self._layer(k, self.vertex_start)
        return self._vertices()[0][lo:hi]

    def next(self, k=None):
        """uint32 [n]: every vertex's successor; for one layer the ids stay global - subtract `vertex_start[k - k0]`"""
        lo, hi = self._layer(k, self.vertex_start)
        return self._vertices()[1][lo:hi]

    def loop_of(self, k=None):
        """uint32 [n]: every vertex's loop; global ids likewise"""
        lo, hi = self._layer(k, self.vertex_start)
        return self._vertices()[2][lo:hi]

    def table(self, k=None):
        """{"leader", "n_vertices", "area2", "perimeter", "lo", "hi"}: a row per loop, of all layers or of layer k"""
        if self._table is None:
            n = self.n_loops
            t = {"leader": np.zeros(n, np.uint32), "n_vertices": np.zeros(n, np.uint32), "area2": np.zeros(n, np.int64), "perimeter": np.zeros(n, np.uint64),
                 "lo": np.zeros((n, 2), np.uint16), "hi": np.zeros((n, 2), np.uint16)}
            self._hip.check(lib().fhip_outlines_loops(self._owner.h, 0, n, *(_p(t[key]) for key in ("leader", "n_vertices", "area2", "perimeter", "lo", "hi"))))
            self._table = t
        lo, hi = self._layer(k, self.loop_start)
        return {key: a[lo:hi] for key, a in self._table.items()}

    def polygons(self, k):
        """layer k's loops as int arrays [m, 2] of corners, each from its leader on, in loop order: walked along `next` on the host"""
        xy, nxt, _ = self._vertices()
        t = self.table(k)
        out = []
        for leader, m in zip(t["leader"], t["n_vertices"]):
            ids, v = np.zeros(int(m), np.int64), int(leader)
            for q in range(int(m)):
                ids[q] = v
                v = int(nxt[v])
            out.append(xy[ids].astype(np.int64))
        return out

    def world(self, k):
        """-> (polygons as float32 [m, 2] in the cube [-1, 1]^3 - corner a at float(2 a - N) / N, as `Voxels.mesh` places it - and the
        layer's z, its centre float(2 k + 1 - N) / N)"""
        N = self.grid
        return [((2 * p - N).astype(np.float32) / np.float32(N)) for p in self.polygons(k)], float(np.float32(2 * int(k) + 1 - N) / np.float32(N))

    def svg(self, k, path=None):
        """Layer k as one <path fill-rule="evenodd"> per loop, `M x y L x y ... Z`, in `world`'s coordinates with y negated - SVG's y
        grows downward - and the cube's square as the viewBox, like `Contours.svg`.  Returns the text; written to `path` when given."""
        polys, _ = self.world(k)
        paths = "".join('<path fill-rule="evenodd" d="M ' + " L ".join(f"{float(x):.9g} {-float(y):.9g}" for x, y in p) + ' Z"/>\n' for p in polys)
        text = f'<svg xmlns="http://www.w3.org/2000/svg" viewBox="-1 -1 2 2">\n{paths}</svg>\n'
        if path is not None:
            with open(path, "w") as f:
                f.write(text)
        return text

    def _device(self, what, shape, typestr):
        ptr = getattr(lib(), f"fhip_outlines_{what}_dev")(self._owner.h)
        return _DeviceArray(self._owner, ptr, shape, typestr) if ptr else None

    def xy_device(self):
        """`.xy()` where it is in device memory ([n, 2] "<i2": the bits of the uint16 corners, which stay below 2^15) as an object
        carrying `__cuda_array_interface__` that keeps the result alive; None when there are no vertices"""
        return self._device("xy", (self.n_vertices, 2), "<i2")

    def next_device(self):
        """... `.next()` ("<i4": the bits of the uint32 ids, as `Contours.segments_device` gives its)"""
        return self._device("next", (self.n_vertices,), "<i4")

    def loop_of_device(self):
        """... and `.loop_of()` ("<i4")"""
        return self._device("loop", (self.n_vertices,), "<i4")

    def nesting(self):
        """fhip_outlines_nesting: which hole belongs to which outer boundary and which island lies in which hole -> Nesting.  One
        blocking call on the device, over this result's arrays and the bitmap that was outlined (`.voxels`, which must not have
        changed since)."""
        if self.voxels is None:
            raise ValueError("these outlines do not know their bitmap")
        v = self.voxels
        h = C.c_void_p()
        self._hip.check(lib().fhip_outlines_nesting(self._hip._h, self._owner.h, v._ptr(), int(v.on_device), C.byref(h)))
        return Nesting(self, _Handle(h.value, lib().fhip_nesting_free))

    def __repr__(self):
        return (f"Outlines(grid={self.grid}, layers={self.k0}..{self.k1}, connectivity={self.connectivity}, vertices={self.n_vertices}, "
                f"loops={self.n_loops})")


class Nesting:
    """The containment tree of the loops of an `Outlines` (`Outlines.nesting()`), per layer.  `.outlines`; `.n_loops`, `.n_outer` (loops
    with area2 > 0), `.n_top` (loops without a parent), `.max_depth`; per layer (index k - k0) `.outer`, `.top` uint64 [K] and
    `.layer_max_depth` uint32 [K].  Per loop, uint32 [n_loops] with global ids and `NONE` = 0xFFFFFFFF for none, copied when first asked
    for: `.left` - the loop that owns the nearest boundary edge left of the loop's leader on the leader's pixel row; `.parent` - the
    first loop of the chain left, left[left], ... whose area2 has the other sign: a hole's outer boundary, an island's hole; `.depth`
    - 0 without a parent, even exactly for outer boundaries; `.n_children`; and `.region_area2` int64 - area2 of the loop and of its
    children: for an outer boundary twice the set pixels of one connected part of the layer.  parent and depth also stay in device
    memory (`.parent_device()`, `.depth_device()`)."""
    NONE = 0xFFFFFFFF

    def __init__(self, outlines, owner):
        self.outlines, self._owner, self._hip = outlines, owner, outlines._hip
        c = np.zeros(8, np.uint64)
        lib().fhip_nesting_counts(owner.h, _p(c))
        self.n_loops, self.n_outer, self.n_top, self.max_depth, self.n_layers, self.k0, self.connectivity = (int(v) for v in c[:7])
        self.k1 = self.k0 + self.n_layers
        K = self.n_layers
        self.outer, self.top, self.layer_max_depth = np.zeros(K, np.uint64), np.zeros(K, np.uint64), np.zeros(K, np.uint32)
        self._hip.check(lib().fhip_nesting_layers(owner.h, _p(self.outer), _p(self.top), _p(self.layer_max_depth)))
        self._loops = None
        self._children = None

    def _table(self):
        if self._loops is None:
            n = self.n_loops
            t = {key: np.zeros(n, np.int64 if key == "region_area2" else np.uint32) for key in ("left", "parent", "depth", "n_children", "region_area2")}
            self._hip.check(lib().fhip_nesting_loops(self._owner.h, 0, n, *(_p(a) for a in t.values())))
            self._loops = t
        return self._loops

    left = property(lambda self: self._table()["left"])
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

    def regions(self, k):
        """layer k's polygons with holes as [(outer loop id, [hole ids])]: every outer boundary of the layer, ascending, with its
        children; ids are global, and every loop of the layer is in exactly one region"""
        lo, hi = self.outlines._layer(k, self.outlines.loop_start)
        area2 = self.outlines.table()["area2"]
        start, kids = self.children()
        return [(l, [int(c) for c in kids[int(start[l]):int(start[l + 1])]]) for l in range(lo, hi) if area2[l] > 0]

    def polygons(self, k):
        """the same regions as [(outer int [m, 2], [holes int [m, 2]])], the loops of `Outlines.polygons(k)`"""
        lo, _ = self.outlines._layer(k, self.outlines.loop_start)
        polys = self.outlines.polygons(k)
        return [(polys[l - lo], [polys[c - lo] for c in holes]) for l, holes in self.regions(k)]

    def svg(self, k, path=None):
        """Layer k as one <path fill-rule="evenodd"> per region, the outer boundary and its holes as its subpaths `M x y L x y ... Z`:
        holes render empty and islands as regions of their own.  Coordinates as in `Outlines.svg`.  Returns the text; written to
        `path` when given."""
        lo, _ = self.outlines._layer(k, self.outlines.loop_start)
        world, _ = self.outlines.world(k)
        sub = lambda p: "M " + " L ".join(f"{float(x):.9g} {-float(y):.9g}" for x, y in p) + " Z"          # noqa: E731
        paths = "".join('<path fill-rule="evenodd" d="' + " ".join(sub(world[q - lo]) for q in [l] + holes) + '"/>\n' for l, holes in self.regions(k))
        text = f'<svg xmlns="http://www.w3.org/2000/svg" viewBox="-1 -1 2 2">\n{paths}</svg>\n'
        if path is not None:
            with open(path, "w") as f:
                f.write(text)
        return text

    def _device(self, what):
        ptr = getattr(lib(), f"fhip_nesting_{what}_dev")(self._owner.h)
        return _DeviceArray(self._owner, ptr, (self.n_loops,), "<i4") if ptr else None

    def parent_device(self):
        """`.parent` where it is in device memory ([n_loops] "<i4": the bits of the uint32 ids, NONE as -1) as an object carrying
        `__cuda_array_interface__` that keeps the result alive; None when there are no loops"""
        return self._device("parent")

    def depth_device(self):
        """... and `.depth` ("<i4")"""
        return self._device("depth")

    def __repr__(self):
        return (f"Nesting(layers={self.k0}..{self.k1}, connectivity={self.connectivity}, loops={self.n_loops}, outer={self.n_outer}, top={self.n_top}, "
                f"max_depth={self.max_depth})")


class Surface:
    """The surface summary of a bitmap (`Voxels.surface`): `.faces` the exposed faces per direction -x, +x, -y, +y, -z, +z; `.vertices`
    the lattice corners whose eight voxels are not all equal; `.edges` the lattice edges whose four voxels are not all equal; `.n` the
    set voxels.  `.n_faces` their sum over the directions, `.area` = n_faces h^2 with h = 2 / N, in the cube [-1, 1]^3; `.euler` =
    vertices - edges + n_faces: 2 for a solid without handles or voids, 2 more for every void, 2 fewer for every handle, 1 more where
    two parts touch along an edge or at a corner only.  Outside the grid is clear: the surface is closed."""
    def __init__(self, grid, raw):
        raw = [int(v) for v in raw]
        self.grid, self.faces, self.vertices, self.edges, self.n_faces, self.n = int(grid), tuple(raw[:6]), raw[6], raw[7], raw[8], raw[9]
        self.area = self.n_faces * (2.0 / self.grid) ** 2
        self.euler = self.vertices - self.edges + self.n_faces

    def __repr__(self):
        return f"Surface(grid={self.grid}, faces={self.faces}, vertices={self.vertices}, edges={self.edges}, area={self.area:.6g}, euler={self.euler})"


class DistanceField:
    """The exact Euclidean distance transform of a bitmap (`Voxels.distance`): per voxel the squared distance to the nearest foreground
    voxel, a uint32 - 0 on the foreground, 0xFFFFFFFF ("no distance"; -1 as int32) everywhere when there is no foreground.
    `.max_squared` the largest finite value, `.argmax` the voxel (i, j, k) of smallest index k N^2 + j N + i that has it (None without
    foreground), `.n` foreground voxels, `.depth`, `.grid`.  The field stays in device memory; results land where the bricks are - for
    bricks on the device those calls are asynchronous on the context's stream, as `Voxels.slices` is."""

    def __init__(self, voxels, owner, complement):
        self.voxels, self._owner, self.complement = voxels, owner, complement
        self._hip, self.depth, self.grid = voxels._hip, voxels.depth, voxels.grid
        c = np.zeros(4, np.uint64)
        lib().fhip_distance_info(owner.h, _p(c))
        self.max_squared, self.n = int(c[0]), int(c[2])
        N, idx = self.grid, int(c[1])
        self.argmax = None if idx == 0xFFFFFFFFFFFFFFFF else (idx % N, idx // N % N, idx // (N * N))

    def slices(self, k0, k1, out=None):
        """fhip_distance_slices: [k1 - k0, N, N], [k - k0, j, i] = the squared distance of voxel (i, j, k): numpy uint32 for bricks on the
        host; for bricks on the device a torch CUDA int32 tensor (`out`, contiguous, 4-byte elements, of that size, or a new one)"""
        v, N = self.voxels, self.grid
        k0, k1 = int(k0), int(k1)
        n = max(k1 - k0, 0) * N * N
        if v.on_device:
            if out is None:
                import torch
                out = torch.empty((max(k1 - k0, 0), N, N), dtype=torch.int32, device=v.bricks.device)
            assert out.is_cuda and out.is_contiguous() and out.element_size() == 4 and out.numel() >= n
            self._hip.check(lib().fhip_distance_slices(self._hip._h, self._owner.h, k0, k1, _dev_ptr(out), 1))
            return out
        assert out is None, "bricks on the host: the layers are returned as a numpy array"
        img = np.zeros((max(k1 - k0, 0), N, N), np.uint32)
        self._hip.check(lib().fhip_distance_slices(self._hip._h, self._owner.h, k0, k1, _p(img), 0))
        return img

    @property
    def squared_device(self):
        """the whole field where it is: uint32 [N, N, N] indexed [k, j, i], as `__cuda_array_interface__`"""
        N = self.grid
        return _DeviceArray(self._owner, lib().fhip_distance_dev(self._owner.h), (N, N, N), "<u4")

    def _threshold(self, r, squared, beyond, out):
        if (r is None) == (squared is None):
            raise ValueError("give exactly one of r and squared")
        if r is not None:
            if r < 0:
                raise ValueError("a radius is not negative")
            squared = math.floor(r * r)
        squared = int(squared)
        if squared < 0 or squared > 0xFFFFFFFF:
            raise FidgetHipError(6, "distance threshold: t at most 0xFFFFFFFE")
        out, ptr, dev = _bitmap_out(self.depth, out, self.voxels._out_device())
        if beyond == 2:          # (ThicknessField.thin)
            self._hip.check(lib().fhip_thickness_thin(self._hip._h, self._owner.h, squared, ptr, dev))
        else:
            self._hip.check(lib().fhip_distance_threshold(self._hip._h, self._owner.h, squared, int(beyond), ptr, dev))
        return _bitmap_of(self._hip, out, dev, self.depth)

    def within(self, r=None, squared=None, out=None):
        """fhip_distance_threshold: the voxels with d2 <= t as a bitmap -> Voxels (`.cells` None).  Exactly one of `r` - a radius in
        voxels, t = floor(r * r) - and `squared` - t itself.  `out` as for `Components.extract`: a contiguous torch CUDA tensor of at
        least 8 B^3 bytes, or a contiguous numpy array of that size, written completely; without it a new one where the bricks are."""
        return self._threshold(r, squared, 0, out)

    def beyond(self, r=None, squared=None, out=None):
        """... the voxels with d2 > t; "no distance" is beyond every t"""
        return self._threshold(r, squared, 1, out)

    def thickness(self):
        """fhip_distance_thickness: per voxel the squared radius of the largest ball that holds it and no foreground voxel of this field
        -> ThicknessField.  Refused for a field without foreground."""
        h = C.c_void_p()
        self._hip.check(lib().fhip_distance_thickness(self._hip._h, self._owner.h, C.byref(h)))
        return ThicknessField(self.voxels, _Handle(h.value, lib().fhip_distance_free), self.complement)

    def __repr__(self):
        return f"DistanceField(depth={self.depth}, grid={self.grid}, max_squared={self.max_squared}, argmax={self.argmax}, n={self.n}, complement={self.complement})"


class ThicknessField(DistanceField):
    """The local thickness of a distance field (`DistanceField.thickness`, `Voxels.thickness`): per voxel T = the largest F(c) over the
    centres c with F(c) > |p - c|^2, the squared radius of the largest ball that fits beside the field's foreground and holds the
    voxel; 0 on that foreground.  A uint32 in squared voxels, exact.  Of `distance(complement=True)` it is the wall thickness of the
    solid: a slab w voxels thick reads ceil(w / 2)^2 - 14 gives 49, 17 gives 81 - so 2 sqrt(T) is the wall in voxels, rounded up to even.
    Of `distance()` it is the local width of the empty space: pores, channels, clearance.
    `.max_squared`, `.argmax` the largest value and the voxel (i, j, k) of smallest index k N^2 + j N + i that has it; `.min_squared`,
    `.argmin` the smallest positive one likewise (None when nothing is covered); `.n` the voxels with T > 0; `.balls` how many balls
    were painted, of `.centres` candidates; `.complement` that of the distance field.  `slices`, `squared_device`, `within` and
    `beyond` are DistanceField's, on T."""

    def __init__(self, voxels, owner, complement):
        super().__init__(voxels, owner, complement)
        c = np.zeros(8, np.uint64)
        lib().fhip_thickness_info(owner.h, _p(c))
        N = self.grid

        def voxel(idx):
            return None if idx == 0xFFFFFFFFFFFFFFFF else (idx % N, idx // N % N, idx // (N * N))
        self.max_squared, self.argmax, self.n, self.centres, self.balls = int(c[0]), voxel(int(c[1])), int(c[4]), int(c[6]), int(c[7])
        self.min_squared, self.argmin = (int(c[2]), voxel(int(c[3]))) if self.n else (None, None)

    def thin(self, r=None, squared=None, out=None):
        """fhip_thickness_thin: the voxels with 0 < T <= t - what no ball larger than that reaches, the walls thinner than about
        2 sqrt(t) -> Voxels.  `r`, `squared` and `out` as for `within`."""
        return self._threshold(r, squared, 2, out)

    def histogram(self, edges_squared):
        """fhip_thickness_histogram: the voxels with e[b] <= T < e[b + 1] for 2 to 1024 ascending edges in squared voxels: numpy uint64
        [len(edges) - 1], or a torch CUDA int64 tensor for bricks on the device"""
        edges = np.ascontiguousarray(edges_squared, dtype=np.int64).reshape(-1)
        if len(edges) < 2 or len(edges) > 1024 or edges.min() < 0 or edges.max() > 0xFFFFFFFF or (np.diff(edges) < 0).any():
            raise ValueError("histogram: 2 to 1024 ascending edges, each a uint32")
        edges = edges.astype(np.uint32)
        if self.voxels.on_device:
            import torch
            dev = self.voxels.bricks.device
            d_edges = torch.from_numpy(edges.view(np.int32)).to(dev)
            out = torch.empty(len(edges) - 1, dtype=torch.int64, device=dev)
            self._hip.check(lib().fhip_thickness_histogram(self._hip._h, self._owner.h, _dev_ptr(d_edges), len(edges), _dev_ptr(out), 1))
            out._edges = d_edges          # (the call is asynchronous and reads them: they live as long as the result)
            return out
        out = np.zeros(len(edges) - 1, np.uint64)
        self._hip.check(lib().fhip_thickness_histogram(self._hip._h, self._owner.h, _p(edges), len(edges), _p(out), 0))
        return out

    def thickness(self):
        raise FidgetHipError(6, "thickness: of a distance field, not of a thickness")

    def __repr__(self):
        return (f"ThicknessField(depth={self.depth}, grid={self.grid}, max_squared={self.max_squared}, argmax={self.argmax}, min_squared={self.min_squared}, "
                f"argmin={self.argmin}, n={self.n}, balls={self.balls}, complement={self.complement})")


class Components:
    """The connected parts of a bitmap (`Voxels.components`), numbered by ascending seed - the voxel of smallest key word * 64 + bit:
    `.count`, `.nodes` (the bricks' own parts, what the union-find joined), `.n` (foreground voxels); per component `.sizes` uint64
    [count], `.seeds`, `.lo`, `.hi` uint32 [count, 3] (i, j, k; bounds inclusive), `.border` bool [count] (touches the grid's border:
    with complement=True the others are the enclosed voids).  It keeps its `Voxels` and hands the bricks to the calls that need them;
    for bricks on the device those calls are asynchronous on the context's stream, as `Voxels.slices` is."""

    def __init__(self, voxels, owner, connectivity, complement):
        self.voxels, self._owner, self.connectivity, self.complement = voxels, owner, connectivity, complement
        self._hip, self.depth, self.grid = voxels._hip, voxels.depth, voxels.grid
        c = np.zeros(4, np.uint64)
        lib().fhip_components_counts(owner.h, _p(c))
        self.count, self.nodes, self.n = int(c[0]), int(c[1]), int(c[2])
        n = self.count
        self.sizes, self.seeds, self.lo, self.hi = np.zeros(n, np.uint64), np.zeros((n, 3), np.uint32), np.zeros((n, 3), np.uint32), np.zeros((n, 3), np.uint32)
        border = np.zeros(n, np.uint8)
        self._hip.check(lib().fhip_components_table(owner.h, _p(self.sizes), _p(self.seeds), _p(self.lo), _p(self.hi), _p(border)))
        self.border = border.astype(bool)

    def largest(self):
        """the id of the largest component (of several, the smallest id)"""
        if not self.count:
            raise ValueError("no components")
        return int(np.argmax(self.sizes))

    def label_slices(self, k0, k1, out=None):
        """fhip_components_label_slices: int32 [k1 - k0, N, N], [k - k0, j, i] = the component of voxel (i, j, k), -1 for background:
        numpy for bricks on the host; for bricks on the device a torch CUDA tensor (`out`, contiguous int32 of that size, or a new one)"""
        v, N = self.voxels, self.grid
        k0, k1 = int(k0), int(k1)
        n = max(k1 - k0, 0) * N * N
        if v.on_device:
            if out is None:
                import torch
                out = torch.empty((max(k1 - k0, 0), N, N), dtype=torch.int32, device=v.bricks.device)
            assert out.is_cuda and out.is_contiguous() and out.element_size() == 4 and out.numel() >= n
            self._hip.check(lib().fhip_components_label_slices(self._hip._h, self._owner.h, v._ptr(), 1, k0, k1, _dev_ptr(out), 1))
            return out
        assert out is None, "bricks on the host: the images are returned as a numpy array"
        img = np.zeros((max(k1 - k0, 0), N, N), np.int32)
        self._hip.check(lib().fhip_components_label_slices(self._hip._h, self._owner.h, v._ptr(), 0, k0, k1, _p(img), 0))
        return img

    def extract(self, ids, out=None):
        """fhip_components_extract: the components `ids` as a bitmap of their own -> Voxels (`.cells` None: no octree made it).  `out`
        as for `voxelize`: a contiguous torch CUDA tensor of at least 8 B^3 bytes, or a contiguous numpy array of that size, written
        completely; without it a new one where the bricks are - a torch CUDA int64 tensor or a numpy uint64 [B, B, B]."""
        v = self.voxels
        ids = np.ascontiguousarray(np.asarray(list(ids) if not isinstance(ids, np.ndarray) else ids, np.int64).reshape(-1))
        if ((ids < 0) | (ids > 0xFFFFFFFF)).any():
            raise FidgetHipError(6, "extract: a component id beyond the number of components")
        ids = ids.astype(np.uint32)
        out, ptr, dev = _bitmap_out(self.depth, out, v._out_device(), aligned=True)
        self._hip.check(lib().fhip_components_extract(self._hip._h, self._owner.h, v._ptr(), int(v.on_device), _p(ids), len(ids), ptr, dev))
        return _bitmap_of(self._hip, out, dev, self.depth)

    def __repr__(self):
        return f"Components(count={self.count}, nodes={self.nodes}, n={self.n}, connectivity={self.connectivity}, complement={self.complement})"


def voxelize(shape, depth, world_to_model=None, vars=None, out=None):
    """fhip_shape_voxels: the solid `shape < 0` on the grid of 4 << depth voxels per axis over [-1, 1]^3 (world_to_model as for `mesh`)
    as a bitmap of 4 x 4 x 4 bricks, written down the octree `occupancy` counts -> Voxels.  `out`: a contiguous torch CUDA tensor of at
    least 8 B^3 bytes, B = 1 << depth (int64 is the natural dtype) - the bitmap stays on the device, `.bricks` views it - or a contiguous
    numpy array of that size, filled in place; without it a new numpy uint64 [B, B, B].  Either is written completely."""
    hip = shape.hip
    depth = int(depth)
    w2m = None if world_to_model is None else np.ascontiguousarray(world_to_model, np.float32)
    vk, vv = _var_arrays(shape, vars)
    ax = None
    if shape._vars is not None:
        ax = np.array(shape._vars, dtype=np.int32)
        vk = np.array([shape._named_slot(k) for k in (vars or {})], dtype=np.uint64)
    cells = np.zeros(4, np.uint64)
    out, ptr, dev = _bitmap_out(depth, out, aligned=True)
    st = lib().fhip_shape_voxels(hip._h, shape._h, depth, _p(w2m), _p(ax), _p(vk), _p(vv), len(vk), ptr, dev, _p(cells))
    if st == 4:
        raise ValueError("MissingVar")
    hip.check(st)
    return _bitmap_of(hip, out, dev, depth, dict(zip(("cells", "full", "empty", "leaf_cells"), (int(v) for v in cells))))
