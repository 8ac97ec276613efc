#!/usr/bin/env python3
"""GPU box: the times of profiles/mesh_voxels/README.md.  `python tools/mesh_voxel_times.py [DEPTH ...]` (default 6 7 8) voxelizes
  - the boundary mesh of gyroid-sphere.vm's bitmap at each depth, back at that depth: many one-voxel triangles;
  - `build_mesh(gyroid-sphere, D)` at the largest depth D: mid-size triangles;
  - a box of 12 triangles at D: a few huge ones;
every mesh resident on the device and the bitmap written to a torch CUDA tensor.  Each is called once to warm up and then REPS times
between two events on the context's stream; the line gives the mean.  The yardstick, in the same run: a device-to-device copy that
moves the bytes the call must move - the bitmap cleared, then read and written by the fill (24 B per brick word), a triangle's record
written and read (96 B) with its column count and two sums (12 B), its three indices (24 B) and the vertices (12 B each) - that is, a
copy of half as many bytes, which reads and writes each of them once.  Then one call per case with FHIP_MESH_TIMES set: the passes'
wall times on stderr.  Last, recorded and not asserted: how the voxelized MDC mesh of a shape differs from the shape's own bitmap."""
import os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fidget_amd as F

REPS = 30
depths = [int(a) for a in sys.argv[1:]] or [6, 7, 8]
stream = torch.cuda.current_stream()
hip = F.HipContext(0, stream=stream.cuda_stream)          # the events below are recorded on the stream the library launches on
gyroid = F.Shape.from_vm(os.path.join(ROOT, "models", "gyroid-sphere.vm"), hip=hip)


def timed(call):
    """-> the mean time in ms of `call`, after one call that is not counted"""
    call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(REPS):
        call()
    t1.record(stream)
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / REPS


def line(what, depth, mesh, out):
    """`mesh`: a Mesh or a pair of CUDA tensors (vertices, triangles)"""
    words = (1 << depth) ** 3
    n_vertices, n_triangles = (len(mesh.vertices), len(mesh.triangles)) if isinstance(mesh, F.Mesh) else (len(mesh[0]), len(mesh[1]))
    moved = 24 * words + (96 + 12 + 24) * n_triangles + 12 * n_vertices
    src, dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    copy = timed(lambda: dst.copy_(src))
    ms = timed(lambda: F.voxelize_mesh(mesh, depth, out=out, hip=hip))
    res = F.voxelize_mesh(mesh, depth, out=out, hip=hip)
    i = res.mesh_info
    print(f"depth {depth} {what:28s} {ms:9.4f} ms   copy of the same {moved / 2 ** 20:8.1f} MiB {copy:9.4f} ms   ratio {ms / copy:6.2f}   "
          f"T {i['triangles']} W {i['W']} crossings {i['crossings']} clipped {i['clipped']} open {i['open_rows']} set {i['set_voxels']}", flush=True)
    os.environ["FHIP_MESH_TIMES"] = "1"
    sys.stderr.write(f"-- depth {depth} {what}\n")
    sys.stderr.flush()
    t0 = time.perf_counter()
    F.voxelize_mesh(mesh, depth, out=out, hip=hip)
    sys.stderr.write(f"the whole call on the host's clock: {time.perf_counter() - t0:.6f} s\n")
    del os.environ["FHIP_MESH_TIMES"]
    return res


def box_mesh():
    """the box [-0.8, 0.7] x [-0.6, 0.9] x [-0.75, 0.85]: 8 vertices and 12 triangles, on the device"""
    lo, hi = (-0.8, -0.6, -0.75), (0.7, 0.9, 0.85)
    v = np.array([[(hi if c >> a & 1 else lo)[a] for a in range(3)] for c in range(8)], np.float32)
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]
    t = np.array([tri for q in quads for tri in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int64)
    return torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda()


def differing(a, b, depth):
    """-> (voxels that differ, surface voxels of b: the set ones with a clear face neighbour)"""
    x = F.Voxels(hip, (a.bricks ^ b.bricks).contiguous(), depth, None)
    inner = b.distance(complement=True).beyond(squared=1)
    return x.n, b.n - inner.n


for depth in depths:
    words = (1 << depth) ** 3
    vox = F.voxelize(gyroid, depth, out=torch.empty(words, dtype=torch.int64, device="cuda"))
    out = torch.empty(words, dtype=torch.int64, device="cuda")
    m = vox.mesh()
    print(f"== depth {depth}: gyroid-sphere, {vox.n} voxels set, {8 * words / 2 ** 20:.0f} MiB of bricks, {len(m.triangles)} triangles", flush=True)
    back = line("voxel mesh of gyroid-sphere", depth, m, out)
    hip.sync()
    assert bool(torch.equal(back.bricks, vox.bricks)) and back.mesh_info["open_rows"] == 0          # what was timed is what it should be
    del m, back
    if depth == max(depths):
        built = F.build_mesh(gyroid, depth)
        res = line("build_mesh(gyroid-sphere)", depth, built, out)
        hip.sync()
        d, s = differing(res, vox, depth)
        print(f"depth {depth} MDC mesh of gyroid-sphere voxelized: {d} voxels differ from voxelize(), {100.0 * d / s:.2f} % of its {s} surface voxels; open rows {res.mesh_info['open_rows']}", flush=True)
        del built, res
        bm = box_mesh()
        res = line(f"box of {len(bm[1])} triangles", depth, bm, out)
        assert res.mesh_info["open_rows"] == 0
        del bm, res
    del vox, out

c = F.Context()
x, y, z = c.x(), c.y(), c.z()
ball = F.Shape(c, c.sub(c.sqrt(c.add(c.add(c.square(x), c.square(y)), c.square(z))), 0.8), hip=hip)
for depth in (4, 6):
    words = (1 << depth) ** 3
    vox = F.voxelize(ball, depth, out=torch.empty(words, dtype=torch.int64, device="cuda"))
    res = F.build_mesh(ball, depth).voxelize(depth, out=torch.empty(words, dtype=torch.int64, device="cuda"))
    hip.sync()
    d, s = differing(res, vox, depth)
    print(f"depth {depth} MDC mesh of a sphere of radius 0.8 voxelized: {d} voxels differ from voxelize(), {100.0 * d / s:.2f} % of its {s} surface voxels; open rows {res.mesh_info['open_rows']}", flush=True)
    assert res.mesh_info["open_rows"] == 0          # the one thing that can be asserted: this mesh closes inside the cube
print("== done")
