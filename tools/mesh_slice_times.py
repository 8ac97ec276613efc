#!/usr/bin/env python3
"""GPU box: the times of profiles/mesh_slices/README.md.  `python tools/mesh_slice_times.py [CASE ...]` (default: all) cuts
  mdc     `build_mesh(gyroid-sphere, 8)` under 1024 planes from -1 to 1: a fine mesh, a few planes through every triangle;
  voxel   `Voxels.mesh()` of gyroid-sphere's depth-6 bitmap under its 256 centre planes: one plane through every side face;
  cube    a cube of twelve triangles under 4096 planes: the slicer's own case, a coarse STL under thousands of planes.
The topology is made once and is not timed; `Topology.slices` is called once to warm up - the context's scratch grows then - and REPS
times between two events on the context's stream: the call blocks, so this is the whole call with its four waits and its six
allocations.  Then one call with FHIP_MESH_TIMES set: the time of every pass on stderr, each after a wait for the stream.  The
yardstick, in the same run: a device-to-device copy that moves the bytes the call must move at the least - the mesh read, 12 bytes a
vertex and 24 a triangle, and 29 bytes written per crossing (xy, plane, edge, next, loop_of, degree) - that is, a copy of half as many
bytes, which reads and writes each of them once.  What was timed is checked: closed meshes give no irregular crossing, the voxel
mesh's cross-sections have the layers' areas, every loop of the cube is its square."""
import os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fidget_amd as F

REPS = 10
cases = sys.argv[1:] or ["mdc", "voxel", "cube"]
stream = torch.cuda.current_stream()
hip = F.HipContext(0, stream=stream.cuda_stream)          # the events below are recorded on the stream the library launches on
gyroid = F.Shape.from_vm(os.path.join(ROOT, "models", "gyroid-sphere.vm"), hip=hip)


def timed(call, reps=REPS):
    call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(reps):
        call()
    t1.record(stream)
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def line(what, topo, zs):
    free0 = torch.cuda.mem_get_info()[0]
    ms = timed(lambda: topo.slices(zs))
    s = topo.slices(zs)
    c, T, V = s.counts, topo.counts["triangles"], len(topo.vertices)
    moved = 12 * V + 24 * T + 29 * c["vertices"]
    n = max(moved // 2, 1)
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    copy = timed(lambda: dst.copy_(src))
    print(f"== {what}: {T} triangles {c['planes']} planes -> {c['vertices']} crossings {c['segments']} segments {c['loops']} loops {c['irregular']} irregular, "
          f"{c['edge_slots']} slots {32 * c['edge_slots'] / 2 ** 20:.1f} MiB", flush=True)
    print(f"   {ms:9.4f} ms a call   copy of the same {moved / 2 ** 20:8.2f} MiB {copy:9.4f} ms   ratio {ms / copy:7.2f}   "
          f"scratch and handle {(free0 - torch.cuda.mem_get_info()[0]) / 2 ** 20:.0f} MiB", flush=True)
    os.environ["FHIP_MESH_TIMES"] = "1"
    sys.stderr.write(f"-- {what}\n")
    sys.stderr.flush()
    t0 = time.perf_counter()
    topo.slices(zs)
    sys.stderr.write(f"the whole call on the host's clock: {time.perf_counter() - t0:.6f} s\n")
    sys.stderr.flush()
    del os.environ["FHIP_MESH_TIMES"]
    return s


if "mdc" in cases:
    topo = F.build_mesh(gyroid, 8).topology()
    s = line("build_mesh(gyroid-sphere, 8) under 1024 planes", topo, np.linspace(-1.0, 1.0, 1024).astype(np.float32))
    print(f"   the mesh: closed {topo.closed} manifold {topo.manifold}", flush=True)
    del s, topo
    hip.check(F.lib().fhip_ctx_trim(hip._h))
if "voxel" in cases:
    depth, N = 6, 256
    vox = F.voxelize(gyroid, depth, out=torch.empty((1 << depth) ** 3, dtype=torch.int64, device="cuda"))
    topo = vox.mesh().topology()
    s = line("Voxels.mesh() at depth 6 under its 256 centre planes", topo, ((2 * np.arange(N) + 1 - N) / N).astype(np.float32))
    area2 = np.zeros(N)
    np.add.at(area2, s.loops["plane"], s.loops["area2"])
    hip.sync()
    assert np.array_equal(area2 / 2 * (N / 2) ** 2, vox.layer_counts().cpu().numpy().astype(np.float64))          # every term a multiple of 1 / N^2
    assert np.all(s.per_plane["crossings"] <= s.per_plane["segments"])          # (equal but where voxels touch along an edge)
    del s, topo, vox
    hip.check(F.lib().fhip_ctx_trim(hip._h))
if "cube" in cases:
    v = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)], np.float32)
    t = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]], np.uint64)
    topo = F.mesh_topology((v, t), hip=hip)
    assert topo.closed and topo.manifold and topo.volume == 1.0
    s = line("a cube under 4096 planes", topo, np.linspace(-0.75, 0.75, 4096).astype(np.float32))
    inside = int(np.count_nonzero((s.zs > -0.5) & (s.zs <= 0.5)))
    assert s.counts["irregular"] == 0 and s.counts["loops"] == inside and s.counts["vertices"] == 8 * inside and np.all(np.abs(s.loops["area2"] - 2.0) < 1e-6)
print("== done")
