#!/usr/bin/env python3
"""GPU box: the times of profiles/slice_nesting/README.md.  `python tools/slice_nesting_times.py [CASE ...]` (default: all) nests the
slices of tools/mesh_slice_times.py's three meshes:
  mdc     `build_mesh(gyroid-sphere, 8)` under 1024 planes from -1 to 1;
  voxel   `Voxels.mesh()` of gyroid-sphere's depth-6 bitmap under its 256 centre planes;
  cube    a cube of twelve triangles under 4096 planes.
`MeshSlices.nesting()` is called once to warm up - the context's scratch grows then - and REPS times between two events on the
context's stream: the call blocks, so this is the whole call with its waits and its two allocations.  In the same run, the same way:
the `Topology.slices` call that made the input, and a device-to-device copy that moves the bytes the nesting must move at the least -
per crossing xy, plane, next and loop_of read (20 bytes), per loop leader, plane and flags read and parent, depth and n_children
written (24 bytes) - that is, a copy of half as many bytes.  Then one call with FHIP_MESH_TIMES set: the time of every pass on stderr,
each after a wait for the stream.  The bands' effect is printed: the bands chosen, the entries per regular segment, the hits per
regular loop.  What was timed is checked: a closed mesh has no improper loop, and every cube loop is a top-level outer boundary."""
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
    slices_ms = timed(lambda: topo.slices(zs))
    s = topo.slices(zs)
    ms = timed(lambda: s.nesting())
    nest = s.nesting()
    c = s.counts
    regular_segments = int(s.loops["crossings"][s.loops["irregular"] == 0].sum())
    moved = 20 * c["vertices"] + 24 * c["loops"]
    n = max(moved // 2, 1)
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    copy = timed(lambda: dst.copy_(src))
    print(f"== {what}: {c['planes']} planes {c['vertices']} crossings {c['loops']} loops {c['irregular']} irregular crossings -> {nest}", flush=True)
    print(f"   nesting {ms:9.4f} ms a call   the slices call beside it {slices_ms:9.4f} ms   copy of the same {moved / 2 ** 20:8.2f} MiB {copy:9.4f} ms   "
          f"ratio to the copy {ms / copy:7.2f}", flush=True)
    print(f"   bands: {nest.index['bands']} in all, per plane min {int(nest.bands.min())} median {int(np.median(nest.bands))} max {int(nest.bands.max())}; "
          f"entries {nest.index['entries']} = {nest.index['entries'] / max(regular_segments, 1):.3f} per regular segment; "
          f"hits {nest.index['hits']} = {nest.index['hits'] / max(nest.n_regular, 1):.3f} per regular loop", flush=True)
    os.environ["FHIP_MESH_TIMES"] = "1"
    sys.stderr.write(f"-- {what}\n")
    sys.stderr.flush()
    t0 = time.perf_counter()
    s.nesting()
    sys.stderr.write(f"the whole call on the host's clock: {time.perf_counter() - t0:.6f} s\n")
    sys.stderr.flush()
    del os.environ["FHIP_MESH_TIMES"]
    return s, nest


if "mdc" in cases:
    topo = F.build_mesh(gyroid, 8).topology()
    s, nest = line("build_mesh(gyroid-sphere, 8) under 1024 planes", topo, np.linspace(-1.0, 1.0, 1024).astype(np.float32))
    print(f"   the mesh: closed {topo.closed} manifold {topo.manifold}; improper {nest.n_improper} misoriented {nest.n_misoriented} max depth {nest.max_depth}", flush=True)
    del s, nest, topo
    hip.check(F.lib().fhip_ctx_trim(hip._h))
if "voxel" in cases:
    depth, N = 6, 256
    vox = F.voxelize(gyroid, depth, out=torch.empty((1 << depth) ** 3, dtype=torch.int64, device="cuda"))
    topo = vox.mesh().topology()
    s, nest = line("Voxels.mesh() at depth 6 under its 256 centre planes", topo, ((2 * np.arange(N) + 1 - N) / N).astype(np.float32))
    print(f"   improper {nest.n_improper} misoriented {nest.n_misoriented} max depth {nest.max_depth} regular {nest.n_regular} of {nest.n_loops}", flush=True)
    del s, nest, topo, vox
    hip.check(F.lib().fhip_ctx_trim(hip._h))
if "cube" in cases:
    v = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)], np.float32)
    t = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]], np.uint64)
    topo = F.mesh_topology((v, t), hip=hip)
    s, nest = line("a cube under 4096 planes", topo, np.linspace(-0.75, 0.75, 4096).astype(np.float32))
    assert nest.n_regular == nest.n_outer == nest.n_top == s.counts["loops"] and nest.max_depth == 0 and nest.n_improper == 0 and nest.n_misoriented == 0
    assert (nest.parent == nest.NONE).all() and (nest.depth == 0).all() and np.array_equal(nest.region_area2, s.loops["area2"])
print("== done")
