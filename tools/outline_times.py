#!/usr/bin/env python3
"""GPU box: the times of profiles/outlines/README.md.  `python tools/outline_times.py [DEPTH ...]` (default 6 8): gyroid-sphere.vm
voxelized at each depth into a torch CUDA tensor; then `Voxels.outlines` over all layers and over the single layer N / 2, with
connectivity 4.  Each is called once to warm up and then REPS times between two events on the context's stream; the line gives the mean.
The call blocks - the host waits for the layers' counts and for the number of loops, and allocates the result's arrays - so the time is
the whole call's, not the kernels' alone.  The yardstick, in the same run: a device-to-device copy that moves the bytes the call must
move - the bitmap's layers read, N^2 / 8 bytes each, and 12 bytes written per vertex (xy, next, loop_of) - that is, a copy of half as
many bytes, which reads and writes each of them once.  What was timed is checked: twice the layers' set voxels against area2, the
exposed faces along x and y against the perimeter."""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fidget_amd as F

REPS = 30
depths = [int(a) for a in sys.argv[1:]] or [6, 8]
stream = torch.cuda.current_stream()
hip = F.HipContext(0, stream=stream.cuda_stream)          # the events below are recorded on the stream the library launches on
shape = F.Shape.from_vm(os.path.join(ROOT, "models", "gyroid-sphere.vm"), hip=hip)


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


for depth in depths:
    B, N = 1 << depth, 4 << depth
    words = B ** 3
    vox = F.voxelize(shape, depth, out=torch.empty(words, dtype=torch.int64, device="cuda"))
    print(f"== depth {depth}: gyroid-sphere, {vox.n} of {N ** 3} voxels set, {8 * words / 2 ** 20:.0f} MiB of bricks", flush=True)
    for what, k0, k1 in (("all layers", 0, N), (f"layer {N // 2}", N // 2, N // 2 + 1)):
        o = vox.outlines(k0, k1)
        moved = (k1 - k0) * N * N // 8 + 12 * o.n_vertices
        half = max(moved // 2, 1)
        src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
        copy = timed(lambda: dst.copy_(src))
        ms = timed(lambda: vox.outlines(k0, k1))
        print(f"depth {depth} outlines {what:12s} {o.n_vertices:9d} vertices {o.n_loops:8d} loops {ms:9.4f} ms   copy of the same {moved / 2 ** 20:8.2f} MiB {copy:9.4f} ms   "
              f"ratio {ms / copy:7.2f}", flush=True)
        # what was timed is what it should be
        counts = vox.layer_counts()
        hip.sync()
        assert o.layer_area2.tolist() == [2 * int(c) for c in counts[k0:k1].tolist()]
        if k1 - k0 == N:
            assert int(o.layer_perimeter.sum()) == sum(vox.surface().faces[0:4])
        del o, src, dst
    del vox
print("== done")
