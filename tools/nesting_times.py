#!/usr/bin/env python3
"""GPU box: the times of profiles/nesting/README.md.  `python tools/nesting_times.py [DEPTH ...]` (default 6 8): gyroid-sphere.vm
voxelized at each depth into a torch CUDA tensor; then `Voxels.outlines` over all layers and over the single layer N / 2, with
connectivity 4, and `Outlines.nesting` of each result.  Each is called once to warm up and then REPS times between two events on the
context's stream; the line gives the mean.  Both calls block - the nesting's host sends the loops' table up, waits once at the end and
allocates the result's arrays - so the times are the whole calls', not the kernels' alone.  Beside the nesting stands the `outlines`
call that made its input, timed the same way in the same run.  What was timed is checked: the outer boundaries' region sums against
twice the layers' set voxels, the parents' signs, the depths' parity."""
import os, sys
import numpy as np
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
        t = o.nesting()
        ms_outlines = timed(lambda: vox.outlines(k0, k1))
        ms = timed(lambda: o.nesting())
        print(f"depth {depth} nesting {what:12s} {o.n_vertices:9d} vertices {t.n_loops:8d} loops {t.n_outer:8d} outer {t.n_top:8d} top   max depth {t.max_depth:3d}   "
              f"{ms:9.4f} ms   its outlines {ms_outlines:9.4f} ms   ratio {ms / ms_outlines:6.3f}", flush=True)
        # what was timed is what it should be
        area2 = o.table()["area2"]
        counts = vox.layer_counts().cpu().numpy()
        for k in range(k0, k1):
            l0, l1 = int(o.loop_start[k - k0]), int(o.loop_start[k - k0 + 1])
            assert int(t.region_area2[l0:l1][area2[l0:l1] > 0].sum()) == 2 * int(counts[k])
        has = t.parent != t.NONE
        assert ((area2[has] < 0) != (area2[t.parent[has]] < 0)).all() and (t.parent[has] < np.nonzero(has)[0]).all()
        assert np.array_equal(t.depth % 2 == 0, area2 > 0) and np.array_equal(t.depth[has], t.depth[t.parent[has]] + 1)
        del o, t
    del vox
print("== done")
