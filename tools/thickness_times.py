#!/usr/bin/env python3
"""GPU box: the times of profiles/thickness/README.md.  `python tools/thickness_times.py [DEPTH] 2> passes.txt` (default 6): at that depth
gyroid-sphere.vm (thin walls: many small balls), a slab a quarter of the grid thick (nothing pruned but off its two medial planes), a
solid ball of half the radius and then, if the first predicts less than a minute for it, the solid ball of radius 0.78 - 100 voxels at
depth 6: few huge balls, the worst case for the scatter (the work grows about as the fifth power of the radius).  Each voxelized into a
torch CUDA tensor; `Voxels.distance(complement=True)` three times as the yardstick, then `DistanceField.thickness()` five times -
blocking, so the host clock around the call is its time - and once more with FHIP_MESH_TIMES set, which makes the library wait for the
stream after every pass and print the pass's wall time on stderr.  Every run checks `.n` against the bitmap's own count."""
import os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fidget_amd as F

depth = int(sys.argv[1]) if len(sys.argv) > 1 else 6
N = 4 << depth


def say(*a):
    sys.stderr.write(" ".join(str(x) for x in a) + "\n")        # (beside the library's own lines)
    sys.stderr.flush()
    print(*a, flush=True)


def ball(r):
    c = F.Context()
    x, y, z = c.x(), c.y(), c.z()
    return F.Shape(c, c.sub(c.sqrt(c.add(c.add(c.square(x), c.square(y)), c.square(z))), r))


def slab(half):
    c = F.Context()
    return F.Shape(c, c.sub(c.abs(c.z()), half))


def measure(name, shape, reps=5):
    tag = f"== depth {depth} {name}"
    out = torch.empty(8 ** depth, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    vox = F.voxelize(shape, depth, out=out)
    n = vox.n
    say(f"{tag}: inside voxels {n} of {N ** 3}")
    times = []
    for rep in range(3):
        t = time.perf_counter()
        dist = vox.distance(complement=True)
        times.append((time.perf_counter() - t) * 1e3)
    say(f"{tag}: distance(complement=True) ms {' '.join(f'{t:.2f}' for t in times)}; max_squared {dist.max_squared}")
    times = []
    for rep in range(reps + 1):
        if rep == reps:
            os.environ["FHIP_MESH_TIMES"] = "1"
        t = time.perf_counter()
        th = dist.thickness()
        dt = (time.perf_counter() - t) * 1e3
        os.environ.pop("FHIP_MESH_TIMES", None)
        assert th.n == n == th.centres
        if rep == 0:
            say(f"{tag}: thickness() first call {dt:.2f} ms; max_squared {th.max_squared} min_squared {th.min_squared} centres {th.centres} balls {th.balls}")
        elif rep < reps:
            times.append(dt)
        del th
    say(f"{tag}: thickness() ms {' '.join(f'{t:.2f}' for t in times)}; median {statistics.median(times):.2f}")
    return statistics.median(times)


measure("gyroid-sphere", F.Shape.from_vm(os.path.join(ROOT, "models", "gyroid-sphere.vm")))
measure("slab |z| < 0.25", slab(0.25))
half = measure("ball 0.39", ball(0.39))
if half * 32 < 60e3:
    measure("ball 0.78", ball(0.78), reps=3)
else:
    say(f"== depth {depth} ball 0.78: not run - {half:.0f} ms at half the radius predicts {half * 32 / 1e3:.0f} s")
say("== done")
