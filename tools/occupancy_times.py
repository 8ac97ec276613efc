#!/usr/bin/env python3
"""GPU box: the times of profiles/occupancy/README.md.  `python tools/occupancy_times.py MODEL DEPTH [brute]`: fidget_amd.occupancy beside
fidget_amd.mesh_sample at the same depth - the nearest cost there was before: the same octree, with the mesher's leaf records - and, with
`brute`, the oracle's count over all N^3 voxel centres (tests/occupancy_ref.py; feasible to depth 7 or so).  Best and worst of REPS runs
after one untimed run; the integers of every run are compared with the first run's."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fidget_amd as F

REPS = int(os.environ.get("REPS", "5"))


def timed(fn, reps=REPS):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
        del r
    return f"min {min(ts) * 1e3:.2f} ms, max {max(ts) * 1e3:.2f} ms of {reps}"


model, depth = sys.argv[1], int(sys.argv[2])
shape = F.Shape.from_vm(os.path.join(ROOT, "models", model))
first = F.occupancy(shape, depth)
print(f"{model} depth {depth}: {first}", flush=True)
print(f"  volume {first.volume:.9f}, centroid {first.centroid}, bounds {first.bounds}", flush=True)


def again():
    o = F.occupancy(shape, depth)
    assert repr(o) == repr(first), (o, first)
    return o


print(f"  occupancy: {timed(again)}", flush=True)
F.mesh_sample(shape, depth)
print(f"  mesh_sample: {timed(lambda: F.mesh_sample(shape, depth)[1])}", flush=True)
if len(sys.argv) > 3 and sys.argv[3] == "brute":
    import oracle as O
    import occupancy_ref as R
    o = O.Shape.from_vm(os.path.join(ROOT, "models", model))
    t0 = time.perf_counter()
    want = R.sums(R.brute_force(o, depth))
    print(f"  the oracle over all {first.grid}^3 centres: {time.perf_counter() - t0:.2f} s, equal: {want == R.fields(first)}", flush=True)
