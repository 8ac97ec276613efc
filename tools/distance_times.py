#!/usr/bin/env python3
"""GPU box: the times of profiles/distance/README.md.  `python tools/distance_times.py [DEPTH ...] 2> passes.txt` (default 6 7 8): sphere 0.9
and gyroid-sphere.vm voxelized at each depth into a torch CUDA tensor; two yardsticks on that bitmap - `layer_counts`, which reads it
once, and `Components.label_slices(0, N)`, which writes N^3 32-bit values once, the floor for producing a field at all; then for the set
bits and for their complement `Voxels.distance` three times - blocking, so the host clock around the call is its time; the third with
FHIP_MESH_TIMES set, which makes the library wait for the stream after every pass and print the pass's wall time on stderr - and `within`
and `slices` of 64 layers, each followed by the context's synchronise.  The summary is checked against the bitmap's own count."""
import os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fidget_amd as F

depths = [int(a) for a in sys.argv[1:]] or [6, 7, 8]


def say(*a):
    sys.stderr.write(" ".join(str(x) for x in a) + "\n")        # (beside the library's own lines)
    sys.stderr.flush()
    print(*a, flush=True)


def sphere09():
    c = F.Context()
    x, y, z = c.x(), c.y(), c.z()
    return F.Shape(c, c.sub(c.sqrt(c.add(c.add(c.square(x), c.square(y)), c.square(z))), 0.9))


shapes = {"sphere0.9": sphere09(), "gyroid-sphere": F.Shape.from_vm(os.path.join(ROOT, "models", "gyroid-sphere.vm"))}
for depth in depths:
    N = 4 << depth
    for name, s in shapes.items():
        tag = f"== depth {depth} {name}"
        out = torch.empty(8 ** depth, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        vox = F.voxelize(s, depth, out=out)
        hip = vox._hip
        hip.sync()
        for rep in range(4):
            t = time.perf_counter()
            lc = vox.layer_counts()
            hip.sync()
            say(f"{tag}: layer_counts pass {rep}: {(time.perf_counter() - t) * 1e3:.3f} ms")
        n = int(lc.sum().item())
        say(f"{tag}: inside voxels {n} of {N ** 3}")
        comps = vox.components(6)
        labels = torch.empty((N, N, N), dtype=torch.int32, device="cuda")
        for rep in range(4):
            t = time.perf_counter()
            comps.label_slices(0, N, out=labels)
            hip.sync()
            say(f"{tag}: label_slices(0, N) pass {rep}: {(time.perf_counter() - t) * 1e3:.3f} ms")
        del comps, labels
        for complement in (False, True):
            ctag = f"{tag} complement {complement}"
            for rep in range(3):
                if rep == 2:
                    os.environ["FHIP_MESH_TIMES"] = "1"
                t = time.perf_counter()
                dist = vox.distance(complement)
                dt = time.perf_counter() - t
                os.environ.pop("FHIP_MESH_TIMES", None)
                say(f"{ctag} rep {rep}: distance() {dt * 1e3:.2f} ms; max_squared {dist.max_squared} argmax {dist.argmax} n {dist.n}")
                if rep < 2:
                    del dist
            assert dist.n == (N ** 3 - n if complement else n)
            for rep in range(2):
                t = time.perf_counter()
                near = dist.within(r=2)
                hip.sync()
                say(f"{ctag}: within(2) rep {rep}: {(time.perf_counter() - t) * 1e3:.3f} ms")
            assert near.n >= dist.n
            layers = torch.empty((min(64, N), N, N), dtype=torch.int32, device="cuda")
            for rep in range(2):
                t = time.perf_counter()
                dist.slices(N // 2 - min(32, N // 2), N // 2 + min(32, N // 2), out=layers)
                hip.sync()
                say(f"{ctag}: slices 64 layers rep {rep}: {(time.perf_counter() - t) * 1e3:.3f} ms")
            del dist, near, layers
        del vox, out
say("== done")
