#!/usr/bin/env python3
"""GPU box: the times of profiles/components/README.md.  `python tools/components_times.py [DEPTH] 2> passes.txt`: sphere 0.9 and
gyroid-sphere.vm voxelized at DEPTH (default 8: 1024^3) into a torch CUDA tensor, then for connectivity 6 and 26, foreground and
complement: `Voxels.components` three times - blocking, so the host clock around the call is its time; the third with FHIP_MESH_TIMES set,
which makes the library wait for the stream after every pass and print the pass's wall time on stderr - `label_slices` of 64 layers and
`extract` of the largest component, each followed by the context's synchronise; and four `layer_counts` passes over the same bitmap, the
cost of merely reading it.  The counts are checked against the bitmap's own (sizes sum to the foreground, the extracted part's voxels)."""
import os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fidget_amd as F

depth = int(sys.argv[1]) if len(sys.argv) > 1 else 8
N = 4 << depth


def say(*a):
    sys.stderr.write(" ".join(str(x) for x in a) + "\n")        # (beside the library's own lines)
    sys.stderr.flush()
    print(*a, flush=True)


def sphere09():
    c = F.Context()
    x, y, z = c.x(), c.y(), c.z()
    return F.Shape(c, c.sub(c.sqrt(c.add(c.add(c.square(x), c.square(y)), c.square(z))), 0.9))


shapes = {"sphere0.9": sphere09(), "gyroid-sphere": F.Shape.from_vm(os.path.join(ROOT, "models", "gyroid-sphere.vm"))}
for name, s in shapes.items():
    out = torch.empty(8 ** depth, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t = time.perf_counter()
    vox = F.voxelize(s, depth, out=out)
    hip = vox._hip
    hip.sync()
    say(f"== {name}: voxelize depth {depth} {time.perf_counter() - t:.3f} s cells {vox.cells}")
    for rep in range(4):
        t = time.perf_counter()
        lc = vox.layer_counts()
        hip.sync()
        say(f"== {name}: layer_counts pass {rep}: {(time.perf_counter() - t) * 1e3:.3f} ms")
    n = int(lc.sum().item())
    say(f"== {name}: inside voxels {n} of {N ** 3}")
    for conn in (6, 26):
        for complement in (False, True):
            tag = f"== {name} conn {conn} complement {complement}"
            for rep in range(3):
                if rep == 2:
                    os.environ["FHIP_MESH_TIMES"] = "1"
                say(f"{tag} rep {rep}")
                t = time.perf_counter()
                comps = vox.components(conn, complement)
                dt = time.perf_counter() - t
                os.environ.pop("FHIP_MESH_TIMES", None)
                say(f"{tag} rep {rep}: components() {dt * 1e3:.2f} ms; count {comps.count} nodes {comps.nodes} n {comps.n} sizes {comps.sizes[:4].tolist()} "
                    f"border {comps.border[:4].tolist()} largest {comps.largest()}")
            assert comps.n == (N ** 3 - n if complement else n) and int(comps.sizes.sum()) == comps.n
            for rep in range(2):
                t = time.perf_counter()
                lab = comps.label_slices(N // 2 - 32, N // 2 + 32)
                hip.sync()
                say(f"{tag}: label_slices 64 layers rep {rep}: {(time.perf_counter() - t) * 1e3:.2f} ms")
            for rep in range(2):
                t = time.perf_counter()
                part = comps.extract([comps.largest()])
                hip.sync()
                say(f"{tag}: extract largest rep {rep}: {(time.perf_counter() - t) * 1e3:.2f} ms")
            pn = int(part.layer_counts().sum().item())
            assert pn == int(comps.sizes[comps.largest()]), (pn, comps.sizes[comps.largest()])
            del comps, lab, part
say("== done")
