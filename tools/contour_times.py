#!/usr/bin/env python3
"""GPU box: the times of profiles/contours/README.md.  `python tools/contour_times.py MODEL SIZE [once]`: fidget_amd.contour at SIZE x SIZE
(fhip_contour2d: blocking, so the host clock around the call is its time) beside, in the same process and alternating with it, the
pixel-perfect render2d of the same configuration into a torch CUDA tensor followed by the context's synchronise - the frame the contours
start from, alone - and the render2d that is not pixel-perfect, likewise.  Best and worst of REPS rounds after one untimed round; every
round's counts are compared with the first round's.
`once`: one untimed and one timed round of each and nothing else - the run to put under `rocprofv3 --kernel-trace --stats` for the
per-kernel times of k_ctr_edges, k_ctr_vertices, k_ctr_cells and k_ctr_segments (and k_scan_block / k_scan_add between them)."""
import os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fidget_amd as F

REPS = 1 if (len(sys.argv) > 3 and sys.argv[3] == "once") else int(os.environ.get("REPS", "5"))
model, n = sys.argv[1], int(sys.argv[2])
shape = F.Shape.from_vm(os.path.join(ROOT, "models", model))
hip = shape.hip
img = torch.empty((n, n), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def render(pixel_perfect):
    F.render2d(shape, n, pixel_perfect=pixel_perfect, out=img)
    hip.sync()


ref = F.contour(shape, n)
render(True)
render(False)
print(f"{model} {n} x {n}: {ref.n_vertices} vertices, {ref.n_segments} segments, {len(ref.loops())} loops; image {4 * n * n / 2 ** 20:.1f} MiB, "
      f"result {(12 * ref.n_vertices + 8 * ref.n_segments) / 2 ** 20:.2f} MiB", flush=True)
t = {"contour": [], "render2d pixel-perfect": [], "render2d": []}
for _ in range(REPS):
    c = []
    t["contour"].append(clock(lambda: c.append(F.contour(shape, n))))
    assert (c[0].n_vertices, c[0].n_segments) == (ref.n_vertices, ref.n_segments)
    t["render2d pixel-perfect"].append(clock(lambda: render(True)))
    t["render2d"].append(clock(lambda: render(False)))
for name, ts in t.items():
    print(f"  {name}: min {min(ts) * 1e3:.3f} ms, max {max(ts) * 1e3:.3f} ms of {REPS}", flush=True)
extra = min(t["contour"]) - min(t["render2d pixel-perfect"])
print(f"  contour - pixel-perfect frame: {extra * 1e3:+.3f} ms (best of each; the contour kernels' own times: the profiler run)", flush=True)
