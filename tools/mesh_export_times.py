#!/usr/bin/env python3
"""GPU box: the times of profiles/mesh_export/README.md.  `build MODEL DEPTH`: fidget_amd.build_mesh with mesh_keep_device off and on;
`stl MODEL DEPTH`: Mesh.stl() to a device and to a host buffer beside tests/stl_ref.py on the host arrays; `grads MODEL DEPTH`:
Mesh.vertex_grads() to a device and to a host buffer beside Shape.eval_grad_slice on the same vertices.  Best and worst of REPS runs."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import fidget_amd as F
from stl_ref import stl_bytes

REPS = int(os.environ.get("REPS", "5"))


def timed(fn, sync=None, reps=REPS):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        if sync:
            sync()
        ts.append(time.perf_counter() - t0)
        del r
    return f"min {min(ts) * 1e3:.2f} ms, max {max(ts) * 1e3:.2f} ms of {reps}"


what, model, depth = sys.argv[1], sys.argv[2], int(sys.argv[3])
hip = F.HipContext(0, torch.cuda.current_stream().cuda_stream)
shape = F.Shape.from_vm(os.path.join(ROOT, "models", model), hip=hip)
F.build_mesh(shape, depth, keep_device=False)          # (the first build of a size pins its landing area and makes room)
if what == "build":
    for keep in (False, True, False, True):
        print(f"{model} depth {depth} build_mesh keep_device={int(keep)}: {timed(lambda: F.build_mesh(shape, depth, keep_device=keep))}", flush=True)
    sys.exit(0)
m = F.build_mesh(shape, depth, keep_device=True)
print(f"{model} depth {depth}: {len(m.triangles)} triangles, {len(m.vertices)} vertices", flush=True)
if what == "stl":
    n = 84 + 50 * len(m.triangles)
    dev = torch.empty(n, dtype=torch.uint8, device="cuda")
    m.stl(out=dev); hip.sync(); m.stl()
    print(f"  fhip_mesh_stl to a device buffer ({n} bytes): {timed(lambda: m.stl(out=dev), hip.sync)}", flush=True)
    print(f"  fhip_mesh_stl to a host buffer: {timed(lambda: m.stl())}", flush=True)
    print(f"  tests/stl_ref.py on the host arrays: {timed(lambda: stl_bytes(m.vertices, m.triangles), reps=2)}", flush=True)
else:
    v = m.vertices
    dev = torch.empty((len(v), 4), dtype=torch.float32, device="cuda")
    m.vertex_grads(shape, out=dev); hip.sync(); m.vertex_grads(shape)
    print(f"  fhip_mesh_vertex_grads to a device buffer: {timed(lambda: m.vertex_grads(shape, out=dev), hip.sync)}", flush=True)
    print(f"  fhip_mesh_vertex_grads to a host buffer: {timed(lambda: m.vertex_grads(shape))}", flush=True)
    print(f"  Shape.eval_grad_slice on the same vertices from the host: {timed(lambda: shape.eval_grad_slice(v[:, 0], v[:, 1], v[:, 2]), reps=2)}", flush=True)
