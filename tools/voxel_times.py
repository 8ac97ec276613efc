#!/usr/bin/env python3
"""GPU box: the times of profiles/voxels/README.md.  `python tools/voxel_times.py MODEL DEPTH [once]`: fidget_amd.voxelize into a torch
CUDA tensor (fhip_shape_voxels with a device `out`: blocking, so the host clock around the call is its time) beside, in the same process
and alternating with it, fidget_amd.occupancy at the same depth - the same level loop without the bitmap - and a bare hipMemset of the
bitmap's size followed by a device synchronise.  Then the layer images of 16 layers in the middle and the layer counts, from the bricks
where they are (asynchronous calls: timed to the context's synchronise).  Best and worst of REPS rounds after one untimed round; every
round's bitmap is compared with the first round's on the device.
`once`: one untimed and one timed round of each and nothing else - the run to put under `rocprofv3 --kernel-trace --stats` for the
per-kernel times of k_vox_full, k_vox_leaves and k_vox_slices."""
import ctypes, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fidget_amd as F

REPS = 1 if (len(sys.argv) > 3 and sys.argv[3] == "once") else int(os.environ.get("REPS", "5"))
model, depth = sys.argv[1], int(sys.argv[2])
shape = F.Shape.from_vm(os.path.join(ROOT, "models", model))
hip = shape.hip
words = 8 ** depth
N = 4 << depth
hiprt = ctypes.CDLL("libamdhip64.so")       # (the runtime already in the process)
hiprt.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
hiprt.hipMemset.restype = ctypes.c_int
hiprt.hipDeviceSynchronize.restype = ctypes.c_int

first = torch.empty(words, dtype=torch.int64, device="cuda")
out = torch.empty(words, dtype=torch.int64, device="cuda")
torch.cuda.synchronize()


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def memset():
    assert hiprt.hipMemset(ctypes.c_void_p(out.data_ptr()), 0, 8 * words) == 0
    assert hiprt.hipDeviceSynchronize() == 0


def slices(v, k0, k1, img):
    v.slices(k0, k1, out=img)
    hip.sync()


def counts(v):
    c = v.layer_counts()
    hip.sync()
    return c


ref = F.voxelize(shape, depth, out=first)
occ = F.occupancy(shape, depth)
memset()
print(f"{model} depth {depth}: grid {N}, bitmap {8 * words / 2 ** 20:.1f} MiB, cells {ref.cells}, inside {ref.n} (occupancy {occ.n})", flush=True)
assert ref.n == occ.n and ref.cells == occ.cells
k0 = N // 2 - min(8, N // 2)
k1 = min(N, k0 + 16)
img = torch.empty((k1 - k0, N, N), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
slices(ref, k0, k1, img)
counts(ref)
t = {"voxels": [], "occupancy": [], "memset": [], "slices": [], "layer_counts": []}
for _ in range(REPS):
    t["voxels"].append(clock(lambda: F.voxelize(shape, depth, out=out)))
    t["occupancy"].append(clock(lambda: F.occupancy(shape, depth)))
    t["memset"].append(clock(memset))
    v = F.voxelize(shape, depth, out=out)
    assert torch.equal(v.bricks, ref.bricks)
    t["slices"].append(clock(lambda: slices(v, k0, k1, img)))
    t["layer_counts"].append(clock(lambda: counts(v)))
for name, ts in t.items():
    print(f"  {name}: min {min(ts) * 1e3:.3f} ms, max {max(ts) * 1e3:.3f} ms of {REPS}", flush=True)
v, o, m = min(t["voxels"]), min(t["occupancy"]), min(t["memset"])
print(f"  expectation voxels <= occupancy + 2 x memset: {v * 1e3:.3f} <= {(o + 2 * m) * 1e3:.3f} ms: {'met' if v <= o + 2 * m else 'NOT met'}", flush=True)
print(f"  memset: {8 * words / m / 1e9:.1f} GB/s;  slices of {k1 - k0} layers: {(k1 - k0) * N * N / min(t['slices']) / 1e9:.1f} GB/s written (call time)", flush=True)
ones = int((ref.bricks == -1).sum())
print(f"  all-ones words: {ones} = {8 * ones / 2 ** 20:.1f} MiB (what k_vox_full stores, plus the leaf cells that came out full): over k_vox_full's kernel time, its bytes/s", flush=True)
