#!/usr/bin/env python3
"""GPU box: the times of profiles/directional/README.md.  `python tools/directional_times.py [DEPTH ...]` (default 6 7 8): gyroid-sphere.vm
voxelized at each depth into a torch CUDA tensor; then, every operand and result on the device, `Voxels.shadow` (a blocked flow) along
x, y and z in both senses, `overhangs` at reach2 = 1 and 16, `supports`, and `heights` along the three axes.  Each is called once to
warm up and then REPS times between two events on the context's stream; the line gives the mean.  The yardstick, in the same run: a
device-to-device copy that moves the bytes the call must move - per brick word 8 read for each input bitmap and 8 written for the
result, so 24 B for a blocked flow, 16 for overhangs, 40 for supports (the two calls it is made of), 8 and 12 B per column of voxels
for heights - that is, a copy of half as many bytes, which reads and writes each of them once.  Results are checked against each
other (supports lie under overhangs; the shadow towards -z against heights)."""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fidget_amd as F

REPS = 30
depths = [int(a) for a in sys.argv[1:]] or [6, 7, 8]
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
    out = torch.empty(words, dtype=torch.int64, device="cuda")
    over = torch.empty(words, dtype=torch.int64, device="cuda")
    hts = torch.empty((3, N, N), dtype=torch.int32, device="cuda")
    src, dst = torch.empty(20 * words, dtype=torch.uint8, device="cuda"), torch.empty(20 * words, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    print(f"== depth {depth}: gyroid-sphere, {vox.n} of {N ** 3} voxels set, {8 * words / 2 ** 20:.0f} MiB of bricks", flush=True)
    copies = {}

    def line(what, call, moved):
        """`moved`: the bytes the call must read and write"""
        if moved not in copies:
            copies[moved] = timed(lambda: dst[:moved // 2].copy_(src[:moved // 2]))
        ms, copy = timed(call), copies[moved]
        print(f"depth {depth} {what:24s} {ms:9.4f} ms   copy of the same {moved / 2 ** 20:7.1f} MiB {copy:9.4f} ms   ratio {ms / copy:5.2f}", flush=True)

    for d, name in enumerate(("-x", "+x", "-y", "+y", "-z", "+z")):
        line(f"shadow {name}", lambda: vox.shadow(d, out=out), 24 * words)
    line("swept +x (no blockers)", lambda: vox.swept(1, out=out), 16 * words)
    for reach2 in (1, 16):
        line(f"overhangs reach2 {reach2}", lambda: vox.overhangs(5, reach2, True, out=out), 16 * words)
    ov = vox.overhangs(5, 1, True, out=over)
    line("flow of the overhangs -z", lambda: ov.flow(4, blockers=vox, out=out), 24 * words)
    line("supports (both calls)", lambda: vox.supports(5, 1, True, out=out), 40 * words)
    for axis in range(3):
        line(f"heights {'xyz'[axis]}", lambda: vox.heights(axis, out=hts), 8 * words + 12 * N * N)
    # what was timed is what it should be
    sup = vox.supports(5, 1, True, out=out)
    assert ov.n > 0 and sup.n > 0
    hip.sync()
    assert not bool((sup.bricks & vox.bricks).any()) and all(int(vox.heights(axis, out=hts)[2].sum().item()) == vox.n for axis in range(3))
    h = vox.heights(2, out=hts)
    hip.sync()
    assert vox.shadow(4).n == int((h[1] + 1 - h[2])[h[2] > 0].sum().item())
    del vox, out, over, hts, src, dst, ov, sup, h
print("== done")
