#!/usr/bin/env python3
"""GPU box: the times of profiles/voxel_mesh/README.md.  `python tools/voxel_mesh_times.py [DEPTH ...] 2> passes.txt` (default 6 7 8):
sphere 0.9 and gyroid-sphere.vm voxelized at each depth into a torch CUDA tensor; `Voxels.surface` and `Voxels.mesh` three times each -
blocking, so the host clock around the call is its time; the third with FHIP_MESH_TIMES set, which makes the library wait for the stream
after every pass and print the pass's wall time on stderr - and `Mesh.stl` into a torch buffer, followed by the context's synchronise.
Yardsticks on the same bitmap: `layer_counts`, which reads the bitmap once; a hipMemsetAsync of as many bytes as the mesh's two arrays
hold, the floor for writing them; and for gyroid-sphere `build_mesh` at depth + 2, the same resolution by the other route.  The mesh is
checked against the summary and the bitmap's own count."""
import ctypes, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fidget_amd as F

depths = [int(a) for a in sys.argv[1:]] or [6, 7, 8]
F.lib()
# the HIP runtime the library itself is linked to, by the path it was loaded from
hiprt = ctypes.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
hiprt.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
hiprt.hipMemsetAsync.restype = ctypes.c_int


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
        for what in ("surface", "mesh"):
            for rep in range(3):
                if rep == 2:
                    os.environ["FHIP_MESH_TIMES"] = "1"
                t = time.perf_counter()
                res = getattr(vox, what)()
                dt = time.perf_counter() - t
                os.environ.pop("FHIP_MESH_TIMES", None)
                shown = repr(res) if what == "surface" else f"{len(res.vertices)} vertices, {len(res.triangles)} triangles"
                say(f"{tag} rep {rep}: {what}() {dt * 1e3:.2f} ms; {shown}")
                if rep < 2:
                    del res
            if what == "surface":
                surf = res
        mesh = res
        assert surf.n == n and len(mesh.triangles) == 2 * surf.n_faces and len(mesh.vertices) == surf.vertices
        n_bytes = mesh.vertices.nbytes + mesh.triangles.nbytes
        n_stl = 84 + 50 * len(mesh.triangles)
        buf = torch.empty(max(n_bytes, n_stl), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for rep in range(4):
            t = time.perf_counter()
            assert hiprt.hipMemsetAsync(buf.data_ptr(), 0, n_bytes, None) == 0
            torch.cuda.synchronize()
            say(f"{tag}: hipMemsetAsync of the arrays' {n_bytes} bytes pass {rep}: {(time.perf_counter() - t) * 1e3:.3f} ms")
        for rep in range(3):
            t = time.perf_counter()
            mesh.stl(out=buf)
            hip.sync()
            say(f"{tag}: stl() of {n_stl} bytes into a torch buffer rep {rep}: {(time.perf_counter() - t) * 1e3:.3f} ms")
        del mesh, res, buf
        if name == "gyroid-sphere":
            for rep in range(2):
                t = time.perf_counter()
                dual = F.build_mesh(s, depth + 2)
                dt = time.perf_counter() - t
                say(f"{tag}: build_mesh at depth {depth + 2} rep {rep}: {dt * 1e3:.2f} ms; {len(dual.vertices)} vertices, {len(dual.triangles)} triangles")
                del dual
        del vox, out
say("== done")
