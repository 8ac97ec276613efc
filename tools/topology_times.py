#!/usr/bin/env python3
"""GPU box: the times of profiles/mesh_topology/README.md.  `python tools/topology_times.py [DEPTH]` (default 8) checks
  - `build_mesh(gyroid-sphere, DEPTH)`, indexed, from the resident arrays: an MDC mesh, 7.1 M triangles at depth 8;
  - the boundary mesh of gyroid-sphere's bitmap at DEPTH (1024^3 voxels and 59 M triangles at depth 8), indexed from the resident
    arrays and as a soup - the same triangles as [T, 3, 3] floats in device memory, welded.
Each case: one call that is not counted, then REPS calls between two events on the context's stream - the call blocks, so this is the
whole call with its waits - and one call with FHIP_MESH_TIMES set: the time of every pass between events on the stream, on stderr.
The yardstick, in the same run: per pass a device-to-device copy of half the bytes the pass must read and write at the least (a copy
reads and writes each of its bytes once), with T triangles, C = 3 T corners, V vertices, E edges, Sv and Se slots:
  k_mt_check   24 T + 12 V indexed, 36 T for a soup        clear        8 Sv + 32 Se
  k_mt_weld    12 C keys + 4 C slots + 8 V of the table    vflag+scan   16 C           k_mt_vemit  12 C + 12 V
  k_mt_ids     13 C + V                                    k_mt_edges   16 C + 4 T + 32 E
  k_mt_link    13 C + 32 E                                 flatten+roots+scan 44 T     k_mt_number 16 T
  k_mt_table   31 T + 12 V
Then what the tables and the scratch take, what fhip_ctx_trim gives back, and for context the same questions asked of the host with
numpy (np.unique over the corners' bytes, a sort of the edge keys) on the smaller mesh."""
import os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fidget_amd as F

REPS = 5
depth = int(sys.argv[1]) if len(sys.argv) > 1 else 8
stream = torch.cuda.current_stream()
hip = F.HipContext(0, stream=stream.cuda_stream)          # the events below are recorded on the stream the library launches on
gyroid = F.Shape.from_vm(os.path.join(ROOT, "models", "gyroid-sphere.vm"), hip=hip)


def timed(call, reps=REPS):
    call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(reps):
        call()
    t1.record(stream)
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def copy_ms(moved):
    n = max(int(moved) // 2, 1)
    src, dst = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    return timed(lambda: dst.copy_(src), 10)


def line(what, mesh, soup):
    free0 = torch.cuda.mem_get_info()[0]
    ms = timed(lambda: F.mesh_topology(mesh, hip=hip))
    t = F.mesh_topology(mesh, hip=hip)
    c = t.counts
    T, V, E, Sv, Se = c["triangles"], c["vertices"], c["edges"], c["vertex_slots"], c["edge_slots"]
    C = 3 * T
    print(f"== {what}: {ms:9.3f} ms a call   T {T} V {V} E {E} shells {c['shells']} closed {t.closed} manifold {t.manifold} euler {t.euler} "
          f"nonmanifold {c['nonmanifold']} degenerate {c['degenerate']}   volume {t.volume:.9g} area {t.area:.9g}", flush=True)
    print(f"   tables: {Sv} vertex slots {8 * Sv / 2 ** 20:.0f} MiB, {Se} edge slots {32 * Se / 2 ** 20:.0f} MiB; load {V / Sv if Sv else 0:.3f} and {E / Se:.3f}; "
          f"the context's scratch and the handle took {(free0 - torch.cuda.mem_get_info()[0]) / 2 ** 20:.0f} MiB of device memory", flush=True)
    passes = {"k_mt_check": 36 * T if soup else 24 * T + 12 * V, "clear": 8 * Sv + 32 * Se, "k_mt_edges": 16 * C + 4 * T + 32 * E, "k_mt_link": 13 * C + 32 * E,
              "flatten + roots + scan": 44 * T, "k_mt_number": 16 * T, "k_mt_table": 31 * T + 12 * V}
    passes.update({"k_mt_weld": 16 * C + 8 * V, "k_mt_vflag + scan": 16 * C, "k_mt_vemit": 12 * C + 12 * V} if soup else {"k_mt_ids": 13 * C + V})
    for name, moved in passes.items():
        print(f"   copy of the bytes of {name:24s} {moved / 2 ** 20:9.1f} MiB {copy_ms(moved):9.4f} ms", flush=True)
    os.environ["FHIP_MESH_TIMES"] = "1"
    sys.stderr.write(f"-- {what}\n")
    sys.stderr.flush()
    t0 = time.perf_counter()
    F.mesh_topology(mesh, hip=hip)
    sys.stderr.write(f"the whole call on the host's clock: {time.perf_counter() - t0:.6f} s\n")
    sys.stderr.flush()
    del os.environ["FHIP_MESH_TIMES"]
    ms_e = timed(lambda: t.edges("nonmanifold", device=True))
    print(f"   edges('nonmanifold', device=True): {ms_e:9.3f} ms for {c['nonmanifold']} edges", flush=True)
    return t


def trim(what):
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    hip.check(F.lib().fhip_ctx_trim(hip._h))
    print(f"   fhip_ctx_trim after {what}: {(torch.cuda.mem_get_info()[0] - before) / 2 ** 20:.0f} MiB given back", flush=True)


def host_reference(vertices, triangles):
    """np.unique over the corners' 12 bytes and a sort of the edge keys, numpy as it comes"""
    t0 = time.perf_counter()
    corners = np.ascontiguousarray(vertices[triangles.reshape(-1).astype(np.int64)] + np.float32(0.0))
    _, inverse = np.unique(corners.view("V12").reshape(-1), return_inverse=True)
    t1 = time.perf_counter()
    tri = inverse.reshape(-1, 3).astype(np.uint64)
    a, b = tri.reshape(-1), np.roll(tri, -1, axis=1).reshape(-1)
    keys = np.sort((np.minimum(a, b) << np.uint64(32)) | np.maximum(a, b))
    n_edges = int(np.count_nonzero(np.diff(keys)) + 1)
    t2 = time.perf_counter()
    print(f"   on the host: np.unique over {len(corners)} corners {t1 - t0:.2f} s ({len(np.unique(inverse))} vertices), the edge keys sorted {t2 - t1:.2f} s ({n_edges} edges), "
          f"{torch.get_num_threads()} threads available", flush=True)


built = F.build_mesh(gyroid, depth)
t = line(f"build_mesh(gyroid-sphere, {depth}), indexed", built, False)
host_reference(built.vertices, built.triangles)
del built, t
trim("the MDC mesh")

words = (1 << depth) ** 3
vox = F.voxelize(gyroid, depth, out=torch.empty(words, dtype=torch.int64, device="cuda"))
m = vox.mesh()
surface = vox.surface()
t = line(f"boundary mesh of gyroid-sphere's {4 << depth}^3 bitmap, indexed", m, False)
assert t.closed and t.counts["boundary"] == 0 and t.euler == surface.euler          # what was timed is what it should be
del t
iface = dict(m.triangles_device().__cuda_array_interface__, typestr="<i8")
tri = torch.as_tensor(type("A", (), {"__cuda_array_interface__": iface})(), device="cuda")
soup = torch.as_tensor(m.vertices_device(), device="cuda")[tri.reshape(-1)].reshape(-1, 3, 3).contiguous()
del tri
t = line("the same as a soup, welded", soup, True)
assert t.closed and t.euler == surface.euler and t.counts["vertices"] == len(m.vertices)
del t, soup, m, vox
trim("the boundary mesh")
print("== done")
