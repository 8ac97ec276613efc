"""bench.py's multi-rank protocol without GPUs: two processes on gloo run bench.main() with the device library replaced by
a stand-in that writes each rank's share of a known frame (shards by the owner map, blocks by their rectangle and z range, whole
frames) and with torch's CUDA entry points stubbed.  What is checked is the control flow the driver's N > 1 runs depend on and
that cannot be run on the one-GPU box: the three shardings are timed (`value` = one frame sharded over the ranks, by columns or blocks), combined through fidget_amd/dist.py (the torch.distributed
collectives here: FHIP_NO_DIRECT_RCCL), every combined image equals the frame, and rank 0 prints ONE JSON line with the
contract's fields."""
import json
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N = 256


def _frame():
    rng = np.random.default_rng(5)
    full = np.zeros((N, N, 4), np.int32)
    depth = rng.integers(0, N - 1, size=(N, N)).astype(np.int32)          # (below the saturation clamp)
    depth[rng.random((N, N)) < 0.3] = 0
    full[..., 3] = depth
    full[..., :3] = np.where(depth[..., None] > 0, rng.integers(1, 1 << 30, size=(N, N, 3)), 0).astype(np.int32)
    return full


def _worker(rank, world, port, out_path, direct, extra=("--full",)):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    if not direct:
        os.environ["FHIP_NO_DIRECT_RCCL"] = "1"
    import fidget_amd as F
    from fidget_amd import dist as D
    from test_multi_gpu import _parts_of, merge_ref
    full = _frame()

    if direct:
        # bench.py's path through a communicator of its own (probe, agreement, unique id broadcast, trial collectives,
        # use_direct_rccl), with the communicator itself played by the process group: RCCL needs the GPUs
        class FakeRccl:
            @staticmethod
            def probe(lib_path=None):
                pass

            def __init__(self, rank, world, bcast_bytes=None, lib_path=None):
                raw = bytes(range(128)) if rank == 0 else bytes(128)
                assert bcast_bytes(raw, 0) == bytes(range(128))             # the unique id reaches every rank
                self.rank, self.world = rank, world

            def reduce_sum(self, t, dst, stream):
                assert stream == 0
                dist.reduce(t, dst=dst, op=dist.ReduceOp.SUM)

            def gather(self, send, recv, dst, stream):
                assert stream == 0 and (recv is not None) == (self.rank == dst)
                dist.gather(send, [recv[r] for r in range(self.world)] if recv is not None else None, dst=dst)

            def close(self):
                pass

        D.DirectRccl = FakeRccl

    # ---- torch: CUDA entry points and device placement stubbed -----------------------------------------------------
    class Stream:
        cuda_stream = 0

    class Event:
        def __init__(self, enable_timing=False):
            self.t = 0.0

        def record(self, stream=None):
            import time
            self.t = time.perf_counter()

        def elapsed_time(self, other):
            return (other.t - self.t) * 1e3

    torch.cuda.set_device = lambda d: None
    torch.cuda.synchronize = lambda d=None: None
    torch.cuda.current_stream = lambda d=None: Stream()
    torch.cuda.Event = Event
    for name in ("zeros", "tensor", "full", "arange", "empty"):
        real = getattr(torch, name)
        setattr(torch, name, (lambda real: lambda *a, **k: real(*a, **{kk: vv for kk, vv in k.items() if kk != "device"}))(real))
    real_init = dist.init_process_group
    dist.init_process_group = lambda backend, rank, world_size, device_id=None: real_init("gloo", rank=rank, world_size=world_size)

    # ---- the device library's stand-in --------------------------------------------------------------------------------
    class Hip:
        tile_phases = None

        def __init__(self, device, stream):
            pass

        def sync(self): pass
        def counters(self): return {"arena_ops": 0, "arena_overflow": 0}
        def profile(self, on): pass
        def profile_read(self): return {k: (0.0, 0) for k in ("tiles", "points", "normals", "other")}
        def profile_read_kernels(self): return {}
        def wave_stats(self): pass
        def leaf_stats(self): return {"leaves": 0, "tape_ops": 0, "tape_words_read": 0, "lane_ops": 0}
        def option(self, name): return 0
        def lane_tune(self): return {"phase": -1, "stage_pipeline_ms": [0.0, 0.0], "frame_lanes_ms": 0.0, "kept": "stage pipeline"}
        def lane_frames(self): return 0
        def set_option(self, name, value=1): pass

        def options(self, **kw):
            import contextlib
            return contextlib.nullcontext(self)

    class Shape:
        @staticmethod
        def from_vm(path, hip=None):
            assert os.path.exists(path)
            return Shape()

    renders = [0]

    def render3d(shape, n, out=None, shard=0, n_shards=1, block=None, **kw):
        assert n == N and out is not None
        renders[0] += 1
        if block is not None:
            part = _parts_of(full, block[1], N, block[0], np.random.default_rng(block[0]))
        elif n_shards > 1:
            own = D.owner_map(N, N, D.root_tile(N), n_shards)
            part = np.where((own == shard)[..., None], full, 0).astype(np.int32)
        else:
            part = full
        out.copy_(torch.from_numpy(part))
        return out, None, None

    F.HipContext, F.Shape, F.render3d = Hip, Shape, render3d
    F.merge_depth = lambda a, b, d, hip=None: merge_ref(a, b, d)

    import bench
    sys.argv = ["bench.py", "--gpus", str(world), "--steps", "3", "--warmup", "1", "--size", str(N)] + list(extra)
    if rank == 0:
        sys.stdout = open(out_path, "w")
    bench.main()
    sys.stdout.flush()
    with open(f"{out_path}.renders{rank}", "w") as f:
        f.write(str(renders[0]))


@pytest.mark.parametrize("direct,world", [(False, 2), (True, 2), (True, 4), (True, 8)])     # 8: the node the scaling run uses (octants 2 x 2 x 2)
def test_bench_two_ranks_protocol(tmp_path, direct, world):
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out_path = str(tmp_path / "rank0.out")
    mp.spawn(_worker, args=(world, port, out_path, direct), nprocs=world, join=True)
    lines = [l for l in open(out_path).read().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    assert len(lines[0]) < 6000, len(lines[0])          # the driver's record keeps a short line whole (round 4's 20.6 KB line came back unparsed)
    r = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in r, key
    assert r["n_gpus"] == world and r["steps"] == 3 and r["warmup"] == 1 and r["unit"] == "Mvoxel/s" and r["higher_is_better"] is True
    assert r["vs_baseline"] is None and r["data"] == "synthetic" and "workload" in r["config"] and "sharding" in r["config"]
    p = r["partitions"]
    assert p["images_equal"] is True and p["frames"]["images_equal"] is True and p["frames"]["frames_per_step"] == world
    for k in ("columns", "blocks", "frames"):
        assert p[k]["ms_per_step"] > 0 and p[k]["value"] > 0
    # `value` is ONE frame sharded over the ranks (the north star's number: total work fixed), by the better of the two
    # partitions of a frame; the frame-sequence sharding (weak scaling) is listed, never the headline
    best = max(p[k]["value"] for k in ("columns", "blocks"))
    assert abs(r["value"] - best) <= 1e-6 * best
    assert r["scaling"] == "strong" and p["frames"]["scaling"] == "weak" and p["columns"]["scaling"] == p["blocks"]["scaling"] == "strong"
    assert "frames" not in r["config"]["sharding"].split(",")[0]
    assert p["columns"]["frame_latency_ms"] > 0 and p["blocks"]["frame_latency_ms"] > 0
    assert ("DirectRccl" in r["collectives"]) if direct else ("torch.distributed" in r["collectives"])
    assert "roofline" not in r and "cpu_baseline" not in r         # rank 0 at N = 1 only
    # every rank's stage times of its share of a frame, gathered to rank 0
    # round 6: what shards - the general path and a z-reading model by blocks - next to `value`, and the model the step can be read against
    for k in ("blocks_general_path", "blocks_colonnade"):
        assert p[k]["ms_per_step"] > 0 and p[k]["value"] > 0 and p[k]["scaling"] == "strong"
    pr = r["predicted"]
    assert {"critical_rank", "render_ms", "coarse_chain_ms", "gather_ms", "merge_ms", "frame_alone_ms", "measured_frame_alone_ms", "measured_ms_per_step"} <= set(pr)
    assert 0 <= pr["critical_rank"] < world and pr["gather_ms"] > 0 and abs(pr["frame_alone_ms"] - (pr["render_ms"] + pr["gather_ms"] + pr["merge_ms"])) < 1e-3    # (the line's figures are rounded to 5 digits)
    assert [q["rank"] for q in r["per_rank"]] == list(range(world))
    assert all({"coarse_chain_ms", "slab_ms", "tile_stage_ms", "leaf_ms", "normals_ms"} <= set(q) for q in r["per_rank"])
    if world == 8:
        assert p["blocks"]["split"] == [2, 2, 2]


def _spawn_bench(tmp_path, world, extra):
    """bench.main() on `world` stand-in ranks (torch.distributed collectives) -> (rank 0's one line, every rank's count of frames rendered)"""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out_path = str(tmp_path / "rank0.out")
    mp.spawn(_worker, args=(world, port, out_path, False, tuple(extra)), nprocs=world, join=True)
    lines = [l for l in open(out_path).read().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), [int(open(f"{out_path}.renders{r}").read()) for r in range(world)]


def _assert_dump_is_the_frame(d):
    full = _frame()
    normal, depth = np.load(d / "normal.npy"), np.load(d / "depth.npy")
    assert normal.dtype == np.float32 and normal.shape == (N, N, 3) and depth.dtype == np.float32 and depth.shape == (N, N)
    assert (normal.view(np.int32) == full[..., :3]).all() and (depth == full[..., 3].astype(np.float32)).all()
    assert not (d / "pixel_index.npy").exists()


@pytest.mark.parametrize("world", [1, 2])
def test_a_plain_run_times_the_headline_and_nothing_else(tmp_path, world):
    """Without --full, bench.py renders the warm-up frames and the timed steps (at N > 1: for each of the two shardings `value` chooses
    from, with the fixed count of untimed frames every rank takes) and nothing more; its line holds the contract's fields, not the legs
    that --full adds; --dump-outputs writes the last timed frame as float32 arrays."""
    d = tmp_path / "outputs"
    r, renders = _spawn_bench(tmp_path, world, ["--dump-outputs", str(d)])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in r, key
    assert r["n_gpus"] == world and r["steps"] == 3 and r["warmup"] == 1 and r["unit"] == "Mvoxel/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
    assert abs(r["value"] - N ** 3 / (r["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * r["value"]
    for key in ("frame_latency_ms", "host_output_frame_ms", "device_bytes", "roofline", "roofline_timed_path", "cpu_baseline", "parity", "c3_bear",
                "c5_mesh", "c2_2d", "c4z_colonnade", "multi_gpu_predicted", "predicted", "per_rank", "details"):
        assert key not in r, key
    assert r["config"]["general_path"] is None
    if world == 1:
        assert renders == [1 + 3]
    else:
        assert set(r["partitions"]) == {"columns", "blocks"}
        assert abs(r["value"] - max(r["partitions"][k]["value"] for k in ("columns", "blocks"))) <= 1e-6 * r["value"]
        assert renders == [2 * (1 + 60 + 3)] * world
    _assert_dump_is_the_frame(d)


def test_full_run_dumps_the_timed_path_s_last_frame(tmp_path):
    """--full renders into the output again after the timed steps (general path, profiled frames, ...); what --dump-outputs writes is still
    the frame of the last timed step."""
    d = tmp_path / "outputs"
    r, _ = _spawn_bench(tmp_path, 2, ["--full", "--dump-outputs", str(d)])
    assert "predicted" in r and "frames" in r["partitions"]
    _assert_dump_is_the_frame(d)


def test_a_large_frame_is_dumped_as_a_fixed_sample(tmp_path, monkeypatch):
    import torch
    bench = _bench_module()
    full = _frame()
    monkeypatch.setattr(bench, "DUMP_BYTES", 24 * 1000)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(torch.from_numpy(full), str(a))
    bench.dump_outputs(torch.from_numpy(full.copy()), str(b))
    idx = np.load(a / "pixel_index.npy")
    assert idx.dtype == np.float64 and idx.shape == (1000,) and (np.diff(idx) > 0).all() and idx[-1] < N * N
    for name in ("pixel_index", "normal", "depth"):
        assert np.load(a / f"{name}.npy").tobytes() == np.load(b / f"{name}.npy").tobytes(), name       # the same pixels every run
    flat = full.reshape(N * N, 4)[idx.astype(np.int64)]
    assert (np.load(a / "normal.npy").view(np.int32) == flat[:, :3]).all() and (np.load(a / "depth.npy") == flat[:, 3]).all()
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= 24 * 1000 + 3 * 256
    monkeypatch.setattr(bench, "DUMP_BYTES", 60_000_000)
    bench.dump_outputs(torch.from_numpy(full), str(a))        # (a whole frame into the same folder: no index left from the sample)
    _assert_dump_is_the_frame(a)


def test_c5_mesh_leg_reads_the_mesh_tools_output():
    """bench.py's `c5_mesh` comes from tools/mesh_times.py run as a process of its own; what it prints is parsed by
    bench.parse_mesh_times - here on the committed output of that very command on an MI355X (profiles/r03z/mesh_times.log)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    log = open(os.path.join(root, "profiles", "r03z", "mesh_times.log")).read()
    c5 = bench.parse_mesh_times(log, log)
    assert c5["triangles"] == 15050590 and c5["vertices"] == 7521871
    assert 1.0 < c5["s_per_build_inside_the_library"] < c5["s_per_build"] < c5["s_first_build"] < 2.0
    import fidget_amd
    assert bench.MESH_LEAF_BYTES == fidget_amd.MESH_LEAF.itemsize
    assert bench.parse_mesh_times("Traceback (most recent call last): ...", "") is None
    assert bench.parse_mesh_times("10 build 0 1.5\n", "") is None          # (one build only: nothing after the first)


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_the_single_gpu_line_is_short_and_has_the_contract_keys():
    """bench.py's N = 1 line is cut down by compact_line from everything the run measured: here on the full record of an MI355X run
    (profiles/r04z/bench.json, the 20.6 KB line the driver could not parse) - under 6 000 bytes, one object per fact, the contract's
    keys, `roofline` and `cpu_baseline` with their fields."""
    bench = _bench_module()
    full = json.loads(open(os.path.join(ROOT, "profiles", "r04z", "bench.json")).read().strip().splitlines()[-1])
    assert len(json.dumps(full)) > 15000
    full["device_bytes"] = 1 << 30
    full["c5_mesh"].update(parity={"triangles_equal": True, "vertices_equal": True}, cpu_s_per_build=10.0, cpu_threads=128)
    # round 6: the tuner's untimed frames, BASELINE configuration 2 and a z-reading model at the headline size, one compact object each
    full["tuning_frames"] = 52
    roof = {"bound": "hbm", "achieved": 250.0, "peak": 8000.0, "unit": "GB/s", "frac": 0.03125, "what": "x" * 200}
    full["c2_2d"] = {"workload": "prospero.vm 2D 4096^2", "ms_per_frame": 0.25, "image_equal": True, "roofline": dict(roof)}
    full["c4z_colonnade"] = {"workload": "colonnade.vm 3D heightmap+normals 1024^3", "ms_per_frame": 0.45, "depth_equal": True, "normals_equal": True, "roofline": dict(roof)}
    line = bench.compact_line(full)
    text = json.dumps(line, separators=(",", ":"))
    assert len(text) < 6000, len(text)
    assert set(line) == {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "ms_per_step_median", "higher_is_better", "scaling",
                         "vs_baseline", "dtype", "data", "tuning_frames", "frame_latency_ms", "host_output_frame_ms", "device_bytes", "config", "roofline",
                         "roofline_timed_path", "cpu_baseline", "parity", "c3_bear", "c5_mesh", "c2_2d", "c4z_colonnade"}
    for k in ("c2_2d", "c4z_colonnade"):
        assert set(line[k]["roofline"]) == {"bound", "achieved", "peak", "unit", "frac"} and line[k]["ms_per_frame"] > 0
    assert set(line["config"]) == {"workload", "sharding", "column_invariance", "general_path"}
    assert set(line["config"]["general_path"]) == {"ms_per_step", "value", "frame_latency_ms"}
    for k in ("roofline", "roofline_timed_path"):
        r = line[k]
        assert {"bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "path", "avg_launch_ms", "alu", "issue", "path_frame"} <= set(r)
        assert r["bound"] == "hbm" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 * r["frac"]
        assert all(isinstance(v, (int, float, str, type(None))) for kk, v in r.items() if kk not in ("alu", "issue", "path_frame"))
    assert line["roofline"]["kernel"] == "fh_columns" and line["roofline"]["path"] == "general"
    assert line["roofline_timed_path"]["path"] == "default"
    assert set(line["cpu_baseline"]) == {"value", "unit", "cores", "kind", "sample"} and line["cpu_baseline"]["kind"] == "port"
    assert line["c5_mesh"]["parity"] == {"triangles_equal": True, "vertices_equal": True} and line["c5_mesh"]["cpu_s_per_build"] == 10.0
    # nothing in the line is said twice, and no value is a paragraph
    def strings(x):
        if isinstance(x, dict):
            for v in x.values():
                yield from strings(v)
        elif isinstance(x, str):
            yield x
    assert max(len(t) for t in strings(line)) < 400


def test_a_line_that_would_outgrow_the_limit_sheds_optional_objects_first():
    bench = _bench_module()
    full = json.loads(open(os.path.join(ROOT, "profiles", "r04z", "bench.json")).read().strip().splitlines()[-1])
    full["per_rank"] = [{"rank": r, "note": "x" * 600} for r in range(8)]
    full["partitions"] = {"columns": {"ms_per_step": 1.0, "value": 1.0, "frame_latency_ms": 1.0, "scaling": "strong"}}
    line = bench.compact_line(full)
    assert len(json.dumps(line, separators=(",", ":"))) < 6000
    assert "per_rank" not in line and "roofline" in line and "cpu_baseline" in line and "config" in line
