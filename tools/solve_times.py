#!/usr/bin/env python3
"""Batch times of the constraint solver (fhip_solve, solve.hip) against its host build on N threads (tests/host_build/solve_host.cpp),
the same instances on both: 65 536 instances of a 2-variable system (small_quadratic), 4 096 starts of one medium_linear system (10 free),
64 of a banded 50-variable system, medium_linear (1 000 draws) and big_linear (50) with the matrix as
fixed parameters, and the projection of 65 536 points onto prospero.vm.  fhip_solve is blocking (it ends with a stream
synchronise), so a call's wall time is the device time plus its copies.  Warm-up, then repeats: median, min and max.
usage: tools/solve_times.py [--repeats R] [--threads N] [--skip-host]   (one JSON line per case)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fidget_amd as F  # noqa: E402
import oracle as O  # noqa: E402
import solver_util as U  # noqa: E402


def timed(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    cases = []
    fs, keys, free = U.quadratic_system(F, 2)
    cases.append(("small_quadratic_65536", fs, U.quadratic_system(O, 2)[0], keys, free, U.quadratic_draws(rng, 2, 65536)[0]))
    mat, vals = U.rand_f32(rng, 10, 10), U.rand_f32(rng, 10)
    fs, keys, free, _ = U.linear_const(F, mat, U.mat_vec(mat, vals))
    cases.append(("medium_linear_4096", fs, U.linear_const(O, mat, U.mat_vec(mat, vals))[0], keys, free,
                  U.rand_f32(rng, 4096, 10)))
    fs, keys, free = U.banded_system(F, 50)
    cases.append(("banded_50_64", fs, U.banded_system(O, 50)[0], keys, free, U.rand_f32(rng, 64, 50)))
    # the reference's medium_linear and big_linear with the matrix as fixed parameters: 21 and 101 inputs per tape, one call per batch
    for n, count in ((10, 1000), (50, 50)):
        fs, keys, free = U.linear_system(F, n)
        cases.append((f"linear_{n}_params_{count}", fs, U.linear_system(O, n)[0], keys, free, U.linear_draws(rng, n, count)[0]))
    p = os.path.join(ROOT, "models", "prospero.vm")
    cases.append(("prospero_projection_65536", [F.Shape.from_vm(p)], [O.Shape.from_vm(p)], ["x", "y"], [True, True],
                  rng.uniform(-1, 1, (65536, 2)).astype(np.float32)))
    for name, fs, os_, keys, free, rows in cases:
        dev = F.solve_batch(fs, keys, free, rows)
        res = {"case": name, "instances": len(rows), "gpu": timed(lambda: F.solve_batch(fs, keys, free, rows), a.repeats),
               "iterations_mean": float(dev[2].mean()), "iterations_max": int(dev[2].max()),
               "exits": np.bincount(dev[3], minlength=7).tolist()}
        if not a.skip_host:
            host = U.host_solve(os_, keys, free, rows, threads=a.threads)
            res["host_equal"] = all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(dev, host))
            res["host_threads"] = a.threads
            res["host"] = timed(lambda: U.host_solve(os_, keys, free, rows, threads=a.threads), max(1, min(a.repeats, 3)), warmup=0)
            res["speedup"] = res["host"]["median_ms"] / res["gpu"]["median_ms"]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
