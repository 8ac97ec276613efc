"""The distance transform without a GPU: the reference of distance_ref.py against the literal definition, against scipy where there is
one and on grids whose answers are known; the line arithmetic of fidget_amd/csrc/mesh_edt.hpp built for the host
(tests/host_build/mesh_edt_host.cpp) - the row pass on bit masks, the envelope pass on a column - against the reference's line; that
program under ASan and UBSan; the entry points as the header states them."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import fidget_amd as F
import distance_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "mesh_edt_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")
ENTRY_POINTS = ("fhip_voxels_distance", "fhip_distance_info", "fhip_distance_slices", "fhip_distance_dev", "fhip_distance_threshold",
                "fhip_distance_free")
NONE = DR.NONE
TOP = 2 * 1023 ** 2          # the largest value the pass along k reads at N = 1024


# ---- the reference against the definition --------------------------------------------------------------------------------------------------
def literal(fg):
    """the definition, six loops deep"""
    N = fg.shape[0]
    out = np.full(fg.shape, NONE, np.uint32)
    for i in range(N):
        for j in range(N):
            for k in range(N):
                best = None
                for a in range(N):
                    for b in range(N):
                        for c in range(N):
                            if fg[a, b, c]:
                                d = (i - a) ** 2 + (j - b) ** 2 + (k - c) ** 2
                                best = d if best is None or d < best else best
                if best is not None:
                    out[i, j, k] = best
    return out


def test_the_reference_is_the_definition():
    rng = np.random.default_rng(11)
    for N, density in ((4, 0.05), (4, 0.5), (8, 0.01), (8, 0.1)):
        fg = rng.random((N, N, N)) < density
        want = literal(fg)
        assert np.array_equal(DR.edt(fg), want) and np.array_equal(DR.direct(fg), want)
    for N, density in ((16, 0.002), (32, 0.0003)):
        fg = rng.random((N, N, N)) < density
        assert fg.any() and np.array_equal(DR.edt(fg), DR.direct(fg))


def test_scipy_computes_the_same():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(12)
    for N, density in ((8, 0.1), (16, 0.02), (32, 0.3), (64, 0.001), (64, 0.6)):
        fg = rng.random((N, N, N)) < density
        want = np.rint(ndimage.distance_transform_edt(~fg) ** 2).astype(np.uint32)
        assert np.array_equal(DR.edt(fg), want)


def test_known_answers():
    N = 16
    one = np.zeros((N, N, N), bool)
    one[3, 9, 14] = True
    i, j, k = np.indices(one.shape)
    quadratic = (i - 3) ** 2 + (j - 9) ** 2 + (k - 14) ** 2
    assert np.array_equal(DR.edt(one), quadratic)
    assert DR.summary(DR.edt(one)) == (int(quadratic.max()), (15, 0, 0), 1)
    empty, full = DR.edt(np.zeros((N, N, N), bool)), DR.edt(np.ones((N, N, N), bool))
    assert empty.dtype == np.uint32 and (empty == 0xFFFFFFFF).all() and (empty.view(np.int32) == -1).all() and (full == 0).all()
    assert DR.summary(empty) == (0, None, 0) and DR.summary(full) == (0, (0, 0, 0), N ** 3)
    assert not DR.within(empty, 0xFFFFFFFE).any() and DR.beyond(empty, 0xFFFFFFFE).all()
    assert np.array_equal(DR.within(DR.edt(one), 0), one) and int(DR.within(DR.edt(one), 1).sum()) == 7
    # the layers' layout: [k, j, i]
    assert DR.field(DR.edt(one))[14, 9, 3] == 0 and DR.field(DR.edt(one))[13, 9, 3] == 1


# ---- the library's line arithmetic, built for the host -------------------------------------------------------------------------------------
def _build(name, flags):
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    deps = [SRC, os.path.join(CSRC, "mesh_edt.hpp"), os.path.join(CSRC, "mesh_vox.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe])      # (plain g++: the header touches no device)
    return exe


def run(exe, queries):
    res = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stdout[-300:], res.stderr[-2000:])
    lines = res.stdout.splitlines()
    assert len(lines) == len(queries)
    return [np.array(line.split(), np.uint64).astype(np.uint32) for line in lines]


@functools.lru_cache(maxsize=None)
def sample_lines():
    """columns of squared distances: all "none", one finite entry at either end, alternating, and random ones of the lengths 4, 8, 64,
    65 and 1024 with values up to 2 * 1023^2 at several shares of "none" """
    rng = np.random.default_rng(2024)
    lines = []
    for n in (4, 8, 64, 65, 1024):
        lines.append(np.full(n, NONE, np.uint32))
        for at in (0, n - 1):
            for v in (0, 1, TOP):
                f = np.full(n, NONE, np.uint32)
                f[at] = v
                lines.append(f)
        for a, b in ((0, NONE), (NONE, 0), (TOP, NONE), (0, TOP), (TOP, 0)):
            f = np.empty(n, np.uint32)
            f[0::2], f[1::2] = a, b
            lines.append(f)
        lines.append(np.zeros(n, np.uint32))
        lines.append(np.full(n, TOP, np.uint32))
        lines.append((np.arange(n, dtype=np.uint32) ** 2))                       # one parabola: every later entry touches it from above
        lines.append(((n - 1 - np.arange(n, dtype=np.uint32)) ** 2))
        for top in (1, 40, n * n, TOP):
            for none_share in (0.0, 0.5, 0.95):
                for _ in range(6 if n < 1024 else 2):
                    f = rng.integers(0, top + 1, n).astype(np.uint32)
                    f[rng.random(n) < none_share] = NONE
                    lines.append(f)
    return lines


def mask_words(row):
    """bool [n] -> hexadecimal words, bit b of word w = row[64 w + b]"""
    bits = np.zeros((len(row) + 63) // 64 * 64, np.uint8)
    bits[:len(row)] = row
    return [f"{int.from_bytes(np.packbits(bits[w:w + 64], bitorder='little').tobytes(), 'little'):x}" for w in range(0, len(bits), 64)]


@functools.lru_cache(maxsize=None)
def sample_rows():
    rng = np.random.default_rng(2025)
    rows = []
    for n in (4, 8, 64, 65, 128, 1024):
        rows += [np.zeros(n, bool), np.ones(n, bool), np.arange(n) % 2 == 0, np.arange(n) % 2 == 1]
        for at in (0, n - 1, n // 2, min(63, n - 1), min(64, n - 1)):
            r = np.zeros(n, bool)
            r[at] = True
            rows.append(r)
        for density in (0.5, 0.1, 0.01, 0.002):
            rows += [rng.random(n) < density for _ in range(6)]
    return rows


def column_queries(lines):
    return [f"C {len(f)} " + " ".join(str(int(v)) for v in f) for f in lines]


def row_queries(rows):
    return [f"R {len(r)} " + " ".join(mask_words(r)) for r in rows]


def test_the_envelope_pass_is_the_references_line():
    lines = sample_lines()
    got = run(_build("mesh_edt_host", ["-O1"]), column_queries(lines))
    for f, g in zip(lines, got):
        want = DR.line(f)
        assert np.array_equal(g, want), (len(f), f[:16], g[:16], want[:16])
    assert sum(int((f == NONE).all()) for f in lines) >= 5 and max(len(f) for f in lines) == 1024


def test_the_row_pass_is_the_references_line():
    rows = sample_rows()
    got = run(_build("mesh_edt_host", ["-O1"]), row_queries(rows))
    for r, g in zip(rows, got):
        want = DR.line(np.where(r, 0, NONE).astype(np.uint32))
        assert np.array_equal(g, want), (len(r), mask_words(r), g[:16], want[:16])


def test_the_arithmetic_runs_clean_under_sanitizers():
    """the same program as a stand-alone executable with ASan and UBSan, on the same input: exit 0, nothing on stderr (`run` asserts
    both), the same answers"""
    queries = column_queries(sample_lines()) + row_queries(sample_rows())
    plain = run(_build("mesh_edt_host", ["-O1"]), queries)
    san = run(_build("mesh_edt_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), queries)
    assert len(plain) == len(san) and all(np.array_equal(a, b) for a, b in zip(plain, san))


# ---- the interface -----------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fidget_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    lib = C.CDLL(F.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in F.EXPORTS and getattr(F.lib(), name).argtypes is not None, name
    assert re.search(r"fhip_voxels_distance\s*\([^;]*void\s*\*\*\s*out\s*\)", hdr)          # the handle is a void*
    assert all(callable(getattr(F.Voxels, m)) for m in ("distance", "offset", "opened", "closed"))
    assert all(callable(getattr(F.DistanceField, m)) for m in ("slices", "within", "beyond")) and isinstance(F.DistanceField.squared_device, property)
    ffi = open(os.path.join(ROOT, "rust", "fidget-hip", "src", "ffi.rs")).read()
    assert all(f"pub fn {name}(" in ffi for name in ENTRY_POINTS)
    mesh_only = open(os.path.join(ROOT, "tools", "src_hash.py")).read()
    assert all(f'"{name}"' in mesh_only for name in ("mesh_edt.hpp", "edt.hip", "capi_edt.hpp"))          # mesh-only: the render path's hash stays
    # no device behind these: a null handle has nothing
    out = np.full(4, 7, np.uint64)
    F.lib().fhip_distance_info(None, out.ctypes.data_as(C.c_void_p))
    assert out.tolist() == [0, 0xFFFFFFFFFFFFFFFF, 0, 0]
    assert not F.lib().fhip_distance_dev(None)
    F.lib().fhip_distance_free(None)
