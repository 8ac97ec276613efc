"""The local thickness without a GPU: the two forms of thickness_ref.py against each other and against the closed form of a slab; the
arithmetic of fidget_amd/csrc/mesh_thick.hpp built for the host (tests/host_build/mesh_thick_host.cpp) - the integer square root, the
rows of a ball, the domination bound, and the serial thickness made of them, pruned and unpruned - against the reference; that program
under ASan and UBSan; the entry points as the header states them."""
import ctypes as C
import functools
import math
import os
import re
import subprocess

import numpy as np

import fidget_amd as F
import distance_ref as DR
import thickness_grids as G
import thickness_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "mesh_thick_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")
ENTRY_POINTS = ("fhip_distance_thickness", "fhip_thickness_info", "fhip_thickness_thin", "fhip_thickness_histogram")
MAX_F = 3 * 1023 ** 2
SMALL = [name for name in G.GRIDS if G.depth_of(name) <= 3]          # up to 32^3


field_of, reference = G.field_of, G.reference


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def test_the_two_forms_of_the_reference_agree():
    for name in SMALL:
        Fd = field_of(name)
        T = reference(name)
        assert np.array_equal(TR.by_offsets(Fd), T), name
        assert np.array_equal(T > 0, Fd > 0) and (T >= Fd).all(), name          # covered exactly where a ball is centred


def test_known_answers():
    # a slab w thick reads ceil(w / 2)^2 in its middle, whatever the side
    for w, want in ((14, 49), (17, 81), (6, 9), (7, 16), (1, 1), (2, 1)):
        t = TR.slab(32, 5, 5 + w)
        assert int(t.max()) == want and (t[5:5 + w] > 0).all() and not t[:5].any() and not t[5 + w:].any(), (w, t)
    # ... and is the definition on the whole grid
    for axis in range(3):
        name = f"d2-plates-{'ijk'[axis]}-spanning"
        line = TR.slab(16, 1, 7) + TR.slab(16, 8, 15)
        want = np.broadcast_to(line.reshape([16 if a == axis else 1 for a in range(3)]), (16, 16, 16))
        assert np.array_equal(reference(name), want), name
        assert set(line.tolist()) == {0, 9, 16}
    # one clear voxel in a full brick: the ball around the far corner, of squared radius 27, just misses it and holds (1, 0, 0), 22 away
    T = reference("d0-clear000")
    assert T[0, 0, 0] == 0 and T[3, 3, 3] == 27 and T[1, 0, 0] == 27
    # the fin does not inherit the block's value; the block's core does not take the fin's
    T = reference("d2-fin-on-block")
    assert T[12:15, 7:9, 4:12].max() == 1 and T[4:8, 4:12, 4:12].min() >= 16 and T[4, 4, 4] == 16
    # the larger ball wins only inside itself
    T, Fd = reference("d2-two-balls"), field_of("d2-two-balls")
    assert T.max() == Fd.max() and T[13, 8, 8] < T[6, 7, 7] and T[13, 8, 8] > 0
    assert TR.summary(reference("d0-empty")) == (0, (0, 0, 0), None, None, 0)
    assert TR.histogram(np.array([[[0, 1, 2, 5, 9]]]), [0, 1, 2, 5, 9, 10]).tolist() == [1, 1, 1, 1, 1]
    assert TR.histogram(np.array([[[0, 1, 2, 5, 9]]]), [1, 5, 5, 9]).tolist() == [2, 0, 1]


# ---- the library's arithmetic, built for the host --------------------------------------------------------------------------------------------
def _build(name, flags):
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    deps = [SRC, os.path.join(CSRC, "mesh_thick.hpp"), os.path.join(CSRC, "mesh_vox.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe])      # (plain g++: the header touches no device)
    return exe


def plain():
    return _build("mesh_thick_host", ["-O2"])


def run(exe, queries):
    res = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stdout[-300:], res.stderr[-2000:])
    lines = res.stdout.splitlines()
    assert len(lines) == len(queries)
    return [np.array(line.split(), np.int64) for line in lines]


def test_isqrt_everywhere():
    """the program prints the root at 0 and wherever it changes up to 3 * 1023^2: that must be w at w^2 for every w and nowhere else, which
    fixes the value at every x"""
    (got,) = run(plain(), [f"Q 0 {MAX_F}"])
    top = math.isqrt(MAX_F)
    assert top == 1771 and np.array_equal(got.reshape(-1, 2), np.array([(w * w, w) for w in range(top + 1)]))


def test_rows_are_the_balls_rows():
    """for every squared radius up to 200: the half-widths of the rows against the reference's ball, a row at a time"""
    fs = list(range(1, 201))
    got = run(plain(), [f"W {f} 15" for f in fs])
    for f, g in zip(fs, got):
        m, R = TR.ball(f)
        assert R <= 14
        full = np.zeros((31, 31, 31), bool)
        full[15 - R:16 + R, 15 - R:16 + R, 15 - R:16 + R] = m          # [dx, dy, dz]
        n = full.sum(axis=0)                                          # voxels per row [dy, dz]
        want = np.where(n > 0, (n - 1) // 2, -1).T                    # the program prints dz outermost
        assert np.array_equal(g.reshape(31, 31), want), f
        assert all(full[15 - w:16 + w, dy, dz].all() for dy in range(31) for dz in range(31) for w in [want[dz, dy]] if w >= 0), f


def test_need_is_the_brute_force_bound():
    """need(v, d) = 1 + max |q - d|^2 over the integer q with |q|^2 < v, for all 26 offsets d and v <= 144"""
    vs = list(range(1, 145))
    got = run(plain(), [f"N {v}" for v in vs])
    a = np.arange(-12, 13)
    q = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    q2 = (q ** 2).sum(1)
    offsets = [d for d in np.ndindex(3, 3, 3) if d != (1, 1, 1)]
    assert len(offsets) == 26
    for v, g in zip(vs, got):
        inside = q[q2 < v]
        for d in offsets:
            d = np.array(d) - 1
            want = 1 + int((((inside - d) ** 2).sum(1)).max())
            assert g[int((d != 0).sum()) - 1] == want, (v, d)
    assert got[0].tolist() == [2, 3, 4] and got[99].tolist() == [119, 130, 137]


def thickness_queries(names, prune):
    return [f"T {len(field_of(n))} {int(prune)} " + " ".join(map(str, DR.field(field_of(n)).reshape(-1).tolist())) for n in names]


@functools.lru_cache(maxsize=None)
def host_fields(exe, prune):
    return run(exe, thickness_queries(SMALL, prune))


def test_thickness_host_is_the_reference_pruned_or_not():
    centres = 0
    for prune in (True, False):
        for name, got in zip(SMALL, host_fields(plain(), prune)):
            N = len(field_of(name))
            assert np.array_equal(got[1:].reshape(N, N, N), TR.field(reference(name))), (name, prune)
            n = int((field_of(name) > 0).sum())
            assert got[0] == n if not prune else got[0] <= n, (name, prune)
            if prune and n:
                assert got[0] > 0
            centres += n
    assert centres > 0
    pruned, whole = host_fields(plain(), True), host_fields(plain(), False)
    assert sum(int(p[0]) for p in pruned) < sum(int(w[0]) for w in whole) // 2          # the test drops most centres
    # the spanning plates keep their medial planes alone: one for 7 voxels, two for 6
    at = SMALL.index("d2-plates-k-spanning")
    assert int(pruned[at][0]) == 3 * 16 * 16
    (refused,) = subprocess.run([plain()], input="T 2 1 " + " ".join(["4294967295"] * 8) + "\n", capture_output=True, text=True).stdout.splitlines()
    assert refused == "refused"


def test_the_arithmetic_runs_clean_under_sanitizers():
    """the same program as a stand-alone executable with ASan and UBSan, on the same input: exit 0, nothing on stderr (`run` asserts
    both), the same answers"""
    small = [n for n in SMALL if G.depth_of(n) <= 2]
    queries = ["Q 0 70000", f"Q {MAX_F - 5000} {MAX_F}"] + [f"W {f} 15" for f in (1, 2, 9, 200)] + [f"N {v}" for v in (1, 2, 100, 144)]
    queries += thickness_queries(small, True) + thickness_queries(small, False)
    san = _build("mesh_thick_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    a, b = run(plain(), queries), run(san, queries)
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the interface -----------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fidget_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    lib = C.CDLL(F.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in F.EXPORTS and getattr(F.lib(), name).argtypes is not None, name
    assert re.search(r"fhip_distance_thickness\s*\([^;]*void\s*\*\*\s*out\s*\)", hdr)          # the handle is a void*
    assert callable(F.Voxels.thickness) and callable(F.DistanceField.thickness) and issubclass(F.ThicknessField, F.DistanceField)
    assert all(callable(getattr(F.ThicknessField, m)) for m in ("slices", "within", "beyond", "thin", "histogram"))
    assert isinstance(F.ThicknessField.squared_device, property)
    ffi = open(os.path.join(ROOT, "rust", "fidget-hip", "src", "ffi.rs")).read()
    assert all(f"pub fn {name}(" in ffi for name in ENTRY_POINTS)
    mesh_only = open(os.path.join(ROOT, "tools", "src_hash.py")).read()
    assert all(f'"{name}"' in mesh_only for name in ("mesh_thick.hpp", "thick.hip", "capi_thick.hpp"))          # mesh-only: the render path's hash stays
    assert all(name in F._SOURCES for name in ("mesh_thick.hpp", "thick.hip", "capi_thick.hpp"))
    # no device behind these: a null handle has nothing
    out = np.full(8, 7, np.uint64)
    F.lib().fhip_thickness_info(None, out.ctypes.data_as(C.c_void_p))
    assert out.tolist() == [0, 0xFFFFFFFFFFFFFFFF, 0, 0xFFFFFFFFFFFFFFFF, 0, 0, 0, 0]
