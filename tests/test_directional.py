"""A voxel bitmap along a direction without a GPU: the reference of directional_ref.py on the 16^3 "table", whose numbers are known, and
against invariants on random grids; the bit arithmetic of fidget_amd/csrc/mesh_flow.hpp built for the host
(tests/host_build/mesh_flow_host.cpp) - the flow inside a word with its carry for all six directions, the pairs (G, P) folded along
rows of bricks in both orders of association, the move by 1 .. 4 voxels with a neighbour, the dilation by the disc for every reach2,
the heights of a word's columns - against the reference; that program under ASan and UBSan; the entry points as the header states
them."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np

import directional_ref as DR
import fidget_amd as F
import voxels_ref as V
from test_voxel_mesh import box, voxels_at

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "mesh_flow_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")
ENTRY_POINTS = ("fhip_voxels_flow", "fhip_voxels_overhangs", "fhip_voxels_heights")
NEW_FILES = ("mesh_flow.hpp", "flow.hip", "capi_flow.hpp")


def table16():
    """a slab on a leg"""
    return box(16, (6, 6, 0), (10, 10, 10), into=box(16, (2, 2, 10), (14, 14, 12)))


# ---- known answers ---------------------------------------------------------------------------------------------------------------------------
def test_the_table():
    t = table16()
    assert int(t.sum()) == 12 * 12 * 2 + 4 * 4 * 10
    for reach2, n in ((0, 128), (1, 112), (2, 108), (4, 92)):
        o = DR.overhangs(t, 5, reach2, True)
        assert int(o.sum()) == n and int(o[:, :, 10].sum()) == n, reach2          # all in layer 10: the slab's underside away from the leg
    s = DR.supports(t, 5, 0, True)
    assert int(s.sum()) == 1280 and not s[:, :, 10:].any()          # ten clear voxels under each of the 128
    # without a bed the leg's foot hangs over nothing, too; under it lies the border: no support is added
    o = DR.overhangs(t, 5, 0, False)
    assert int(o.sum()) == 128 + 16 and int(o[6:10, 6:10, 0].sum()) == 16
    assert np.array_equal(DR.supports(t, 5, 0, False), s)
    h = DR.heights(t, 2)
    assert h.shape == (3, 16, 16) and h.dtype == np.int32
    leg, slab = box(16, (6, 6, 0), (10, 10, 1))[:, :, 0].T, box(16, (2, 2, 0), (14, 14, 1))[:, :, 0].T          # [j][i]
    # over the leg 10 + 2 voxels; over the slab alone its two layers, the lower of them layer 10; elsewhere none
    assert (h[2][leg] == 12).all() and (h[2][slab & ~leg] == 2).all() and (h[2][~slab] == 0).all()
    assert (h[0][leg] == 0).all() and (h[0][slab & ~leg] == 10).all() and (h[1][slab] == 11).all()
    assert (h[0][~slab] == -1).all() and (h[1][~slab] == -1).all()


def test_the_definitions_on_voxels_written_out_by_hand():
    s, k = voxels_at(8, [(1, 2, 3)]), voxels_at(8, [(5, 2, 3)])
    assert np.array_equal(DR.flow(s, k, 1), box(8, (2, 2, 3), (5, 3, 4)))          # from the voxel after the seed up to the blocker
    assert np.array_equal(DR.flow(s, k, 0), box(8, (0, 2, 3), (1, 3, 4)))
    assert np.array_equal(DR.flow(s, None, 3, True), box(8, (1, 2, 3), (2, 8, 4)))
    assert np.array_equal(DR.flow(s, s, 5), box(8, (1, 2, 4), (2, 3, 8)))          # a seed that is itself blocked still emits
    assert not DR.flow(s, voxels_at(8, [(1, 2, 4)]), 5).any()
    assert len(DR.disc(0)) == 1 and len(DR.disc(1)) == 5 and len(DR.disc(2)) == 9 and len(DR.disc(4)) == 13 and len(DR.disc(16)) == 49
    # a diagonal neighbour below supports from reach2 = 2 on; towards -y "below" is j + 1
    pair = voxels_at(8, [(3, 3, 3), (4, 4, 4)])
    assert DR.overhangs(pair, 5, 1, True)[4, 4, 4] and not DR.overhangs(pair, 5, 2, True)[4, 4, 4]
    assert DR.overhangs(pair, 2, 1, True)[3, 3, 3] and not DR.overhangs(pair, 2, 2, True)[3, 3, 3]
    # heights' layout: axis 0 gives [k][j], axis 1 [k][i]
    g = voxels_at(8, [(1, 2, 3), (6, 2, 3)])
    assert DR.heights(g, 0)[:, 3, 2].tolist() == [1, 6, 2] and DR.heights(g, 1)[:, 3, 6].tolist() == [2, 2, 1] and DR.heights(g, 2)[:, 2, 1].tolist() == [3, 3, 1]


# ---- invariants --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_grids():
    rng = np.random.default_rng(81)
    return [(rng.random((N, N, N)) < ds, rng.random((N, N, N)) < dk) for N in (4, 8, 16) for ds, dk in ((0.05, 0.1), (0.3, 0.3), (0.6, 0.05))]


def test_the_invariants_on_random_grids():
    for solid, other in random_grids():
        N = solid.shape[0]
        for d in range(6):
            r = DR.flow(solid, other, d)
            assert not (r & other).any()
            flip = lambda a: np.flip(a, axis=d >> 1)          # noqa: E731
            assert np.array_equal(flip(DR.flow(flip(solid), flip(other), d ^ 1)), r)          # the mirrored grid, the mirrored direction
            assert np.array_equal(DR.flow(solid, None, d, True), DR.flow(solid, solid, d) | solid)          # swept = shadow u solid
            last = solid
            for reach2 in (0, 1, 2, 4, 5, 8, 9, 16):
                o = DR.overhangs(solid, d, reach2, False)
                assert not (o & ~last).any()          # overhangs shrink as reach2 grows
                last = o
            sup = DR.supports(solid, d, 1, True)
            assert not (sup & solid).any()
            # below every run of supports lies a set voxel or the border: one step towards d ^ 1 from a support is a support or solid
            step = np.roll(sup | solid, 1 if d & 1 else -1, axis=d >> 1)
            edge = [slice(None)] * 3
            edge[d >> 1] = 0 if d & 1 else N - 1
            step[tuple(edge)] = True
            assert not (sup & ~step).any()
        h = DR.heights(solid, 2)
        full = h[2] > 0
        assert int(DR.flow(solid, solid, 4).sum()) == int((h[1] + 1 - h[2])[full].sum())          # shadow(4): the clear voxels under a set one


# ---- the library's bit arithmetic, built for the host --------------------------------------------------------------------------------------
def _build(name, flags):
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("mesh_flow.hpp", "mesh_vmesh.hpp", "mesh_vox.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe])      # (plain g++: the header touches no device)
    return exe


LINES = [("F", 6), ("X", 4), ("M", 24), ("O", 204), ("H", 3)]


def run(exe, grids):
    """-> per pair (seeds, blockers) the program's lines as {tag: uint64 [lines, numbers]}"""
    queries = []
    for seeds, blockers in grids:
        s, k = V.pack(seeds), V.pack(blockers)
        queries.append(f"G {s.shape[0].bit_length() - 1} " + " ".join(f"{int(w):x}" for w in list(s.reshape(-1)) + list(k.reshape(-1))))
    res = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
    assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stdout[-300:], res.stderr[-2000:])
    lines = res.stdout.splitlines()
    per = sum(n for _, n in LINES)
    assert len(lines) == per * len(grids)
    out = []
    for g in range(len(grids)):
        at, got = per * g, {}
        for tag, n in LINES:
            assert all(line[0] == tag for line in lines[at:at + n])
            got[tag] = np.array([[int(x, 16) for x in line.split()[1:]] for line in lines[at:at + n]], np.uint64)
            at += n
        out.append(got)
    return out


@functools.lru_cache(maxsize=None)
def sample_grids():
    """pairs (seeds, blockers) at depth 0, 1, 2: empty, full, random at several densities, single voxels at both ends of every axis"""
    rng = np.random.default_rng(82)
    grids = []
    for N in (4, 8, 16):
        e, f = np.zeros((N, N, N), bool), np.ones((N, N, N), bool)
        grids += [(e, e), (f, e), (f, f), (e, f)]
    grids += [(rng.random((4, 4, 4)) < ds, rng.random((4, 4, 4)) < dk) for ds, dk in ((0.05, 0.1), (0.5, 0.5), (0.9, 0.02), (0.2, 0.0))]
    grids += [(rng.random((8, 8, 8)) < ds, rng.random((8, 8, 8)) < dk) for ds, dk in ((0.02, 0.05), (0.3, 0.3), (0.6, 0.05), (0.95, 0.5))]
    grids += [(rng.random((16, 16, 16)) < ds, rng.random((16, 16, 16)) < dk) for ds, dk in ((0.005, 0.01), (0.3, 0.1))]
    for N in (4, 8, 16):
        ends = [tuple(e if a == axis else 1 for a in range(3)) for axis in range(3) for e in (0, N - 1)]
        grids += [(voxels_at(N, [p]), voxels_at(N, [q])) for p, q in zip(ends, ends[1:] + ends[:1])]
    grids.append((table16(), table16()))
    return grids


def shifted(a, axis, s):
    """[p] -> a[p - s e_axis], clear outside"""
    out = np.zeros_like(a)
    n = a.shape[0]
    src, dst = [slice(None)] * 3, [slice(None)] * 3
    dst[axis], src[axis] = slice(max(s, 0), min(n, n + s)), slice(max(-s, 0), min(n, n - s))
    out[tuple(dst)] = a[tuple(src)]
    return out


def compare(got, seeds, blockers):
    words = lambda a: V.pack(a).reshape(-1)          # noqa: E731
    for d in range(6):
        assert np.array_equal(got["F"][d], words(DR.flow(seeds, blockers, d))), d
    for line, d in enumerate((0, 0, 1, 1)):
        assert np.array_equal(got["X"][line], words(DR.flow(seeds, blockers, d))), (line, d)
    moves = [(axis, s) for axis in range(3) for s in (-4, -3, -2, -1, 1, 2, 3, 4)]
    for line, (axis, s) in enumerate(moves):
        assert np.array_equal(got["M"][line], words(shifted(seeds, axis, s))), (axis, s)
    line = 0
    for up in range(6):
        for bed in (False, True):
            for reach2 in range(17):
                assert np.array_equal(got["O"][line], words(DR.overhangs(seeds, up, reach2, bed))), (up, bed, reach2)
                line += 1
    for axis in range(3):
        assert np.array_equal(got["H"][axis].astype(np.uint32).view(np.int32), DR.heights(seeds, axis).reshape(-1)), axis


def test_the_bit_arithmetic_is_the_references():
    grids = sample_grids()
    for got, (seeds, blockers) in zip(run(_build("mesh_flow_host", ["-O1"]), grids), grids):
        compare(got, seeds, blockers)


def test_the_arithmetic_runs_clean_under_sanitizers():
    """the same program as a stand-alone executable with ASan and UBSan, on the same input: exit 0, nothing on stderr (`run` asserts
    both), the same output"""
    grids = sample_grids()
    plain = run(_build("mesh_flow_host", ["-O1"]), grids)
    san = run(_build("mesh_flow_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), grids)
    assert len(plain) == len(san)
    for a, b in zip(plain, san):
        assert all(np.array_equal(a[tag], b[tag]) for tag, _ in LINES)


# ---- the interface -----------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fidget_hip.h")).read()
    stated = " ".join(re.sub(r"^ \* ?", "", hdr, flags=re.M).split())          # (the comment's lines without their leading " * ")
    for words in ("R(p) = (R(p - e) | S(p - e)) & ~K(p)", "a seed that is itself blocked still emits", "a blocked voxel is never in R",
                  "(q - p) . e(up) = -1", "is at most reach2", "every q counts as set iff `bed`", "flow(S = overhangs, K = A, d = up ^ 1)",
                  "a = 2 gives [j][i], a = 1 [k][i], a = 0 [k][j]", "-1 in an empty column", "the AND of the two opposite shadows"):
        assert words in stated, words          # the definitions are in the comment
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert re.search(r"#define\s+FHIP_FLOW_WITH_SEEDS\s+1u", hdr)
    lib = C.CDLL(F.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in F.EXPORTS and getattr(F.lib(), name).argtypes is not None, name
    assert re.search(r"fhip_voxels_flow\s*\([^;]*uint32_t\s+dir\s*,\s*uint32_t\s+flags\s*,\s*uint64_t\s*\*\s*out\s*,\s*int\s+out_on_device\s*\)", hdr)
    assert re.search(r"fhip_voxels_overhangs\s*\([^;]*uint32_t\s+up\s*,\s*uint32_t\s+reach2\s*,\s*int\s+bed\s*,\s*uint64_t\s*\*\s*out\s*,", hdr)
    assert re.search(r"fhip_voxels_heights\s*\([^;]*uint32_t\s+axis\s*,\s*int32_t\s*\*\s*out\s*,", hdr)
    assert all(callable(getattr(F.Voxels, m)) for m in ("flow", "shadow", "swept", "overhangs", "supports", "heights"))
    assert "opposite shadows" in F.Voxels.flow.__doc__ and "(q - p) . e(up) = -1" in F.Voxels.overhangs.__doc__
    ffi = open(os.path.join(ROOT, "rust", "fidget-hip", "src", "ffi.rs")).read()
    assert all(f"pub fn {name}(" in ffi for name in ENTRY_POINTS)
    mesh_only = open(os.path.join(ROOT, "tools", "src_hash.py")).read()
    assert all(f'"{name}"' in mesh_only for name in NEW_FILES)          # mesh-only: the render path's hash stays
    assert all(name in F._SOURCES for name in NEW_FILES)
