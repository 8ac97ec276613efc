"""Connected-component labelling without a GPU: the bit arithmetic of fidget_amd/csrc/mesh_cc.hpp built for the host
(tests/host_build/mesh_cc_host.cpp) against the reference of components_ref.py run on the 4^3 block and on two adjacent bricks of an 8^3
grid; that program under ASan and UBSan; the reference against a second implementation, against scipy where there is one, and on cases
whose answers are known; the entry points as the header states them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fidget_amd as F
import components_ref as CR
import voxels_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "mesh_cc_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")
ENTRY_POINTS = ("fhip_voxels_components", "fhip_components_counts", "fhip_components_table", "fhip_components_label_slices",
                "fhip_components_extract", "fhip_components_free")
ALL_ONES = (1 << 64) - 1
CHECKERBOARD = sum(1 << (lx + 4 * ly + 16 * lz) for lz in range(4) for ly in range(4) for lx in range(4) if (lx + ly + lz) % 2 == 0)


def _build(name, flags):
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    deps = [SRC, os.path.join(CSRC, "mesh_cc.hpp"), os.path.join(CSRC, "mesh_vox.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", exe])      # (plain g++: the header touches no device)
    return exe


@pytest.fixture(scope="module")
def ask():
    exe = _build("mesh_cc_host", ["-O1"])

    def run(queries, program=exe):
        res = subprocess.run([program], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
        assert res.returncode == 0 and res.stderr == "", (res.returncode, res.stdout[-300:], res.stderr[-2000:])
        lines = res.stdout.splitlines()
        assert len(lines) == len(queries)
        return lines
    return run


def word_of(block):
    """bool [4, 4, 4] indexed [lx, ly, lz] -> the brick's word"""
    return int(V.pack(block)[0, 0, 0])


def block_of(word):
    return V.unpack(np.array([[[word]]], np.uint64))


def ref_masks(word, conn):
    """the components of the brick alone by the reference, as masks in seed order (on one brick the key is the bit number)"""
    labels, count = CR.labels_bfs(block_of(word), conn)
    bit_order = labels.transpose(2, 1, 0).reshape(64)          # [16 lz + 4 ly + lx]
    return [int.from_bytes(np.packbits(bit_order == c, bitorder="little").tobytes(), "little") for c in range(count)]


def sample_words():
    rng = np.random.default_rng(20240)
    words = [0, ALL_ONES, CHECKERBOARD, ALL_ONES ^ CHECKERBOARD]
    words += [1 << b for b in range(64)]                                                      # single voxels
    words += [0xF << (4 * r) for r in range(16)]                                              # single rows along x
    words += [sum(1 << (lx + 4 * q + 16 * lz) for q in range(4)) for lx in range(4) for lz in range(4)]      # ... along y
    words += [sum(1 << (lx + 4 * ly + 16 * q) for q in range(4)) for lx in range(4) for ly in range(4)]      # ... along z
    words += [0x8000000000000001, 0x0000000000010008, 0x9, 0x11, 0x10001, 0x21, 0x12, 0x100020]            # pairs: apart, wrapping rows, diagonal
    for density in (0.05, 0.15, 0.3, 0.5, 0.7, 0.9):
        words += [word_of(rng.random((4, 4, 4)) < density) for _ in range(350)]
    return words


def test_local_components_are_the_references(ask):
    """the same masks in the same order, for both connectivities: 2 100 random words at six densities and the special ones"""
    words = sample_words()
    assert len(words) > 2200
    for conn in (6, 26):
        got = ask([f"L {w:x} {conn}" for w in words])
        for w, line in zip(words, got):
            n, *masks = line.split()
            masks = [int(m, 16) for m in masks]
            assert int(n) == len(masks)
            assert masks == ref_masks(w, conn), (hex(w), conn)


def test_the_checkerboard_is_the_most(ask):
    (six,), (twenty_six,) = ask([f"L {CHECKERBOARD:x} 6"]), ask([f"L {CHECKERBOARD:x} 26"])
    n, *masks = six.split()
    assert int(n) == 32 and [int(m, 16) for m in masks] == [1 << b for b in range(64) if CHECKERBOARD >> b & 1]
    assert twenty_six.split() == ["1", f"{CHECKERBOARD:x}"]
    assert ask(["L 0 6", "L 0 26", f"L {ALL_ONES:x} 6", f"L {ALL_ONES:x} 26"]) == ["0", "0", f"1 {ALL_ONES:x}", f"1 {ALL_ONES:x}"]


def test_the_thirteen_directions(ask):
    (line,) = ask(["D"])
    dirs = [tuple(int(v) for v in d.split(",")) for d in line.split()]
    assert dirs[:3] == [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    assert len(set(dirs)) == 13 and all((dz, dy, dx) > (0, 0, 0) for dx, dy, dz in dirs)           # the positive half ...
    assert set(dirs) | {(-x, -y, -z) for x, y, z in dirs} == set(CR.offsets(26))                 # ... of all 26
    assert [sum(map(abs, d)) for d in dirs] == [1] * 3 + [2] * 6 + [3] * 4


def test_carry_is_the_definition(ask):
    """masks a and b in two adjacent bricks of an 8^3 grid: carry(a) & b != 0 exactly when some voxel of a and some voxel of b are
    neighbours; and carry(a) itself is exactly the positions of the other brick that have a neighbour in a"""
    rng = np.random.default_rng(77)
    (line,) = ask(["D"])
    dirs = [tuple(int(v) for v in d.split(",")) for d in line.split()]
    dirs += [(-x, -y, -z) for x, y, z in dirs]          # carry takes any of the 26
    queries, cases = [], []
    for conn in (6, 26):
        offs = CR.offsets(conn)
        for d in dirs:
            for density_a, density_b in ((0.1, 0.1), (0.3, 0.05), (0.02, 0.5), (0.6, 0.6)):
                for _ in range(6):
                    a, b = rng.random((4, 4, 4)) < density_a, rng.random((4, 4, 4)) < density_b
                    oa = [4 if v < 0 else 0 for v in d]          # brick A where brick B = A + d stays in the grid
                    ob = [o + 4 * v for o, v in zip(oa, d)]
                    ga = np.zeros((8, 8, 8), bool)
                    ga[oa[0]:oa[0] + 4, oa[1]:oa[1] + 4, oa[2]:oa[2] + 4] = a
                    touched = np.zeros((8, 8, 8), bool)          # every voxel with a neighbour in A's mask
                    for i, j, k in zip(*np.nonzero(ga)):
                        for dx, dy, dz in offs:
                            u, v, w = i + dx, j + dy, k + dz
                            if 0 <= u < 8 and 0 <= v < 8 and 0 <= w < 8:
                                touched[u, v, w] = True
                    image = touched[ob[0]:ob[0] + 4, ob[1]:ob[1] + 4, ob[2]:ob[2] + 4]
                    queries.append(f"C {word_of(a):x} {d[0]} {d[1]} {d[2]} {conn}")
                    cases.append((conn, d, word_of(a), word_of(b), word_of(image), bool((image & b).any())))
    got = ask(queries)
    hits = 0
    for (conn, d, wa, wb, image, meet), line in zip(cases, got):
        c = int(line, 16)
        assert c == image, (conn, d, hex(wa), hex(c), hex(image))
        assert ((c & wb) != 0) == meet
        hits += meet
    assert 100 < hits < len(cases) - 100
    # connectivity 6: nothing crosses an edge or a corner
    assert set(ask([f"C {ALL_ONES:x} {d[0]} {d[1]} {d[2]} 6" for d in dirs if sum(map(abs, d)) > 1])) == {"0"}


def test_bounds_border_and_keys(ask):
    rng = np.random.default_rng(5)
    queries, want = [], []
    for _ in range(300):
        m = rng.random((4, 4, 4)) < rng.choice([0.03, 0.2, 0.6])
        if not m.any():
            continue
        nb = int(rng.choice([1, 2, 4]))
        b = [int(v) for v in rng.integers(0, nb, 3)]
        idx = np.nonzero(m)
        coords = [4 * b[a] + idx[a] for a in range(3)]
        border = any(((c == 0) | (c == 4 * nb - 1)).any() for c in coords)
        queries.append(f"B {word_of(m):x} {b[0]} {b[1]} {b[2]} {nb}")
        want.append(" ".join(str(int(idx[a].min())) for a in range(3)) + " " + " ".join(str(int(idx[a].max())) for a in range(3)) + f" {int(border)}")
    assert ask(queries) == want
    for depth in (0, 1, 3):
        N = 4 << depth
        key = CR.keys(N)
        pts = rng.integers(0, N, (50, 3))
        assert ask([f"K {int(key[i, j, k])} {depth}" for i, j, k in pts]) == [f"{i} {j} {k}" for i, j, k in pts]
        assert sorted(key.reshape(-1)) == list(range(N ** 3))


def test_the_arithmetic_runs_clean_under_sanitizers(ask):
    """the same program as a stand-alone executable with ASan and UBSan"""
    exe = _build("mesh_cc_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    words = sample_words()[:400]
    queries = [f"L {w:x} {conn}" for conn in (6, 26) for w in words] + ["D", f"K {64 * 511 + 63} 3"]
    queries += [f"C {w:x} {dx} {dy} {dz} {conn}" for w in words[::7] for conn in (6, 26) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
    queries += [f"B {w:x} 0 1 0 2" for w in words if w]
    assert ask(queries, program=exe) == ask(queries)


# ---- the reference against itself ----------------------------------------------------------------------------------------------------------
def same(a, b):
    return (np.array_equal(a.labels, b.labels) and a.count == b.count and np.array_equal(a.sizes, b.sizes) and np.array_equal(a.seeds, b.seeds)
            and np.array_equal(a.lo, b.lo) and np.array_equal(a.hi, b.hi) and np.array_equal(a.border, b.border))


@pytest.mark.parametrize("conn", [6, 26])
def test_the_two_references_agree(conn):
    rng = np.random.default_rng(300 + conn)
    for N, density in ((4, 0.5), (8, 0.1), (8, 0.3), (16, 0.15), (16, 0.25), (16, 0.6)):
        fg = rng.random((N, N, N)) < density
        a, b = CR.components(fg, conn), CR.components_bfs(fg, conn)
        assert same(a, b) and a.count > 0 and int(a.sizes.sum()) == int(fg.sum()) and ((a.labels >= 0) == fg).all()


@pytest.mark.parametrize("conn", [6, 26])
def test_scipy_finds_the_same_partition(conn):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(17 + conn)
    structure = ndimage.generate_binary_structure(3, 1 if conn == 6 else 3)
    for density in (0.1, 0.25, 0.5):
        fg = rng.random((16, 16, 16)) < density
        lab, n = ndimage.label(fg, structure)
        r = CR.components(fg, conn)
        assert n == r.count
        pairs = set(zip(lab[fg].tolist(), r.labels[fg].tolist()))          # a bijection between the two numberings
        assert len(pairs) == n == len({p for p, _ in pairs}) == len({q for _, q in pairs})


def two_cubes():
    fg = np.zeros((8, 8, 8), bool)
    fg[1:4, 1:4, 1:4] = True
    fg[4:6, 4:6, 4:6] = True          # (3, 3, 3) and (4, 4, 4) meet at a corner only
    return fg


def hollow_box(N=16, lo=3, hi=12):
    """a box [lo, hi]^3 with walls one voxel thick: the cavity is (hi - lo - 1)^3 voxels"""
    fg = np.zeros((N, N, N), bool)
    fg[lo:hi + 1, lo:hi + 1, lo:hi + 1] = True
    fg[lo + 1:hi, lo + 1:hi, lo + 1:hi] = False
    return fg


def test_two_cubes_touching_at_a_corner():
    six, twenty_six = CR.components(two_cubes(), 6), CR.components(two_cubes(), 26)
    assert six.count == 2 and six.sizes.tolist() == [27, 8] and twenty_six.count == 1 and twenty_six.sizes.tolist() == [35]
    assert six.seeds.tolist() == [[1, 1, 1], [4, 4, 4]] and six.lo.tolist() == [[1, 1, 1], [4, 4, 4]] and six.hi.tolist() == [[3, 3, 3], [5, 5, 5]]
    assert not six.border.any()


def test_a_hollow_box_encloses_one_void():
    box = hollow_box()
    solid = CR.components(box, 6)
    assert solid.count == 1 and int(solid.sizes[0]) == 10 ** 3 - 8 ** 3 and not solid.border[0]
    voids = CR.components(CR.foreground(box, complement=True), 6)
    assert voids.count == 2 and voids.border.tolist() == [True, False]
    assert int(voids.sizes[1]) == 8 ** 3 and voids.lo[1].tolist() == [4, 4, 4] and voids.hi[1].tolist() == [11, 11, 11]
    assert int(voids.sizes[0]) == 16 ** 3 - 10 ** 3 and voids.seeds[0].tolist() == [0, 0, 0]


# ---- the interface -----------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "fidget_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    lib = C.CDLL(F.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in F.EXPORTS and getattr(F.lib(), name).argtypes is not None, name
    assert re.search(r"fhip_voxels_components\s*\([^;]*void\s*\*\*\s*out\s*\)", hdr)          # the handle is a void*
    assert callable(F.Voxels.components) and all(callable(getattr(F.Components, m)) for m in ("largest", "label_slices", "extract"))
    ffi = open(os.path.join(ROOT, "rust", "fidget-hip", "src", "ffi.rs")).read()
    assert all(f"pub fn {name}(" in ffi for name in ENTRY_POINTS) and os.path.exists(os.path.join(ROOT, "rust", "fidget-hip", "src", "components.rs"))
    # no device behind these: a null handle counts nothing and has no table
    out = np.full(4, 7, np.uint64)
    F.lib().fhip_components_counts(None, out.ctypes.data_as(C.c_void_p))
    assert out.tolist() == [0, 0, 0, 0]
    F.lib().fhip_components_free(None)
