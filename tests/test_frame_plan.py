"""The plan of a frame's set-up (fidget_amd/csrc/frame_plan.hpp: slabs and layers of a part, root groups, queue capacities, buffer sizes,
kernel paths, refusals - pure functions of the tape's numbers, the options and the image) built for the host
(tests/host_build/frame_plan_host.cpp) and compared with the same rules restated here for the geometry, and with pinned tables for the
kernel paths and the refusals.  The GPU parity tests pass for ANY consistent plan (the image does not depend on tiles, slabs or paths):
a rule that wrongly drops a fast path, or sizes a buffer too generously, shows here, not there.  No GPU.

Line format: `name: key=value ...`; roots as first,n,stride,z,x joined by ';' in queue order; a refusal's text with '_' for spaces."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "frame_plan_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")

LDS_MAX = 160 * 1024


@pytest.fixture(scope="module")
def plans():
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "frame_plan_host")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("frame_plan.hpp", "render_state.h", "tape_format.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        # (plain g++, no HIP headers: the plan touches no device)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-I", CSRC, SRC, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, check=True)
    lines = {}
    for line in res.stdout.splitlines():
        name, _, rest = line.partition(":")
        lines[name] = dict(kv.split("=", 1) for kv in rest.split())
    return lines


def ceil_div(a, b):
    return (a + b - 1) // b


def tiles_lds(regs, choices, tl):
    return (regs * tl * 8 + ceil_div(choices, 16) * tl * 4 + regs * tl + 256 + 15) // 16 * 16


class Frame:
    """A case of the host program: what it was given.  The defaults are the program's: prospero.vm's kind of tape, 1024^3, a whole frame."""

    def __init__(self, size=(1024, 1024, 1024), is3d=True, part=None, slab_layers=4, no_zrep=0, no_column_inv=0, use_split=True, one_level_64=False, slab_contexts=4,
                 regs=72, choices=3000, ops=6363, n_cu=256):
        self.w, self.h, self.d = size
        self.is3d, self.slab_layers, self.no_zrep, self.no_column_inv, self.use_split = is3d, slab_layers, no_zrep, no_column_inv, use_split
        self.one_level_64, self.slab_contexts, self.regs, self.choices, self.ops, self.n_cu = one_level_64, slab_contexts, regs, choices, ops, n_cu
        self.part = dict(shard=0, n_shards=1, ix=0, nx=1, iy=0, ny=1, iz=0, nz=1)
        self.part.update(part or {})


def expected_geometry(f, ts, sizes):
    """The rules, restated: `ts` is the tile list the plan took (pinned separately)."""
    p, w, h, d = f.part, f.w, f.h, f.d if f.is3d else 0
    dim = 3 if f.is3d else 2
    fanout = max([1] + [(a // b) ** dim for a, b in zip(ts, ts[1:])])
    tl = 64 if fanout > 16 or (not f.is3d and len(ts) == 1 and f.one_level_64) else 16
    rx, ry = ceil_div(w, ts[0]), ceil_div(h, ts[0])
    n_layers = ceil_div(d, ts[0]) if f.is3d else 1
    prepass = f.is3d and len(ts) >= 2 and n_layers <= 64
    # layers per slab: option slab_layers (1 .. 8) counts 128-voxel layers; halved until a slab has at most 64 leaf layers and there are two slabs
    sl = max(1, min(8, f.slab_layers)) * max(1, 128 // ts[0]) if prepass else 1
    while sl > 1 and (ts[0] * sl // 8 > 64 or sl * 2 > n_layers):
        sl //= 2
    slab = ts[0] * sl
    n_slabs = ceil_div(d, slab) if f.is3d else 1
    pre = min(2, len(ts) - 1) if prepass else 0
    # the part's layers: layer k belongs to block k * nz // n_layers; its slabs are those that hold one of them
    mine = [k for k in range(n_layers) if k * p["nz"] // n_layers == p["iz"]]
    lo, hi = (mine[0], mine[-1] + 1) if mine else (0, 0)
    assert mine == list(range(lo, hi))
    slab_lo, slab_hi = (lo // sl, ceil_div(hi, sl)) if pre else (lo, hi)
    # runs of at most tl root tiles (x-major numbering): a block's columns, one run set per column; or every n_shards-th tile
    runs = []
    if p["nx"] > 1 or p["ny"] > 1:
        for tx in range(rx):
            if tx * p["nx"] // rx != p["ix"]:
                continue
            ys = [ty for ty in range(ry) if ty * p["ny"] // ry == p["iy"]]
            runs += [(tx * ry + ys[i], len(ys[i:i + tl]), 1) for i in range(0, len(ys), tl)]
    else:
        tiles = list(range(p["shard"], rx * ry, p["n_shards"]))
        runs = [(tiles[i], len(tiles[i:i + tl]), p["n_shards"]) for i in range(0, len(tiles), tl)]
    xy_fixed = f.is3d      # (identity camera; a 2D frame does not ask)
    root_invariant = f.is3d and not f.no_column_inv      # (the tape reads x and y, only z changes along a pixel column)
    column_inv = xy_fixed and root_invariant and f.no_zrep in (0, 3)
    root_zrep = f.is3d and pre > 0 and f.use_split and tl == 64 and column_inv
    front_only = root_zrep and f.no_zrep == 0
    slab_stop = slab_hi - 1 if front_only and slab_hi > slab_lo else slab_lo
    roots = []      # in evaluation order: front first
    if root_zrep:      # one group set per slab, standing for the part's layers in it
        for sb in range(slab_hi - 1, slab_stop - 1, -1):
            ks = [k for k in range(lo, hi) if k // sl == sb]
            if ks:
                roots += [(first, n, stride, ks[0] * ts[0], len(ks)) for first, n, stride in runs]
        sets = len({r[3] for r in roots})
    else:
        sets = hi - lo if pre else 1
        for k in range(sets):
            roots += [(first, n, stride, (hi - 1 - k) * ts[0], 0) for first, n, stride in runs]
    groups_per_slab = len(roots) // max(sets, 1) if mine else 0
    if not mine:
        roots = []
    roots.reverse()      # (they sit at the back of queue 0 in reverse)
    qcap = [max(len(roots), 1)]
    for l in range(1, len(ts)):
        tp = ts[l - 1]
        c = ceil_div(w, tp) * ceil_div(h, tp) * (slab // tp if f.is3d else 1) * (n_slabs if l < pre else 1)
        qcap.append(max(c, 1))
    leaf = ts[-1]
    n_fp = ceil_div(w, leaf) * ceil_div(h, leaf)
    leaf_cap = n_fp * (slab // leaf if f.is3d else 1)
    extra = min(f.slab_contexts, max(n_slabs, 1)) - 1
    hit_cap = ceil_div(n_fp, 64) * (slab // leaf) if f.is3d else 0
    hit_words = 64 * (64 + hit_cap) if f.is3d else 0
    mind_words = sum(ceil_div(w, t) * ceil_div(h, t) for t in ts) if f.is3d else 0
    fp_bytes = (3 * n_fp + hit_words) * 4 if f.is3d else 0
    join = lambda xs: "/".join(str(x) for x in xs)
    return dict(tl=tl, roots_x=rx, roots_y=ry, slab=slab, n_slabs=n_slabs, n_layers=n_layers, slab_lo=slab_lo, slab_hi=slab_hi, slab_stop=slab_stop, pre_levels=pre,
                roots=";".join(",".join(str(v) for v in r) for r in roots) or "-", groups_per_slab=groups_per_slab, qcap=join(qcap), squeue_cap=qcap[pre], leaf_cap=leaf_cap,
                table_words=leaf_cap if f.is3d else 0, n_footprints=n_fp, hit_bucket_cap=hit_cap, hit_words=hit_words, mind_words=mind_words,
                b_queue=join(q * sizes["group"] for q in qcap), b_squeue=qcap[pre] * n_slabs * sizes["group"] if pre else 0, b_leaves=leaf_cap * sizes["leaf"],
                b_leaves_b=extra * leaf_cap * sizes["leaf"] if f.is3d else 0, b_leaf_table=leaf_cap * sizes["leaf_ref"] if f.is3d else 0,
                b_leaf_table_b=extra * leaf_cap * sizes["leaf_ref"] if f.is3d else 0, b_zbuf=w * h * 8 if f.is3d else 0, b_normals=w * h * 12 if f.is3d else 0,
                b_fp_lists=fp_bytes, b_fp_lists_b=extra * fp_bytes, b_mind=mind_words * 4,
                xy_fixed=int(xy_fixed), root_invariant=int(root_invariant), column_inv=int(column_inv), root_zrep=int(root_zrep), front_only=int(front_only))


NOINV = dict(no_column_inv=1)
BLOCK = dict(ix=1, nx=2, iy=0, ny=2, iz=1, nz=2)
# name -> (what the host program was given, the tile list the plan must have taken)
GEOMETRY = {
    "whole_1024": (Frame(), [32, 8]),
    "whole_1024_noinv": (Frame(**NOINV), [128, 32, 8]),
    "whole_2048": (Frame((2048,) * 3), [128, 32, 8]),
    "whole_2048_noinv": (Frame((2048,) * 3, **NOINV), [128, 32, 8]),
    "whole_64": (Frame((64,) * 3), [64, 16, 8]),
    "odd_200x120x72": (Frame((200, 120, 72)), [32, 8]),
    "odd_200x120x72_noinv": (Frame((200, 120, 72), **NOINV), [32, 8]),
    "no_zrep1": (Frame(no_zrep=1), [128, 32, 8]),
    "no_zrep2": (Frame(no_zrep=2), [128, 32, 8]),
    "no_zrep3": (Frame(no_zrep=3), [32, 8]),
    "slab_layers1": (Frame(slab_layers=1), [32, 8]),
    "slab_layers1_noinv": (Frame(slab_layers=1, **NOINV), [128, 32, 8]),
    "slab_layers8": (Frame(slab_layers=8), [32, 8]),
    "slab_layers8_noinv": (Frame(slab_layers=8, **NOINV), [128, 32, 8]),
    "shard_1_of_3": (Frame((512,) * 3, part=dict(shard=1, n_shards=3)), [32, 8]),
    "shard_1_of_3_noinv": (Frame((512,) * 3, part=dict(shard=1, n_shards=3), **NOINV), [32, 8]),
    "block_101": (Frame((512,) * 3, part=BLOCK), [32, 8]),
    "block_101_noinv": (Frame((512,) * 3, part=BLOCK, **NOINV), [32, 8]),
    "block_101_128": (Frame((512,) * 3, part=BLOCK, **NOINV), [128, 32, 8]),
    "more_parts_than_layers": (Frame((256,) * 3, part=dict(iz=1, nz=4)), [128, 32, 8]),
    "tall_block": (Frame((64, 4096, 64), part=dict(ix=1, nx=2), **NOINV), [32, 8]),
    "2d_4096": (Frame((4096, 4096, 0), is3d=False), [128, 16]),
    "2d_inserted_level": (Frame((1024, 1024, 0), is3d=False), [128, 16, 8]),
    "2d_one_level_64": (Frame((256, 256, 0), is3d=False, one_level_64=True), [16]),
    "2d_one_level_plain": (Frame((256, 256, 0), is3d=False), [16]),
    "no_split": (Frame(use_split=False), [128, 32, 8]),
    "regs_300": (Frame(regs=300), [32, 8]),
}


@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_geometry(plans, name):
    f, ts = GEOMETRY[name]
    got = plans[name]
    assert got["status"] == "0" and got["tiles"] == "/".join(str(t) for t in ts)
    sizes = {k: int(v) for k, v in plans["sizes"].items()}
    want = expected_geometry(f, ts, sizes)
    assert {k: got[k] for k in want} == {k: str(v) for k, v in want.items()}


def test_geometry_by_hand(plans):
    # 1024^3, nothing varies along a pixel column: 32 x 32 root tiles of 32^3 in 16 runs of 64; slabs of 16 layers; the front slab alone,
    # ONE group set standing for its 16 layers (z = the slab's first voxel), queued back to front
    g = plans["whole_1024"]
    assert g["slab"] == "512" and g["groups_per_slab"] == "16" and g["qcap"] == "16/16384"
    assert g["roots"].split(";")[0] == "960,64,1,512,16" and g["roots"].split(";")[-1] == "0,64,1,512,16" and g["roots"].count(";") == 15
    # every input varies: 8 x 8 root tiles of 128^3, one run; a group set per layer, the front layer (z = 896) at the back of the list
    g = plans["whole_1024_noinv"]
    assert g["roots"] == ";".join(f"0,64,1,{z},0" for z in range(0, 1024, 128)) and g["groups_per_slab"] == "1"
    # a one-layer frame: one root tile, one slab
    g = plans["whole_64"]
    assert (g["roots"], g["n_slabs"], g["n_layers"], g["slab"], g["qcap"]) == ("0,1,1,0,1", "1", "1", "64", "1/1/64")
    # 200 x 120 x 72: 7 x 4 root tiles of 32^3 in one run, three one-layer slabs
    g = plans["odd_200x120x72_noinv"]
    assert (g["roots_x"], g["roots_y"], g["n_slabs"], g["roots"]) == ("7", "4", "3", "0,28,1,0,0;0,28,1,32,0;0,28,1,64,0")
    assert g["n_footprints"] == str(25 * 15) and g["leaf_cap"] == str(25 * 15 * 4)
    # shard 1 of 3 of 16 x 16 root tiles: tiles 1, 4, .. 253 - 85 of them, as runs of 64 and 21 with stride 3
    assert plans["shard_1_of_3"]["roots"] == "193,21,3,256,8;1,64,3,256,8"
    # block (1, 0, 1) of 2 x 2 x 2: columns x = 8 .. 15, their y = 0 .. 7, the front slab (layers 8 .. 15)
    assert plans["block_101"]["roots"] == ";".join(f"{x * 16},8,1,256,8" for x in range(15, 7, -1)) and plans["block_101"]["slab_lo"] == "1"
    # more parts than layers: nothing to render
    g = plans["more_parts_than_layers"]
    assert (g["roots"], g["groups_per_slab"], g["slab_lo"], g["slab_hi"], g["qcap"]) == ("-", "0", "0", "0", "1/8/256")
    # 128 root tiles in a column: two runs per column and layer
    assert plans["tall_block"]["roots"] == "192,64,1,0,0;128,64,1,0,0;192,64,1,32,0;128,64,1,32,0" and plans["tall_block"]["groups_per_slab"] == "2"
    # 2D: one group set; the one-level pass of 256^2 takes the 64-lane tile stage when told to
    assert plans["2d_4096"]["groups_per_slab"] == "16" and plans["2d_4096"]["qcap"] == "16/1024" and plans["2d_4096"]["leaf_cap"] == str(256 * 256)
    assert plans["2d_inserted_level"]["qcap"] == "1/64/4096" and plans["2d_inserted_level"]["tl"] == "64"
    assert plans["2d_one_level_64"]["tl"] == "64" and plans["2d_one_level_64"]["qcap"] == "4"
    assert plans["2d_one_level_plain"]["tl"] == "16" and plans["2d_one_level_plain"]["qcap"] == "16"


def paths(**kw):
    base = dict(full=0, split=1, asm_points=1, asm_points_t=0, asm_normals=1, asm_tiles=1, asm_tiles_t=0, hip_tiles_unasked=0, prune1=1, exp_levels=1, groups=1, prune2=1,
                leaf_asm_regs=40, norm_asm_regs=40, n_tgroups=16, big_hbm=0, zrep=1)
    base.update(kw)
    return base


# the root tape at 0 .. 6363, the 16 groups of 400 ops behind it, 16 words of slack after each
GROUPS_END = 6363 + 16 + 16 * (400 + 16)
NO_GROUPS = dict(groups=0, prune2=0, n_tgroups=0, arena_head=6363, arena_root_end=6363, arena_frame_end=6363)
PATHS = {
    "whole_1024": paths(arena_head=GROUPS_END, arena_root_end=GROUPS_END, arena_frame_end=GROUPS_END, smooth=0),
    "whole_1024_noinv": paths(zrep=0, arena_head=GROUPS_END),
    "no_zrep1": paths(zrep=0), "no_zrep2": paths(zrep=1), "no_zrep3": paths(zrep=1),
    # 2048^3: 256 root tiles, 4 groups for the front slab; all 16 layers are 64 groups = 4 096 root tiles, beyond the linked prune's two rounds
    "whole_2048": paths(), "whole_2048_noinv": paths(zrep=0, prune2=0),
    # 2D: no leaf kernels of the 3D kind, the root level exports its choices
    "2d_4096": paths(asm_points=0, asm_normals=0, leaf_asm_regs=32, norm_asm_regs=32, zrep=0),
    "2d_one_level_64": paths(asm_points=0, asm_normals=0, leaf_asm_regs=32, norm_asm_regs=32, zrep=0),
    # 16 lanes: the monolithic tile kernel
    "2d_one_level_plain": paths(asm_points=0, asm_normals=0, leaf_asm_regs=32, norm_asm_regs=32, zrep=0, split=0, asm_tiles=0, prune1=0, **NO_GROUPS),
    # more than 128 registers: the HIP tile kernels, counted; 140 registers still fit LDS, 200 and 300 do not (the gradients' 16 bytes x 64 lanes per register)
    "regs_140": paths(asm_tiles=0, hip_tiles_unasked=1, prune1=0, big_hbm=0, **NO_GROUPS),
    "regs_200": paths(asm_tiles=0, hip_tiles_unasked=1, prune1=0, big_hbm=1, **NO_GROUPS),
    "regs_300": paths(asm_tiles=0, hip_tiles_unasked=1, prune1=0, big_hbm=1, **NO_GROUPS),
    "groups_do_not_fit": paths(**NO_GROUPS),
    # transcendental opcodes: the *_t kernels, which have no export mode; a modulo keeps the C++ normals kernel
    "transcendental": paths(full=1, asm_points_t=1, asm_tiles_t=1, prune1=0, leaf_asm_regs=44, **NO_GROUPS),
    "transcendental_mod": paths(full=1, asm_points_t=1, asm_tiles_t=1, prune1=0, leaf_asm_regs=44, asm_normals=0, norm_asm_regs=32, **NO_GROUPS),
    "no_asm": paths(asm_points=0, asm_normals=0, asm_tiles=0, prune1=0, leaf_asm_regs=32, norm_asm_regs=32, **NO_GROUPS),
    "no_split": paths(split=0, asm_tiles=0, prune1=0, zrep=0, **NO_GROUPS),
}


@pytest.mark.parametrize("name", sorted(PATHS))
def test_kernel_paths(plans, name):
    got, want = plans[name], PATHS[name]
    assert got["status"] == "0"
    assert {k: got[k] for k in want} == {k: str(v) for k, v in want.items()}


def test_lds_budgets(plans):
    g = plans["whole_1024"]
    want = dict(lds_big=tiles_lds(72, 3000, 64), lds_small=tiles_lds(32, 256, 64), lds_mid=tiles_lds(64, 768, 64), lds_points_big=72 * 64 * 4, lds_normals_big=72 * 64 * 16,
                lds_normals_small=32 * 64 * 16, lds_group=tiles_lds(40, 190, 64))
    assert {k: g[k] for k in want} == {k: str(v) for k, v in want.items()}
    assert (want["lds_big"], want["lds_small"], want["lds_mid"]) == (89856, 22784, 49408)
    # the linked prune: four children's areas and the root chain's 63 entries
    wave = 1024 + 256 + (3000 * 2 + 15) // 16 * 16 + 1280 * 15 + 64
    assert g["lds_prune2"] == str(4 * wave + (63 * 4 + 15) // 16 * 16) and 4 * wave <= LDS_MAX
    # the group buffers: one block per root group
    assert (g["b_tvals"], g["b_topch"], g["b_chwr"]) == (str(16 * 64 * 64 * 8), str(16 * 63 * 64), str(16 * 16 * ceil_div(3000, 16) * 64 * 4 + 256))
    # choice words of the exported level: 16 groups x 16 term groups slots; slots for the largest level
    assert g["b_chw"] == f"{256 * 16 * 256}/{256 * ceil_div(3000, 16) * 256}"
    sizes = {k: int(v) for k, v in plans["sizes"].items()}
    assert g["slot_cap"] == "16384" and g["b_slots"] == str(16384 * sizes["slot"])
    assert g["arena_cap"] == str((128 << 20) // 8 - 64)


def test_register_file_in_hbm(plans):
    for name, n_cu in (("regs_300", 256), ("regs_300_few_cus", 8)):
        g = plans[name]
        stride = max(tiles_lds(300, 3000, 64), 300 * 64 * 16, 300 * 64 * 4)
        assert stride > LDS_MAX
        stride = ceil_div(stride, 256) * 256
        waves = max(64, min(4 * n_cu, (1 << 30) // stride))
        assert g["big_hbm"] == "1" and g["stride"] == str(stride) and int(g["stride"]) % 256 == 0
        assert g["hbm_waves"] == str(waves) and 64 <= waves <= max(64, 4 * n_cu) and g["b_gscratch"] == str(waves * stride)
        assert (g["lds_big"], g["lds_points_big"], g["lds_normals_big"]) == ("0", "0", "0")
    assert plans["regs_300"]["hbm_waves"] == "1024" and plans["regs_300_few_cus"]["hbm_waves"] == "64"
    assert plans["whole_1024"]["b_gscratch"] == "0" and plans["whole_1024"]["stride"] == "0"


REFUSALS = {
    "refuse_outputs": (5, "shape tapes have exactly one output"),      # (before the tile list is looked at)
    "refuse_no_levels": (6, "1..8 tile levels supported"),
    "refuse_nine_levels": (6, "1..8 tile levels supported"),
    "refuse_ascending": (6, "bad tile size list"),
    "refuse_not_a_multiple": (6, "bad tile size list"),
    "refuse_fanout": (6, "tile fan-out above 64 children"),
    "refuse_3d_fanout": (6, "tile fan-out above 64 children"),
    "refuse_leaves": (6, "3D leaves must be 8^3 (one 8x8 footprint per wave)"),      # (before the tape's registers)
    "refuse_registers": (6, "renders support up to 4095 registers"),                # (before its ops)
    "refuse_ops": (6, "renders support tapes of up to 2^24 ops"),                   # (before its register file)
    "refuse_register_file": (6, "register file too large"),                         # (before the image)
    "refuse_65536_wide": (6, "3D renders support images up to 65535 x 65535"),      # (before the arena)
    "refuse_65536_high": (6, "3D renders support images up to 65535 x 65535"),
    "refuse_2p29_pixels": (6, "3D renders support images of fewer than 2^29 pixels"),
    "refuse_arena": (6, "tape larger than the arena"),
    "refuse_arena_2d": (6, "tape larger than the arena"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(plans, name):
    status, text = REFUSALS[name]
    assert plans[name] == {"status": str(status), "msg": text.replace(" ", "_")}


def test_limits_are_inclusive_where_they_should_be(plans):
    assert plans["accept_4095_registers"]["status"] == "0" and plans["accept_arena"]["status"] == "0"
