"""The schedule of a 3D frame (fidget_amd/csrc/frame_schedule.hpp: which stream every stage goes to, which launches exist, how the slabs
are arranged - a pure function of facts) built for the host (tests/host_build/frame_schedule_host.cpp) and pinned for named frames of
prospero.vm's kind.  A change to which launches a frame makes, or where, shows as a diff of the tables below.  No GPU.

Line format: `name: key=value ...`; a level reads PATH+launches@role-of-what-follows-fh_tiles_v64."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "frame_schedule_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")


@pytest.fixture(scope="module")
def schedules():
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "frame_schedule_host")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("frame_schedule.hpp", "frame_plan.hpp", "render_state.h", "tape_format.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        # (plain g++, no HIP headers: the schedule touches no device)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-I", CSRC, SRC, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    frames = {}
    for line in res.stdout.splitlines():
        name, _, rest = line.partition(":")
        frames[name] = dict(kv.split("=", 1) for kv in rest.split()) if name != "sweep" else rest.strip()
    return res.returncode, frames


def check(frame, **want):
    got = {k: frame[k] for k in want}
    assert got == {k: str(v) for k, v in want.items()}


# the three arrangements of a queued frame, and the same frames alone
DEFAULT = dict(tiles="32/8", slab=512, slabs=2, rendered=1, NC=2, walk="LIST", by_list=1, table_words=0, reset_blocks=1, rare=1,
               L0="GROUPS+exp@{root}", L1="ASM+v32+rare@SIDE")
GENERAL = dict(tiles="128/32/8", slab=512, slabs=2, rendered=2, NC=2, walk="COLUMNS", g=2, by_list=0, table_words=1048576, reset_blocks=1024, rare=1,
               L2="ASM+v32+rare@SIDE")
BIG = dict(tiles="128/32/8", slab=512, slabs=4, rendered=1, NC=4, walk="LIST", by_list=1, table_words=0, rare=1)


def test_no_input_varies_along_a_column_1024(schedules):
    _, f = schedules
    # queued: the root level on the pre-pass and the tail stream in turn; flags + mark + fork at the head of the tile chain on the side stream;
    # lists, leaf kernel (by the list) and normals on the caller's stream, which waits for the tile chain's event and nothing else
    for name, root in (("default_queued", "PRE"), ("default_queued_turn", "TAIL")):
        want = dict(DEFAULT, L0=DEFAULT["L0"].format(root=root))
        check(f[name], fpipe=1, lone=0, alt_pre=1, takes_turn=1, root=root, fork_on="SIDE", tiles_on="SIDE", lists="CALLER", leaf="CALLER", normals="CALLER",
              pipe=1, tiles_first=0, fork_to_side=0, fork_to_tail=0, ev_pre=0, pre_implied=1, aux_edge=0, list_waves=6208, **want)
    # alone: upload and root level on the caller's stream, no turn taken; the tile chain still on the side stream
    check(f["default_alone"], fpipe=1, lone=1, alt_pre=1, takes_turn=0, root="CALLER", fork_on="CALLER", tiles_on="SIDE", lists="CALLER", leaf="CALLER", normals="CALLER",
          fork_to_side=1, ev_pre=0, pre_implied=0, aux_edge=0, **dict(DEFAULT, L0="GROUPS+exp@CALLER"))


def test_general_path_1024(schedules):
    _, f = schedules
    # queued: root level on the pre-pass stream, level 1 on the side stream (ev_l0: a hop), tile chains on the side stream, lists and normals on
    # the tail stream around the leaf kernel on the caller's; the leaf kernel by groups of 2^column_group layers
    check(f["general_queued"], fpipe=1, lone=0, alt_pre=0, root="PRE", l1_flags="SIDE", l1="SIDE", fork_on="SIDE", tiles_on="SIDE", lists="TAIL", leaf="CALLER", normals="TAIL",
          pipe=1, tiles_first=0, fork_to_side=0, ev_pre=1, pre_implied=0, aux_edge=1, L0="GROUPS+exp@PRE", L1="ASM+v64both+rest@SIDE", **GENERAL)
    # alone: both coarse levels on the caller's stream, the big-list launches of level 1 forked to the side stream
    check(f["general_alone"], fpipe=1, lone=1, root="CALLER", l1="CALLER", fork_on="CALLER", tiles_on="SIDE", lists="TAIL", leaf="CALLER", normals="TAIL",
          fork_to_side=1, ev_pre=0, aux_edge=1, L0="GROUPS+exp@CALLER", L1="ASM+v32+v64+rest+fork@CALLER", **GENERAL)


def test_no_input_varies_along_a_column_2048(schedules):
    _, f = schedules
    # 4 096 children of 32^3: over 2 048 and the image over 512 -> 128 / 32 / 8; four slabs, the front one rendered, four slab contexts.
    # Level 1's flags at the end of the root level, its evaluate on the side stream, what follows fh_tiles_v64 on the tail stream; every tile
    # chain there before the first slab's tail work; lists and normals on the caller's stream
    check(f["big_queued"], fpipe=1, lone=0, alt_pre=0, root="PRE", l1_flags="PRE", l1="SIDE", fork_on="TAIL", tiles_on="TAIL", lists="CALLER", leaf="CALLER", normals="CALLER",
          pipe=1, tiles_first=1, fork_to_side=1, fork_to_tail=1, ev_pre=1, pre_implied=0, aux_edge=0, L0="GROUPS+exp@PRE", L1="ASM+v64both+rest@TAIL", L2="ASM+v32+rare@TAIL", **BIG)
    check(f["big_alone"], lone=1, root="CALLER", l1="CALLER", fork_on="CALLER", tiles_on="SIDE", tiles_first=0, lists="TAIL", normals="TAIL", aux_edge=1,
          L1="ASM+v32+v64+rest+fork@CALLER", L2="ASM+v32+rare@SIDE", **BIG)


@pytest.mark.parametrize("kind", ["default", "general", "big"])
def test_one_stream_arrangements(schedules, kind):
    _, f = schedules
    # no_pipeline (and a lane, which is a child context under no_pipeline), a profiled frame: one stream, one slab context, no edge
    for variant in ("no_pipeline", "lane", "profiling"):
        check(f[f"{kind}_{variant}"], fpipe=0, pipe=0, NC=1, root="CALLER", l1_flags="CALLER", l1="CALLER", fork_on="CALLER", tiles_on="CALLER", lists="CALLER",
              leaf="CALLER", normals="CALLER", fork_to_side=0, fork_to_tail=0, ev_pre=0, pre_implied=0, aux_edge=0, tiles_first=0, takes_turn=0)
    # a host output buffer: no frame pipelining (coarse levels on the caller's stream), the slabs still pipelined over their contexts
    check(f[f"{kind}_host_output"], fpipe=0, pipe=1, root="CALLER", fork_on="CALLER", tiles_on="SIDE", lists="TAIL", leaf="CALLER", normals="TAIL", fork_to_side=1, ev_pre=0,
          aux_edge=1)


@pytest.mark.parametrize("kind,last", [("default", "L1"), ("general", "L2"), ("big", "L2")])
def test_rare_mode_off_puts_the_launches_back(schedules, kind, last):
    _, f = schedules
    role = f[f"{kind}_queued"]["tiles_on"]
    assert f[f"{kind}_queued"][last] == f"ASM+v32+rare@{role}"
    check(f[f"{kind}_rare_seen"], rare=0, **{last: f"ASM+v32+v64+rest@{role}"})
    # nothing else moves
    same = [k for k in f[f"{kind}_queued"] if k not in ("rare", last)]
    assert {k: f[f"{kind}_rare_seen"][k] for k in same} == {k: f[f"{kind}_queued"][k] for k in same}


def test_column_walk_option(schedules):
    _, f = schedules
    # 0 never by columns: groups of 2^column_group layers; 2 always by columns; 3 the sparse-column frames by the table; 1 (default) those by the list
    for kind, sparse in (("default", True), ("general", False), ("big", True)):
        check(f[f"{kind}_column_walk0"], walk="COLUMNS", g=2, by_list=0)
        check(f[f"{kind}_column_walk2"], walk="COLUMNS", g=6, by_list=0)
        check(f[f"{kind}_column_walk3"], walk="COLUMNS", g=6 if sparse else 2, by_list=0)
        assert f[f"{kind}_column_walk3"]["table_words"] != "0"
        # the streams do not depend on the walk
        for k in ("root", "l1", "fork_on", "tiles_on", "lists", "leaf", "normals"):
            assert f[f"{kind}_column_walk0"][k] == f[f"{kind}_queued"][k]


def test_every_stage_behind_another_role_has_an_edge(schedules):
    # sizes 64 .. 2048, the options above, queued / alone, both turns: at most the four roles, the leaf kernel and k_finish3d on the caller's
    # stream, and every stage that follows another role's work waits for an event of it (or is on the same role)
    rc, f = schedules
    assert f["sweep"] == "24576 schedules, 0 violations" and rc == 0
