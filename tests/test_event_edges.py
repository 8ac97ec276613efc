"""Which events a 3D frame records (fidget_amd/csrc/frame_schedule.hpp: rec_fork, records_leaves; the staging slot's guard) - decided by
the schedule, an event only where somebody waits for it - built for the host (tests/host_build/event_edges_host.cpp, which models the
driver's waits) and pinned for named frames of prospero.vm's kind.  The host program is built with -fsanitize=address,undefined and run
on its own: it also drives the staging ring and its guard through 20 frames with early exits in the middle.  No GPU.

Line format: `name: key=value ...`; leaves / waited: the slabs (in the order rendered) whose ev_leaves is recorded / waited for."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "event_edges_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")


@pytest.fixture(scope="module")
def edges():
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "event_edges_host")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("frame_schedule.hpp", "frame_plan.hpp", "render_state.h", "tape_format.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I", CSRC, SRC, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    frames = {}
    for line in res.stdout.splitlines():
        name, _, rest = line.partition(":")
        frames[name] = rest.strip() if name in ("sweep", "staging") else dict(kv.split("=", 1) for kv in rest.split())
    return res, frames


def check(frame, **want):
    got = {k: frame[k] for k in want}
    assert got == {k: str(v) for k, v in want.items()}


def test_the_host_program_ends_clean_under_the_sanitizers(edges):
    res, _ = edges
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]


def test_every_record_has_a_waiter_and_every_wait_its_record(edges):
    # 6 sizes x 256 option bits x 4 column walks x 4 no_zrep values x 1..4 slab contexts
    _, f = edges
    assert f["sweep"].startswith("98304 schedules, 0 violations, ")
    assert "VIOLATION" not in f


def test_the_rule_recorded_whenever_pipe_fails_the_same_check(edges):
    # what the driver did before: ev_leaves for every slab and ev_fork whenever the slabs are pipelined
    _, f = edges
    assert int(f["sweep"].split(",")[2].split()[0]) > 0
    for name in ("default_queued", "default_queued_turn", "default_alone"):
        assert int(f[name]["parents_rule"]) > 0 and f[name]["violations"] == "0"


def test_front_slab_frames_record_no_ev_leaves(edges):
    _, f = edges
    for name in ("default_queued", "default_queued_turn", "default_alone"):
        check(f[name], rendered=1, NC=2, pipe=1, aux_edge=0, leaves="-", waited="-")
    # a frame without slab contexts (profiled: one stream) records nothing either
    check(f["default_profiling"], pipe=0, leaves="-", rec_fork=0)
    # with a host output the normals run on the tail stream: the caller's stream waits for the one slab's event
    check(f["default_host_output"], aux_edge=1, leaves="0", waited="0")


def test_ev_fork_only_where_a_stream_waits_for_it(edges):
    _, f = edges
    # queued: the fork rides at the head of the tile chain on the side stream, nobody waits
    check(f["default_queued"], fork_to_side=0, fork_to_tail=0, rec_fork=0)
    check(f["default_queued_turn"], rec_fork=0)
    check(f["general_queued"], rec_fork=0)
    # alone: the coarse levels on the caller's stream, the tile chain on the side stream waits for the fork
    check(f["default_alone"], fork_to_side=1, rec_fork=1)
    check(f["general_alone"], fork_to_side=1, rec_fork=1)
    check(f["big_queued"], fork_to_side=1, fork_to_tail=1, rec_fork=1)


def test_general_queued_records_the_last_slab_only(edges):
    _, f = edges
    check(f["general_queued"], rendered=2, NC=2, aux_edge=1, leaves="1", waited="1")


@pytest.mark.parametrize("nc,want", [(1, "0,1,2,3"), (2, "0,1,3"), (3, "0,3")])
def test_more_slabs_than_slab_contexts(edges, nc, want):
    # four slabs rendered: all but the last NC (their contexts are taken again), plus the last slab where the normals run on the tail stream
    _, f = edges
    for kind in ("general_queued", "host_output", "default_queued"):
        check(f[f"slabs4_nc{nc}_{kind}"], rendered=4, NC=nc, aux_edge=1, leaves=want, waited=want, violations=0)


def test_one_launch_for_the_rare_leaves_of_a_by_list_frame(edges):
    # rare mode + by the list + a root tape beyond the leaf kernel's file (72 registers): k_rare_leaves3d for points and normals; told of
    # a large tape, by the table, or no rare mode at all: the launches as they were
    _, f = edges
    for name in ("default_queued", "default_queued_turn", "default_alone", "default_host_output", "default_profiling", "big_queued"):
        check(f[name], rare=1, by_list=1, rare_leaves=1)
    check(f["default_rare_seen"], rare=0, by_list=1, rare_leaves=0)
    check(f["default_column_walk3"], rare=1, by_list=0, rare_leaves=0)
    check(f["general_queued"], rare=1, by_list=0, rare_leaves=0)


def test_staging_ring_guards_every_slot_on_every_way_out(edges):
    # 20 frames over the ring of 8: a cancelled frame, a failed launch and a frame refused before its launch in the middle; a slot is
    # written again only behind a record that lies behind its last read; one record per frame that queued k_frame_begin
    _, f = edges
    assert f["staging"] == "frames=20 armed=19 records=19 violations=0"
