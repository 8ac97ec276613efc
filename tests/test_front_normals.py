"""Which 3D frames run their normals kernels (fidget_amd/csrc/frame_schedule.hpp FrameSchedule::normals_on): not a whole front-slab-only
frame - no tape of it reads anything that changes along a pixel column, every hit lies in the volume's top voxel layer and k_finish3d writes
(0, 0, 1, depth) for it whatever its normal.  Built for the host (tests/host_build/front_normals_host.cpp) with
-fsanitize=address,undefined and run on its own: named frames, and a sweep over all combinations of the schedule inputs.  No GPU.

Line format: `name: key=value ...`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "front_normals_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")


@pytest.fixture(scope="module")
def host():
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "front_normals_host")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("frame_schedule.hpp", "frame_plan.hpp", "render_state.h", "tape_format.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-I", CSRC, SRC, "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    lines = {}
    for line in res.stdout.splitlines():
        name, _, rest = line.partition(":")
        lines[name] = rest.strip() if name == "sweep" else dict(kv.split("=", 1) for kv in rest.split())
    return res, lines


def check(line, **want):
    got = {k: line[k] for k in want}
    assert got == {k: str(v) for k, v in want.items()}


def test_the_host_program_ends_clean_under_the_sanitizers(host):
    res, _ = host
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]


def test_whole_front_slab_frames(host):
    """every arrangement and size of a whole frame without z: one slab rendered, no normals launch; the one launch that stays is
    k_rare_leaves3d, which has the POINTS of the leaves beyond the leaf kernel's file (a root tape of 72 registers, rare mode, by the list)"""
    _, f = host
    for name in ("default_queued", "default_alone", "default_host_output", "default_profiling", "default_lane", "size_64", "size_128", "size_256", "size_512", "size_2048",
                 "size_96x64x40"):
        check(f[name], front_only=1, whole=1, rendered=1, clamped=1, normals_on=0, normals_launches=0, rare_leaves=1, rare_leaves_launch=1)
    # a tape within the leaf kernel's file, transcendental opcodes (files of 44 / 40: k_classify3d's blocks have the points), a frame told of
    # a large tape, the leaf stage by the table, the HIP leaf kernels: nothing at all behind the leaf kernel
    for name in ("small_tape", "transcendental", "default_rare_seen", "default_by_table", "default_no_asm"):
        check(f[name], front_only=1, whole=1, clamped=1, normals_on=0, normals_launches=0, rare_leaves=0, rare_leaves_launch=0)


def test_parts_of_a_frame_and_frames_with_z_keep_their_normals(host):
    _, f = host
    # a shard, a block of columns, the front and the back z-block of a frame without z: front slab of the part only, but not the whole frame
    for name in ("shard", "block_xy", "block_z_front", "block_z_back"):
        check(f[name], front_only=1, whole=0, clamped=0, normals_on=1, normals_launches=1, rare_leaves_launch=1)
    # every slab rendered (no_zrep 3), the short cuts off, a camera tilted about x, a tape that reads z
    for name in ("every_slab", "no_column_inv", "tilted", "reads_z"):
        check(f[name], front_only=0, whole=1, rendered=2, clamped=0, normals_on=1, normals_launches=1)


def test_the_rule_over_all_schedule_inputs(host):
    # 4 sizes x 256 option bits x 4 column walks x 4 no_zrep values x 4 parts x 4 tapes: no normals exactly where every hit is clamped, never
    # in a part; k_rare_leaves3d launched wherever the schedule has it; and, normals aside, no schedule differs from the same frame's as a part
    _, f = host
    n, off, rest = f["sweep"].split(",", 2)
    assert n == "262144 schedules" and int(off.split()[0]) > 1000
    assert rest.strip() == "0 against the rule, 0 large leaves without their points, 0 moved otherwise"
