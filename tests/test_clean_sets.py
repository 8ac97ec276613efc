"""The clean-buffer-set rule (fidget_amd/csrc/frame_plan.hpp: when a 3D frame may skip the clears of z-buffer, normals and min-depth pyramid
because the set's last frame left them zeroed, and which frames leave a record) built for the host (tests/host_build/clean_sets_host.cpp)
and held case by case.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_build", "clean_sets_host.cpp")
CSRC = os.path.join(ROOT, "fidget_amd", "csrc")

PIX, MIND = 1024 * 1024, 1024 + 16384      # a 1024^2 image with 32 / 8 tiles


@pytest.fixture(scope="module")
def rule():
    out = os.path.join(ROOT, "tests", "host_build", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "clean_sets_host")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("frame_plan.hpp", "render_state.h", "tape_format.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Wno-unused-variable", "-I", CSRC, SRC, "-o", exe])

    def run(left=(1, PIX, MIND), want=(PIX, MIND), out_is_device=1, profiling=0, queued_whole=1):
        args = [str(int(v)) for v in (*left, *want, out_is_device, profiling, queued_whole)]
        line = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout.strip()
        return {k: int(v) for k, v in (kv.split("=") for kv in line.split())}
    return run


def test_matching_record_skips(rule):
    r = rule()
    assert r["skip"] == 1 and r["cleans"] == 1
    assert (r["valid"], r["pixels"], r["mind_words"]) == (1, PIX, MIND)


@pytest.mark.parametrize("left", [(1, PIX // 4, MIND), (1, PIX * 4, MIND), (1, PIX, MIND + 64), (1, PIX, MIND - 1), (1, 0, 0)])
def test_each_mismatching_field_clears(rule, left):
    r = rule(left=left)
    assert r["skip"] == 0
    assert (r["valid"], r["pixels"], r["mind_words"]) == (1, PIX, MIND)      # ... and the record is rewritten for this frame


def test_first_use_clears(rule):
    assert rule(left=(0, 0, 0))["skip"] == 0
    assert rule(left=(0, PIX, MIND))["skip"] == 0      # (a dropped record with the right numbers is still no record)


@pytest.mark.parametrize("kind", [dict(queued_whole=0), dict(out_is_device=0), dict(profiling=1), dict(out_is_device=0, profiling=1)])
def test_frames_that_leave_no_record(rule, kind):
    """cancelled or failed half way, image to the host, profiled: the next frame of the set - whatever its size - clears everything"""
    r = rule(**kind)
    assert r["valid"] == 0
    if "queued_whole" not in kind:
        assert r["cleans"] == 0
    assert rule(left=(r["valid"], r["pixels"], r["mind_words"]))["skip"] == 0


def test_a_clean_set_serves_a_frame_that_leaves_none(rule):
    """a host-output frame on a set left clean may skip its clears like any other; it is what comes AFTER it that clears"""
    assert rule(out_is_device=0)["skip"] == 1
