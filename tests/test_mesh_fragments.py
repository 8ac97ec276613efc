"""The layout of the mesh path's sources (tools/src_hash.py), read from the `#include "..."` lines that lead from
fidget_amd/csrc/capi.hip: every file reached is in `_SOURCES` - that list decides whether build() finds the library stale, so a missing
name means a stale library; every file of MESH_ONLY exists and is reached through the mesh path's gates alone; capi_mesh.hpp is the one
file that includes the C ABI's mesh fragments, capi_mesh_util.hpp among them exactly once; and the copies that capi_mesh_util.hpp
replaced have not come back."""
import glob
import os
import re
import sys

import fidget_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from src_hash import MESH_ONLY  # noqa: E402

CSRC = os.path.join(ROOT, "fidget_amd", "csrc")
INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)
# The ways into the mesh path: the C ABI's fragment and the kernels' file - and host_mesh.hpp, the host's half of the mesher, which
# capi.hip includes itself (with mesh_collapse.hpp and mesh_qef.hpp behind it)
GATES = ("capi_mesh.hpp", "mesh.hip", "host_mesh.hpp")


def includes(path):
    with open(path) as f:
        return [os.path.normpath(os.path.join(os.path.dirname(path), name)) for name in INCLUDE.findall(f.read())]


def reached(start, barred=()):
    """the files the quoted includes lead to from `start`, not going through the `barred` ones"""
    seen, todo = set(), [start]
    while todo:
        f = todo.pop()
        if f in seen or os.path.basename(f) in barred:
            continue
        assert os.path.isfile(f), f"{f} is included and does not exist"
        seen.add(f)
        todo += includes(f)
    return seen


def test_every_included_file_is_a_source_of_the_build():
    sources = {os.path.normpath(os.path.join(CSRC, s)) for s in F._SOURCES}
    missing = sorted(os.path.relpath(f, CSRC) for f in reached(os.path.join(CSRC, "capi.hip")) - sources)
    assert not missing, f"included from capi.hip but not in fidget_amd._SOURCES: {missing}"


def test_mesh_only_files_exist_and_lie_behind_the_gates():
    for name in MESH_ONLY:
        assert os.path.isfile(os.path.join(CSRC, name)), name
    all_files = {os.path.basename(f) for f in reached(os.path.join(CSRC, "capi.hip"))}
    assert set(MESH_ONLY) <= all_files, sorted(set(MESH_ONLY) - all_files)
    outside = {os.path.basename(f) for f in reached(os.path.join(CSRC, "capi.hip"), barred=GATES)}
    assert not outside & set(MESH_ONLY), sorted(outside & set(MESH_ONLY))


def test_capi_mesh_hpp_is_the_one_list_of_the_fragments():
    fragments = {n for n in MESH_ONLY if n.startswith("capi_") and n != "capi_mesh.hpp"}
    assert "capi_mesh_util.hpp" in fragments
    count = dict.fromkeys(fragments, 0)
    for f in reached(os.path.join(CSRC, "capi.hip")):
        for inc in includes(f):
            if os.path.basename(inc) in fragments:
                assert os.path.basename(f) == "capi_mesh.hpp", f"{os.path.basename(f)} includes {os.path.basename(inc)}"
                count[os.path.basename(inc)] += 1
    assert all(n == 1 for n in count.values()), count
    # the shared helpers stand before everything that uses them
    first = INCLUDE.findall(open(os.path.join(CSRC, "capi_mesh.hpp")).read())[:2]
    assert first == ["mesh_split.hpp", "capi_mesh_util.hpp"], first


def test_the_copies_have_not_come_back():
    for path in glob.glob(os.path.join(CSRC, "**", "*"), recursive=True):
        if os.path.isfile(path) and path.rsplit(".", 1)[-1] in ("hip", "hpp", "h", "cpp", "py"):
            text = open(path, errors="replace").read()
            for gone in ("auto mark = [&]", "contours_to_host", "topology_to_host"):
                assert gone not in text, f"{gone!r} in {os.path.relpath(path, CSRC)}"
