"""FHIP_MESH_TIMES on the device: with the variable set, the bitmap and mesh calls wait for the stream after every pass and print the
pass's time on stderr.  Two things are held here, per call and depth: the results are the very ones of the same call without the
variable, and the lines on stderr are the sequence recorded in tests/golden/mesh_times_labels.json - prefix, label and order, the time
at the end of a line (`[0-9.]+ (s|ms)$`) stripped.  The golden file was recorded from the library as it stood before the pass timers
became one struct (PassTimes, capi_mesh_util.hpp); it is data, not derived from the code it checks.

The bitmap is a sphere of radius 0.9 without its (+, +, +) octant: depth 0 is one brick - one word, one block of every scan and grid -,
depth 2 has 64 bricks, depth 5 (128^3) is the smallest grid whose distance columns do not fit LDS and runs distance and thickness alone.
Every result compared is an integer, or a float that is exact: the boundary mesh's vertices are multiples of 2 / N, so the shells' volume
and area sums are exact in float64 in any order of arrival."""
import functools
import json
import os
import re

import numpy as np
import pytest

import fidget_amd as F
import voxels_ref as V

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_times_labels.json")
TIME = re.compile(r"\s+[0-9.]+ (s|ms)$")


@functools.lru_cache(maxsize=None)
def bricks_of(depth):
    N = 4 << depth
    c = (np.arange(N) * 2 + 1 - N) / N          # the voxels' centres in [-1, 1]
    x, y, z = np.meshgrid(c, c, c, indexing="ij")
    inside = (x * x + y * y + z * z < 0.81) & ~((x > 0) & (y > 0) & (z > 0))
    assert inside.any() and not inside.all()
    b = V.pack(inside)
    b.setflags(write=False)
    return b


def voxels(depth):
    return F.Voxels(F.default_context(), np.array(bricks_of(depth)), depth, None)


def _components(connectivity, complement):
    def call(v):
        c = v.components(connectivity, complement)
        return [c.count, c.nodes, c.n, c.sizes, c.seeds, c.lo, c.hi, c.border, c.label_slices(0, v.grid)]
    return voxels, call


def _field(d):
    return [d.max_squared, d.argmax, d.n, d.slices(0, d.grid)]


def _thickness(t):
    return _field(t) + [t.min_squared, t.argmin, t.centres, t.balls]


def _mesh_of(depth):
    return voxels(depth).mesh()


def _voxelize_mesh(mesh_and_depth):
    v = F.voxelize_mesh(*mesh_and_depth)
    return [v.bricks, sorted(v.mesh_info.items())]


def _topology(m):
    t = F.mesh_topology(m)
    return [sorted(t.counts.items()), t.vertices, t.triangles, t.triangle_shell] + [t.shells[k] for k in sorted(t.shells)]


# name -> (what is made before, without the variable; the call under test, whose results are a flat list)
CALLS = {
    "components6": _components(6, False),
    "components26-complement": _components(26, True),
    "distance": (voxels, lambda v: _field(v.distance())),
    "thickness": (lambda depth: voxels(depth).distance(complement=True), lambda d: _thickness(d.thickness())),
    "mesh": (voxels, lambda v: (lambda m: [m.vertices, m.triangles])(v.mesh())),
    "voxelize_mesh": (lambda depth: (_mesh_of(depth), depth), _voxelize_mesh),
    "mesh_topology": (_mesh_of, _topology),
}
CASES = [(name, depth) for name in CALLS for depth in ((0, 2, 5) if name in ("distance", "thickness") else (0, 2))]


def run(name, depth, times):
    """the results of one call, with or without FHIP_MESH_TIMES set around it (the library reads it per call)"""
    before, call = CALLS[name]
    arg = before(depth)
    if not times:
        return call(arg)
    os.environ["FHIP_MESH_TIMES"] = "1"
    try:
        return call(arg)
    finally:
        del os.environ["FHIP_MESH_TIMES"]


def labels(stderr):
    """the library's lines without the time they end in"""
    return [TIME.sub("", line) for line in stderr.splitlines() if line.startswith("fhip ")]


def same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(a, b)
    return a == b


@pytest.mark.parametrize("name,depth", CASES, ids=[f"{n}-d{d}" for n, d in CASES])
def test_times_change_nothing_and_print_the_recorded_lines(name, depth, capfd):
    with open(GOLDEN) as f:
        golden = json.load(f)
    plain = run(name, depth, False)
    capfd.readouterr()
    timed = run(name, depth, True)
    err = capfd.readouterr().err
    assert len(plain) == len(timed) and all(same(a, b) for a, b in zip(plain, timed))
    lines = [line for line in err.splitlines() if line.startswith("fhip ")]
    print("\n".join(lines))
    assert lines and all(TIME.search(line) or "balls painted" in line for line in lines)          # (the thickness summary carries no time)
    assert labels(err) == golden[f"{name}-d{depth}"]
