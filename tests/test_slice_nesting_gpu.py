"""fhip_slices_nesting on the device against slice_nesting_ref.py, run on the MeshSlices' own arrays - the reference walks every loop's
polygon for every leader and knows no bands and no hit lists.  Every array and every count is compared with np.array_equal; the
reference adds region_area2 from the device's area2 in ascending child id, so that is equal by its bits too.  The hand-made cases of
slice_nesting_cases.py, on which exact rational arithmetic confirms the reference's hit counts; the field under every number of bands;
build_mesh of a model; a bitmap's own mesh against the bitmap's nesting; empty results and refusals; two runs, the device views, the
regions, the SVG."""
import ctypes as C
import functools
import re
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import fidget_amd as F
import slice_nesting_cases as K
import slice_nesting_ref as NR
import voxels_ref as V
from conftest import model_path
from test_slice_nesting import HAND_MADE, mesh_of

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
LOOP_ARRAYS = ("parent", "depth", "n_children")


@functools.lru_cache(maxsize=None)
def slices_of(name):
    """-> MeshSlices of a case of test_slice_nesting.mesh_of"""
    tri, zs = mesh_of(name)
    return F.mesh_slices(tri, zs)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the reference's nesting of the device's slices - the same for every number of bands"""
    res = NR.from_device(slices_of(name))
    return NR.nesting(res, NR.check_exact(res) if name in HAND_MADE else None)


def check(got, want, name):
    """a SliceNesting against the reference's dict, everything"""
    assert got.n_loops == want["n_loops"], name
    for key in ("n_regular", "n_outer", "n_top", "max_depth", "n_improper", "n_misoriented"):
        assert getattr(got, key) == want[key], (name, key, getattr(got, key), want[key])
    for key in NR.PLANE_COUNTS:
        assert got.per_plane[key].dtype == np.uint64 and np.array_equal(got.per_plane[key], want["per_plane"][key]), (name, key)
    for key in LOOP_ARRAYS:
        a = getattr(got, key)
        assert a.dtype == np.uint32 and np.array_equal(a, want[key]), (name, key)
    assert got.region_area2.dtype == np.float64 and np.array_equal(got.region_area2, want["region_area2"]), name
    start, kids = got.children()
    assert [kids[int(start[l]):int(start[l + 1])].tolist() for l in range(got.n_loops)] == [want["children"][l] for l in range(got.n_loops)], name


# ---- 1. the hand-made cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HAND_MADE)
def test_the_device_is_the_reference(name):
    ms, want = slices_of(name), reference(name)
    for bands in (0, 1, 5):
        got = ms.nesting(bands)
        check(got, want, f"{name}, bands {bands}")
        assert bands == 0 or (got.bands == bands).all()
    got = ms.nesting()
    print(f"{name}: {got}, index {got.index}")
    as_dict = NR.from_device(ms)
    if name == "chain":
        assert got.plane_max_depth.tolist() == K.CHAIN_MAX_DEPTH and got.outer.tolist() == [d // 2 + 1 for d in K.CHAIN_MAX_DEPTH] and got.top.tolist() == [1] * 7
        assert got.n_misoriented == 0 and got.n_improper == 0
    if name == "chain, prism 1 reversed":
        assert got.misoriented.tolist() == [0, 1, 1, 1, 1, 1, 0] and got.n_misoriented == 5          # the planes that cut prism 1
    if name == "siblings":
        assert want["hit_counts"][0] == {1: 2, 2: 1, 3: 1} and got.parent.tolist() == [3, 3, NONE, 2] and got.depth.tolist() == [2, 2, 0, 1]
    if name in ("comb", "long comb"):
        teeth = K.COMB_TEETH if name == "comb" else K.LONG_COMB_TEETH
        assert [want["hit_counts"][l][6] for l in range(5)] == K.comb_multiplicities(teeth) and got.depth.tolist()[:5] == [0, 0, 0, 1, 1] and got.parent.tolist()[3:5] == [6, 6]
        assert got.index["hits"] >= sum(K.comb_multiplicities(teeth)) and (name == "comb" or 2 * teeth + 2 > 512)          # (the long one: beyond a wave's LDS list)
    if name == "vertex on the row":
        assert K.leader_at(as_dict, K.ROW_Q) and [want["hit_counts"][0][m] for m in range(1, 8)] == [w for _, _, _, w in K.ROW_DIAMONDS]
        assert got.parent[0] == 3 and got.depth[0] == 1
    if name == "flat on the row":
        assert K.leader_at(as_dict, (0.0, 0.0)) and len(np.unique(ms.xy[ms.plane == 1], axis=0)) < int((ms.plane == 1).sum())
        assert got.parent.tolist()[:2] == [6, 7] and got.depth.tolist()[:2] == [1, 1]
    if name == "shared edge":
        irregular = np.flatnonzero(ms.loops["irregular"] > 0)
        assert len(irregular) == 2 and (got.parent[irregular] == NONE).all() and (got.depth[irregular] == NONE).all() and (got.n_children[irregular] == 0).all()
        assert not np.isin(got.parent, irregular).any() and got.regular.tolist() == [5, 5] and got.depth[-2:].tolist() == [2, 2]
    if name == "crossing":
        assert got.n_improper == 1 and got.depth.tolist() == [0, 0, 2] and got.parent.tolist() == [NONE, NONE, 0]          # the smaller id among equals


# ---- 2. the bands --------------------------------------------------------------------------------------------------------------------------------
def test_no_result_depends_on_the_bands():
    ms, want = slices_of("field"), reference("field")
    assert ms.counts["irregular"] == 0 and want["n_improper"] == 0 and min(want["per_plane"]["regular"][:5]) > 150
    results = {}
    for b in K.BANDS:          # the context's scratch given back before each: every piece the call carves makes the buffer grow, and move
        ms._hip.check(F.lib().fhip_ctx_trim(ms._hip._h))
        results[b] = ms.nesting(b)
    for b, got in results.items():
        check(got, want, f"field, bands {b}")
        print(f"bands {b}: {got.index}, per plane {got.bands.tolist()}")
        assert b == 0 or (got.bands == b).all()
    # more bands than segments; segment ends exactly on the borders of 2, 64 and 4096 bands of [-1, 1]; a plane of zero extent
    assert results[4096].index["bands"] == 6 * 4096 > ms.counts["segments"]
    y = ms.xy[:, 1]
    assert all(np.any((y * nb / 2) % 1 == 0) for nb in (2, 64, 4096)) and ms.loops["lo"][:, 1].min() == -1.0 and ms.loops["hi"][:, 1].max() == 1.0
    last = ms.loops_of(5)
    assert len(last) == 2 and (ms.loops["lo"][last, 1] == 0.5).all() and (ms.loops["hi"][last, 1] == 0.5).all()
    # the host's rule: a band per 32 regular segments, and no more than 4 entries per segment
    rule = results[0]
    assert rule.index["entries"] <= 4 * ms.counts["segments"] and (rule.bands[:5] > 1).all()


# ---- 3. a real mesh ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["gyroid-sphere.vm", "bear.vm"])
def test_a_built_mesh(model):
    """build_mesh at depth 5 under 24 planes: a thousand loops of a gyroid's sheets, and the bear's few with holes in them"""
    shape = F.Shape.from_vm(model_path(model))
    ms = F.build_mesh(shape, 5).slices(np.linspace(-0.95, 0.95, 24).astype(np.float32))
    got = ms.nesting()
    print(f"{model} at depth 5: {ms}, {got}, index {got.index}, bands {got.bands.tolist()}")
    assert 24 < ms.counts["loops"] < 5000
    check(got, NR.nesting(NR.from_device(ms)), model)
    assert got.n_regular > 24 and got.n_top > 0 and got.max_depth >= 1


# ---- 4. against the bitmap's nesting -------------------------------------------------------------------------------------------------------------
def test_a_bitmaps_mesh_nests_as_the_bitmap():
    """a box with a cavity that holds an island, voxelized at depth 3: no two pixels of a layer touch at a corner alone, so the mesh's
    slices at the layers' centres are the layers' outlines, loop for loop"""
    N = 32
    g = np.zeros((N, N, N), bool)
    g[4:28, 4:28, 4:28] = True
    g[8:24, 8:24, 8:24] = False
    g[12:20, 12:20, 12:20] = True
    vox = F.Voxels(F.default_context(), V.pack(g), 3, None)
    ms = vox.mesh().slices(((2 * np.arange(N) + 1 - N) / N).astype(np.float32))
    got = ms.nesting()
    check(got, NR.nesting(NR.from_device(ms)), "box, cavity, island")
    outlines = vox.outlines(0, N)
    bitmap = outlines.nesting()
    assert ms.counts["irregular"] == 0 and got.n_misoriented == 0 and got.n_improper == 0
    assert np.array_equal(got.outer, bitmap.outer) and np.array_equal(got.top, bitmap.top) and np.array_equal(got.plane_max_depth, bitmap.layer_max_depth)
    assert got.max_depth == 2 and got.plane_max_depth[16] == 2 and got.plane_max_depth[9] == 1 and got.plane_max_depth[5] == 0
    table = outlines.table()
    world = lambda a: tuple(((2 * a.astype(np.int64) - N).astype(np.float32) / np.float32(N)).tolist())          # noqa: E731
    for k in range(N):
        lo, hi = int(outlines.loop_start[k]), int(outlines.loop_start[k + 1])
        of_bitmap = {(world(table["lo"][l]), world(table["hi"][l])): int(bitmap.n_children[l]) for l in range(lo, hi) if table["area2"][l] > 0}
        of_mesh = {(tuple(ms.loops["lo"][l].tolist()), tuple(ms.loops["hi"][l].tolist())): int(got.n_children[l]) for l in ms.loops_of(k) if got.depth[l] % 2 == 0}
        assert of_bitmap == of_mesh and len(of_mesh) == int(got.outer[k]), k


# ---- 5. empty results and refusals ---------------------------------------------------------------------------------------------------------------
def test_empty_results():
    tri, _ = K.chain()
    for zs in (np.zeros(0, np.float32), np.array([-2.0, 1.5], np.float32)):          # no planes; planes that miss the mesh
        got = F.mesh_slices(tri, zs).nesting()
        assert (got.n_loops, got.n_regular, got.n_outer, got.n_top, got.max_depth, got.n_improper, got.n_misoriented) == (0,) * 7 and got.n_planes == len(zs)
        assert all(len(a) == len(zs) and not a.any() for a in got.per_plane.values()) and len(got.parent) == 0 and len(got.region_area2) == 0
        assert got.parent_device() is None and got.depth_device() is None and got.children()[0].tolist() == [0]
        assert [got.regions(p) for p in range(len(zs))] == [[]] * len(zs)
    # irregular loops alone: every loop gets NONE, and there are no device arrays
    open_cube = F.mesh_slices(K.prism(K.square(0.0, 0.0, 0.5), -0.5, 0.5)[1:], np.array([0.0], np.float32))
    got = open_cube.nesting()
    assert open_cube.counts["loops"] == 1 and open_cube.counts["irregular"] > 0 and got.n_regular == 0 and got.parent.tolist() == [NONE] and got.depth.tolist() == [NONE]
    assert got.parent_device() is None and got.regions(0) == []


def test_missing_arguments_are_refused():
    ms = slices_of("chain")
    hip = F.default_context()
    h = C.c_void_p()
    assert F.lib().fhip_slices_nesting(hip._h, None, 0, C.byref(h)) == 5 and F.lib().fhip_slices_nesting(hip._h, ms._owner.h, 0, None) == 5          # BadTape
    assert not h.value


def test_slices_of_another_device_are_refused():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device: no handle of another device to refuse")
    ms = slices_of("chain")
    h = C.c_void_p()
    assert F.lib().fhip_slices_nesting(F.HipContext(1)._h, ms._owner.h, 0, C.byref(h)) == 6 and not h.value          # Unsupported


# ---- 6. two runs, the device views, the regions, the SVG ---------------------------------------------------------------------------------------------
def test_two_runs_device_views_regions_and_svg(tmp_path):
    import torch
    ms = slices_of("field")
    a, b = ms.nesting(), ms.nesting()
    for key in LOOP_ARRAYS + ("region_area2",):
        assert np.array_equal(getattr(a, key), getattr(b, key)), key
    assert all(np.array_equal(a.per_plane[k], b.per_plane[k]) for k in a.per_plane) and a.index == b.index
    again = F.mesh_slices(*mesh_of("field")).nesting()          # the slices made anew: everything but what inherits area2's order of arrival
    assert all(np.array_equal(getattr(a, key), getattr(again, key)) for key in LOOP_ARRAYS)
    assert all(np.array_equal(a.per_plane[k], again.per_plane[k]) for k in a.per_plane if k != "misoriented")
    for view, host in ((a.parent_device(), a.parent), (a.depth_device(), a.depth)):
        assert view.__cuda_array_interface__["shape"] == (a.n_loops,) and view.__cuda_array_interface__["typestr"] == "<i4"
        assert np.array_equal(torch.as_tensor(view, device="cuda").cpu().numpy().view(np.uint32), host)
    want = reference("field")
    for p in range(ms.counts["planes"]):
        regions = a.regions(p)
        assert regions == NR.regions(NR.from_device(ms), want, p)
        members = [l for outer, holes in regions for l in [outer] + holes]
        assert sorted(members) == [int(l) for l in ms.loops_of(p) if ms.loops["irregular"][l] == 0]          # every regular loop in exactly one region
        polys, flat = a.polygons(p), ms.polygons(p)[0]
        assert len(polys) == len(regions) and sum(1 + len(h) for _, h in polys) == len(flat)
    p = 2
    text = a.svg(p, path=str(tmp_path / "plane.svg"))
    assert open(tmp_path / "plane.svg").read() == text
    root = ET.fromstring(text)
    paths = [e for e in root if e.tag.endswith("path")]
    assert len(paths) == len(a.regions(p)) == int(a.outer[p]) and all(e.get("fill-rule") == "evenodd" for e in paths)
    assert [e.get("d").count("M") for e in paths] == [1 + len(h) for _, h in a.regions(p)]
    assert root.get("viewBox") == re.search(r'viewBox="([^"]*)"', ms.svg(p)).group(1)          # MeshSlices.svg's coordinates and viewBox
