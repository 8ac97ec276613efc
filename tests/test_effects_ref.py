"""tests/effects_ref.py - the numpy restatement of effects.rs the device tests compare with - held to the oracle bit for bit on the
adversarial inputs it builds, to the hand-computed cases of test_effects.py, and to the condition that makes the device tests worth
something: every mutant of a rule changes 3 pixels or more of some input those tests use."""
import types

import numpy as np
import pytest

import effects_ref as R

GEOMETRY = [c[0] for c in R.geometry_cases()]
MERGE_N = (1, 257, 4099)


def case(name):
    return next(c for c in R.geometry_cases() if c[0] == name)


@pytest.mark.parametrize("name", GEOMETRY)
def test_reference_equals_oracle_on_geometry_images(name, oracle_mod):
    O = oracle_mod
    _, img, d, k, nz = case(name)
    dn, s, b, rgb, rgb0 = R.chain(name)
    assert R.same(O.denoise_normals(img), dn)
    assert R.same(O.compute_ssao(img, d, k, nz), R.compute_ssao(img, d, k, nz))          # the raw image: NaN and zero normals reach SSAO
    assert R.same(O.compute_ssao(dn, d, k, nz), s)
    assert R.same(O.blur_ssao(s), b)
    assert R.same(O.apply_shading(dn, d, b), rgb) and R.same(O.apply_shading(dn, d), rgb0)
    assert R.same(O.apply_shading(img, d, s), R.apply_shading(img, d, s))                # NaN normals and NaN occlusion through the cast


@pytest.mark.parametrize("name", [m[0] for m in R.ssao_maps()])
def test_reference_equals_oracle_on_ssao_maps(name, oracle_mod):
    s = dict(R.ssao_maps())[name]
    assert R.same(oracle_mod.blur_ssao(s), R.blur_ssao(s))


def test_reference_equals_oracle_on_distance_image(oracle_mod):
    O, img = oracle_mod, R.distance_image()
    assert R.same(O.to_rgba_bitmap(img), R.to_rgba_bitmap(img))
    assert R.same(O.to_rgba_bitmap(img, True), R.to_rgba_bitmap(img, True))
    assert R.same(O.to_debug_bitmap(img), R.to_debug_bitmap(img))
    assert R.same(O.to_rgba_distance(img), R.to_rgba_distance(img))                     # exact: both call this host's expf and cosf


def test_hand_computed_cases_hold_for_the_reference():
    """the cases tests/test_effects.py pins the oracle with, asked of the reference"""
    import test_effects as TE
    ref = types.SimpleNamespace(denoise_normals=R.denoise_normals, compute_ssao=R.compute_ssao, blur_ssao=R.blur_ssao,
                                apply_shading=R.apply_shading, to_rgba_bitmap=R.to_rgba_bitmap, to_debug_bitmap=R.to_debug_bitmap,
                                to_rgba_distance=R.to_rgba_distance)
    TE.test_denoise_keeps_front_facing_and_empty(ref)
    TE.test_denoise_replaces_back_facing_by_best_window_mean(ref)
    TE.test_blur_picks_lowest_variance_window_and_keeps_nan(ref)
    TE.test_shading_values(ref)
    TE.test_ssao_flat_plane_is_unoccluded_and_empty_is_nan(ref)
    TE.test_colour_maps_of_fill_and_distance_pixels(ref)


def test_same_and_differing_compare_bits():
    """the comparison every test here and on the device rests on: NaN equals NaN whatever its payload, +0 is not -0, one differing
    component makes a differing pixel"""
    a = np.array([[0.0, np.nan, 1.0], [2.0, -0.0, np.inf]], np.float32)
    b = a.copy()
    b.view(np.uint32)[0, 1] = 0xFFC00001
    assert R.same(a, b) and R.differing(a, b) == 0
    b[1, 1] = 0.0
    assert not R.same(a, b)
    b[1, 1], b[0, 2] = -0.0, np.nextafter(np.float32(1), np.float32(2))
    assert not R.same(a, b) and R.differing(a, b) == 1
    g, h = np.zeros((2, 2), R.GEOMETRY_PIXEL), np.zeros((2, 2), R.GEOMETRY_PIXEL)
    g["normal"][0, 0], h["normal"][0, 0] = (np.nan, 1, 2), (np.nan, 1, 2)
    assert R.same(g, h) and R.differing(g, h) == 0
    h["depth"][1, 0], h["normal"][0, 1, 2] = 1, 0.5
    assert not R.same(g, h) and R.differing(g, h) == 2
    assert not R.same(np.zeros((2, 2, 3), np.uint8), np.ones((2, 2, 3), np.uint8))
    assert R.differing(np.zeros((2, 2, 3), np.uint8), np.eye(2, dtype=np.uint8)[..., None] * np.ones(3, np.uint8)) == 2


def test_rng_hash_and_mix():
    def hash1(v):                # rng/mod.rs:8-12 on Python integers
        state = (v * 747796405 + 2891336453) & 0xFFFFFFFF
        word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xFFFFFFFF
        return (word >> 22) ^ word

    vs = [0, 1, 2, 36, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 123456789]
    assert R.rng_hash(np.array(vs, np.uint32)).tolist() == [hash1(v) for v in vs]
    assert R.rng_hash(np.array(vs, np.uint32)).dtype == np.uint32
    a, b = np.array(vs, np.uint32), np.array(vs[::-1], np.uint32)
    assert R.rng_mix(a, b).tolist() == [hash1((x + hash1(y)) & 0xFFFFFFFF) for x, y in zip(vs, vs[::-1])]
    assert R.rng_mix(a, b).tolist() != R.rng_mix(b, a).tolist()


def test_merge_depth_by_hand():
    f, b = np.zeros(8, R.GEOMETRY_PIXEL), np.zeros(8, R.GEOMETRY_PIXEL)
    f["depth"], b["depth"] = [10, 40, 22, 63, 7, 64, 0, 62], [30, 5, 22, 7, 63, 3, 0, 62]
    f["normal"], b["normal"] = (1, 2, 3), (4, 5, 6)
    out = R.merge_depth(f, b, 64)
    assert out["depth"].tolist() == [30, 40, 22, 64, 64, 64, 0, 62]
    sat, fr, bk = [0.0, 0.0, 1.0], [1.0, 2.0, 3.0], [4.0, 5.0, 6.0]
    assert out["normal"].tolist() == [bk, fr, fr, sat, sat, sat, fr, fr]                 # the tie at 22 and at 62 keeps the front pixel
    raw = R.merge_depth(f, b, 0)                                                       # image_depth 0: no clamp
    assert raw["depth"].tolist() == [30, 40, 22, 63, 63, 64, 0, 62] and raw["normal"].tolist() == [bk, fr, fr, fr, bk, fr, fr, fr]
    assert f["depth"][0] == 10                                                         # (the inputs are left alone)


def mutant_counts():
    """{(function, mutant): [(input, pixels that differ from the unmutated reference)]} over the inputs of tests/test_effects_gpu.py"""
    out = {}
    for name, img, d, k, nz in R.geometry_cases():
        dn, s, b, rgb, rgb0 = R.chain(name)
        for m in R.MUTANTS["denoise_normals"]:
            out.setdefault(("denoise_normals", m), []).append((name, R.differing(R.denoise_normals(img, mutant=m), dn)))
        for m in R.MUTANTS["compute_ssao"]:
            out.setdefault(("compute_ssao", m), []).append((name, R.differing(R.compute_ssao(dn, d, k, nz, mutant=m), s)))
        for m in R.MUTANTS["blur_ssao"]:
            out.setdefault(("blur_ssao", m), []).append((name, R.differing(R.blur_ssao(s, mutant=m), b)))
        for m in R.MUTANTS["apply_shading"]:
            out.setdefault(("apply_shading", m), []).append((name, R.differing(R.apply_shading(dn, d, b, mutant=m), rgb)))
            out[("apply_shading", m)].append((name + " no ssao", R.differing(R.apply_shading(dn, d, mutant=m), rgb0)))
    for name, s in R.ssao_maps():
        for m in R.MUTANTS["blur_ssao"]:
            out[("blur_ssao", m)].append((name, R.differing(R.blur_ssao(s, mutant=m), R.blur_ssao(s))))
    img = R.distance_image()
    for m in R.MUTANTS["colour_maps"]:
        for fn in (R.to_rgba_bitmap, R.to_debug_bitmap, R.to_rgba_distance):
            out.setdefault(("colour_maps", m), []).append((fn.__name__, R.differing(fn(img, mutant=m), fn(img))))
    for n in MERGE_N:
        f, b = R.merge_case(n)
        for m in R.MUTANTS["merge_depth"]:
            out.setdefault(("merge_depth", m), []).append(("n=%d" % n, R.differing(R.merge_depth(f, b, 64, mutant=m), R.merge_depth(f, b, 64), 1)))
    return out


def test_every_mutant_changes_three_pixels_of_some_gpu_input():
    counts = mutant_counts()
    assert set(counts) == {(fn, m) for fn, ms in R.MUTANTS.items() for m in ms}
    for key, seen in sorted(counts.items()):
        print(key, [c for c in seen if c[1]])
    weak = {key: seen for key, seen in counts.items() if max(c[1] for c in seen) < 3}
    assert not weak, weak


def test_inputs_hold_what_they_are_built_for():
    for name, img, d, k, nz in R.geometry_cases()[:3]:
        n, filled = img["normal"], img["depth"] != 0
        assert 0.15 < (~filled).mean() < 0.35
        zero = filled & (n == 0).all(axis=-1)
        assert 0.04 < zero.sum() / filled.sum() < 0.2
        assert np.isnan(n[filled]).any() and np.isinf(n[filled]).any()
        assert (filled & (n[..., 2] <= 0)).sum() > (filled & (n[..., 2] > 0)).sum()
    s = R.chain("plane")[1]
    assert (s < 1).any()                        # the equality case occludes: samples with sample_pos.z == actual_z count
    img = R.distance_image()
    assert np.isinf(img).any() and (img == 0).any() and (np.abs(img) == np.float32(0.005)).any() and (np.abs(img) == np.float32(0.015)).any()
