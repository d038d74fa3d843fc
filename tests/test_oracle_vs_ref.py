"""Oracle vs the reference, bit for bit, on seeded inputs beyond the committed golden vectors (tests/ref_cases.py).
Everywhere: against the reference's outputs stored as digests (tests/golden/ref_digests.json, oracle/make_ref_digests.py).
Where the LIVE reference has been built as well (oracle/_ref/libyh_ref.so: `make -C oracle ref`): against it directly."""
import numpy as np
import pytest

import oracle_capi as oc
import ref_cases as rc
from conftest import scene_path


@pytest.fixture(scope="module")
def ref():
    """The live reference, or None where it has not been built."""
    return oc.Ref() if oc.have_ref() else None


def _check(key, run, oracle, ref):
    got = run(oracle)
    want = rc.stored(key)
    assert sorted(got) == sorted(want), key
    differ = [k for k in got if rc.digest(got[k]) != want[k]]
    assert not differ, f"{key}: the oracle's {differ} differ from the reference's (tests/golden/ref_digests.json)"
    if ref is not None:
        live = run(ref)
        for k in got:
            assert np.array_equal(got[k], live[k], equal_nan=True), f"{key}: {k} differs from the live reference"


def test_bsdf_random_inputs(oracle, ref):
    _check("bsdf_random_inputs", rc.bsdf_random_inputs, oracle, ref)


def test_surface_lobes_random_inputs(oracle, ref, yh):
    _check("surface_lobes_random_inputs", rc.surface_lobes_random_inputs, oracle, ref)


def test_curve_conversion_random_inputs(oracle, ref):
    _check("curve_conversion_random_inputs", rc.curve_conversion_random_inputs, oracle, ref)


@pytest.mark.parametrize("name", list("abcdefg"))
def test_volume_functions_on_every_stratum(oracle, ref, name):
    """Every row of the unit-level volume strata (tests/volume_cases.py), both tex forms: the oracle's free flight and scatter against
    the live reference's public functions on the same medium, bit for bit. Where the reference is not built, the committed rows
    (tests/golden/volumes_unit.npz, test_oracle_golden.py) are what holds the oracle."""
    import volume_cases as vc
    s = vc.inputs(name)
    for tex in (0, 1):
        orc = oracle.volume(tex, s.mats, s.nrm, s.wo, s.wi, s.tex, s.rn)
        view, covered = vc.reference_view(orc)
        assert covered.any()
        if ref is not None and ref.has_volume:
            live = ref.volume(orc[:, 1:4], orc[:, 7], s.wo, s.wi, s.rn)
            differ = np.flatnonzero(~((view == live) | (np.isnan(view) & np.isnan(live))).all(axis=1) & covered)
            assert len(differ) == 0, (name, tex, differ[:5], view[differ[:2]], live[differ[:2]])


@pytest.mark.parametrize("name", list("abcdefg"))
def test_surface_lobes_on_every_stratum(oracle, ref, yh, name):
    """Every row of the unit-level surface strata (tests/surface_cases.py): the oracle's Fresnel terms and nine lobes against the
    live reference, bit for bit. Where the reference is not built, the committed rows (tests/golden/lobes_edges.npz,
    test_oracle_golden.py) are what holds the oracle."""
    import surface_cases as sc
    s = sc.inputs(name)
    args = (s.params, s.nrm, s.wo, s.wi, s.rn)
    got = [oracle.fresnel(*args[:3])] + [oracle.surface_lobe(kind, *args) for kind in range(yh.LOBE_COUNT)]
    assert all(len(x) == s.n for x in got)
    if ref is not None:
        live = [ref.fresnel(*args[:3])] + [ref.surface_lobe(kind, *args) for kind in range(yh.LOBE_COUNT)]
        for k, (a, b) in enumerate(zip(got, live)):
            assert np.array_equal(a, b, equal_nan=True), (name, k - 1, np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))).all(axis=1))[:5])


def test_selftests_match_reference(oracle, ref):
    # the reference prints "OK!"; ours returns 1. Only the two cheap ones here (the 300k-sample
    # furnace tests take ~12 s on the reference and are covered by the GPU self-tests).
    for which in (2, 3):
        if ref is not None:
            assert ref.lib.ref_selftest(which) == 1
        assert oracle.selftest(which)[0]


@pytest.mark.parametrize("name,kw,res,spp", rc.IMAGE_CASES)
def test_images_bit_identical_to_reference(oracle, ref, yh, name, kw, res, spp):
    _check(rc.image_key(name, kw, res, spp), lambda api: rc.render(api, scene_path, name, kw, res, spp), oracle, ref)


@pytest.mark.parametrize("shader", rc.SHADERS)
@pytest.mark.parametrize("name,kw,res,spp", rc.SHADER_CASES)
def test_other_shaders_bit_identical_to_reference(oracle, ref, yh, name, kw, res, spp, shader):
    _check(rc.image_key(name, kw, res, spp, shader), lambda api: rc.render(api, scene_path, name, kw, res, spp, shader), oracle, ref)


@pytest.mark.parametrize("prefix,kw,res_key,shaders", rc.MAPS_CASES, ids=[c[0].strip("/") or "maps" for c in rc.MAPS_CASES])
def test_material_maps_bit_identical_to_reference(oracle, ref, yh, prefix, kw, res_key, shaders):
    """The `maps` scene and its one-map variants: the oracle's renders against the LIVE reference's, bit for bit, where it is
    built. Everywhere else the reference's committed images of the same renders (tests/golden/maps.npz,
    test_oracle_golden.py::test_material_maps_bit_exact) are what holds the oracle."""
    from conftest import golden
    g = golden("maps.npz")
    got = rc.maps_entries(oracle, scene_path, g, prefix, kw, res_key, shaders)
    assert got
    if ref is not None:
        live = rc.maps_entries(ref, scene_path, g, prefix, kw, res_key, shaders)
        for k in got:
            assert np.array_equal(got[k], live[k], equal_nan=True), f"{k} differs from the live reference"


HITS_VARIANTS = ("four", "six", "far", "deep", "ties")


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("name", list("bcde"))
def test_primitive_tests_on_the_edge_strata(oracle, ref, name):
    """The primitive-level form of the closest-hit edge strata (tests/hit_cases.py: the ray and the segment or triangle it was aimed
    at, the primitive's box and the shape's): yo_intersect_line, _triangle and _bbox against the live reference's, bit for bit. Where
    the reference is not built, the scene-level rows of tests/golden/hits_unit.npz are what holds the oracle."""
    import hit_cases as hc
    if ref is None:
        pytest.skip("oracle/_ref has not been built")
    lines, tris, boxes = hc.primitive_form("four", name)
    for what, args in (("intersect_line", lines), ("intersect_triangle", tris), ("intersect_bbox", boxes)):
        if len(args[0]) == 0:
            continue
        got, want = getattr(oracle, what)(*args), getattr(ref, what)(*args)
        got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
        hit = want[0] != 0
        assert (got[0] != 0).tolist() == hit.tolist(), (name, what)
        for a, b in zip(got[1:], want[1:]):  # (uv and distance are written on a hit only)
            assert _same_bits(a[hit], b[hit]), (name, what)
        assert 0 < hit.mean() < 1, (name, what, hit.mean())


@pytest.mark.parametrize("variant", HITS_VARIANTS)
def test_closest_hits_on_every_stratum(oracle, ref, yh, variant):
    """yo_scene_intersect against the live reference's intersect_scene_bvh on every row of every stratum of tests/hit_cases.py and
    on the quad-only batch, bit for bit (a NaN uv — an r = 0 tip met exactly — included); on `deep`, on hit_cases.deep_rays; on `ties`, on hit_cases.ties_rays."""
    import hit_cases as hc
    if ref is None:
        pytest.skip("oracle/_ref has not been built")
    rsc = ref.scene(scene_path("hits-unit", variant=variant))
    batches = (hc.deep_rays(),) if variant == "deep" else (hc.ties_rays(),) if variant == "ties" else (hc.main_batch(variant), hc.quad_only(variant).rays)
    for rays, got in zip(batches, hc.oracle_hits(variant, yh, oracle, scene_path)):
        want = rsc.intersect(rays)
        for what, a, b in zip(("object", "element", "uv", "distance"), got, want):
            same = (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).reshape(len(a), -1).all(1)
            bad = np.flatnonzero(~same)
            assert bad.size == 0, f"{what} differs on {bad.size} rows, first {hc.where(bad[0]) if len(rays) == 65536 else bad[0]}: oracle {a[bad[0]]} reference {b[bad[0]]}"
    rsc.close()
