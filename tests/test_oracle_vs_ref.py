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
