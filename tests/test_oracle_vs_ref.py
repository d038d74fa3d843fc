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
