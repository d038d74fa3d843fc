"""yh_atrous_filter, the host's form of the denoiser's a-trous filter (unit/atrous_math.h through host/denoise.cpp), without a GPU:
bit for bit the numpy float32 restatement of tests/denoise_f32.py on the strata of tests/denoise_cases.py, the properties the
interface states (misses, alpha, other objects' colours, iterations = 0), and the restatement itself against float64."""
import numpy as np
import pytest

import denoise_f32
import denoise_f64
from denoise_cases import ITERATIONS, SIZES, STRATA, bits, make_case, restated

F = np.float32


def _params(yh, P, iterations):
    return yh.DenoiseParams(iterations, P["sigma_color"], P["sigma_normal"], P["sigma_position"], P["demodulate"], P["match_object"])


def _host(yh, P, it, arrays):
    return yh.atrous_filter(_params(yh, P, it), *arrays)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("stratum", STRATA)
def test_host_form_is_the_restatement_bit_for_bit(yh, stratum, size):
    P, *arrays = make_case(stratum, *size)
    rgba, ids = arrays[0], arrays[1]
    for it in ITERATIONS:
        got = _host(yh, P, it, arrays)
        want = restated(stratum, *size, it)
        diff = bits(got) != bits(want)
        assert not diff.any(), f"{stratum} {size} x{it}: {np.count_nonzero(diff)} of {diff.size} entries differ, first at {np.argwhere(diff)[0]}"
        assert np.array_equal(bits(got[..., 3]), bits(rgba[..., 3])), "alpha is the input's"
        miss = ids == -1
        assert np.array_equal(bits(got[miss]), bits(rgba[miss])), "a miss leaves with its input's bits"
        if it == 0:
            assert np.array_equal(bits(got), bits(rgba)), "iterations = 0: the output is the input"


def test_strata_hold_what_they_are_named_for():
    """The generator's cases contain what the strata promise (so that the comparison above covers it)."""
    for size in SIZES:
        P, rgba, ids, n, x, a = make_case("non-finite", *size)
        assert np.isnan(rgba[size[1] // 2, size[0] // 2, 0])
        P, rgba, ids, n, x, a = make_case("checker-match", *size)
        assert P["match_object"] == 1 and (size == (1, 1) or set(np.unique(ids)) == {0, 1})
    P, rgba, ids, n, x, a = make_case("non-finite", 96, 40)
    assert np.isnan(rgba).any() and np.isposinf(rgba).any() and np.isneginf(rgba).any()
    P, rgba, ids, n, x, a = make_case("misses", 96, 40)
    assert (ids == -1).any() and (a[ids == -1] > 0.01).any()
    P, rgba, ids, n, x, a = make_case("albedo-edges", 96, 40)
    t = F(1e-3)
    for v in (F(0), t, np.nextafter(t, F(0)), np.nextafter(t, F(1))):
        assert (a == v).any()
    # ... and the filter does something on them: with five iterations the full stratum's image changes on most hit pixels
    P, *arrays = make_case("full", 33, 65)
    out = denoise_f32.atrous_filter(dict(P, iterations=5), *arrays)
    assert (bits(out[..., :3]) != bits(arrays[0][..., :3])).mean() > 0.9


@pytest.mark.parametrize("size", [(5, 5), (17, 19), (96, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_match_object_keeps_the_other_objects_colours_out(yh, size):
    """On an id checkerboard with match_object, new colours (NaN among them) on the pixels of id 1 leave every pixel of id 0 with the bits
    it had; without match_object they do not."""
    P, rgba, ids, n, x, a = make_case("checker-match", *size)
    other = rgba.copy()
    rng = np.random.default_rng(5)
    other[ids == 1, :3] = rng.uniform(0, 50, (int((ids == 1).sum()), 3)).astype(F)
    other[ids == 1, 0][::3] = np.nan
    for it in (1, 3, 6):
        a0, a1 = _host(yh, P, it, (rgba, ids, n, x, a)), _host(yh, P, it, (other, ids, n, x, a))
        assert np.array_equal(bits(a0[ids == 0]), bits(a1[ids == 0])), f"x{it}"
        loose = dict(P, match_object=0)
        b0, b1 = _host(yh, loose, it, (rgba, ids, n, x, a)), _host(yh, loose, it, (other, ids, n, x, a))
        assert not np.array_equal(bits(b0[ids == 0]), bits(b1[ids == 0]))


def test_planes_the_parameters_do_not_read_may_be_missing(yh):
    """A sigma that is off and demodulate = 0 make their plane optional: NULL gives the bits the plane gives."""
    P, rgba, ids, n, x, a = make_case("color", 17, 19)
    assert np.array_equal(bits(_host(yh, P, 4, (rgba, ids, None, None, None))), bits(_host(yh, P, 4, (rgba, ids, n, x, a))))


def test_float32_restatement_against_float64():
    """The float32 form's error against the same formula in float64, per stratum: at most 4 x the worst that profiles/denoise/errors.txt
    records (the inputs are seeded: the margin is for other seeds and other libm-free roundings, not for these)."""
    bar = 4 * denoise_f64.recorded_worst()
    errs = denoise_f64.stratum_errors()
    for k, v in errs.items():
        print(f"{k:16s} {v:.3e}  (bar {bar:.3e})")
    assert 0 < bar < 1e-4, "the recorded worst is a float32 rounding figure"
    assert max(errs.values()) <= bar
