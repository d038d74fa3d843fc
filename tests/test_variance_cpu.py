"""The host's forms of the variance stage (unit/variance_math.h through host/variance.cpp; include/yhair.h: VARIANCE), without a GPU: bit
for bit the numpy float32 restatement of tests/variance_f32.py on the strata of tests/variance_cases.py, the ties to yh_reproject and
yh_atrous_filter, the saturation of `steps`, the cancellation of M2 - M1^2 against float64, a synthetic step and a synthetic noise region,
and the proof that the strata hit the edges they are named after."""
import numpy as np
import pytest

import variance_f32
import variance_f64
from variance_cases import (F_ITERATIONS, F_SIZES, F_STRATA, M_SIZES, M_STRATA, MIN_STEPS, S_SIZES, S_STRATA, bits, f_restated, m_arguments, m_restated,
                            make_f_case, make_m_case, make_s_case, s_arguments, s_restated)

F = np.float32
_size = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


def _tparams(yh, P):
    return yh.TemporalParams(P["max_history"], P["sigma_position"], P["match_object"])


def _vparams(yh, V):
    return yh.VarianceParams(V["iterations"], V["sigma_luminance"], V["sigma_normal"], V["sigma_position"], V["demodulate"], V["match_object"], V["epsilon"],
                             V["min_steps"])


def _same(got, want, what):
    diff = bits(got) != bits(np.ascontiguousarray(want, got.dtype))
    assert not diff.any(), f"{what}: {np.count_nonzero(diff)} of {diff.size} entries differ, first at {np.argwhere(diff)[0]}"


@pytest.mark.parametrize("size", M_SIZES, ids=_size)
@pytest.mark.parametrize("stratum", M_STRATA)
def test_stage_m_is_the_restatement_and_its_colour_is_yh_reproject(yh, stratum, size):
    case = make_m_case(stratum, *size)
    P, args = _tparams(yh, case["P"]), m_arguments(case)
    out, length, moments, steps = yh.reproject_moments(P, *args)
    w_out, w_length, w_moments, w_steps, info = m_restated(stratum, *size)
    _same(out, w_out, "colour"), _same(moments, w_moments, "moments")
    assert np.array_equal(length, w_length) and np.array_equal(steps, w_steps)
    plain, plain_len = yh.reproject(P, *[case[k] for k in ("rgba", "samples", "ids", "position", "history", "camera", "prev_camera", "frames", "prev_frames", "usable")])
    _same(out, plain, "colour against yh_reproject")
    assert np.array_equal(length, plain_len), "length_out is yh_reproject's whatever the moments do"
    assert (steps[~info["live"]] == 0).all() and (moments[~info["live"]] == 0).all(), "a pass-through pixel has no moments"
    assert (steps[info["live"] & ~info["moment_history"]] == 1).all() and (steps[info["live"]] >= 1).all()
    assert steps.max() <= variance_f32.MAX_STEPS


def test_steps_saturate_at_the_maximum(yh):
    case = make_m_case("saturate", 17, 33)
    hs = case["moment_history"][1]
    out = yh.reproject_moments(_tparams(yh, case["P"]), *m_arguments(case))
    took = m_restated("saturate", 17, 33)[4]["moment_history"]
    assert took.any() and (hs[took] >= variance_f32.MAX_STEPS - 1).any() and (hs[took] == variance_f32.MAX_STEPS - 2).any()
    assert np.array_equal(out[3][took], np.minimum(hs[took], variance_f32.MAX_STEPS - 1) + 1), "a still view's tap is the pixel itself"
    assert out[3].max() == variance_f32.MAX_STEPS


@pytest.mark.parametrize("size", S_SIZES, ids=_size)
@pytest.mark.parametrize("stratum", S_STRATA)
def test_stage_s_is_the_restatement(yh, stratum, size):
    case = make_s_case(stratum, *size)
    got = yh.variance_spatial(_tparams(yh, case["P"]), *s_arguments(case))
    want, info = s_restated(stratum, *size)
    _same(got, want, "variance")
    assert (got[case["steps"] == 0] == 0).all(), "no moments: no variance"
    assert not (got < 0).any()


@pytest.mark.parametrize("iterations", F_ITERATIONS)
@pytest.mark.parametrize("size", F_SIZES, ids=_size)
@pytest.mark.parametrize("stratum", F_STRATA)
def test_stage_f_is_the_restatement(yh, stratum, size, iterations):
    V, *arrays = make_f_case(stratum, *size)
    out, var = yh.atrous_variance_filter(_vparams(yh, dict(V, iterations=iterations)), *arrays)
    w_out, w_var, _ = f_restated(stratum, *size, iterations)
    _same(out, w_out, "colour"), _same(var, w_var, "variance")
    rgba, v, ids = arrays[0], arrays[1], arrays[2]
    _same(out[..., 3], rgba[..., 3], "alpha is the input's")
    miss = ids == -1
    _same(out[miss], rgba[miss], "a miss keeps its bits"), _same(var[miss], v[miss], "a miss keeps its variance")


@pytest.mark.parametrize("sigma_luminance", (0.0, -1.0))
@pytest.mark.parametrize("stratum", ("full", "misses", "non-finite", "albedo-edges"))
def test_without_the_luminance_term_the_colour_is_yh_atrous_filter(yh, stratum, sigma_luminance):
    V, rgba, var, ids, n, x, a = make_f_case(stratum, 33, 40)
    for iterations in (1, 3, 5):
        out, _ = yh.atrous_variance_filter(_vparams(yh, dict(V, iterations=iterations, sigma_luminance=sigma_luminance)), rgba, var, ids, n, x, a)
        want = yh.atrous_filter(yh.DenoiseParams(iterations, 0.0, V["sigma_normal"], V["sigma_position"], V["demodulate"], V["match_object"]), rgba, ids, n, x, a)
        _same(out[..., :3], want[..., :3], f"{stratum}, {iterations} iterations")


def test_cancellation_of_the_variance_on_a_constant_image(yh):
    """M2 - M1 M1 where it cancels worst: a constant image at luminance 1e3 accumulated over a still view. In exact arithmetic the variance
    is 0; float32 leaves the rounding of l l and of the blends, of the order of 2^-24 l^2 = 0.06. Reported, and bounded by 8 ulp of l^2."""
    w, h, l = 9, 7, F(1e3)
    cam = np.concatenate([np.eye(3).reshape(9), [0, 0, 3], [0.05, 0.036, 0.028, 10000.0, 0.0]]).astype(F)
    ids, pos = np.zeros((h, w), np.int32), np.zeros((h, w, 3), F)
    pos[..., 2] = -1
    rgba = np.full((h, w, 4), l, F)  # lum of a grey (l, l, l) is l up to the rounding of its three weights
    P = yh.TemporalParams(1 << 20, 0.0, 1)
    Pd = dict(max_history=1 << 20, sigma_position=0.0, match_object=1)
    hist = mom = mom64 = hist64 = None
    worst = 0.0
    for step in range(12):
        out, length, m, s = yh.reproject_moments(P, rgba, 1, ids, pos, None, hist, mom, cam, cam)
        o64, l64, m64, s64, _ = variance_f64.reproject_moments(Pd, rgba, 1, ids, pos, None, hist64, mom64, cam, cam)
        hist, mom, hist64, mom64 = (out, length, ids, pos), (m, s), (o64.astype(F), l64, ids, pos), (m64.astype(F), s64)
        var = yh.variance_spatial(P, 1, m, s, ids, pos)
        v64 = variance_f32.variance_of(m64[..., 0], m64[..., 1])
        worst = max(worst, float(np.abs(var - v64).max()))
        assert (s == step + 1).all()
    l2 = float(m[0, 0, 1])
    print(f"\nconstant image at luminance {float(l):g}: |M2 - M1 M1| against float64 at most {worst:.4g} = {worst / (l2 * 2.0 ** -24):.2f} ulp of l^2 over 12 steps")
    assert worst <= 8 * l2 * 2.0 ** -23


def _flat(w, h):
    ids, n, x = np.zeros((h, w), np.int32), np.zeros((h, w, 3), F), np.zeros((h, w, 3), F)
    n[..., 2] = 1
    return ids, n, x


def test_a_noise_free_step_with_no_variance_stays_a_step(yh):
    """One id, one normal, flat positions, v = 0: g = 0, so a tap across a luminance step of height d has xl = d^2 / epsilon and weight at
    most h / (1 + xl + xl^2 / 2) < 2 h epsilon^2 / d^4; its own side's taps weigh at least the centre's 9/64. A level therefore moves a
    pixel by at most d x (sum of the far side's h <= 1) x 2 epsilon^2 / d^4 / (9/64), and five levels by five times that (the step only
    shrinks by as much, which the bound's slack of 2 covers)."""
    w, h, d, eps, levels = 24, 16, 0.5, 1e-4, 5
    ids, n, x = _flat(w, h)
    rgba = np.ones((h, w, 4), F)
    rgba[:, w // 2:, :3] = F(1 + d)
    V = variance_f32.variance_params(iterations=levels, sigma_luminance=4.0, epsilon=eps, match_object=1)
    out, var = yh.atrous_variance_filter(_vparams(yh, V), rgba, np.zeros((h, w), F), ids, n, x, None)
    tol = 2 * levels * d * (2 * eps ** 2 / d ** 4) / (9 / 64) + 4 * 2.0 ** -24 * (1 + d)
    print(f"\nstep of {d}: moved by at most {np.abs(out[..., :3] - rgba[..., :3]).max():.3g}, tolerance {tol:.3g}")
    assert np.abs(out[..., :3] - rgba[..., :3]).max() <= tol
    assert (var == 0).all()


def test_noise_of_known_variance_loses_it_by_the_float64_factor(yh):
    rng = np.random.default_rng(7)
    w, h, sigma = 40, 32, 0.1
    ids, n, x = _flat(w, h)
    rgba = np.ones((h, w, 4), F)
    rgba[..., :3] = (1 + rng.normal(0, sigma, (h, w, 1))).astype(F)
    v = np.full((h, w), sigma * sigma, F)
    V = variance_f32.variance_params(iterations=3, sigma_luminance=4.0, epsilon=1e-4, match_object=1)
    out, var = yh.atrous_variance_filter(_vparams(yh, V), rgba, v, ids, n, x, None)
    _, v64, _ = variance_f64.atrous_variance_filter(V, rgba, v, ids, n, x, None)
    factor, factor64 = var.astype(np.float64) / v, v64 / v
    assert (factor64 < 0.2).all() and (factor64 > 0).all(), "three levels of up to 25 taps each"
    rel = np.abs(factor - factor64) / factor64
    print(f"\nvariance falls by x {factor64.mean():.4f} (mean); float32 against float64 within {rel.max():.3g} relative")
    assert rel.max() <= 1e-4
    inner = (slice(8, -8), slice(8, -8))
    assert out[inner][..., 0].var() < 0.25 * sigma * sigma, "and the colour is smoother for it"


def test_the_strata_hit_their_edges(yh):
    """Counted on the restatement's own bookkeeping and on what the host forms make of the same cases, so that a case generator that drifts
    away from an edge fails here."""
    m = {s: m_restated(s, 64, 64)[4] for s in M_STRATA}
    lib = {}
    for s in ("still", "pan", "no-moments"):
        case = make_m_case(s, 64, 64)
        lib[s] = (case, yh.reproject_moments(_tparams(yh, case["P"]), *m_arguments(case)))
    case, (_, length, moments, steps) = lib["pan"]
    mixed = m["pan"]["mixed_steps"]
    assert mixed.sum() > 20 and (steps[mixed] == 1).all() and (length[mixed] > case["samples"]).all(), "a tap with steps = 0 among them: the colour goes on, the moments start"
    assert (~np.isfinite(lib["still"][1][2][..., 1]) & (lib["still"][1][3] > 0)).sum() > 100, "the host form hands out moments that are not finite"
    assert (lib["no-moments"][1][3] <= 1).all() and (lib["no-moments"][1][1] > lib["no-moments"][0]["samples"]).any()
    assert m["still"]["shortcut"].sum() > 1000 and (m["still"]["taps_added"][m["still"]["shortcut"]] <= 1).all(), "the one-tap still view"
    four = {k: sum(int((i["invalid_taps"][~i["shortcut"] & i["history"]] == k).sum()) for i in m.values()) for k in (1, 2, 3)}
    assert min(four.values()) > 20, f"four taps with one, two and three of them invalid: {four}"
    assert sum(int(i["mixed_steps"].sum()) for i in m.values()) > 100, "taps with steps = 0 beside taps with steps > 0"
    assert m["non-finite"]["hm_non_finite"].sum() > 20, "non-finite moments in a tap"
    still = m_restated("still", 64, 64)
    assert (~np.isfinite(still[2][..., 1]) & (still[3] > 0)).sum() > 100, "moments that are not finite come out of stage M"
    assert m["no-moments"]["history"].any() and not m["no-moments"]["moment_history"].any()
    s = {k: (make_s_case(k, 33, 20), s_restated(k, 33, 20)[1]) for k in S_STRATA}
    steps = s["mixed"][0]["steps"]
    for k in (MIN_STEPS - 1, MIN_STEPS, MIN_STEPS + 1):
        assert (steps == k).sum() > 20, f"steps on {k}"
    case, info = s["mixed"]
    assert (info["window"] & (info["count"] < 49) & ~info["cut"]).sum() > 20, "misses inside the 7 x 7 window"
    assert (s["lonely"][1]["count"][s["lonely"][1]["window"]] == 1).all() and s["lonely"][1]["window"].sum() >= 12, "a window with only its centre valid"
    lonely, alone = s["lonely"][0], s["lonely"][1]["window"]
    got = yh.variance_spatial(_tparams(yh, lonely["P"]), *s_arguments(lonely))
    mo = lonely["moments"]
    _same(got[alone], variance_f32.variance_of(mo[..., 0], mo[..., 1])[alone], "alone in its window: the spatial estimate is the pixel's own")
    nf_case, nf = s["non-finite"]
    bad = ~np.isfinite(nf_case["moments"]).all(-1)
    assert (bad & nf["window"]).any() and (nf["window"] & ~bad).any(), "non-finite moments in the centre and in a tap"
    assert not s["settled"][1]["window"].any()
    b = s["borders"][1]["window"]
    assert b[0, 0] and b[0, -1] and b[-1, 0] and b[-1, -1] and b[0, 10] and b[-1, 10] and b[10, 0] and b[10, -1], "windows cut by each border and corner"
    assert s["borders"][1]["cut"].sum() == b.sum()
    f = {k: (make_f_case(k, 33, 40), f_restated(k, 33, 40, 1)[2]) for k in F_STRATA}
    assert f["v-zero"][1]["g_zero"].all(), "g = 0 exactly"
    V, *arrays = f["v-zero"][0]
    assert (yh.atrous_variance_filter(_vparams(yh, dict(V, iterations=1)), *arrays)[1] == 0).all(), "... and no variance comes out of none"
    taps = f["full"][1]["g_taps"]
    assert taps[0, 0] <= 4 and taps[0, -1] <= 4 and taps[-1, 0] <= 4 and taps[-1, -1] <= 4 and (taps[0, 1:-1] <= 6).all() and (taps[1:-1, 0] <= 6).all()
    ids = f["misses"][0][3]
    near = np.zeros(ids.shape, bool)
    near[1:-1, 1:-1] = np.stack([ids[1 + dy:ids.shape[0] - 1 + dy, 1 + dx:ids.shape[1] - 1 + dx] == -1 for dy in (-1, 0, 1) for dx in (-1, 0, 1)]).any(0)
    assert (near & (ids != -1)).sum() > 100, "misses inside the 3 x 3 window"
    var = f["v-non-finite"][0][2]
    assert not np.isfinite(var[20, 16]) and (~np.isfinite(var)).sum() > 50, "non-finite variances in the centre and in a tap"
    assert (f["v-non-finite"][1]["g_taps"] < 9).any()
