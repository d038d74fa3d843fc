"""yh_reproject, the host's form of the temporal stage (unit/reproject_math.h through host/temporal.cpp), without a GPU: bit for bit the
numpy float32 restatement of tests/reproject_f32.py on the strata of tests/temporal_cases.py, the properties the interface states (misses
and non-finite pixels, alpha, a still view, a constant history), and the restatement itself against float64."""
import numpy as np
import pytest

import reproject_f32
import reproject_f64
from temporal_cases import SIZES, STRATA, arguments, bits, camera, make_case, restated, EYE, AT

F = np.float32


def _params(yh, P):
    return yh.TemporalParams(P["max_history"], P["sigma_position"], P["match_object"])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("stratum", STRATA)
def test_host_form_is_the_restatement_bit_for_bit(yh, stratum, size):
    case = make_case(stratum, *size)
    got, got_len = yh.reproject(_params(yh, case["P"]), *arguments(case))
    want, want_len, info = restated(stratum, *size)
    diff = bits(got) != bits(want)
    assert not diff.any(), f"{stratum} {size}: {np.count_nonzero(diff)} of {diff.size} entries differ, first at {np.argwhere(diff)[0]}"
    assert np.array_equal(got_len, want_len), f"{stratum} {size}: lengths differ at {np.argwhere(got_len != want_len)[:3]}"
    rgba, ids = case["rgba"], case["ids"]
    assert np.array_equal(bits(got[..., 3]), bits(rgba[..., 3])), "alpha is the input's"
    through = (ids == -1) | ~np.isfinite(rgba[..., :3]).all(-1)
    assert np.array_equal(bits(got[through]), bits(rgba[through])) and (got_len[through] == 0).all(), "misses and non-finite pixels keep their bits"
    fresh = ~through & ~info["history"]
    assert np.array_equal(bits(got[fresh]), bits(rgba[fresh])) and (got_len[fresh] == case["samples"]).all(), "without a history: the input"


def test_the_first_frame_seeds_the_history(yh):
    case = make_case("non-finite", 17, 33)
    args = arguments(case)
    args[4] = None
    got, got_len = yh.reproject(_params(yh, case["P"]), *args)
    want, want_len, _ = reproject_f32.reproject(case["P"], *args)
    assert np.array_equal(bits(got), bits(case["rgba"])) and np.array_equal(bits(got), bits(want))
    live = (case["ids"] != -1) & np.isfinite(case["rgba"][..., :3]).all(-1)
    assert np.array_equal(got_len, np.where(live, case["samples"], 0)) and np.array_equal(got_len, want_len)


@pytest.mark.parametrize("size", [(17, 33), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_still_view_accumulates_to_the_mean(yh, size):
    """K = 4 frames of n samples each under one camera: the running blend is the mean of the frames, within K roundings of a convex
    update (1e-5 relative), and the lengths are K n: no blur, no loss."""
    case = make_case("still", *size)
    P = _params(yh, dict(case["P"], max_history=1 << 20))
    rng = np.random.default_rng(11)
    ids, pos, cam, n, K = case["ids"], case["position"], case["camera"], 3, 4
    frames = [np.concatenate([rng.uniform(0, 4, ids.shape + (3,)), rng.uniform(0, 1, ids.shape + (1,))], -1).astype(F) for _ in range(K)]
    hist = None
    for k, f in enumerate(frames):
        out, length = yh.reproject(P, f, n, ids, pos, hist, cam, cam)
        hist = (out, length, ids, pos)
    hit = ids != -1
    mean = np.mean([f.astype(np.float64) for f in frames], 0)[..., :3]
    assert (length[hit] == K * n).all() and (length[~hit] == 0).all()
    rel = np.abs(out[..., :3][hit] - mean[hit]) / np.abs(mean[hit])
    print(f"still, {K} frames: max relative error {rel.max():.3e}")
    assert rel.max() <= 1e-5
    assert np.array_equal(bits(out[~hit]), bits(frames[-1][~hit]))


@pytest.mark.parametrize("stratum", ("pan", "orbit", "edges", "moving"))
def test_a_constant_history_comes_back(yh, stratum):
    """With the history's colour one constant and the current colour the same constant, every pixel leaves with it within 1e-6 relative
    whatever the weights of its taps (h = sum w c / sum w, then a convex blend of c with itself)."""
    case = make_case(stratum, 64, 64)
    args = arguments(case)
    const = np.array([0.7317, 2.113, 0.0519], F)
    rgba = args[0].copy()
    rgba[..., :3] = const
    hr, hl, hi, hp = args[4]
    hr = hr.copy()
    hr[..., :3] = const
    args[0], args[4] = rgba, (hr, hl, hi, hp)
    out, length = yh.reproject(_params(yh, case["P"]), *args)
    took = length > case["samples"]
    assert took.sum() > 100
    rel = np.abs(out[..., :3].astype(np.float64) - const.astype(np.float64)) / const.astype(np.float64)
    print(f"{stratum}: max relative error {rel.max():.3e}")
    assert rel.max() <= 1e-6


def test_projection_against_float64():
    """The float32 projection's error in pixels against float64, per stratum: at most 4 x the worst that profiles/temporal/errors.txt
    records (the inputs are seeded: the margin is for other shapes of the same magnitude, not for these)."""
    bar = 4 * reproject_f64.recorded_worst()
    errs = reproject_f64.stratum_errors()
    for k, (p, b) in errs.items():
        print(f"{k:16s} projection {p:.3e} px, blend {b:.3e}  (bar {bar:.3e} px)")
    assert 0 < bar < 1e-3, "the recorded worst is a float32 rounding figure: far below a pixel"
    assert max(p for p, _ in errs.values()) <= bar


def test_the_projection_inverts_the_centre_ray():
    """A point on the centre-mode ray of pixel (i, j) projects back to fx = i, fy = j, within the projection bar."""
    w, h = 130, 70
    cam = camera(EYE, AT, w, h)
    c = cam.astype(np.float64)
    jj, ii = np.mgrid[0:h, 0:w]
    d = np.stack([c[13] * ((ii + 0.5) / w - 0.5), c[14] * (0.5 - (jj + 0.5) / h), np.full((h, w), -c[12])], -1)
    world = c[9:12] + 40.0 * (d[..., 0:1] * c[0:3] + d[..., 1:2] * c[3:6] + d[..., 2:3] * c[6:9])
    lz, fx, fy = reproject_f32.project(cam, world.astype(F), w, h)
    assert (lz < 0).all()
    bar = 4 * reproject_f64.recorded_worst()
    assert np.abs(fx - ii).max() <= bar + 130 * 2.0 ** -23 and np.abs(fy - jj).max() <= bar + 70 * 2.0 ** -23  # (+ the rounding of the point itself)
