"""Synthetic inputs of the variance stage (include/yhair.h: VARIANCE) for the CPU and GPU tests, one builder per stratum and stage.
  stage M   tests/temporal_cases.py's scenes and cameras with an albedo plane and a moment history beside the colour's
  stage S   seeded moments, steps around min_steps, ids in blobs with misses, positions on a bumpy sheet
  stage F   tests/denoise_cases.py's images with a variance plane
The float32 restatement of every case is computed once per session and shared read-only."""
import functools
import zlib

import numpy as np

import denoise_cases
import temporal_cases
import variance_f32

F = np.float32
MIN_STEPS = 4

M_STRATA = ("still", "pan", "orbit", "edges", "ids", "lengths", "non-finite", "sigma", "moving", "no-moments", "saturate")
M_SIZES = ((1, 1), (17, 33), (64, 64))  # width x height
S_STRATA = ("mixed", "lonely", "borders", "non-finite", "sigma", "settled")
S_SIZES = ((1, 1), (5, 5), (17, 19), (33, 20))
F_STRATA = ("all-off", "luminance", "checker-match", "misses", "non-finite", "albedo-edges", "full", "v-zero", "v-non-finite")
F_SIZES = ((1, 1), (2, 3), (5, 5), (17, 19), (33, 40))
F_ITERATIONS = (0, 1, 2, 3, 5)


def _rng(name, w, h):
    return np.random.default_rng(zlib.crc32(f"variance-{name}-{w}x{h}".encode()))


# ---- stage M ----
def make_m_case(stratum, w, h):
    base = {"no-moments": "pan", "saturate": "still"}.get(stratum, stratum)
    case = temporal_cases.make_case(base, w, h)
    rng = _rng("M-" + stratum, w, h)
    jj, ii = np.mgrid[0:h, 0:w]
    albedo = rng.uniform(0.05, 1.0, (h, w, 3)).astype(F)
    albedo[(ii + 3 * jj) % 7 == 0] = 5e-4  # (below the threshold: effective albedo 1)
    m1 = rng.uniform(0.1, 2.0, (h, w))
    hm = np.stack([m1, m1 * m1 + rng.uniform(0.0, 0.5, (h, w))], -1).astype(F)
    hs = rng.integers(1, 12, (h, w)).astype(np.int32)
    hs[(2 * ii + jj) % 5 == 0] = 0  # taps without a moment history beside taps with one
    if stratum == "non-finite":
        bad = rng.random((h, w))
        hm[..., 0][bad < 0.06] = np.nan
        hm[..., 1][(bad >= 0.06) & (bad < 0.12)] = np.inf
    if stratum == "saturate":
        hs = np.choose((ii + jj) % 4, [variance_f32.MAX_STEPS - 2, variance_f32.MAX_STEPS - 1, variance_f32.MAX_STEPS, variance_f32.MAX_STEPS + 5]).astype(np.int32)
    if stratum == "still" and w > 1:
        case["rgba"][..., :3] *= F(1e20)  # l l overflows in float32: moments that are not finite come out and go into stage S
    case.update(albedo=None if stratum == "ids" else albedo, moment_history=None if stratum == "no-moments" else (hm, hs))
    return case


def m_arguments(case):
    """what follows the parameters in variance_f32.reproject_moments, yhair_capi.reproject_moments and Context.reproject_moments_gpu"""
    return [case[k] for k in ("rgba", "samples", "ids", "position", "albedo", "history", "moment_history", "camera", "prev_camera", "frames", "prev_frames", "usable")]


@functools.lru_cache(maxsize=None)
def m_restated(stratum, w, h):
    case = make_m_case(stratum, w, h)
    res = variance_f32.reproject_moments(case["P"], *m_arguments(case))
    for a in res[:4]:
        a.setflags(write=False)
    return res


# ---- stage S ----
def make_s_case(stratum, w, h):
    rng = _rng("S-" + stratum, w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    ids = ((xs // 4 + ys // 3) % 3).astype(np.int32)
    ids[rng.random((h, w)) < 0.15] = -1
    pos = np.stack([0.1 * xs, 0.1 * ys, 0.3 * np.sin(0.4 * xs) + ids], -1).astype(F)
    m1 = rng.uniform(0.1, 2.0, (h, w))
    m = np.stack([m1, m1 * m1 + rng.uniform(-0.05, 0.5, (h, w))], -1).astype(F)
    steps = rng.integers(MIN_STEPS - 2, MIN_STEPS + 3, (h, w)).astype(np.int32)  # min_steps - 1, min_steps and min_steps + 1 among them
    steps[ids == -1] = 0
    P = dict(max_history=4, sigma_position=0.0, match_object=1)
    if stratum == "lonely":  # a window with only its centre valid
        steps[:] = 0
        steps[::8, ::8] = 1
        ids = np.abs(ids)
    elif stratum == "borders":  # young pixels along every border and in every corner
        ids = np.abs(ids)
        steps[:] = MIN_STEPS + 1
        steps[0, :] = steps[-1, :] = steps[:, 0] = steps[:, -1] = 1
    elif stratum == "non-finite":
        bad = rng.random((h, w))
        m[..., 0][bad < 0.08] = np.nan
        m[..., 1][(bad >= 0.08) & (bad < 0.16)] = np.inf
        m[h // 2, w // 2] = np.nan  # a centre whatever the draw
        steps[h // 2, w // 2], ids[h // 2, w // 2] = 1, max(int(ids[h // 2, w // 2]), 0)
    elif stratum == "sigma":
        P["sigma_position"] = 0.25
        P["match_object"] = 0
    elif stratum == "settled":  # no pixel below min_steps: no tile reads a neighbour
        steps = np.where(ids == -1, 0, steps.clip(MIN_STEPS)).astype(np.int32)
    return dict(P=P, min_steps=MIN_STEPS, moments=m, steps=steps, ids=ids, position=pos)


def s_arguments(case):
    return [case[k] for k in ("min_steps", "moments", "steps", "ids", "position")]


@functools.lru_cache(maxsize=None)
def s_restated(stratum, w, h):
    case = make_s_case(stratum, w, h)
    var, info = variance_f32.spatial(case["P"], *s_arguments(case))
    var.setflags(write=False)
    return var, info


# ---- stage F ----
def make_f_case(stratum, w, h):
    """(variance parameters without `iterations`, rgba, variance, ids, normal, position, albedo)"""
    base = {"luminance": "color", "v-zero": "full", "v-non-finite": "misses"}.get(stratum, stratum)
    P, rgba, ids, n, x, a = denoise_cases.make_case(base, w, h)
    rng = _rng("F-" + stratum, w, h)
    V = variance_f32.variance_params(sigma_luminance=P["sigma_color"] * 2.0, sigma_normal=P["sigma_normal"], sigma_position=P["sigma_position"],
                                     demodulate=P["demodulate"], match_object=P["match_object"], epsilon=1e-3, min_steps=MIN_STEPS)
    del V["iterations"]
    var = (rng.uniform(0.0, 0.3, (h, w)) ** 2).astype(F)
    if stratum == "v-zero":
        var[:] = 0
    elif stratum == "v-non-finite":
        bad = rng.random((h, w))
        var[bad < 0.06] = np.nan
        var[(bad >= 0.06) & (bad < 0.12)] = np.inf
        var[h // 2, w // 2] = np.nan  # a centre whatever the draw
    return V, rgba, var, ids, n, x, a


@functools.lru_cache(maxsize=None)
def f_restated(stratum, w, h, iterations):
    V, *arrays = make_f_case(stratum, w, h)
    out, var, info = variance_f32.atrous_variance_filter(dict(V, iterations=iterations), *arrays)
    out.setflags(write=False), var.setflags(write=False)
    return out, var, info


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a
