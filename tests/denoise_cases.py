"""Synthetic inputs of the a-trous filter for the CPU and GPU tests of yh_denoise: seeded images with their guide planes, one builder per
stratum. Every case is (parameters without `iterations`, rgba, ids, normal, position, albedo); the tests run each over iterations 0 .. 6,
so that a tap spacing of 32 exceeds every image here in at least one dimension."""
import functools
import zlib

import numpy as np

import denoise_f32
from denoise_f32 import params_dict

F = np.float32
SIZES = ((1, 1), (2, 3), (5, 5), (17, 19), (33, 65), (96, 40))  # width x height
ITERATIONS = tuple(range(7))
STRATA = ("all-off", "color", "normal", "position", "checker-match", "misses", "non-finite", "albedo-edges", "demodulate-off", "full")


def _rng(name, w, h):
    return np.random.default_rng(zlib.crc32(f"{name}-{w}x{h}".encode()))


def base_image(rng, w, h):
    """A smooth image with noise and a few outliers, ids in blobs, unit normals, positions on a bumpy sheet, albedo in [0.05, 1]."""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    smooth = np.stack([0.5 + 0.4 * np.sin(0.3 * xs + k) * np.cos(0.2 * ys - k) for k in range(3)], -1)
    rgb = smooth * rng.uniform(0.5, 1.5, (h, w, 3))
    rgb[rng.random((h, w)) < 0.03] *= 20.0  # fireflies
    rgba = np.concatenate([rgb, rng.uniform(0, 1, (h, w, 1))], -1).astype(F)
    ids = ((xs // 7 + ys // 5) % 3).astype(np.int32)
    n = np.stack([0.3 * np.sin(0.5 * xs), 0.3 * np.cos(0.4 * ys), np.ones((h, w))], -1) + rng.normal(0, 0.05, (h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    pos = np.stack([0.1 * xs, 0.1 * ys, 0.5 * np.sin(0.25 * xs) + ids], -1) + rng.normal(0, 0.01, (h, w, 3))
    alb = rng.uniform(0.05, 1.0, (h, w, 3))
    return rgba, ids, n.astype(F), pos.astype(F), alb.astype(F)


def make_case(stratum, w, h):
    rng = _rng(stratum, w, h)
    rgba, ids, n, x, a = base_image(rng, w, h)
    on = dict(sigma_color=0.8, sigma_normal=0.4, sigma_position=0.7)
    if stratum == "all-off":
        P = params_dict()
    elif stratum in ("color", "normal", "position"):
        P = params_dict(**{"sigma_" + stratum: on["sigma_" + stratum]})
    elif stratum == "checker-match":
        ys, xs = np.mgrid[0:h, 0:w]
        ids = ((xs + ys) & 1).astype(np.int32)
        P = params_dict(match_object=1, demodulate=1, **on)
    elif stratum == "misses":
        ids[rng.random((h, w)) < 0.3] = -1  # (their albedo stays non-zero: a miss has the effective albedo 1 all the same)
        P = params_dict(match_object=1, demodulate=1, **on)
    elif stratum == "non-finite":
        bad = rng.random((h, w, 3))
        rgba[..., :3][bad < 0.04] = np.nan
        rgba[..., :3][(bad >= 0.04) & (bad < 0.08)] = np.inf
        rgba[..., :3][(bad >= 0.08) & (bad < 0.10)] = -np.inf
        rgba[h // 2, w // 2, :3] = np.nan  # a NaN centre whatever the draw
        P = params_dict(demodulate=1, **on)
    elif stratum == "albedo-edges":
        t = F(1e-3)
        edges = np.array([0.0, t, np.nextafter(t, F(0)), np.nextafter(t, F(1)), 1.0, np.nextafter(F(1), F(0)), 5e-4, 2e-3], F)
        a = edges[rng.integers(0, len(edges), (h, w, 3))]
        P = params_dict(demodulate=1, match_object=1, **on)
    elif stratum == "demodulate-off":
        P = params_dict(demodulate=0, match_object=1, **on)
    elif stratum == "full":
        P = params_dict(demodulate=1, match_object=1, **on)
    else:
        raise KeyError(stratum)
    del P["iterations"]
    return P, rgba, ids, n, x, a


@functools.lru_cache(maxsize=None)
def restated(stratum, w, h, iterations):
    """The float32 restatement's image of a case, computed once per session and shared (read-only)."""
    P, *arrays = make_case(stratum, w, h)
    out = denoise_f32.atrous_filter(dict(P, iterations=iterations), *arrays)
    out.setflags(write=False)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a
