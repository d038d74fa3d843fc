"""Synthetic inputs of the temporal stage for the CPU and GPU tests of yh_reproject: analytic scenes of rectangles and spheres seen by two
cameras, one builder per stratum. Ids and positions come from float64 ray intersections of the centre-mode ray (unit/gbuffer.hip) and are
cast to float32; colours, alphas and history lengths are seeded noise. A case is a dict with the arguments of reproject_f32.reproject."""
import functools
import zlib

import numpy as np

import reproject_f32
from reproject_f32 import params_dict

F = np.float32
SIZES = ((1, 1), (17, 33), (64, 64), (130, 70))  # width x height
STRATA = ("still", "pan", "orbit", "behind", "edges", "ids", "lengths", "non-finite", "sigma", "moving")
SIGMA = 2.0 ** -3  # the `sigma` stratum's sigma_position: 128 steps of its 2^-10 position grid


def _rng(name, w, h):
    return np.random.default_rng(zlib.crc32(f"temporal-{name}-{w}x{h}".encode()))


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def camera(eye, at, w, h, up=(0, 1, 0), lens=0.05, film=0.036, scale=(1.0, 1.0)):
    """17 floats: a camera at `eye` looking at `at` (down its -z axis), square pixels for a w x h image; scale: the film's, per axis"""
    z = _unit(np.subtract(eye, at))
    x = _unit(np.cross(up, z))
    y = np.cross(z, x)
    return np.concatenate([x, y, z, eye, [lens, film * scale[0], film * h / w * scale[1], 10000.0, 0.0]]).astype(F)


def rotation(axis, degrees):
    a, t = _unit(axis), np.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def frame_of(R=np.eye(3), t=(0, 0, 0)):
    """12 floats: the columns of R, then t"""
    return np.concatenate([np.asarray(R, np.float64).T.reshape(9), t]).astype(F)


# the objects, in object space: ("rect", half x, half z) in the plane y = 0, or ("sphere", radius) at the origin
STATIC = ((("rect", 2.2, 3.0), frame_of(t=(0, 0, -2))),                              # 0 the floor
          (("rect", 2.0, 1.3), frame_of(rotation((1, 0, 0), 90), (0, 1.3, -4.5))),   # 1 the back wall (the rays above and beside it miss)
          (("sphere", 1.0), frame_of(t=(0, 1, -2))))                                 # 2
EYE, AT = (0.3, 1.6, 3.0), (0.0, 0.9, -2.0)


def trace(cam, w, h, objects):
    """(ids, positions) of the centre-mode rays of `cam` (float32 values, float64 arithmetic) against [(shape, frame12)]"""
    cam = cam.astype(np.float64)
    jj, ii = np.mgrid[0:h, 0:w]
    u, v = (ii + 0.5) / w, (jj + 0.5) / h
    d = np.stack([cam[13] * (u - 0.5), cam[14] * (0.5 - v), np.full((h, w), -cam[12])], -1)
    d = d[..., 0:1] * cam[0:3] + d[..., 1:2] * cam[3:6] + d[..., 2:3] * cam[6:9]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = cam[9:12]
    best, ids = np.full((h, w), np.inf), np.full((h, w), -1, np.int32)
    for k, (shape, frame) in enumerate(objects):
        f = frame.astype(np.float64)
        M = f[:9].reshape(3, 3).T
        Mi = np.linalg.inv(M)
        lo, ld = Mi @ (o - f[9:12]), d @ Mi.T
        with np.errstate(all="ignore"):
            if shape[0] == "rect":
                t = -lo[1] / ld[..., 1]
                p = lo + t[..., None] * ld
                ok = (t > 1e-6) & (np.abs(p[..., 0]) <= shape[1]) & (np.abs(p[..., 2]) <= shape[2])
            else:
                a, b, c = (ld * ld).sum(-1), (ld * lo).sum(-1), lo @ lo - shape[1] ** 2
                disc = b * b - a * c
                t = (-b - np.sqrt(disc)) / a
                ok = (disc > 0) & (t > 1e-6)
        ok &= t < best
        best, ids = np.where(ok, t, best), np.where(ok, k, ids).astype(np.int32)
    pos = np.where((ids >= 0)[..., None], o + np.where(np.isfinite(best), best, 0)[..., None] * d, 0.0)
    return ids, pos.astype(F)


def _colours(rng, pos, ids):
    h, w = ids.shape
    smooth = np.stack([0.5 + 0.4 * np.sin(1.3 * pos[..., 0] + k) * np.cos(0.9 * pos[..., 2] - k) for k in range(3)], -1)
    rgb = smooth * rng.uniform(0.5, 1.5, (h, w, 3))
    return np.concatenate([rgb, rng.uniform(0, 1, (h, w, 1))], -1).astype(F)


def make_case(stratum, w, h):
    rng = _rng(stratum, w, h)
    P, n = params_dict(max_history=32, sigma_position=0.25, match_object=1), 4
    objects = prev_objects = [(s, f) for s, f in STATIC]
    usable = None
    cam = camera(EYE, AT, w, h)
    pan = camera(np.add(EYE, (0.13, 0.07, 0)), np.add(AT, (0.13, 0.07, 0)), w, h)
    orbit = camera(AT + rotation((0, 1, 0), 3.0) @ np.subtract(EYE, AT), AT, w, h)
    pcam = {"still": cam, "sigma": cam, "moving": cam, "orbit": orbit, "lengths": orbit}.get(stratum, pan)
    if stratum == "behind":  # the previous camera stands where this one does and faces the other way
        pcam = camera(EYE, 2 * np.asarray(EYE) - AT, w, h)
    if stratum == "edges":  # the same pose with a smaller film: column 0 falls on fx = -0.5, column w - 1 on w - 0.5, rows likewise
        s = [1 + 0.5 / (m / 2 - 0.5) if m > 1 else 1.5 for m in (w, h)]
        pcam = camera(EYE, AT, w, h, scale=(1 / s[0], 1 / s[1]))
        objects = prev_objects = [(("rect", 30.0, 30.0), STATIC[0][1]), (("rect", 30.0, 30.0), STATIC[1][1]), STATIC[2]]  # (hits along every border)
    if stratum == "moving":  # four spheres in front of the wall: frames bit-equal, translated, rotated and scaled, unusable
        centres = ((-1.8, 0.8, -1.5), (-0.6, 0.8, -1.0), (0.6, 0.8, -1.0), (1.8, 0.8, -1.5))
        now = [frame_of(t=centres[0]), frame_of(t=centres[1]), frame_of(1.1 * rotation((0.3, 1, 0.2), 25), centres[2]), frame_of(t=centres[3])]
        was = [now[0].copy(), frame_of(t=np.add(centres[1], (0.11, -0.05, 0.07))), frame_of(rotation((0, 0, 1), -10), np.add(centres[2], (0, 0.04, 0))),
               frame_of(t=np.add(centres[3], (0.02, 0, 0)))]
        objects = [(("sphere", 0.55), f) for f in now] + [STATIC[0], STATIC[1]]
        prev_objects = [(("sphere", 0.55), f) for f in was] + [STATIC[0], STATIC[1]]
        usable = np.array([1, 1, 1, 0, 1, 1], np.int32)
        if w == 1:  # (the one pixel looks at the translated sphere)
            cam = pcam = camera(EYE, centres[1], w, h)
    ids, pos = trace(cam, w, h, objects)
    hids, hpos = trace(pcam, w, h, prev_objects)
    rgba, hrgba = _colours(rng, pos, ids), _colours(rng, hpos, hids)
    hlen = rng.integers(1, 21, (h, w)).astype(np.int32)
    hlen[hids == -1] = 0
    jj, ii = np.mgrid[0:h, 0:w]
    if stratum == "ids":
        hids = np.where(((ii + jj) & 1) == 1, hids + 10, hids).astype(np.int32)
    elif stratum == "lengths":
        P["max_history"] = 8
        hlen = rng.integers(1, 101, (h, w)).astype(np.int32)
        hlen[(3 * ii + 5 * jj) % 4 == 1] = 0
        hlen[(3 * ii + 5 * jj) % 11 == 3] = -2
    elif stratum == "non-finite":
        bad = rng.random((h, w, 3))
        bad[0, 0] = 1.0  # (pixel (0, 0) stays clean: it is the whole 1 x 1 case)
        hrgba[..., :3][bad < 0.05] = np.nan
        hrgba[..., :3][(bad >= 0.05) & (bad < 0.10)] = np.inf
        rgba[..., :3][(bad >= 0.10) & (bad < 0.13)] = -np.inf
        rgba[..., :3][(bad >= 0.13) & (bad < 0.16)] = np.nan
        pos[(bad >= 0.16) & (bad < 0.18)] = np.nan
        hpos[(bad >= 0.18) & (bad < 0.20)] = np.inf
    elif stratum == "sigma":  # positions on the 2^-10 grid; the history's offset by exactly sigma, by one grid step more, or by sigma's next float
        P["sigma_position"] = SIGMA
        pos = (np.round(pos.astype(np.float64) * 1024) / 1024).astype(F)
        kind = (ii + 2 * jj) % 3
        pos[..., 0] = np.where(kind == 2, 0, pos[..., 0])
        hpos, hids = pos.copy(), ids.copy()
        hlen = np.where(ids >= 0, hlen.clip(1), 0).astype(np.int32)
        hpos[..., 0] = np.where(kind == 0, pos[..., 0] + F(SIGMA), np.where(kind == 1, pos[..., 0] + F(SIGMA + 2.0 ** -10), np.nextafter(F(SIGMA), F(1))))
    frames = prev_frames = None
    if stratum == "moving":
        frames, prev_frames = np.stack([f for _, f in objects]), np.stack([f for _, f in prev_objects])
    return dict(P=P, samples=n, rgba=rgba, ids=ids, position=pos, history=(hrgba, hlen, hids, hpos), camera=cam, prev_camera=pcam, frames=frames,
                prev_frames=prev_frames, usable=usable)


def arguments(case):
    """what follows the parameters in reproject_f32.reproject, yhair_capi.reproject and Context.reproject_gpu"""
    return [case[k] for k in ("rgba", "samples", "ids", "position", "history", "camera", "prev_camera", "frames", "prev_frames", "usable")]


@functools.lru_cache(maxsize=None)
def restated(stratum, w, h):
    """(out_rgba, out_length, info) of the float32 restatement on a case, computed once per session and shared (read-only)."""
    case = make_case(stratum, w, h)
    out, length, info = reproject_f32.reproject(case["P"], *arguments(case))
    out.setflags(write=False), length.setflags(write=False)
    return out, length, info


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a
