"""The start and the end of a path in float64 (pt.cpp:211-229, 1499-1507, 1676-1689), on the float32 inputs of tests/path_cases.py:
the independent restatement that tests/test_path_ends.py measures the camera ray against and that tests/test_path_cases.py holds to
the oracle. Every comparison of path_continue and path_end is between float32 values, so the DECISIONS made here are exact; only the
products and quotients differ from float arithmetic, in the last place."""
import types

import numpy as np

F = np.float32
PIF = np.float64(F(3.14159274101257324))  # (float)pi, as the reference multiplies by it
P99 = np.float64(F(0.99))


def _normalize(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def begin64(cams, ijwh, d4):
    """sample_camera (pt.cpp:211-229) with sample_disk (math.h:4895-4899) for the draws d4 = lu, lv, pu, pv: (origin, direction), float64."""
    cams, ijwh, d4 = np.asarray(cams, np.float64), np.asarray(ijwh, np.float64), np.asarray(d4, np.float64)
    frame, lens, film, focus, aperture = cams[:, :12].reshape(-1, 4, 3), cams[:, 12], cams[:, 13:15], cams[:, 15], cams[:, 16]
    lu, lv, pu, pv = d4.T
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u, v = (ijwh[:, 0] + pu) / ijwh[:, 2], (ijwh[:, 1] + pv) / ijwh[:, 3]
        r, phi = np.sqrt(lv), 2 * PIF * lu
        q = np.stack([film[:, 0] * (0.5 - u), film[:, 1] * (v - 0.5), lens], axis=1)
        dc = -_normalize(q)
        e = np.stack([np.cos(phi) * r * aperture / 2, np.sin(phi) * r * aperture / 2, np.zeros_like(r)], axis=1)
        p = dc * focus[:, None] / np.abs(dc[:, 2:3])
        d = _normalize(p - e)
        origin = np.einsum("nk,nkc->nc", e, frame[:, :3]) + frame[:, 3]
        direction = _normalize(np.einsum("nk,nkc->nc", d, frame[:, :3]))
    return origin, direction


def continue64(weight, bb, draw):
    """path_continue / the tail of trace_path's loop. draw: each row's next draw. dead: zero or non-finite weight; roulette: the draw was
    made; killed: by the draw; flag, bounce: as returned; weight: afterwards (float64)."""
    w, draw = np.asarray(weight, np.float64), np.asarray(draw, np.float64)
    bounce, bounces = np.asarray(bb)[:, 0].astype(np.int64), np.asarray(bb)[:, 1].astype(np.int64)
    dead = (w == 0).all(axis=1) | ~np.isfinite(w).all(axis=1)
    roulette = ~dead & (bounce > 3)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rr = np.minimum(P99, np.nanmax(np.where(np.isnan(w), -np.inf, w), axis=1))
        killed = roulette & (draw >= rr)
        scaled = w * (1 / rr)[:, None]
    survives = ~dead & ~killed
    out_w = np.where((roulette & ~killed)[:, None], scaled, w)
    out_bounce = np.where(survives, bounce + 1, bounce)
    return types.SimpleNamespace(dead=dead, roulette=roulette, killed=killed, flag=survives & (out_bounce < bounces), bounce=out_bounce, weight=out_w)


def end64(rad, hit):
    """path_end / the tail of trace_sample. sanitized: the radiance was non-finite; clamped: it was scaled; acc: afterwards (float64)."""
    rad = np.asarray(rad, np.float64)
    rgb, clamp, acc = rad[:, :3], rad[:, 3], rad[:, 4:8].copy()
    sanitized = ~np.isfinite(rgb).all(axis=1)
    rgb = np.where(sanitized[:, None], 0.0, rgb)
    top = rgb.max(axis=1)
    clamped = top > clamp
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rgb = np.where(clamped[:, None], rgb * (clamp / top)[:, None], rgb)
    acc[:, :3] += rgb
    acc[:, 3] += (np.asarray(hit).reshape(-1) != 0)
    return types.SimpleNamespace(sanitized=sanitized, clamped=clamped, acc=acc)
