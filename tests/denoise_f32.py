"""The a-trous filter of yh_denoise (include/yhair.h: DENOISE) restated in numpy from the interface's prose — not from
unit/atrous_math.h — one float32 operation per arithmetic step, in the order the prose gives, so that its bits are the library's.

`dtype` exists for tests/denoise_f64.py, which runs the same formula in float64; every decision the prose states on float32 values (the
albedo threshold 1e-3f) is then taken on the same constants."""
import numpy as np

F = np.float32
KERNEL = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)  # k[|d|], exact in either format


def params_dict(iterations=5, sigma_color=0.0, sigma_normal=0.0, sigma_position=0.0, demodulate=0, match_object=0):
    return dict(iterations=iterations, sigma_color=sigma_color, sigma_normal=sigma_normal, sigma_position=sigma_position,
                demodulate=demodulate, match_object=match_object)


def _dist2(p, q):
    d = p - q
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def effective_albedo(albedo, ids, demodulate, dtype=F):
    """Per channel (a < 1e-3f) ? 1 : a; 1 without demodulation and on a miss."""
    h, w = ids.shape
    if not demodulate or albedo is None:
        return np.ones((h, w, 3), dtype)
    a = np.asarray(albedo, F)
    eff = np.where(a < F(1e-3), F(1), a).astype(dtype)
    eff[ids == -1] = 1
    return eff


def atrous_filter(P, rgba, ids, normal=None, position=None, albedo=None, dtype=F):
    """(H, W, 4) rgba, (H, W) int ids, (H, W, 3) planes -> the filtered (H, W, 4) image in `dtype`."""
    T = dtype
    rgba = np.asarray(rgba, F)
    ids = np.asarray(ids, np.int32)
    h, w = ids.shape
    if P["iterations"] == 0:
        return rgba.astype(T)
    one = T(1)
    eff = effective_albedo(albedo, ids, P["demodulate"], T)
    with np.errstate(all="ignore"):
        u = rgba[..., :3].astype(T) / eff
        n = np.asarray(normal, F).astype(T) if P["sigma_normal"] > 0 else None
        x = np.asarray(position, F).astype(T) if P["sigma_position"] > 0 else None
        sn2 = T(F(P["sigma_normal"])) * T(F(P["sigma_normal"]))
        sx2 = T(F(P["sigma_position"])) * T(F(P["sigma_position"]))
        miss = ids == -1
        ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
        for level in range(P["iterations"]):
            s = 1 << level
            scl = T(F(P["sigma_color"])) * T(1.0 / s)
            sc2 = scl * scl
            acc = np.zeros((h, w, 3), T)
            sw = np.zeros((h, w), T)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + s * dy, xs + s * dx
                    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                    qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    uq = u[qy, qx]
                    hk = T(KERNEL[abs(dx)]) * T(KERNEL[abs(dy)])
                    xn = _dist2(n, n[qy, qx]) / sn2 if n is not None else T(0)
                    xx = _dist2(x, x[qy, qx]) / sx2 if x is not None else T(0)
                    xc = _dist2(u, uq) / sc2 if P["sigma_color"] > 0 else T(0)
                    xt = xn + xx + xc
                    wgt = hk / (one + xt + T(0.5) * xt * xt)
                    ok = inside & np.isfinite(uq).all(-1) & (xt >= 0)
                    if P["match_object"]:
                        ok &= ids[qy, qx] == ids
                    wgt = np.where(ok, wgt, T(0)) * np.ones((h, w), T)
                    add = wgt != 0  # a tap of weight 0 is not added
                    acc = np.where(add[..., None], acc + wgt[..., None] * uq, acc)
                    sw = np.where(add, sw + wgt, sw)
            keep = miss | (sw == 0) | ~np.isfinite(u).all(-1)
            u = np.where(keep[..., None], u, acc / sw[..., None])
        out = np.empty((h, w, 4), T)
        out[..., :3] = u * eff
        out[..., 3] = rgba[..., 3]
    return out
