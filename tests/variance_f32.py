"""The variance stage of include/yhair.h (VARIANCE) restated in numpy from the interface's prose — not from unit/variance_math.h — one
float32 operation per arithmetic step, in the order the prose gives, over whole images at once, so that its bits are the library's. Stage M
repeats TEMPORAL's steps 1 - 7 (tests/reproject_f32.py has them for the colour alone) because the moments share its taps and weights.
With dtype=np.float64 the same formulas in double (tests/variance_f64.py); every decision the prose states on float32 inputs (bit-equal
frames and cameras, the albedo threshold) is then taken on the same values.

reproject_moments(P, rgba, samples, ids, position, albedo, history, moment_history, camera, ...) -> (out_rgba, out_length, moments, steps, info)
spatial(P, min_steps, moments, steps, ids, position)                                              -> (variance, info)
atrous_variance_filter(V, rgba, variance, ids, normal, position, albedo)                          -> (out_rgba, out_variance, info)
  P   dict(max_history, sigma_position, match_object)                      V   variance_params(...)
  info: per-pixel masks and counts, for the tests that prove the strata hit their edges"""
import numpy as np

from denoise_f32 import KERNEL, _dist2, effective_albedo
from reproject_f32 import _bits_equal, dot, inverse_frames, project, transform_point

F = np.float32
MAX_STEPS = 1024
K3 = (1.0 / 4.0, 1.0 / 8.0, 1.0 / 16.0)  # by |dx| + |dy|, exact in either format


def variance_params(iterations=5, sigma_luminance=0.0, sigma_normal=0.0, sigma_position=0.0, demodulate=0, match_object=0, epsilon=1e-4, min_steps=4):
    return dict(iterations=iterations, sigma_luminance=sigma_luminance, sigma_normal=sigma_normal, sigma_position=sigma_position, demodulate=demodulate,
                match_object=match_object, epsilon=epsilon, min_steps=min_steps)


def lum(v):
    T = v.dtype.type
    return (T(F(0.2126)) * v[..., 0] + T(F(0.7152)) * v[..., 1]) + T(F(0.0722)) * v[..., 2]


def variance_of(m1, m2):
    d = m2 - m1 * m1
    return np.where(d > 0, d, d.dtype.type(0))


def reproject_moments(P, rgba, samples, ids, position, albedo, history, moment_history, camera, prev_camera=None, frames=None, prev_frames=None, usable=None,
                      dtype=F):
    T = np.dtype(dtype).type
    rgba32, ids = np.ascontiguousarray(rgba, F), np.ascontiguousarray(ids, np.int32)
    H, W = ids.shape
    c, x = rgba32.astype(T), np.ascontiguousarray(position, F).astype(T)
    n = int(samples)
    out, length = c.copy(), np.zeros((H, W), np.int32)
    live = (ids != -1) & np.isfinite(rgba32[..., :3]).all(-1)  # 1. pass-through
    length[live] = n
    with np.errstate(all="ignore"):
        lu = lum(c[..., :3] / effective_albedo(albedo, ids, albedo is not None, T))
        m = np.stack([lu, lu * lu], -1)
    moments = np.where(live[..., None], m, T(0))
    steps = live.astype(np.int32)
    info = dict(live=live, history=np.zeros((H, W), bool), moment_history=np.zeros((H, W), bool), invalid_taps=np.zeros((H, W), np.int32),
                mixed_steps=np.zeros((H, W), bool), shortcut=np.zeros((H, W), bool), taps_added=np.zeros((H, W), np.int32))
    if history is None:
        return out, length, moments, steps, info
    hr, hl, hi, hp = history
    hr32 = np.ascontiguousarray(hr, F)
    hc, hl, hi, hx = hr32.astype(T), np.ascontiguousarray(hl, np.int32), np.ascontiguousarray(hi, np.int32), np.ascontiguousarray(hp, F).astype(T)
    if moment_history is None:
        hm, hs = np.zeros((H, W, 2), T), np.zeros((H, W), np.int32)
    else:
        hm, hs = np.ascontiguousarray(moment_history[0], F).astype(T), np.ascontiguousarray(moment_history[1], np.int32)
    cam32, pcam32 = np.ascontiguousarray(camera, F).reshape(17), np.ascontiguousarray(prev_camera, F).reshape(17)
    same_camera = bool(_bits_equal(cam32, pcam32).all())
    pcam = pcam32.astype(T)
    with np.errstate(all="ignore"):
        # 2. the previous world position
        y, still, use = x, np.ones((H, W), bool), np.ones((H, W), bool)
        if frames is not None and len(frames) > 0:
            fr32, pf32 = np.ascontiguousarray(frames, F).reshape(-1, 12), np.ascontiguousarray(prev_frames, F).reshape(-1, 12)
            known = (ids >= 0) & (ids < len(fr32))
            row = np.where(known, ids, 0)
            moved = known & ~_bits_equal(fr32, pf32).all(-1)[row]
            inv = inverse_frames(fr32.astype(T))
            y = np.where(moved[..., None], transform_point(pf32.astype(T)[row], transform_point(inv[row], x)), x)
            still = ~moved
            if usable is not None:
                use = ~(known & (np.ascontiguousarray(usable, np.int32)[row] == 0))
        # 3. projection into the previous camera
        lz, fx, fy = project(pcam, y, W, H)
        inside = np.isfinite(fx) & np.isfinite(fy) & (T(-1) < fx) & (fx < T(W)) & (T(-1) < fy) & (fy < T(H))
        cand = live & use & (lz < 0) & inside
        # 4. taps
        shortcut = still if same_camera else np.zeros((H, W), bool)
        jj, ii = np.mgrid[0:H, 0:W]
        fxs, fys = np.where(cand, fx, T(0)), np.where(cand, fy, T(0))
        i0f, j0f = np.floor(fxs), np.floor(fys)
        tx, ty = fxs - i0f, fys - j0f
        i0, j0 = i0f.astype(np.int64), j0f.astype(np.int64)
        one = T(1)
        taps = [(i0, j0, (one - tx) * (one - ty)), (i0 + 1, j0, tx * (one - ty)), (i0, j0 + 1, (one - tx) * ty), (i0 + 1, j0 + 1, tx * ty)]
        # 5., 6. the valid taps, summed in tap order; the moments take every tap the colour takes
        s2 = T(F(P["sigma_position"])) * T(F(P["sigma_position"]))
        acc, am, S = np.zeros((H, W, 3), T), np.zeros((H, W, 2), T), np.zeros((H, W), T)
        N, Tm, Tmax = np.full((H, W), 0x7fffffff, np.int64), np.full((H, W), 0x7fffffff, np.int64), np.full((H, W), -1, np.int64)
        added, offered = np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)
        for k, (qx, qy, w) in enumerate(taps):
            qx, qy, w = np.where(shortcut, ii, qx), np.where(shortcut, jj, qy), np.where(shortcut, one, w)
            on = cand & ~(shortcut & (k > 0))
            ok = on & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            qlen, qid, qc, qpos = hl[cy, cx], hi[cy, cx], hc[cy, cx], hx[cy, cx]
            ok &= qlen > 0
            if P["match_object"]:
                ok &= qid == ids
            ok &= np.isfinite(hr32[cy, cx, :3]).all(-1)
            if P["sigma_position"] > 0:
                e = y - qpos
                ok &= dot(e, e) <= s2
            ok &= w != 0
            offered += on
            added += ok
            acc = np.where(ok[..., None], acc + w[..., None] * qc[..., :3], acc)
            am = np.where(ok[..., None], am + w[..., None] * hm[cy, cx], am)
            S = np.where(ok, S + w, S)
            N = np.where(ok, np.minimum(N, qlen), N)
            Tm = np.where(ok, np.minimum(Tm, hs[cy, cx]), Tm)
            Tmax = np.where(ok, np.maximum(Tmax, hs[cy, cx]), Tmax)
        took = cand & (S > 0)
        N = np.minimum(N, int(P["max_history"]))
        # 7. blend
        h = acc / S[..., None]
        a = T(n) / (N + n).astype(T)
        blend = h + (c[..., :3] - h) * a[..., None]
        Hm = am / S[..., None]
        with_m = took & (Tm > 0) & np.isfinite(Hm).all(-1)
        mblend = Hm + (m - Hm) * a[..., None]
    out[..., :3] = np.where(took[..., None], blend, c[..., :3])
    length = np.where(took, N + n, length).astype(np.int32)
    moments = np.where(with_m[..., None], mblend, moments)
    steps = np.where(with_m, np.minimum(Tm, MAX_STEPS - 1) + 1, steps).astype(np.int32)
    info.update(history=took, moment_history=with_m, invalid_taps=np.where(cand, offered - added, 0), taps_added=np.where(cand, added, 0),
                mixed_steps=took & (Tm <= 0) & (Tmax > 0), shortcut=cand & shortcut, hm_non_finite=took & (Tm > 0) & ~np.isfinite(Hm).all(-1))
    return out, length, moments, steps, info


def spatial(P, min_steps, moments, steps, ids, position, dtype=F):
    T = np.dtype(dtype).type
    m32 = np.ascontiguousarray(moments, F)
    m, steps, ids = m32.astype(T), np.ascontiguousarray(steps, np.int32), np.ascontiguousarray(ids, np.int32)
    x = np.ascontiguousarray(position, F).astype(T)
    H, W = steps.shape
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    with np.errstate(all="ignore"):
        vt = variance_of(m[..., 0], m[..., 1])
        s2 = T(F(P["sigma_position"])) * T(F(P["sigma_position"]))
        a, k = np.zeros((H, W, 2), T), np.zeros((H, W), np.int32)
        cut = np.zeros((H, W), bool)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                qy, qx = ys + dy, xs + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                cut |= ~inside
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                ok = inside & (steps[qy, qx] > 0)
                if P["match_object"]:
                    ok &= ids[qy, qx] == ids
                if P["sigma_position"] > 0:
                    e = x - x[qy, qx]
                    ok &= dot(e, e) <= s2
                ok &= np.isfinite(m32[qy, qx]).all(-1)
                a = np.where(ok[..., None], a + m[qy, qx], a)
                k += ok
        A = a / k.astype(T)[..., None]
        e = A[..., 1] - A[..., 0] * A[..., 0]
        vs = np.where((k > 0) & (e > 0), e, T(0))
        window = (steps > 0) & (steps < min_steps)
        var = np.where(steps >= min_steps, vt, np.where(window, np.where(vt > vs, vt, vs), T(0)))
    return var, dict(window=window, count=np.where(window, k, 0), cut=window & cut)


def atrous_variance_filter(V, rgba, variance, ids, normal=None, position=None, albedo=None, dtype=F):
    T = np.dtype(dtype).type
    rgba, ids = np.asarray(rgba, F), np.asarray(ids, np.int32)
    var32 = np.asarray(variance, F)
    h, w = ids.shape
    info = dict(g_zero=np.zeros((h, w), bool), g_taps=np.full((h, w), 9, np.int32))
    if V["iterations"] == 0:
        return rgba.astype(T), var32.astype(T), info
    one = T(1)
    eff = effective_albedo(albedo, ids, V["demodulate"], T)
    with np.errstate(all="ignore"):
        u, v = rgba[..., :3].astype(T) / eff, var32.astype(T)
        n = np.asarray(normal, F).astype(T) if V["sigma_normal"] > 0 else None
        x = np.asarray(position, F).astype(T) if V["sigma_position"] > 0 else None
        sn2 = T(F(V["sigma_normal"])) * T(F(V["sigma_normal"]))
        sx2 = T(F(V["sigma_position"])) * T(F(V["sigma_position"]))
        sl, eps = T(F(V["sigma_luminance"])), T(F(V["epsilon"]))
        miss = ids == -1
        ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
        for level in range(V["iterations"]):
            s = 1 << level
            # the centre: the variance through the 3 x 3 kernel at spacing 1
            sv, sk, kt = np.zeros((h, w), T), np.zeros((h, w), T), np.zeros((h, w), np.int32)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    qy, qx = ys + dy, xs + dx
                    ok = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                    qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    vq = v[qy, qx]
                    ok &= np.isfinite(vq)
                    if V["match_object"]:
                        ok &= ids[qy, qx] == ids
                    k3 = T(K3[abs(dx) + abs(dy)])
                    sv = np.where(ok, sv + k3 * vq, sv)
                    sk = np.where(ok, sk + k3, sk)
                    kt += ok
            g = np.where(sk > 0, sv / sk, T(0))
            if level == 0:
                info.update(g_zero=~miss & (g == 0), g_taps=np.where(miss, 9, kt))
            sl2 = (sl * sl) * g + eps
            lp = lum(u)
            acc, av, sw = np.zeros((h, w, 3), T), np.zeros((h, w), T), np.zeros((h, w), T)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + s * dy, xs + s * dx
                    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                    qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    uq, vq = u[qy, qx], v[qy, qx]
                    hk = T(KERNEL[abs(dx)]) * T(KERNEL[abs(dy)])
                    xn = _dist2(n, n[qy, qx]) / sn2 if n is not None else T(0)
                    xx = _dist2(x, x[qy, qx]) / sx2 if x is not None else T(0)
                    dl = lp - lum(uq)
                    xl = (dl * dl) / sl2 if V["sigma_luminance"] > 0 else T(0)
                    xt = xn + xx + xl
                    wgt = hk / (one + xt + T(0.5) * xt * xt)
                    ok = inside & np.isfinite(uq).all(-1) & np.isfinite(vq) & (xt >= 0)
                    if V["match_object"]:
                        ok &= ids[qy, qx] == ids
                    wgt = np.where(ok, wgt, T(0)) * np.ones((h, w), T)
                    add = wgt != 0  # a tap of weight 0 is not added
                    acc = np.where(add[..., None], acc + wgt[..., None] * uq, acc)
                    av = np.where(add, av + (wgt * wgt) * vq, av)
                    sw = np.where(add, sw + wgt, sw)
            keep = miss | (sw == 0) | ~np.isfinite(u).all(-1)
            u = np.where(keep[..., None], u, acc / sw[..., None])
            v = np.where(keep, v, av / (sw * sw))
        out = np.empty((h, w, 4), T)
        out[..., :3] = u * eff
        out[..., 3] = rgba[..., 3]
    return out, v, info
