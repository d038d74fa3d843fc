"""The temporal stage of include/yhair.h (TEMPORAL) restated in numpy: every operation of unit/reproject_math.h in float32, in its order,
over whole images at once. yh_reproject and yh_reproject_gpu are compared with this bit for bit. With dtype=np.float64 the same formula
in double (tests/reproject_f64.py); the bit-equal rules (frames, cameras) read the float32 inputs either way.

reproject(P, rgba, samples, ids, position, history, camera, prev_camera, frames, prev_frames, usable) -> (out_rgba, out_length, info)
  P         dict(max_history, sigma_position, match_object)
  history   None, or (rgba, length, ids, position) of the previous step
  cameras   17 floats: frame (x, y, z axes, origin), lens, film x, film y, focus, aperture
  frames    (n, 12) per object, or None: no motion is given
  info      per-pixel masks and the projection, for the tests of the strata (tests/test_temporal_cases.py)
"""
import numpy as np

F = np.float32
U = np.uint32


def params_dict(max_history=32, sigma_position=0.0, match_object=1):
    return dict(max_history=max_history, sigma_position=sigma_position, match_object=match_object)


def _bits_equal(a, b):
    return np.ascontiguousarray(a, F).view(U) == np.ascontiguousarray(b, F).view(U)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def transform_point(f, b):
    """unit/object_math.h: ld3(f) * b.x + ld3(f + 3) * b.y + ld3(f + 6) * b.z + ld3(f + 9)"""
    return ((f[..., 0:3] * b[..., 0:1] + f[..., 3:6] * b[..., 1:2]) + f[..., 6:9] * b[..., 2:3]) + f[..., 9:12]


def inverse_frames(f):
    """unit/object_math.h: inverse_frame(f, non_rigid = true), rows of 12"""
    x, y, z, o = f[..., 0:3], f[..., 3:6], f[..., 6:9], f[..., 9:12]
    c0, c1, c2 = cross(y, z), cross(z, x), cross(x, y)
    s = (f.dtype.type(1) / dot(x, cross(y, z)))[..., None]
    rx = np.stack([c0[..., 0], c1[..., 0], c2[..., 0]], -1) * s
    ry = np.stack([c0[..., 1], c1[..., 1], c2[..., 1]], -1) * s
    rz = np.stack([c0[..., 2], c1[..., 2], c2[..., 2]], -1) * s
    ro = -((rx * o[..., 0:1] + ry * o[..., 1:2]) + rz * o[..., 2:3])
    return np.concatenate([rx, ry, rz, ro], -1)


def project(cam, y, W, H):
    """Step 3 without its refusals: (lz, fx, fy) of world points y in camera `cam`"""
    T = y.dtype.type
    d = y - cam[9:12]
    lx, ly, lz = dot(d, cam[0:3]), dot(d, cam[3:6]), dot(d, cam[6:9])
    u = T(0.5) - (cam[12] * lx) / (cam[13] * lz)
    v = T(0.5) + (cam[12] * ly) / (cam[14] * lz)
    return lz, u * T(W) - T(0.5), v * T(H) - T(0.5)


def reproject(P, rgba, samples, ids, position, history, camera, prev_camera=None, frames=None, prev_frames=None, usable=None, dtype=F):
    T = np.dtype(dtype).type
    rgba32, ids = np.ascontiguousarray(rgba, F), np.ascontiguousarray(ids, np.int32)
    H, W = ids.shape
    c, x = rgba32.astype(T), np.ascontiguousarray(position, F).astype(T)
    n = int(samples)
    out, length = c.copy(), np.zeros((H, W), np.int32)
    live = (ids != -1) & np.isfinite(rgba32[..., :3]).all(-1)  # 1. pass-through
    length[live] = n
    info = dict(live=live, history=np.zeros((H, W), bool))
    if history is None:
        return out, length, info
    hr, hl, hi, hp = history
    hr32 = np.ascontiguousarray(hr, F)
    hc, hl, hi, hx = hr32.astype(T), np.ascontiguousarray(hl, np.int32), np.ascontiguousarray(hi, np.int32), np.ascontiguousarray(hp, F).astype(T)
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
        front = lz < 0
        inside = np.isfinite(fx) & np.isfinite(fy) & (T(-1) < fx) & (fx < T(W)) & (T(-1) < fy) & (fy < T(H))
        cand = live & use & front & inside
        # 4. taps
        shortcut = still if same_camera else np.zeros((H, W), bool)
        jj, ii = np.mgrid[0:H, 0:W]
        fxs, fys = np.where(cand, fx, T(0)), np.where(cand, fy, T(0))
        i0f, j0f = np.floor(fxs), np.floor(fys)
        tx, ty = fxs - i0f, fys - j0f
        i0, j0 = i0f.astype(np.int64), j0f.astype(np.int64)
        one = T(1)
        taps = [(i0, j0, (one - tx) * (one - ty)), (i0 + 1, j0, tx * (one - ty)), (i0, j0 + 1, (one - tx) * ty), (i0 + 1, j0 + 1, tx * ty)]
        # 5., 6. the valid taps, summed in tap order
        s2 = T(F(P["sigma_position"])) * T(F(P["sigma_position"]))
        acc, S = np.zeros((H, W, 3), T), np.zeros((H, W), T)
        N = np.full((H, W), 0x7fffffff, np.int64)
        why = {k: np.zeros((H, W), bool) for k in ("off_image", "empty", "other_id", "non_finite", "far")}
        for k, (qx, qy, w) in enumerate(taps):
            qx, qy, w = np.where(shortcut, ii, qx), np.where(shortcut, jj, qy), np.where(shortcut, one, w)
            on = cand & ~(shortcut & (k > 0))
            ok = on & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            why["off_image"] |= on & ~ok
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            qlen, qid, qc, qpos = hl[cy, cx], hi[cy, cx], hc[cy, cx], hx[cy, cx]
            step = ok & (qlen > 0)
            why["empty"] |= ok & ~step
            ok = step
            if P["match_object"]:
                step = ok & (qid == ids)
                why["other_id"] |= ok & ~step
                ok = step
            step = ok & np.isfinite(hr32[cy, cx, :3]).all(-1)
            why["non_finite"] |= ok & ~step
            ok = step
            if P["sigma_position"] > 0:
                e = y - qpos
                step = ok & (dot(e, e) <= s2)
                why["far"] |= ok & ~step
                ok = step
            ok = ok & (w != 0)
            acc = np.where(ok[..., None], acc + w[..., None] * qc[..., :3], acc)
            S = np.where(ok, S + w, S)
            N = np.where(ok, np.minimum(N, qlen), N)
        took = cand & (S > 0)
        N = np.minimum(N, int(P["max_history"]))
        # 7. blend
        h = acc / S[..., None]
        a = T(n) / (N + n).astype(T)
        blend = h + (c[..., :3] - h) * a[..., None]
    out[..., :3] = np.where(took[..., None], blend, c[..., :3])
    length = np.where(took, N + n, length).astype(np.int32)
    info.update(history=took, unusable=live & ~use, behind=live & use & ~front, outside=live & use & front & ~inside, no_weight=cand & ~took,
                shortcut=cand & shortcut, fx=fx, fy=fy, lz=lz, candidates=cand, **{"tap_" + k: v for k, v in why.items()})
    return out, length, info
