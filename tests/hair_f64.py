"""The hair BSDF in float64 (numpy): a restatement of csrc/dev_hair.h and oracle/yh_oracle.cpp (eval_hair_scattering,
sample_hair_scattering, sample_hair_scattering_pdf, compute_ap_pdf) that the unit tests of tests/test_hair_unit.py measure both the
oracle and the device against. Test infrastructure only.

The inputs — the 30 floats of a hair_brdf, the directions, the random numbers — are float32 values taken as exact. The formulas are the
ones the code has, not textbook ones: the ten-term i0 and its x > 12 asymptote, the v <= 0.1 form of mp with its 0.6931f, sinh in the
other form, compute_ap_pdf's re-derived sin_theta_o, the trimmed logistic over [-pi, pi], demux_float's integer de-interleave, the
1e-5 clamp, and the float constant pif wherever the code writes it. gamma_o alone is not taken from the 30 floats: it is asin(h) again,
so that its rounding to float counts as an error of whoever rounded it.

Branches the code takes on float32 values (v <= 0.1f, x > 12, the 2 pi wrap, u < 1e-5f) are taken on the float32 rounding of this
module's float64 value, so that both sides are on the same branch away from a boundary. Lobe selection is the exception: it compares
the float64 lobe pdfs, and boundaries() gives a test the cumulative pdfs to keep rows near a boundary apart.
"""
import numpy as np

F = np.float32
PIF = float(F(np.pi))           # (float)pi
LN2F = float(F(0.6931))         # mp's 0.6931f
EPS_U = float(F(1e-5))          # the clamp of u[1][0]
LUM = tuple(float(F(c)) for c in (0.2126, 0.7152, 0.0722))
P_MAX = 3
_I0_DEN = [1.0, 4.0, 64.0, 2304.0, 147456.0, 14745600.0, 2123366400.0, 416179814400.0, 106542032486400.0,
           34519618525593600.0]  # 4^i (i!)^2


def _f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(F)


def _safe_sqrt(x):
    return np.sqrt(np.maximum(0.0, x))


def _safe_asin(x):
    return np.arcsin(np.clip(x, -1.0, 1.0))


def _normalize(a):
    l = np.sqrt(np.sum(a * a, axis=-1, keepdims=True))
    return np.where(l != 0, a / np.where(l != 0, l, 1.0), a)


class Brdf:
    """The 30 floats of n hair_brdf rows as float64 fields."""

    def __init__(self, brdf30):
        b = np.asarray(brdf30, F).astype(np.float64).reshape(-1, 30)
        self.n = len(b)
        self.sigma_a, self.alpha, self.eta, self.h = b[:, 0:3], b[:, 3], b[:, 4], b[:, 5]
        self.v, self.s = b[:, 6:10], b[:, 10]
        self.v_le = np.asarray(brdf30, F).reshape(-1, 30)[:, 6:10] <= F(0.1)  # the branch of mp, on the floats themselves
        self.sin2k, self.cos2k = b[:, 11:14], b[:, 14:17]
        self.gamma_o = _safe_asin(self.h)
        self.M = b[:, 18:27].reshape(-1, 3, 3)  # M[j] = the j-th vector of world_to_brdf

    def to_local(self, w):
        return _normalize(np.einsum("njk,nj->nk", self.M, np.asarray(w, F).astype(np.float64)))

    def to_world(self, l):  # inverse(world_to_brdf, false): the transpose
        return _normalize(np.einsum("njk,nk->nj", self.M, l))


def i0(x):
    val, x2i = np.zeros_like(x), np.ones_like(x)
    for d in _I0_DEN:
        val = val + x2i / d
        x2i = x2i * (x * x)
    return val


def log_i0(x):
    big = _f32(x) > F(12)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        hi = x + 0.5 * (-np.log(2 * PIF) + np.log(1 / x) + 1 / (8 * x))
        lo = np.log(i0(np.where(big, 0.0, x)))
    return np.where(big, hi, lo)


def mp(cos_i, cos_o, sin_i, sin_o, v, v_le):
    a, b = cos_i * cos_o / v, sin_i * sin_o / v
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        small = np.exp(log_i0(a) - b - 1 / v + LN2F + np.log(1 / (2 * v)))
        vv = np.where(v_le, 1.0, v)
        big = np.exp(-b) * i0(np.where(v_le, 0.0, a)) / (np.sinh(1 / vv) * 2 * vv)
    return np.where(v_le, small, big)


def fresnel_dielectric_cos(eta, cosw):
    cosw = np.abs(cosw)
    sin2 = 1 - cosw * cosw
    cos2t = 1 - sin2 / (eta * eta)
    t0 = np.sqrt(np.maximum(cos2t, 0.0))
    t1, t2 = eta * t0, eta * cosw
    with np.errstate(invalid="ignore", divide="ignore"):
        rs, rp = (cosw - t1) / (cosw + t1), (t0 - t2) / (t0 + t2)
    return np.where(cos2t < 0, 1.0, (rs * rs + rp * rp) / 2)


def ap(cos_o, eta, h, T):
    """(n, 4, 3)"""
    cos_gamma_o = _safe_sqrt(1 - h * h)
    f = fresnel_dielectric_cos(eta, cos_o * cos_gamma_o)[:, None]
    a0 = np.repeat(f, 3, axis=1)
    a1 = (1 - f) ** 2 * T
    a2 = a1 * T * f
    with np.errstate(invalid="ignore", divide="ignore"):
        a3 = a2 * f * T / (1.0 - T * f)
    return np.stack([a0, a1, a2, a3], axis=1)


def transmittance(b, sin_o, cos_o):
    """T (n, 3) and gamma_t for (sin_theta_o, cos_theta_o)."""
    sin_t = sin_o / b.eta
    cos_t = _safe_sqrt(1 - sin_t * sin_t)
    with np.errstate(invalid="ignore", divide="ignore"):
        etap = np.sqrt(b.eta * b.eta - sin_o * sin_o) / cos_o
        sin_gt = b.h / etap
        cos_gt = _safe_sqrt(1 - sin_gt * sin_gt)
        T = np.exp(-b.sigma_a * (2 * cos_gt / cos_t)[:, None])
    return T, _safe_asin(sin_gt)


def phi_fn(p, gamma_o, gamma_t):
    return 2 * p * gamma_t - 2 * gamma_o + p * PIF


def np_(phi, p, s, gamma_o, gamma_t):
    dphi = phi - phi_fn(p, gamma_o, gamma_t)
    for _ in range(8):  # the code's while loops: |dphi| stays below 16
        dphi = np.where(_f32(dphi) > F(PIF), dphi - 2 * PIF, dphi)
    for _ in range(8):
        dphi = np.where(_f32(dphi) < F(-PIF), dphi + 2 * PIF, dphi)
    x = np.abs(dphi)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(-x / s)
        norm = 1 / (1 + np.exp(-PIF / s)) - 1 / (1 + np.exp(PIF / s))
        return e / (s * (1 + e) ** 2) / norm


def tilt(b, p, sin_o, cos_o):
    k = (1, 0, 2)[p] if p < 3 else None
    if k is None:
        return sin_o, cos_o
    c, s = b.cos2k[:, k], b.sin2k[:, k]
    if p == 0:
        return sin_o * c - cos_o * s, cos_o * c + sin_o * s
    return sin_o * c + cos_o * s, cos_o * c - sin_o * s


def _outgoing(b, wo):
    o = b.to_local(wo)
    sin_o = o[:, 0]
    return sin_o, _safe_sqrt(1 - sin_o * sin_o), np.arctan2(o[:, 2], o[:, 1])


def lobe_pdfs(b, wo):
    """compute_ap_pdf at the outgoing direction: (n, 4)."""
    _, cos_o, _ = _outgoing(b, wo)
    sin_o = _safe_sqrt(1 - cos_o * cos_o)  # re-derived (ext.cpp:372)
    T, _ = transmittance(b, sin_o, cos_o)
    y = np.einsum("npc,c->np", ap(cos_o, b.eta, b.h, T), np.array(LUM))
    with np.errstate(invalid="ignore", divide="ignore"):
        return y / np.sum(y, axis=1, keepdims=True)


def eval_pdf(b, wo, wi):
    """f (n, 3) and pdf (n) at wi."""
    sin_o, cos_o, phi_o = _outgoing(b, wo)
    i = b.to_local(wi)
    sin_i = i[:, 0]
    cos_i, phi_i = _safe_sqrt(1 - sin_i * sin_i), np.arctan2(i[:, 2], i[:, 1])
    T, gamma_t = transmittance(b, sin_o, cos_o)
    apv, q = ap(cos_o, b.eta, b.h, T), lobe_pdfs(b, wo)
    phi = phi_i - phi_o
    f, pdf = np.zeros((b.n, 3)), np.zeros(b.n)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(P_MAX):
            sop, cop = tilt(b, p, sin_o, cos_o)
            m = mp(cos_i, np.abs(cop), sin_i, sop, b.v[:, p], b.v_le[:, p]) * np_(phi, p, b.s, b.gamma_o, gamma_t)
            f, pdf = f + m[:, None] * apv[:, p], pdf + m * q[:, p]
        m = mp(cos_i, cos_o, sin_i, sin_o, b.v[:, 3], b.v_le[:, 3])
        return f + m[:, None] * apv[:, 3] / (2 * PIF), pdf + m * q[:, 3] * (1 / (2 * PIF))


def _compact1by1(x):
    x = x & np.uint32(0x55555555)
    x = (x ^ (x >> np.uint32(1))) & np.uint32(0x33333333)
    x = (x ^ (x >> np.uint32(2))) & np.uint32(0x0F0F0F0F)
    x = (x ^ (x >> np.uint32(4))) & np.uint32(0x00FF00FF)
    x = (x ^ (x >> np.uint32(8))) & np.uint32(0x0000FFFF)
    return x


def demux_float(f):
    """The two 16-bit halves of a float32 in [0, 1): its even and its odd bits, each over 65536 (exact)."""
    v = (np.asarray(f, F).astype(np.float64) * 4294967296.0).astype(np.uint64)
    a = _compact1by1((v & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    b = _compact1by1(((v >> np.uint64(1)) & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    return a.astype(np.float64) / 65536.0, b.astype(np.float64) / 65536.0


def mux_float(a16, b16):
    """The float32 whose demux_float halves are a16 / 65536 and b16 / 65536 — exact when the interleaved word has at most 24
    significant bits (e.g. both halves multiples of 16)."""
    def spread(x):
        x = np.asarray(x, np.uint64) & np.uint64(0xFFFF)
        x = (x | (x << np.uint64(8))) & np.uint64(0x00FF00FF)
        x = (x | (x << np.uint64(4))) & np.uint64(0x0F0F0F0F)
        x = (x | (x << np.uint64(2))) & np.uint64(0x33333333)
        x = (x | (x << np.uint64(1))) & np.uint64(0x55555555)
        return x
    v = spread(a16) | (spread(b16) << np.uint64(1))
    f = (v.astype(np.float64) / 4294967296.0).astype(F)
    assert np.array_equal((f.astype(np.float64) * 4294967296.0).astype(np.uint64), v), "not representable in float32"
    return f


def boundaries(q):
    """The values of u[0][0] at which the selected lobe changes: cumulative lobe pdfs (n, 3)."""
    return np.cumsum(q[:, :3], axis=1)


def sample(b, wo, rn):
    """The sampled direction (n, 3, world) and the lobe index."""
    sin_o, cos_o, phi_o = _outgoing(b, wo)
    rn = np.asarray(rn, F).reshape(-1, 2)
    u00, u01 = demux_float(rn[:, 0])
    u10, u11 = demux_float(rn[:, 1])
    q = lobe_pdfs(b, wo)
    p, u = np.zeros(b.n, np.int64), u00.copy()
    live = np.ones(b.n, bool)
    for k in range(P_MAX):  # for (p = 0; p < p_max; p++) { if (u < ap_pdf[p]) break; u -= ap_pdf[p]; }
        stop = live & (u < q[:, k])
        live = live & ~stop
        u = np.where(live, u - q[:, k], u)
        p = np.where(live, k + 1, p)
    sop, cop = np.zeros(b.n), np.zeros(b.n)
    for k in range(4):
        s_, c_ = tilt(b, k, sin_o, cos_o)
        sop, cop = np.where(p == k, s_, sop), np.where(p == k, c_, cop)
    vp = np.take_along_axis(b.v, p[:, None], axis=1)[:, 0]
    u10 = np.where(u10 > EPS_U, u10, EPS_U)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        cos_t = 1 + vp * np.log(u10 + (1 - u10) * np.exp(-2 / vp))
        sin_t = _safe_sqrt(1 - cos_t * cos_t)
        cos_phi = np.cos(2 * PIF * u11)
        sin_i = -cos_t * sop + sin_t * cos_phi * cop
        cos_i = _safe_sqrt(1 - sin_i * sin_i)
        _, gamma_t = transmittance(b, sin_o, cos_o)
        ca, cb = 1 / (1 + np.exp(PIF / b.s)), 1 / (1 + np.exp(-PIF / b.s))
        x = -b.s * np.log(1 / (u01 * (cb - ca) + ca) - 1)
        x = np.minimum(np.maximum(x, -PIF), PIF)
        dphi = np.where(p < P_MAX, phi_fn(p, b.gamma_o, gamma_t) + x, 2 * PIF * u01)
    phi_i = phi_o + dphi
    local = np.stack([sin_i, cos_i * np.cos(phi_i), cos_i * np.sin(phi_i)], axis=1)
    return b.to_world(local), p
