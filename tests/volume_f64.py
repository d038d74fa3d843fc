"""The homogeneous medium of a path in float64: a numpy restatement of eval_vsdf (yocto_pathtrace.cpp:504-527), the crossing of
:1458-1467 and the volume functions of yocto_math.h:4758-4813 (eval_transmittance ... sample_phasefunction_pdf, with the
eval_scattering / sample_scattering / sample_scattering_pdf wrappers of yocto_pathtrace.cpp:1360-1377), in the manner of
tests/hair_f64.py: the float inputs taken as they are, every operation in float64.

The INTEGER decisions are not float64's to make: which side of a surface a direction lies on, which channel rl picks and which side of
|g| < 1e-3f the anisotropy falls are functions of the float inputs alone, made of float products and comparisons. They are evaluated
here in numpy's float32 (IEEE, one rounding per operation, the reference's order of operations), so they are exact.
"""
import types

import numpy as np

F = np.float32
FLT_MAX = float(np.finfo(F).max)
CLAMP_LO = float(F(0.0001))
G_SWITCH = float(F(1e-3))
PI_F = float(F(np.pi))  # pif: the reference's float pi, in every formula


def dot32(a, b):
    """dot (math.h: a.x * b.x + a.y * b.y + a.z * b.z) in float arithmetic."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def in_medium(mats10, normal, wo, wi):
    """Whether the crossing from outside enters a medium: has_volume (pt.cpp:531) and the two directions on opposite sides."""
    m = np.asarray(mats10, F)
    has_volume = (m[:, 4] == 0) & (m[:, 3] != 0)
    with np.errstate(under="ignore"):
        return has_volume & (dot32(normal, wo) * dot32(normal, wi) < 0)


def channel(rl):
    """clamp((int)(rl * 3), 0, 2) in float arithmetic."""
    return np.clip((np.asarray(rl, F) * F(3)).astype(np.int32), 0, 2)


def eval_vsdf(mats10, texval4, tex, inside):
    """density, scatter, anisotropy of the medium entered (zeros where `inside` is False). tex 0: an untextured material."""
    m, t = np.asarray(mats10, np.float64), np.asarray(texval4, np.float64)
    if tex:  # `if (transmission)` tests a float product: that decision is float's
        with np.errstate(under="ignore"):
            transmission = np.asarray(mats10, F)[:, 3] * np.asarray(texval4, F)[:, 3]
        base = m[:, 0:3] * t[:, 0:3]
    else:
        base, transmission = m[:, 0:3], m[:, 3]
    c = np.clip(base, CLAMP_LO, 1.0)
    density = np.where((transmission != 0)[:, None], -np.log(c) / m[:, 5:6], 0.0) + 0.0  # (+ 0.0: no negative zero)
    keep = np.asarray(inside, bool)[:, None]
    return types.SimpleNamespace(density=np.where(keep, density, 0.0), scatter=np.where(keep, m[:, 6:9], 0.0),
                                 anisotropy=np.where(keep[:, 0], m[:, 9], 0.0))


def free_flight_unclamped(density, rl, rd):
    """-log(1 - rd) / density[channel], flt_max where that density is 0."""
    d = density[np.arange(len(density)), channel(rl)]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0, FLT_MAX, -np.log1p(-np.asarray(rd, np.float64)) / np.where(d == 0, 1.0, d))


def free_flight(density, rl, rd, max_distance):
    """distance, the weight factor eval_transmittance / sample_transmittance_pdf, and that pdf."""
    maxd = np.asarray(max_distance, np.float64)
    dist = np.minimum(free_flight_unclamped(density, rl, rd), maxd)
    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        below = density * np.exp(-density * dist[:, None])
        at = np.exp(-density * maxd[:, None])
        tpdf = np.where(dist < maxd, below.sum(axis=1), at.sum(axis=1)) / 3
        weight = np.exp(-density * dist[:, None]) / tpdf[:, None]
    return dist, weight, tpdf


def eval_phasefunction(g, wo, wi):
    wo, wi = np.asarray(wo, np.float64), np.asarray(wi, np.float64)
    cosine = -np.sum(wo * wi, axis=1)
    denom = 1 + g * g - 2 * g * cosine
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (1 - g * g) / (4 * PI_F * denom * np.sqrt(denom))


def sample_phasefunction(g, wo, rx, ry):
    wo, rx, ry = np.asarray(wo, np.float64), np.asarray(rx, np.float64), np.asarray(ry, np.float64)
    iso = np.abs(np.asarray(g, F)) < F(1e-3)  # the float comparison
    gs = np.where(iso, 1.0, g)
    square = (1 - gs * gs) / (1 + gs - 2 * gs * ry)
    cos_theta = np.where(iso, 1 - 2 * ry, (1 + gs * gs - square * square) / (2 * gs))
    sin_theta = np.sqrt(np.maximum(0.0, 1 - cos_theta * cos_theta))
    phi = 2 * PI_F * rx
    local = np.stack([sin_theta * np.cos(phi), sin_theta * np.sin(phi), cos_theta], axis=1)
    z = -wo
    length = np.sqrt(np.sum(z * z, axis=1, keepdims=True))
    zz = np.where(length != 0, z / np.where(length != 0, length, 1.0), z)  # normalize (math.h:2036-2039)
    sign = np.copysign(1.0, zz[:, 2])  # basis_fromz (math.h:2743-2752)
    a = -1.0 / (sign + zz[:, 2])
    b = zz[:, 0] * zz[:, 1] * a
    x = np.stack([1.0 + sign * zz[:, 0] * zz[:, 0] * a, sign * b, -sign * zz[:, 0]], axis=1)
    y = np.stack([b, sign + zz[:, 1] * zz[:, 1] * a, -zz[:, 1]], axis=1)
    return x * local[:, 0:1] + y * local[:, 1:2] + zz * local[:, 2:3]


def _empty(v):
    return np.all(v.density == 0, axis=1)


def eval_scattering(v, wo, wi):
    f = v.scatter * v.density * eval_phasefunction(v.anisotropy, wo, wi)[:, None]
    return np.where(_empty(v)[:, None], 0.0, f)


def sample_scattering(v, wo, rx, ry):
    return np.where(_empty(v)[:, None], 0.0, sample_phasefunction(v.anisotropy, wo, rx, ry))


def sample_scattering_pdf(v, wo, wi):
    return np.where(_empty(v), 0.0, eval_phasefunction(v.anisotropy, wo, wi))


def batch(tex, mats10, normal, wo, wi, texval4, rn5):
    """The rows of yh_volume_batch in float64: a namespace of inside, density, scatter, anisotropy, dist, unclamped, weight, tpdf,
    dir, f, pdf (at wi); f and pdf at another direction come from eval_scattering / sample_scattering_pdf on `.medium`."""
    rn5 = np.asarray(rn5, F)
    inside = in_medium(mats10, normal, wo, wi)
    v = eval_vsdf(mats10, texval4, tex, inside)
    r = types.SimpleNamespace(inside=inside, medium=v, density=v.density, scatter=v.scatter, anisotropy=v.anisotropy)
    r.unclamped = free_flight_unclamped(v.density, rn5[:, 0], rn5[:, 1])
    r.dist, r.weight, r.tpdf = free_flight(v.density, rn5[:, 0], rn5[:, 1], rn5[:, 2])
    r.dir = sample_scattering(v, wo, rn5[:, 3], rn5[:, 4])
    r.f, r.pdf = eval_scattering(v, wo, wi), sample_scattering_pdf(v, wo, wi)
    return r
