"""The non-hair surface lobes in float64: a numpy restatement of yocto_math.h:4212-4273 (fresnel_dielectric, fresnel_conductor,
reflectivity_to_eta), 4307-4375 (the GGX distribution, shadowing and sampling), 4427-4755 (the nine lobes: value x |cos|, pdf,
sample) and of the mixture's dispatch (yocto_pathtrace.cpp:1069-1280: eval_brdfcos, sample_brdfcos, sample_brdfcos_pdf and the
delta forms), in the manner of tests/hair_f64.py: the float inputs taken as they are, every operation in float64.

The mixture takes the lobe weights, the roughness and the lobe pdfs as the oracle made them (the 22 leading floats of
yo_surface_bsdf, which the device must render bit for bit): eval_brdf itself is + - x / sqrt and held exactly. Which lobe rnl
selects is float arithmetic's decision (a running float sum compared with rnl) and is made here in numpy's float32.
"""
import numpy as np

F = np.float32
PI_F = float(F(np.pi))
(DIFFUSE, SPECULAR, METAL, TRANSMISSION, REFRACTION, DELTA_SPECULAR, DELTA_METAL, DELTA_TRANSMISSION, DELTA_REFRACTION) = range(9)


def dot(a, b):
    return np.sum(a * b, axis=1)


def col(x):
    return np.asarray(x, np.float64)[:, None]


def normalize(a):
    length = np.sqrt(dot(a, a))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(col(length) != 0, a / col(np.where(length != 0, length, 1.0)), a)


def reflect(w, n):
    return -w + 2 * col(dot(n, w)) * n


def refract(w, n, inv_eta):
    cosine = dot(n, w)
    k = 1 + inv_eta * inv_eta * (cosine * cosine - 1)
    with np.errstate(invalid="ignore"):
        r = -w * col(inv_eta) + col(inv_eta * cosine - np.sqrt(np.maximum(k, 0))) * n
    return np.where(col(k) < 0, 0.0, r)


def fresnel_dielectric_cos(eta, cosw):
    cosw = np.abs(cosw)
    sin2 = 1 - cosw * cosw
    cos2t = 1 - sin2 / (eta * eta)
    t0 = np.sqrt(np.maximum(cos2t, 0))
    t1, t2 = eta * t0, eta * cosw
    with np.errstate(invalid="ignore", divide="ignore"):
        rs, rp = (cosw - t1) / (cosw + t1), (t0 - t2) / (t0 + t2)
    return np.where(cos2t < 0, 1.0, (rs * rs + rp * rp) / 2)


def fresnel_dielectric(eta, normal, outgoing):
    return fresnel_dielectric_cos(eta, dot(normal, outgoing))


def fresnel_conductor(eta, etak, normal, outgoing):
    """eta, etak: (n, 3)."""
    cosw = dot(normal, outgoing)
    up = cosw > 0
    cosw = np.clip(cosw, -1, 1)
    cos2 = col(cosw * cosw)
    sin2 = np.clip(1 - cos2, 0, 1)
    eta2, etak2 = eta * eta, etak * etak
    t0 = eta2 - etak2 - sin2
    a2plusb2 = np.sqrt(t0 * t0 + 4 * eta2 * etak2)
    t1 = a2plusb2 + cos2
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.sqrt((a2plusb2 + t0) / 2)
        t2 = 2 * a * col(cosw)
        rs = (t1 - t2) / (t1 + t2)
        t3 = cos2 * a2plusb2 + sin2 * sin2
        t4 = t2 * sin2
        rp = rs * (t3 - t4) / (t3 + t4)
    return np.where(col(up), (rp + rs) / 2, 0.0)


def reflectivity_to_eta(color):
    r = np.clip(np.asarray(color, np.float64), 0, float(F(0.99)))
    return (1 + np.sqrt(r)) / (1 - np.sqrt(r))


def microfacet_distribution(roughness, normal, halfway):
    cosine = dot(normal, halfway)
    r2, c2 = roughness * roughness, cosine * cosine
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = r2 / (PI_F * (c2 * r2 + 1 - c2) * (c2 * r2 + 1 - c2))
    return np.where(cosine <= 0, 0.0, d)


def microfacet_shadowing1(roughness, normal, halfway, direction):
    cosine, cosineh = dot(normal, direction), dot(halfway, direction)
    r2, c2 = roughness * roughness, cosine * cosine
    with np.errstate(invalid="ignore", divide="ignore"):
        g = 2 * np.abs(cosine) / (np.abs(cosine) + np.sqrt(c2 - r2 * c2 + r2))
    return np.where(cosine * cosineh <= 0, 0.0, g)


def microfacet_shadowing(roughness, normal, halfway, outgoing, incoming):
    return microfacet_shadowing1(roughness, normal, halfway, outgoing) * microfacet_shadowing1(roughness, normal, halfway, incoming)


def from_local_z(normal, local):
    zz = normalize(normal)
    sign = np.copysign(1.0, zz[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        a = -1.0 / (sign + zz[:, 2])
    b = zz[:, 0] * zz[:, 1] * a
    x = np.stack([1.0 + sign * zz[:, 0] * zz[:, 0] * a, sign * b, -sign * zz[:, 0]], axis=1)
    y = np.stack([b, sign + zz[:, 1] * zz[:, 1] * a, -zz[:, 1]], axis=1)
    return normalize(x * local[:, 0:1] + y * local[:, 1:2] + zz * local[:, 2:3])


def sample_microfacet(roughness, normal, rx, ry):
    phi = 2 * PI_F * rx
    with np.errstate(divide="ignore"):
        theta = np.arctan(roughness * np.sqrt(ry / (1 - ry)))
    st, ct = np.sin(theta), np.cos(theta)
    return from_local_z(normal, np.stack([np.cos(phi) * st, np.sin(phi) * st, ct], axis=1))


def sample_microfacet_pdf(roughness, normal, halfway):
    cosine = dot(normal, halfway)
    return np.where(cosine < 0, 0.0, microfacet_distribution(roughness, normal, halfway) * cosine)


def sample_hemisphere_cos(normal, rx, ry):
    z = np.sqrt(ry)
    r = np.sqrt(1 - z * z)
    phi = 2 * PI_F * rx
    return from_local_z(normal, np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1))


def _both_above(n, o, i):
    return ~((dot(n, i) <= 0) | (dot(n, o) <= 0))


def _reflection(Fv, rough, n, h, o, i):
    D, G = microfacet_distribution(rough, n, h), microfacet_shadowing(rough, n, h, o, i)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return Fv * col(D) * col(G) / col(4 * dot(n, o) * dot(n, i)) * col(dot(n, i))


def _side(ior, n, o):
    entering = dot(n, o) >= 0
    return entering, np.where(col(entering), n, -n), np.where(entering, ior, 1 / ior)


def refraction_fresnel(ior, rough, n, o, rx, ry):
    """The Fresnel value that rnl is compared with in sample_microfacet_refraction, and the sampled halfway vector."""
    entering, up, rel = _side(ior, n, o)
    h = sample_microfacet(rough, up, rx, ry)
    return fresnel_dielectric(rel, h, o), h


def delta_refraction_fresnel(ior, n, o):
    entering, up, rel = _side(ior, n, o)
    return fresnel_dielectric(rel, up, o)


def ior_is_one(ior):
    return np.abs(np.asarray(ior, F) - F(1)).astype(np.float64) < 1e-3  # (double)fabs(ior - 1) < 1e-3: the float difference, a double bound


def lobe(kind, params, n, o, i, rn):
    """One YH_LOBE_* kind in float64: (f [n, 3], pdf [n], sampled [n, 3])."""
    p, n, o, i, rn = (np.asarray(x, np.float64) for x in (params, n, o, i, rn))
    ior, rough, eta, etak = p[:, 0], p[:, 1], p[:, 2:5], p[:, 5:8]
    rnl, rx, ry = rn[:, 0], rn[:, 1], rn[:, 2]
    one = np.ones((len(p), 3))
    above_o = dot(n, o) > 0
    both = _both_above(n, o, i)
    through = ~((dot(n, i) >= 0) | (dot(n, o) <= 0))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if kind == DIFFUSE:
            f = np.where(col(both), one / PI_F * col(dot(n, i)), 0.0)
            pdf = np.where(both, dot(n, i) / PI_F, 0.0)
            w = np.where(col(above_o), sample_hemisphere_cos(n, rx, ry), 0.0)
        elif kind in (SPECULAR, METAL):
            h = normalize(i + o)
            Fv = one * col(fresnel_dielectric(ior, h, i)) if kind == SPECULAR else fresnel_conductor(eta, etak, h, i)
            f = np.where(col(both), _reflection(Fv, rough, n, h, o, i), 0.0)
            pdf = np.where(both, sample_microfacet_pdf(rough, n, h) / (4 * np.abs(dot(o, h))), 0.0)
            w = np.where(col(above_o), reflect(o, sample_microfacet(rough, n, rx, ry)), 0.0)
        elif kind == TRANSMISSION:
            refl = reflect(-i, n)
            h = normalize(refl + o)
            D, G = microfacet_distribution(rough, n, h), microfacet_shadowing(rough, n, h, o, refl)
            f = np.where(col(through), one * col(D) * col(G) / col(4 * dot(n, o) * dot(n, refl)) * col(dot(n, refl)), 0.0)
            pdf = np.where(through, sample_microfacet_pdf(rough, n, h) / (4 * np.abs(dot(o, h))), 0.0)
            w = np.where(col(above_o), -reflect(reflect(o, sample_microfacet(rough, n, rx, ry)), n), 0.0)
        elif kind == REFRACTION:
            entering, up, rel = _side(ior, n, o)
            same = dot(n, i) * dot(n, o) >= 0
            h1 = normalize(i + o)
            F1 = fresnel_dielectric(rel, h1, o)
            f1 = one * col(F1 * microfacet_distribution(rough, up, h1) * microfacet_shadowing(rough, up, h1, o, i)
                           / np.abs(4 * dot(n, o) * dot(n, i)) * np.abs(dot(n, i)))
            p1 = F1 * sample_microfacet_pdf(rough, up, h1) / (4 * np.abs(dot(o, h1)))
            h2 = -normalize(col(rel) * i + o) * col(np.where(entering, 1.0, -1.0))
            F2 = fresnel_dielectric(rel, h2, o)
            D2, G2 = microfacet_distribution(rough, up, h2), microfacet_shadowing(rough, up, h2, o, i)
            den = rel * dot(h2, i) + dot(h2, o)
            f2 = one * col(np.abs((dot(o, h2) * dot(i, h2)) / (dot(o, n) * dot(i, n))) * (1 - F2) * D2 * G2 / (den * den) * np.abs(dot(n, i)))
            p2 = (1 - F2) * sample_microfacet_pdf(rough, up, h2) * np.abs(dot(h2, o)) / (den * den)
            f, pdf = np.where(col(same), f1, f2), np.where(same, p1, p2)
            Fs, hs = refraction_fresnel(ior, rough, n, o, rx, ry)
            w = np.where(col(rnl < Fs), reflect(o, hs), refract(o, hs, 1 / rel))
        elif kind in (DELTA_SPECULAR, DELTA_METAL):
            Fv = one * col(fresnel_dielectric(ior, n, o)) if kind == DELTA_SPECULAR else fresnel_conductor(eta, etak, n, o)
            f, pdf = np.where(col(both), Fv, 0.0), np.where(both, 1.0, 0.0)
            w = np.where(col(above_o), reflect(o, n), 0.0)
        elif kind == DELTA_TRANSMISSION:
            f, pdf = np.where(col(through), one, 0.0), np.where(through, 1.0, 0.0)
            w = np.where(col(above_o), -o, 0.0)
        elif kind == DELTA_REFRACTION:
            entering, up, rel = _side(ior, n, o)
            is1 = ior_is_one(p[:, 0])
            prod = dot(n, i) * dot(n, o)
            Fd = fresnel_dielectric(rel, up, o)
            f = np.where(col(is1), np.where(col(prod <= 0), one, 0.0), np.where(col(prod >= 0), one * col(Fd), one * col((1 / (rel * rel)) * (1 - Fd))))
            pdf = np.where(is1, np.where(prod < 0, 1.0, 0.0), np.where(prod >= 0, Fd, 1 - Fd))
            w = np.where(col(is1), -o, np.where(col(rnl < Fd), reflect(o, up), refract(o, up, 1 / rel)))
        else:
            raise ValueError(kind)
    return f, pdf, w


# ---- the mixture's dispatch on the oracle's lobe set-up ------------------------------------------------------------------
ROUGH_KINDS = (DIFFUSE, SPECULAR, METAL, TRANSMISSION, REFRACTION)
DELTA_KINDS = (None, DELTA_SPECULAR, DELTA_METAL, DELTA_TRANSMISSION, DELTA_REFRACTION)


def selected_lobe(lead22, rnl):
    """Which of the five lobes rnl selects (sample_brdfcos / sample_delta), -1 for none, and the float cumulative pdfs the
    selection compares rnl with: (lobe [n], cdf [n, 5]); a lobe that cannot be selected has cdf NaN."""
    lead = np.asarray(lead22, F)
    pdfs = lead[:, 17:22].copy()
    delta = lead[:, 15] == 0
    live = pdfs != 0
    live[:, 1] &= pdfs[:, 4] == 0  # the specular lobe hands over to refraction
    live[:, 0] &= ~delta
    run = np.where(delta, pdfs[:, 0], F(0)).astype(F)  # sample_delta adds the diffuse pdf without a test
    lobe = np.full(len(lead), -1)
    cdf = np.full((len(lead), 5), np.nan, F)
    rnl = np.asarray(rnl, F)
    for k in range(5):
        run = np.where(live[:, k], run + pdfs[:, k], run).astype(F)
        cdf[live[:, k], k] = run[live[:, k]]
        lobe = np.where((lobe < 0) & live[:, k] & (rnl < run), k, lobe)
    return lobe, cdf


def mixture(lead22, ior, color, n, o, i, rn):
    """eval_brdfcos / sample_brdfcos_pdf / sample_brdfcos (rough) or eval_delta / sample_delta_pdf / sample_delta (roughness 0)
    in float64 on the oracle's lobe weights, roughness and lobe pdfs: (f [n, 3], pdf [n], sampled [n, 3], selected lobe [n])."""
    lead = np.asarray(lead22, np.float64)
    m = len(lead)
    weights = [lead[:, 3 * k:3 * k + 3] for k in range(5)]
    pdfs = lead[:, 17:22]
    delta = lead[:, 15] == 0
    params = np.zeros((m, 8))
    params[:, 0], params[:, 1], params[:, 2:5] = np.asarray(ior, np.float64), lead[:, 15], reflectivity_to_eta(color)
    f, pdf, w = np.zeros((m, 3)), np.zeros(m), np.zeros((m, 3))
    lobe_sel, _ = selected_lobe(lead22, np.asarray(rn)[:, 0])
    refr = pdfs[:, 4] != 0
    for k in range(5):
        for is_delta, kind in ((False, ROUGH_KINDS[k]), (True, DELTA_KINDS[k])):
            if kind is None:
                continue
            rows = delta == is_delta
            lf, lp, lw = lobe(kind, params, n, o, i, rn)
            nz = (weights[k] != 0).any(axis=1)
            in_f = rows & nz & ~((k == 1) & is_delta & (weights[4] != 0).any(axis=1))  # eval_delta: specular only without refraction
            in_p = rows & (pdfs[:, k] != 0) & ~((k == 1) & refr)
            with np.errstate(invalid="ignore"):
                f = np.where(col(in_f), f + weights[k] * lf, f)
                pdf = np.where(in_p, pdf + pdfs[:, k] * lp, pdf)
            w = np.where(col(rows & (lobe_sel == k)), lw, w)
    return f, pdf, w, lobe_sel
