"""The shading point of a hit in float64: a numpy restatement of yocto_pathtrace.cpp:147-200 (lookup_texture, eval_texture), 232-369
(eval_position, eval_normal, eval_texcoord, eval_element_tangents, eval_normalmap, eval_shading_normal), 396-471 (eval_emission,
eval_brdf) and 504-527 (eval_vsdf) with yocto_math.h:3360-3383 (triangle_tangents_fromuv), on the scenes of tests/point_cases.py, in
the manner of tests/volume_f64.py: the float inputs taken as they are, every operation in float64. The row layout is yh_point_batch's.

Next to the values, `batch` returns the DECISION quantities of a row — dot(n, outgoing) against 0 (the thin flip and the crossing),
opacity against 0.999, div against 0, dot(frame.y, tv) against 0 (flip_v) — and which rows lie within `ulps` float ulps of a
threshold without lying on it (`aside`): there float arithmetic may decide the other way. A quantity that float64 finds exactly ON
its threshold comes from operands chosen so that float arithmetic is exact too (identity frame, axis-aligned normals, small integers).
The texel index needs no such care: the bilinear lookup with its wrap is continuous across every texel boundary.
"""
import ctypes as C
import types

import numpy as np

import oracle_capi as oc
import surface_f64 as s64
from surface_f64 import col, dot, normalize

F = np.float32
EPS = 2.0 ** -24  # half a float ulp of 1: an ulp of x is at most 2 EPS |x|
# The row layout is the binding's (yhair_capi.POINT_COLUMNS, held to the header's YH_POINT_* by tests/test_abi.py). The quantities of the
# tests: the emission texture with its linear x, and the bsdf's 22 floats as lobe weights, roughness, opacity and pdfs.
POINT_FLOATS = oc.yh.POINT_FLOATS
_P = oc.yh.POINT_COLUMNS
_B = _P["bsdf"].start
COLS = {**{k: _P[k] for k in ("position", "normal", "shading_normal", "texcoord", "color_tex")},
        "emission_tex": slice(_P["emission_tex"].start, _P["emission_tex_x"].stop), "scattering_tex": _P["scattering_tex"], "emission": _P["emission"],
        "weights": slice(_B, _B + 15), "roughness": slice(_B + 15, _B + 16), "opacity": slice(_B + 16, _B + 17), "pdfs": slice(_B + 17, _B + 22),
        "density": _P["density"], "scatter": _P["scatter"], "anisotropy": _P["anisotropy"]}
assert _B + 22 == _P["bsdf"].stop and _P["emission_tex"].stop == _P["emission_tex_x"].start


def _srgb_to_linear(c):
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def lookup64(px, tu, tv):
    """eval_texture (pt.cpp:167-200) on float64 texels px (h, w, 3): wrap, bilinear."""
    h, w = px.shape[:2]
    s, tt = np.fmod(tu, 1.0) * w, np.fmod(tv, 1.0) * h
    s, tt = np.where(s < 0, s + w, s), np.where(tt < 0, tt + h, tt)
    i, j = np.clip(s.astype(np.int64), 0, w - 1), np.clip(tt.astype(np.int64), 0, h - 1)
    ii, jj = (i + 1) % w, (j + 1) % h
    u, v = (s - i)[:, None], (tt - j)[:, None]
    return px[j, i] * (1 - u) * (1 - v) + px[jj, i] * (1 - u) * v + px[j, ii] * u * (1 - v) + px[jj, ii] * u * v


def texels64(is_byte, px, linear=False):
    """lookup_texture (pt.cpp:147-164): bytes / 255, decoded from sRGB unless the lookup asks for linear; floats as they are."""
    px = np.asarray(px).astype(np.float64)
    if not is_byte:
        return px
    return px / 255 if linear else _srgb_to_linear(px / 255)


def _texture64(t, tu, tv, linear=False):
    """eval_texture (pt.cpp:167-200) of a yh_texture, float64: wrap, bilinear, bytes decoded from sRGB (linear: bytes / 255)."""
    w, h = t.width, t.height
    raw = np.ctypeslib.as_array(C.cast(t.pixels, C.POINTER(C.c_uint8 if t.is_byte else C.c_float)), (h, w, 3))
    return lookup64(texels64(t.is_byte, raw, linear), tu, tv)


def _tex(sc, index, tu, tv, linear):
    """eval_texture of the scene's 1-based texture `index` (0: none, the value 1)."""
    if index == 0:
        return np.ones((len(tu), 3))
    t = sc.textures[index - 1]
    return lookup64(texels64(t["is_byte"], t["px"], linear), tu, tv)


def _tv(f, v):  # transform_vector
    return v[:, 0:1] * f[0:3] + v[:, 1:2] * f[3:6] + v[:, 2:3] * f[6:9]


def _brdf(m, mp, normal, outgoing, ctex, etex_x, maps):
    """eval_brdf (pt.cpp:405-471): (weights (n, 15), roughness, opacity after its snap, pdfs (n, 5), opacity before it)."""
    n = len(normal)
    col = lambda x: np.broadcast_to(np.asarray(x, np.float64), (n,))[:, None]  # noqa: E731  (scalars too)
    base = np.asarray(m["color"], F).astype(np.float64) * ctex
    specular, metallic, roughness = float(F(m["specular"])) * maps["specular"], float(F(m["metallic"])) * maps["metallic"], float(F(m["roughness"])) * maps["roughness"]
    ior = float(F(m["ior"]))
    transmission = float(F(m["transmission"])) * etex_x
    opacity = float(F(m["opacity"])) * maps["opacity"]
    thin = bool(m["thin"]) or not m["transmission"]
    one = np.ones((n, 3))
    weight = one.copy()
    metal = weight * col(metallic)
    weight = weight * col(1 - metallic)
    refraction = np.zeros((n, 3)) if thin else weight * col(transmission)
    weight = weight * col(1 - (0 if thin else transmission))
    spec = weight * col(specular)
    weight = weight * col(1 - specular * s64.fresnel_dielectric(ior, outgoing, normal))
    trans = weight * col(transmission) * base if thin else np.zeros((n, 3))
    weight = weight * col(1 - (transmission if thin else 0))
    diffuse = weight * base
    meta = s64.reflectivity_to_eta(base)
    rough = roughness * roughness
    rough = np.where((diffuse != 0).any(axis=1) | (rough != 0), np.clip(rough, float(F(0.03)) * float(F(0.03)), 1.0), rough)
    none = ~((spec != 0).any(axis=1) | (metal != 0).any(axis=1) | (trans != 0).any(axis=1) | (refraction != 0).any(axis=1))
    rough = np.where(none, 1.0, rough)
    snapped = np.where(opacity > float(F(0.999)), 1.0, opacity)
    with np.errstate(invalid="ignore", divide="ignore"):
        pdfs = np.stack([diffuse.max(axis=1), (spec * col(s64.fresnel_dielectric(ior, normal, outgoing))).max(axis=1),
                         (metal * s64.fresnel_conductor(meta, np.zeros((n, 3)), normal, outgoing)).max(axis=1), trans.max(axis=1), refraction.max(axis=1)], axis=1)
        total = pdfs.sum(axis=1)
        pdfs = np.where(col(total) != 0, pdfs / col(np.where(total != 0, total, 1.0)), pdfs)
    return np.concatenate([diffuse, spec, metal, trans, refraction], axis=1), rough, snapped, pdfs, opacity


def batch(sc, obj, elem, uv, outgoing, ulps=4):
    """The rows of yh_point_batch in float64 on point_cases.Scene `sc`: .out (n, POINT_FLOATS), the decision quantities .dot_no,
    .opacity (before its snap), .div, .flip_dot (NaN where a row takes no such decision) and .aside."""
    n = len(obj)
    out = np.zeros((n, POINT_FLOATS))
    r = types.SimpleNamespace(out=out, dot_no=np.full(n, np.nan), opacity=np.full(n, np.nan), div=np.full(n, np.nan), flip_dot=np.full(n, np.nan),
                              aside=np.zeros(n, bool), flips=np.zeros(n, bool), mapped=np.zeros(n, bool), uses_texcoord=np.zeros(n, bool))
    uv64, wo_all = np.asarray(uv, F).astype(np.float64), np.asarray(outgoing, F).astype(np.float64)
    for k in np.unique(obj):
        rows = np.flatnonzero(obj == k)
        o = sc.objects[k]
        s, m, mp = sc.shapes[o["shape"]], sc.materials[o["material"]], sc.maps[o["material"]] if sc.general else {q: 0 for q in ("specular_tex", "metallic_tex", "roughness_tex", "opacity_tex", "normal_tex")}
        f = o["frame"].astype(np.float64)
        e, u, v, wo = elem[rows], uv64[rows, 0:1], uv64[rows, 1:2], wo_all[rows]
        lines = s["lines"] is not None
        idx = (s["lines"] if lines else s["tris"])[e]
        P = s["pos"].astype(np.float64)
        w = [1 - u, u] if lines else [1 - u - v, u, v]
        interp = lambda a: sum(a[idx[:, c]] * w[c] for c in range(len(w)))  # noqa: E731
        p = interp(P)
        position = _tv(f, p) + f[9:12]
        p0, p1 = P[idx[:, 0]], P[idx[:, 1]]
        gn = normalize(p1 - p0) if lines else normalize(np.cross(p1 - p0, P[idx[:, 2]] - p0))
        element_normal = normalize(_tv(f, gn))
        normal = element_normal if s["nrm"] is None else normalize(_tv(f, normalize(interp(s["nrm"].astype(np.float64)))))
        tc = uv64[rows] if s["tc"] is None else interp(s["tc"].astype(np.float64))
        tu, tv = tc[:, 0], tc[:, 1]
        nrm = normal
        if mp["normal_tex"] and not lines:  # eval_normalmap (pt.cpp:329-347)
            nm = -1 + 2 * _tex(sc, mp["normal_tex"], tu, tv, True)
            tgu, tgv = np.zeros_like(p), np.zeros_like(p)
            if s["tc"] is not None:  # eval_element_tangents, triangle_tangents_fromuv
                T = s["tc"].astype(np.float64)
                pp, qq = p1 - p0, P[idx[:, 2]] - p0
                sx, sy = T[idx[:, 1], 0] - T[idx[:, 0], 0], T[idx[:, 2], 0] - T[idx[:, 0], 0]
                tx, ty = T[idx[:, 1], 1] - T[idx[:, 0], 1], T[idx[:, 2], 1] - T[idx[:, 0], 1]
                div = sx * ty - sy * tx
                r.div[rows] = div
                ulp_div = 2 * EPS * (np.abs(sx * ty) + np.abs(sy * tx))
                r.aside[rows] |= (div != 0) & (np.abs(div) <= ulps * ulp_div)
                safe = np.where(div != 0, div, 1.0)
                tu3 = np.where(col(div) != 0, (col(ty) * pp - col(tx) * qq) / col(safe), [1.0, 0, 0])
                tv3 = np.where(col(div) != 0, (col(sx) * qq - col(sy) * pp) / col(safe), [0, 1.0, 0])
                tgu, tgv = normalize(_tv(f, tu3)), normalize(_tv(f, tv3))
            fz = normal
            fx = normalize(tgu - fz * col(dot(tgu, fz)))
            fy = normalize(np.cross(fz, fx))
            fd = dot(fy, tgv)
            r.flip_dot[rows] = fd
            r.aside[rows] |= (fd != 0) & (np.abs(fd) <= ulps * 2 * EPS * np.sum(np.abs(fy * tgv), axis=1))
            nm[:, 1] *= np.where(fd < 0, 1.0, -1.0)
            nrm = normalize(fx * nm[:, 0:1] + fy * nm[:, 1:2] + fz * nm[:, 2:3])
            r.mapped[rows] = True
        if lines:
            shading = normalize(wo - nrm * col(dot(wo, nrm)))
        else:
            d = dot(nrm, wo)
            flip = bool(m["thin"]) & (d < 0)
            shading = np.where(col(flip), -nrm, nrm)
            r.flips[rows] = flip
            if m["thin"] or (not m["thin"] and m["transmission"]):
                r.dot_no[rows] = d
                r.aside[rows] |= (d != 0) & (np.abs(d) <= ulps * 2 * EPS * np.sum(np.abs(nrm * wo), axis=1))
        ctex = _tex(sc, m["color_tex"], tu, tv, False)
        etex = _tex(sc, m["emission_tex"], tu, tv, False)
        etex_x = _tex(sc, m["emission_tex"], tu, tv, True)[:, 0]
        stex = _tex(sc, m["scattering_tex"], tu, tv, False)
        maps = dict(specular=_tex(sc, mp["specular_tex"], tu, tv, True)[:, 0], metallic=_tex(sc, mp["metallic_tex"], tu, tv, True)[:, 0],
                    roughness=_tex(sc, mp["roughness_tex"], tu, tv, True)[:, 0], opacity=_tex(sc, mp["opacity_tex"], tu, tv, True).sum(axis=1) / 3)
        weights, rough, opacity, pdfs, raw_opacity = _brdf(m, mp, shading, wo, ctex, etex_x, maps)
        r.opacity[rows] = raw_opacity
        thr = float(F(0.999))
        r.aside[rows] |= (raw_opacity != thr) & (np.abs(raw_opacity - thr) <= ulps * 2 * EPS)
        r.uses_texcoord[rows] = bool(m["color_tex"] or m["emission_tex"] or m["scattering_tex"] or mp["specular_tex"] or mp["metallic_tex"] or mp["roughness_tex"]
                                     or mp["opacity_tex"] or mp["normal_tex"])
        density, scatter, aniso = np.zeros((len(rows), 3)), np.zeros((len(rows), 3)), np.zeros(len(rows))
        if not m["thin"] and m["transmission"]:  # the crossing of pt.cpp:1458-1467 with incoming = -outgoing, then eval_vsdf (504-527)
            d = dot(shading, wo)
            cross = d * dot(shading, -wo) < 0
            transmission = float(F(m["transmission"])) * etex_x
            base = np.asarray(m["color"], F).astype(np.float64) * ctex
            with np.errstate(divide="ignore"):
                dens = -np.log(np.clip(base, float(F(0.0001)), 1.0)) / float(F(m["trdepth"]))
            density = np.where(col(cross & (transmission != 0)), dens, 0.0)
            scatter = np.where(col(cross), np.asarray(m["scattering"], F).astype(np.float64) * stex, 0.0)
            aniso = np.where(cross, float(F(m["scanisotropy"])), 0.0)
        O = out[rows]
        for q, val in (("position", position), ("normal", normal), ("shading_normal", shading), ("texcoord", tc), ("color_tex", ctex),
                       ("emission_tex", np.concatenate([etex, etex_x[:, None]], axis=1)), ("scattering_tex", stex),
                       ("emission", np.asarray(m["emission"], F).astype(np.float64) * etex), ("weights", weights), ("roughness", rough[:, None]),
                       ("opacity", opacity[:, None]), ("pdfs", pdfs), ("density", density), ("scatter", scatter), ("anisotropy", aniso[:, None])):
            O[:, COLS[q]] = val
        out[rows] = O
    return r
