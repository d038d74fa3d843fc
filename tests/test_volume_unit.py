"""The homogeneous medium of a path on the device as the sample loops run it (yh_volume_batch: unit/volume_shade.h), at unit level and at
its edges: medium_crossing, the free flight and the scatter of path_step (csrc/dev_path.h) with the volume functions of
csrc/dev_surface.h, a quad per row (k_trace<GENERAL>) and a lane per row (k_stream: the medium through the path's slot), on the
material row the upload's own code makes (tex 0: the host-made density) and on that row with its colour texture set (tex 1: the
density derived on the device). And the quad forms of the trimmed 512-thread kernels next to the plain forms whose bits they must
render (yh_quad_forms_batch: sample_hemisphere_cos_quad, quad_div).

References: the oracle (float arithmetic, the reference's operations; held to the real reference bit for bit by
tests/test_oracle_vs_ref.py and tests/test_oracle_golden.py) and tests/volume_f64.py, the same formulas in float64.
Strata (tests/volume_cases.py; ROWS rows each, fixed seeds): a today's domain, b the anisotropy's edges, c density per channel,
d the random numbers' edges, e max_distance, f the outgoing direction's edges, g the crossing.

Quantities: density, distance, weight (eval_transmittance / sample_transmittance_pdf), tpdf, direction (the sampled one), f and pdf
(eval_scattering, sample_scattering_pdf at `incoming`), f@s and pdf@s (the two at the sampled direction: each side's value at ITS
OWN sampled direction against float64 at that same direction, so that the figure is the evaluation's error and not the direction's).

Bars (none of them taken from what the device gives):
  1  quad and lane forms: all 24 floats of every row bit for bit, NaN pattern included, both tex forms, every stratum.
     sample_hemisphere_cos_quad = sample_hemisphere_cos and quad_div(a, b) = a / b bit for bit, b in {0, -0, denormal, inf, NaN} included;
  2  exact: in_medium, scatter and anisotropy against the oracle on every stratum in both tex forms; the host-made density (tex 0) bit for
     bit; the channel rl picks, recovered from the device's distance on stratum d, is float arithmetic's clamp((int)(rl * 3), 0, 2);
  3  stratum a against the oracle: every value and pdf within REL_BSDF (1e-4, floor 1e-7), the direction within ABS_DIR (5e-5);
  4  strata b-g against float64: median and p99 of the relative error (floor 1e-7; per row the largest over the components) of every
     value and pdf and of the absolute error of the direction at most K = 2 x max(the oracle's same statistic on the same rows, 1e-6);
     the device-derived density (tex 1) among them, against float64 -log(c) / trdepth;
  5  the non-finite mask equals the oracle's on every row of every stratum;
  6  set aside from distance, weight and tpdf: rows whose float64 free-flight distance lies within 4 float ulps of max_distance
     (decided on the inputs); at most 2e-4 of a stratum's rows, asserted on the CPU too. Statistics run over the rows whose float64
     value and oracle value are finite (an unnormalised outgoing direction makes Henyey-Greenstein's denominator negative);
  7  n in {1, 3, 4097}: each row equals the same row of the ROWS-row call bit for bit; the refusals of the two entry points.
The CPU test holds the restatement to the oracle: on every stratum the median relative difference of every value and pdf below 1e-5.

What the bars catch, tried once on copies of the library whose kernels were compiled from a dev_surface.h with one one-token error each:
  sample_phasefunction's 1e-3f written 1e-2f: bar 3 (stratum a: the direction, 1.2e-2 against 5e-5) and bar 4 on strata b, c and e (the
    direction: on b median 6.4e-5 against the oracle's 8.4e-6 and p99 2.7e-3 against 2.0e-4), both forms, no other bar;
  iclamp((int)(rl * 3), 0, 2) written with 0, 1: bar 2 on stratum d (the channel recovered from the distance), bar 3 (the distance, 41 against
    1e-4) and bar 4 on every stratum b-g (distance, weight and tpdf: p99 of 4 to 4e6 against 1e-6), both forms;
  (1 / ior and ior swapped in sample_microfacet_refraction's refract: caught by tests/test_surface_unit.py, no volume bar.)

MEASURED (2026-10-19, AMD Instinct MI355X, gfx950; also profiles/surface_volume_unit/errors.txt): no assertion fails.
median and p99 per stratum of the error against float64 (relative with a floor of 1e-7, per row the largest over the components;
direction: absolute), 8192 rows each. reference = the oracle on the CPU; device = the quad form = the lane form (bit for bit on every
stratum, both tex forms). tex 0: the host-made density; tex 1: the density derived on the device.
                density             distance            weight              tpdf                direction           f                   pdf                 f@s                 pdf@s               
  a tex 0
    reference   3.94e-08 8.51e-08   0.00e+00 1.25e-06   6.87e-08 7.24e-07   3.26e-08 2.24e-07   1.44e-07 5.40e-06   1.09e-07 4.83e-07   6.30e-08 4.35e-07   1.22e-07 1.69e-06   7.61e-08 1.63e-06
    device      3.94e-08 8.51e-08   0.00e+00 1.27e-06   7.02e-08 8.57e-07   3.39e-08 2.69e-07   1.45e-07 5.40e-06   1.09e-07 4.83e-07   6.30e-08 4.35e-07   1.21e-07 1.65e-06   7.62e-08 1.61e-06
  a tex 1
    reference   5.22e-08 1.81e-07   9.19e-09 1.29e-06   7.12e-08 6.01e-07   3.54e-08 2.51e-07   1.44e-07 5.40e-06   1.19e-07 5.00e-07   6.30e-08 4.35e-07   1.34e-07 1.69e-06   7.61e-08 1.63e-06
    device      8.06e-08 2.02e-07   1.18e-08 1.32e-06   7.81e-08 7.87e-07   3.91e-08 2.92e-07   1.45e-07 5.40e-06   1.31e-07 5.11e-07   6.30e-08 4.35e-07   1.45e-07 1.67e-06   7.62e-08 1.61e-06
  b tex 0
    reference   4.00e-08 8.55e-08   0.00e+00 1.13e-06   6.98e-08 6.76e-07   3.38e-08 2.12e-07   8.41e-06 1.96e-04   1.37e-07 4.52e-01   8.84e-08 4.52e-01   1.20e-07 4.20e-01   7.33e-08 4.20e-01
    device      4.00e-08 8.55e-08   0.00e+00 1.13e-06   7.13e-08 7.54e-07   3.52e-08 2.60e-07   8.41e-06 1.96e-04   1.37e-07 4.52e-01   8.84e-08 4.52e-01   1.20e-07 4.20e-01   7.32e-08 4.20e-01
  b tex 1
    reference   4.00e-08 8.55e-08   0.00e+00 1.13e-06   6.98e-08 6.76e-07   3.38e-08 2.12e-07   8.41e-06 1.96e-04   1.37e-07 4.52e-01   8.84e-08 4.52e-01   1.20e-07 4.20e-01   7.33e-08 4.20e-01
    device      6.58e-08 1.44e-07   0.00e+00 1.13e-06   7.58e-08 9.85e-07   3.67e-08 2.63e-07   8.41e-06 1.96e-04   1.58e-07 4.52e-01   8.84e-08 4.52e-01   1.39e-07 4.20e-01   7.32e-08 4.20e-01
  c tex 0
    reference   3.36e-08 8.49e-08   1.28e-08 8.30e-07   5.65e-08 8.99e-07   2.86e-08 2.40e-07   1.24e-07 6.20e-06   9.41e-08 4.72e-07   5.21e-08 4.26e-07   1.04e-07 1.72e-06   6.16e-08 1.68e-06
    device      3.36e-08 8.49e-08   1.59e-08 8.30e-07   5.79e-08 9.39e-07   2.98e-08 2.81e-07   1.24e-07 6.19e-06   9.41e-08 4.72e-07   5.21e-08 4.26e-07   1.04e-07 1.71e-06   6.20e-08 1.67e-06
  c tex 1
    reference   3.36e-08 8.49e-08   1.28e-08 8.30e-07   5.65e-08 8.99e-07   2.86e-08 2.40e-07   1.24e-07 6.20e-06   9.41e-08 4.72e-07   5.21e-08 4.26e-07   1.04e-07 1.72e-06   6.16e-08 1.68e-06
    device      5.07e-08 1.37e-07   1.57e-08 8.48e-07   6.19e-08 1.08e-06   3.04e-08 2.96e-07   1.24e-07 6.19e-06   1.03e-07 4.78e-07   5.21e-08 4.26e-07   1.16e-07 1.73e-06   6.20e-08 1.67e-06
  d tex 0
    reference   3.95e-08 8.61e-08   6.84e-09 9.37e-08   6.52e-08 8.98e-07   3.76e-08 5.15e-07   1.47e-07 6.18e-06   1.09e-07 5.09e-07   6.32e-08 4.80e-07   1.24e-07 1.70e-06   7.76e-08 1.65e-06
    device      3.95e-08 8.61e-08   9.37e-09 1.17e-07   6.52e-08 8.98e-07   3.76e-08 5.21e-07   1.47e-07 6.17e-06   1.09e-07 5.09e-07   6.32e-08 4.80e-07   1.23e-07 1.69e-06   7.66e-08 1.65e-06
  d tex 1
    reference   3.95e-08 8.61e-08   6.84e-09 9.37e-08   6.52e-08 8.98e-07   3.76e-08 5.15e-07   1.47e-07 6.18e-06   1.09e-07 5.09e-07   6.32e-08 4.80e-07   1.24e-07 1.70e-06   7.76e-08 1.65e-06
    device      6.67e-08 1.48e-07   9.98e-09 1.39e-07   7.52e-08 1.17e-06   4.61e-08 6.73e-07   1.47e-07 6.17e-06   1.22e-07 5.18e-07   6.32e-08 4.80e-07   1.37e-07 1.71e-06   7.66e-08 1.65e-06
  e tex 0
    reference   4.09e-08 8.64e-08   1.23e-12 4.07e-07   8.45e-08 1.01e-06   3.84e-08 2.22e-07   1.59e-07 6.41e-06   1.15e-07 5.37e-07   6.96e-08 5.10e-07   1.28e-07 1.78e-06   8.23e-08 1.72e-06
    device      4.09e-08 8.64e-08   1.23e-12 4.03e-07   8.63e-08 1.15e-06   4.16e-08 2.69e-07   1.59e-07 6.41e-06   1.15e-07 5.37e-07   6.96e-08 5.10e-07   1.28e-07 1.81e-06   8.21e-08 1.77e-06
  e tex 1
    reference   4.09e-08 8.64e-08   1.23e-12 4.07e-07   8.45e-08 1.01e-06   3.84e-08 2.22e-07   1.59e-07 6.41e-06   1.15e-07 5.37e-07   6.96e-08 5.10e-07   1.28e-07 1.78e-06   8.23e-08 1.72e-06
    device      6.66e-08 1.43e-07   3.49e-11 4.10e-07   9.50e-08 1.50e-06   4.36e-08 2.83e-07   1.59e-07 6.41e-06   1.27e-07 5.56e-07   6.96e-08 5.10e-07   1.43e-07 1.84e-06   8.21e-08 1.77e-06
  f tex 0
    reference   4.11e-08 8.64e-08   2.09e-09 1.45e-06   7.28e-08 7.60e-07   3.55e-08 2.18e-07   5.96e-07 1.29e-03   1.15e-07 5.02e-07   6.68e-08 4.57e-07   1.18e-07 1.72e-06   7.05e-08 1.66e-06
    device      4.11e-08 8.64e-08   2.40e-09 1.43e-06   7.46e-08 8.75e-07   3.77e-08 2.66e-07   5.96e-07 1.29e-03   1.15e-07 5.02e-07   6.68e-08 4.57e-07   1.18e-07 1.72e-06   7.04e-08 1.66e-06
  f tex 1
    reference   4.11e-08 8.64e-08   2.09e-09 1.45e-06   7.28e-08 7.60e-07   3.55e-08 2.18e-07   5.96e-07 1.29e-03   1.15e-07 5.02e-07   6.68e-08 4.57e-07   1.18e-07 1.72e-06   7.05e-08 1.66e-06
    device      6.80e-08 1.45e-07   2.32e-09 1.42e-06   7.97e-08 1.14e-06   3.95e-08 2.64e-07   5.96e-07 1.29e-03   1.26e-07 5.25e-07   6.68e-08 4.57e-07   1.30e-07 1.74e-06   7.04e-08 1.66e-06
  g tex 0
    reference   0.00e+00 6.32e-08   0.00e+00 1.09e-07   0.00e+00 1.54e-07   0.00e+00 8.89e-08   0.00e+00 6.32e-07   0.00e+00 2.33e-07   0.00e+00 1.77e-07   0.00e+00 2.96e-07   0.00e+00 2.56e-07
    device      0.00e+00 6.32e-08   0.00e+00 1.26e-07   0.00e+00 1.64e-07   0.00e+00 9.63e-08   0.00e+00 6.22e-07   0.00e+00 2.33e-07   0.00e+00 1.77e-07   0.00e+00 2.94e-07   0.00e+00 2.54e-07
  g tex 1
    reference   0.00e+00 6.32e-08   0.00e+00 1.09e-07   0.00e+00 1.54e-07   0.00e+00 8.89e-08   0.00e+00 6.32e-07   0.00e+00 2.33e-07   0.00e+00 1.77e-07   0.00e+00 2.96e-07   0.00e+00 2.56e-07
    device      0.00e+00 1.02e-07   0.00e+00 1.41e-07   0.00e+00 1.87e-07   0.00e+00 1.08e-07   0.00e+00 6.22e-07   0.00e+00 2.45e-07   0.00e+00 1.77e-07   0.00e+00 3.04e-07   0.00e+00 2.54e-07
rows set aside from distance, weight and tpdf (float64 free flight within 4 ulps of max_distance): none on any stratum
stratum a quad tex 0: largest difference from the oracle: density 0.00e+00  distance 2.28e-07  weight 2.89e-06  tpdf 7.09e-07  direction 1.19e-07  f 0.00e+00  pdf 0.00e+00  f@s 5.40e-06  pdf@s 5.34e-06  (set aside 0 rows)
stratum a quad tex 1: largest difference from the oracle: density 2.37e-07  distance 2.70e-07  weight 3.62e-06  tpdf 8.54e-07  direction 1.19e-07  f 3.41e-07  pdf 0.00e+00  f@s 5.38e-06  pdf@s 5.34e-06  (set aside 0 rows)
rows non-finite in the oracle / rows where the device's mask differs: b 872 / 0, c 0 / 0, d 0 / 0, e 0 / 0, f 520 / 0, g 0 / 0
The GPU tests of the module: 41 passed, 8 deselected in 1.33s
"""
import types

import numpy as np
import pytest

import volume_cases as vc
import volume_f64 as v64
from test_gpu_parity import ABS_DIR, REL_BSDF, _rel

F = np.float32
ROWS = vc.ROWS
FORMS = [("quad", 0), ("lane", 1)]
K_BAR = 2.0
E_FLOOR = 1e-6
ASIDE_ULPS, ASIDE_CAP = 4, 2e-4
CPU_MEDIAN = 1e-5
QUANTITIES = ("density", "distance", "weight", "tpdf", "direction", "f", "pdf", "f@s", "pdf@s")
COLS = {"density": slice(1, 4), "distance": slice(8, 9), "weight": slice(9, 12), "tpdf": slice(12, 13), "direction": slice(13, 16),
        "f": slice(16, 19), "pdf": slice(19, 20), "f@s": slice(20, 23), "pdf@s": slice(23, 24)}
FREE_FLIGHT = ("distance", "weight", "tpdf")


def _row_err(got, want, absolute=False):
    """Per row the largest error over the components: relative with a floor of 1e-7, or absolute."""
    got, want = np.asarray(got, np.float64).reshape(len(want), -1), np.asarray(want, np.float64).reshape(len(want), -1)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.max(np.abs(got - want) if absolute else _rel(got, want, 1e-7), axis=1)


def _stat(err):
    return (float(np.median(err)), float(np.percentile(err, 99))) if len(err) else (0.0, 0.0)


def _finite_rows(a):
    return np.isfinite(np.asarray(a, np.float64).reshape(len(a), -1)).all(axis=1)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


_CACHE = {}


def _stratum(name, oracle):
    """Inputs and, per tex form, the float64 values, the oracle's values and the oracle's errors against float64, made once."""
    if name in _CACHE:
        return _CACHE[name]
    s = vc.inputs(name)
    s.rows = None
    s.args = (s.nrm, s.wo, s.wi, s.tex, s.rn)
    s.tex_form = []
    for tex in (0, 1):
        t = types.SimpleNamespace(tex=tex)
        t.f64 = v64.batch(tex, s.mats, *s.args)
        maxd = s.rn[:, 2].astype(np.float64)
        ulp = maxd - np.nextafter(s.rn[:, 2], F(0)).astype(np.float64)  # (towards zero: finite at flt_max too)
        t.aside = np.abs(t.f64.unclamped - maxd) <= ASIDE_ULPS * ulp
        t.orc = oracle.volume(tex, s.mats, *s.args)
        t.e_ref = _errors(s, t, t.orc, t.orc)
        s.tex_form.append(t)
    _CACHE[name] = s
    return s


def _reference(s, t, out, q):
    """float64's value of quantity q; f@s and pdf@s at the sampled direction of `out`."""
    r = t.f64
    if q in ("f@s", "pdf@s"):
        at = out[:, COLS["direction"]].astype(np.float64)
        with np.errstate(invalid="ignore"):
            return v64.eval_scattering(r.medium, s.wo, at) if q == "f@s" else v64.sample_scattering_pdf(r.medium, s.wo, at)
    return {"density": r.density, "distance": r.dist, "weight": r.weight, "tpdf": r.tpdf, "direction": r.dir, "f": r.f, "pdf": r.pdf}[q]


def _errors(s, t, out, orc):
    """(median, p99) against float64 for each of QUANTITIES, over the rows where float64 and the oracle are finite."""
    e = {}
    for q in QUANTITIES:
        want = _reference(s, t, out, q)
        keep = _finite_rows(want) & _finite_rows(orc[:, COLS[q]]) & (~t.aside if q in FREE_FLIGHT else True)
        e[q] = _stat(_row_err(out[keep][:, COLS[q]], want[keep], absolute=q == "direction"))
    return e


def _fmt(e):
    return "  ".join(f"{q} {a:.2e} {b:.2e}" for q, (a, b) in e.items())


# ---------------------------------------------------------------------------------------------------------------
# CPU: the restatement is the oracle's function; the strata are what they claim to be
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(vc.STRATA))
def test_float64_restatement_is_the_oracles_function(oracle, name):
    s = _stratum(name, oracle)
    for t in s.tex_form:
        assert t.aside.mean() <= ASIDE_CAP, f"{t.aside.sum()} rows within {ASIDE_ULPS} ulps of max_distance"
        assert np.array_equal(t.orc[:, 0] != 0, t.f64.inside)  # the crossing's decision is float arithmetic's
        print(f"stratum {name} tex {t.tex}: oracle against float64 (median, p99): {_fmt(t.e_ref)}")
        for q in QUANTITIES:
            if q != "direction":
                assert t.e_ref[q][0] < CPU_MEDIAN, (t.tex, q, t.e_ref[q])
        assert t.e_ref["direction"][0] < 1e-5, t.e_ref["direction"]
    a, b = s.tex_form
    if name != "a":  # texture values of 1: the device-derived density is the host-made one's formula
        assert np.array_equal(a.f64.density, b.f64.density)


def test_strata_reach_the_edges_they_name(oracle):
    b = _stratum("b", oracle)
    assert set(np.unique(b.mats[:, 9])) == set(vc.G_EDGES.tolist()) and len(vc.G_EDGES) == 13
    iso = np.abs(b.mats[:, 9]) < F(1e-3)
    assert 0 < iso.mean() < 0.5 and (np.abs(b.mats[~iso, 9]) == F(1e-3)).any()  # 1e-3f itself takes the anisotropic form
    peak = np.abs(b.mats[:, 9]) >= 0.99
    cosine = -np.sum(vc.unit(b.wo.astype(np.float64)) * vc.unit(b.wi.astype(np.float64)), axis=1)
    assert (np.arccos(np.clip(cosine[peak], -1, 1)) <= 1.001e-3).all()
    c = _stratum("c", oracle)
    d0 = c.tex_form[0].orc[:, 1:4]
    inside = c.tex_form[0].f64.inside
    assert ((d0[inside & (c.case == 0)] == 0).sum(axis=1) == 1).all() and (c.tex_form[0].orc[inside & (c.case == 0), 8] == c.rn[inside & (c.case == 0), 2]).mean() > 0.4
    assert (d0[c.case == 1] == 0).all() and (c.tex_form[0].orc[c.case == 1, 13:24] == 0).all()  # is_zero: no scattering
    clamp = -np.log(F(0.0001)) / c.mats[:, 5]
    for k in (2, 3, 4):
        m = inside & (c.case == k)
        assert (np.abs(d0[m].max(axis=1) / clamp[m] - 1) < 1e-6).all(), k
    assert (c.mats[c.case == 5, 5] == F(1e-4)).all()
    wide = inside & (c.case >= 6)
    ratio = np.sort(d0[wide], axis=1)
    assert (ratio[:, 1] / ratio[:, 0] > 5e2).all() and (ratio[:, 2] / ratio[:, 0] > 3e4).all()
    tr = np.sort(np.exp(-c.tex_form[0].f64.density[wide] * c.tex_form[0].f64.dist[wide, None]), axis=1)  # float64's transmittances
    denormal = (tr[:, 1] < 2.0 ** -126) & (tr[:, 1] > 2.0 ** -149)
    assert denormal.mean() > 0.5 and (tr[:, 1] < 2.0 ** -150).mean() > 0.03 and (tr[:, 0] < 1e-300).all()
    d = _stratum("d", oracle)
    assert len(set(zip(d.rn[:, 0].tolist(), d.rn[:, 1].tolist()))) == 32
    assert set(np.unique(v64.channel(vc.RL_EDGES))) == {0, 1, 2} and (np.bincount(v64.channel(vc.RL_EDGES)) >= 2).all()
    e = _stratum("e", oracle)
    rel = e.tex_form[0].f64.unclamped / e.rn[:, 2].astype(np.float64) - 1
    near = np.isin(e.case, (0, 1, 2, 3, 7))
    assert (np.abs(np.abs(rel[near]) - 1e-3) < 2e-6).all() and (rel[near] > 0).mean() > 0.5 and (rel[near] < 0).mean() > 0.3
    assert {F(1e-6), F(1e30), vc.FLT_MAX} <= set(np.unique(e.rn[:, 2]))
    f = _stratum("f", oracle)
    assert (f.wo[f.case == 0] == [0, 0, 1]).all() and (f.wo[f.case == 1] == [0, 0, -1]).all()
    assert np.signbit(f.wo[f.case == 2, 2]).all() and (f.wo[f.case == 2, 2] == 0).all() and not np.signbit(f.wo[f.case == 3, 2]).any()
    tilt = np.arccos(np.clip(np.abs(f.wo[np.isin(f.case, (4, 5)), 2].astype(np.float64)), 0, 1))
    assert (np.hypot(*f.wo[np.isin(f.case, (4, 5)), 0:2].T.astype(np.float64)) > 0.9e-4).all() and (tilt < 4e-4).all()
    length = np.linalg.norm(f.wo.astype(np.float64), axis=1)
    assert (np.abs(length[f.case == 6] - 0.5) < 1e-6).all() and (np.abs(length[f.case == 7] - 3) < 1e-6).all()
    assert len(set(zip(f.rn[:, 3].tolist(), f.rn[:, 4].tolist())) & {(x, y) for x in (0.0, 0.25, float(vc.BELOW1)) for y in (0.0, float(vc.BELOW1))}) == 6
    g = _stratum("g", oracle)
    assert len(set(zip(g.no.tolist(), g.ni.tolist(), g.kind.tolist()))) == 100
    assert np.array_equal(v64.dot32(g.nrm, g.wo), g.no.astype(F)) and np.array_equal(v64.dot32(g.nrm, g.wi), g.ni.astype(F))
    inside = g.tex_form[0].f64.inside
    assert not inside[g.kind < 3].any() and np.array_equal(inside[g.kind == 3], (g.no * g.ni < 0)[g.kind == 3]) and inside.any()


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
_DEV = {}


def _device(ctx, yh, s, form, tex):
    key = (s.name, form, tex)
    if key not in _DEV:
        if s.rows is None:
            s.rows = yh.volume_material_rows(s.mats)
        _DEV[key] = ctx.volume(form, tex, s.rows, *s.args)
    return _DEV[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(vc.STRATA))
def test_quad_and_lane_forms_agree_bit_for_bit(ctx, yh, oracle, name):
    s = _stratum(name, oracle)
    for tex in (0, 1):
        q, l = _device(ctx, yh, s, 0, tex), _device(ctx, yh, s, 1, tex)
        differ = np.flatnonzero((q.view(np.uint32) != l.view(np.uint32)).any(axis=1))
        assert len(differ) == 0, f"tex {tex}: {len(differ)} rows differ between the forms, first {differ[:5]}: {q[differ[:2]]} {l[differ[:2]]}"


@pytest.mark.gpu
@pytest.mark.parametrize("form", [f[0] for f in FORMS])
@pytest.mark.parametrize("name", list(vc.STRATA))
def test_decisions_and_host_made_medium_are_exact(ctx, yh, oracle, name, form):
    s = _stratum(name, oracle)
    for t in s.tex_form:
        out = _device(ctx, yh, s, dict(FORMS)[form], t.tex)
        assert np.array_equal(out[:, 0], t.orc[:, 0]), "in_medium"
        assert _same_bits(out[:, 4:8], t.orc[:, 4:8]), "scatter, anisotropy"
        if t.tex == 0:
            assert _same_bits(out[:, 1:4], t.orc[:, 1:4]), "the host-made density"
        bad = np.flatnonzero((np.isfinite(out) != np.isfinite(t.orc)).any(axis=1))
        print(f"stratum {name} {form} tex {t.tex}: {int((~np.isfinite(t.orc)).any(axis=1).sum())} of {s.n} rows non-finite in the oracle, {len(bad)} rows with another mask")
        assert len(bad) == 0, (bad[:5], out[bad[:2]], t.orc[bad[:2]])
    if name == "d":  # the channel, recovered from the distance: three well-separated densities, max_distance out of the way
        t = s.tex_form[0]
        out = _device(ctx, yh, s, dict(FORMS)[form], 0)
        rows = np.flatnonzero(t.f64.inside & (s.rn[:, 1] > 0))
        with np.errstate(divide="ignore"):
            cand = -np.log1p(-s.rn[rows, 1].astype(np.float64))[:, None] / t.f64.density[rows]
        got = np.argmin(np.abs(cand / out[rows, 8:9].astype(np.float64) - 1), axis=1)
        assert len(rows) > ROWS // 2 and np.array_equal(got, v64.channel(s.rn[rows, 0])), np.flatnonzero(got != v64.channel(s.rn[rows, 0]))[:5]
        assert (np.min(np.abs(cand / out[rows, 8:9].astype(np.float64) - 1), axis=1) < 1e-5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [f[0] for f in FORMS])
def test_stated_bars_hold_on_todays_domain(ctx, yh, oracle, form):
    s = _stratum("a", oracle)
    for t in s.tex_form:
        assert t.aside.mean() <= ASIDE_CAP  # on the inputs, before the device is looked at
        out = _device(ctx, yh, s, dict(FORMS)[form], t.tex)
        fig = {}
        for q in QUANTITIES:
            keep = _finite_rows(t.orc[:, COLS[q]]) & (~t.aside if q in FREE_FLIGHT else True)
            fig[q] = float(np.max(_row_err(out[keep][:, COLS[q]], t.orc[keep][:, COLS[q]], absolute=q == "direction")))
        print(f"stratum a {form} tex {t.tex}: largest difference from the oracle: " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items())
              + f"  (set aside {int(t.aside.sum())} rows)")
        for q in QUANTITIES:
            assert fig[q] <= (ABS_DIR if q == "direction" else REL_BSDF), (t.tex, q, fig[q])


@pytest.mark.gpu
@pytest.mark.parametrize("form", [f[0] for f in FORMS])
@pytest.mark.parametrize("name", list(vc.STRATA))
def test_error_against_float64_is_the_references_own(ctx, yh, oracle, name, form):
    s = _stratum(name, oracle)
    for t in s.tex_form:
        assert t.aside.mean() <= ASIDE_CAP  # on the inputs, before the device is looked at
        out = _device(ctx, yh, s, dict(FORMS)[form], t.tex)
        e_dev = _errors(s, t, out, t.orc)
        print(f"stratum {name} {form} tex {t.tex} (median, p99 | reference's):  "
              + "  ".join(f"{q} {e_dev[q][0]:.2e} {e_dev[q][1]:.2e} | {t.e_ref[q][0]:.2e} {t.e_ref[q][1]:.2e}" for q in QUANTITIES)
              + f"  (set aside {int(t.aside.sum())} rows)")
        if name == "a":
            continue  # stratum a is held to the stated bars (test_stated_bars_hold_on_todays_domain); its figures are printed for the table
        bad = [(q, i, e_dev[q][i], t.e_ref[q][i]) for q in QUANTITIES for i in (0, 1) if not e_dev[q][i] <= K_BAR * max(t.e_ref[q][i], E_FLOOR)]
        assert not bad, f"tex {t.tex}: (quantity, 0 median / 1 p99, device, reference) beyond {K_BAR} x max(reference, {E_FLOOR}): {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("form", [f[0] for f in FORMS])
def test_batch_shape_does_not_change_a_row(ctx, yh, oracle, form):
    s = _stratum("a", oracle)
    for tex in (0, 1):
        whole = _device(ctx, yh, s, dict(FORMS)[form], tex)
        for n in (1, 3, 4097):  # one row, a ragged quad, a ragged last block
            part = ctx.volume(dict(FORMS)[form], tex, s.mats[:n], *(x[:n] for x in s.args))
            assert _same_bits(part, whole[:n]), (tex, n)


def _quad_form_inputs():
    rng = np.random.default_rng(2190)
    n = ROWS
    row = np.arange(n)
    nrm = vc.unit(rng.normal(size=(n, 3))).astype(F)
    nrm[row % 16 == 0] = [0, 0, 1]
    nrm[row % 16 == 1] = [0, 0, -1]
    nrm[row % 16 == 2, 2] = -0.0
    nrm[row % 16 == 3] *= F(3)
    nrm[row % 16 == 4] *= F(1e-20)  # the squared length underflows: the `l != 0` switch
    nrm[row % 16 == 5] = 0
    rn = np.minimum(rng.uniform(0, 1, (n, 2)).astype(F), vc.BELOW1)
    edge = np.array([0, 0.25, 0.5, vc.BELOW1], F)
    rn[row % 3 == 0, 0], rn[row % 3 == 0, 1] = edge[(row // 3) % 4][row % 3 == 0], edge[(row // 12) % 4][row % 3 == 0]
    special = np.array([0, -0.0, 1e-45, -1e-40, 1e-38, np.inf, -np.inf, np.nan, 1, 3, 1e38, 1e-3], F)
    a = (rng.normal(size=(n, 3)) * 10 ** rng.uniform(-6, 6, (n, 3))).astype(F)
    a[row % 5 == 0, 0] = special[(row // 5) % len(special)][row % 5 == 0]
    a[row % 7 == 0, 2] = special[(row // 7) % len(special)][row % 7 == 0]
    b = (rng.normal(size=n) * 10 ** rng.uniform(-6, 6, n)).astype(F)
    b[row % 2 == 0] = special[(row // 2) % len(special)][row % 2 == 0]
    return nrm, rn, a, b


@pytest.mark.gpu
def test_quad_forms_render_the_plain_forms_bits(ctx, yh):
    nrm, rn, a, b = _quad_form_inputs()
    for k in (0.0, 1e-45, np.inf, np.nan):
        assert (b == F(k)).any() or (np.isnan(k) and np.isnan(b).any())
    out = ctx.quad_forms(nrm, rn, a, b)
    bits = out.view(np.uint32)
    differ = np.flatnonzero((bits[:, 0:3] != bits[:, 3:6]).any(axis=1))
    assert len(differ) == 0, f"sample_hemisphere_cos_quad: {len(differ)} rows differ, first {differ[:5]}: {nrm[differ[:2]]} {rn[differ[:2]]} {out[differ[:2], 0:6]}"
    differ = np.flatnonzero((bits[:, 6:9] != bits[:, 9:12]).any(axis=1))
    assert len(differ) == 0, f"quad_div: {len(differ)} rows differ, first {differ[:5]}: {a[differ[:2]]} {b[differ[:2]]} {out[differ[:2], 6:12]}"
    # ... and the plain forms are the operations they name: IEEE division, and the oracle's cosine-weighted direction
    with np.errstate(all="ignore"):
        want = a / b[:, None]
    nan = np.isnan(want)  # (a NaN's sign and payload are the platform's)
    assert np.array_equal(np.isnan(out[:, 9:12]), nan) and _same_bits(np.where(nan, F(0), out[:, 9:12]), np.where(nan, F(0), want))
    ok = np.linalg.norm(nrm.astype(np.float64), axis=1) > 0.5
    z = np.sqrt(rn[ok, 1].astype(np.float64))
    assert np.max(np.abs(np.sum(out[ok, 3:6].astype(np.float64) * vc.unit(nrm[ok].astype(np.float64)), axis=1) - z)) < 1e-6  # cos to the normal is sqrt(ry)
    for n in (1, 3, 4097):
        assert _same_bits(ctx.quad_forms(nrm[:n], rn[:n], a[:n], b[:n]), out[:n]), n


@pytest.mark.gpu
def test_refusals(ctx, yh, oracle):
    s = _stratum("a", oracle)
    n = 8
    m = yh.volume_material_rows(s.mats[:n])
    out = np.full((n, yh.VOLUME_FLOATS), 7, F)
    rows = [np.ascontiguousarray(x[:n]) for x in s.args]
    ptrs = [yh.fptr(x) for x in rows] + [yh.fptr(out)]
    call = ctx.lib.yh_volume_batch
    for form, tex in ((0, 0), (1, 0), (0, 1), (1, 1)):
        out[:] = 7
        assert call(ctx.h, form, tex, n, m, *ptrs) == yh.YH_OK and not (out == 7).any()
    for form, tex in ((2, 0), (-1, 0), (0, 2), (0, -1)):
        assert call(ctx.h, form, tex, n, m, *ptrs) == yh.YH_E_INVALID
    for bad_n in (0, -1):
        assert call(ctx.h, 0, 0, bad_n, m, *ptrs) == yh.YH_E_INVALID
    assert call(None, 0, 0, n, m, *ptrs) == yh.YH_E_INVALID
    assert call(ctx.h, 0, 0, n, None, *ptrs) == yh.YH_E_INVALID
    for k in range(len(ptrs)):
        assert call(ctx.h, 0, 0, n, m, *[None if i == k else p for i, p in enumerate(ptrs)]) == yh.YH_E_INVALID
    nrm, rn, a, b = (np.ascontiguousarray(x[:n]) for x in _quad_form_inputs())
    qout = np.full((n, yh.QUAD_FORMS_FLOATS), 7, F)
    qptrs = [yh.fptr(x) for x in (nrm, rn, a, b, qout)]
    qcall = ctx.lib.yh_quad_forms_batch
    assert qcall(ctx.h, n, *qptrs) == yh.YH_OK and not (qout == 7).any()
    for bad_n in (0, -1):
        assert qcall(ctx.h, bad_n, *qptrs) == yh.YH_E_INVALID
    assert qcall(None, n, *qptrs) == yh.YH_E_INVALID
    for k in range(len(qptrs)):
        assert qcall(ctx.h, n, *[None if i == k else p for i, p in enumerate(qptrs)]) == yh.YH_E_INVALID
    # ... and each refusal leaves a usable context
    assert _same_bits(ctx.volume(0, 0, s.mats[:n], *rows), _device(ctx, yh, s, 0, 0)[:n])
