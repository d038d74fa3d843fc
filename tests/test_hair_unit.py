"""The hair BSDF on the device in every form the integrators run it (yh_hair_shade_batch: unit/hair_shade.h), at unit level and at its
edges: a quad per row in the default arithmetic (k_trace and its kin), a lane per row in the default arithmetic (k_stream), a quad per
row in the exact arithmetic (csrc/exact.hip) — hair_setup, hair_prepare, hair_sample from that hair_out and the fused eval + pdf, on the
material row the upload's own code makes (host/scene_upload.cpp: make_material).

References: the oracle (float arithmetic, the reference's operations) and tests/hair_f64.py, the same formulas in float64. At the edges
of the domain the oracle's own float arithmetic leaves the 1e-4 band around float64 (conditioning: 1 / v in mp's exponent, cos_theta_o
-> 0), so there the device is held to the ORACLE'S OWN error against float64, measured by the test on the same rows each time it runs.

Strata (ROWS rows each, fixed seeds):
  a  today's domain: beta_m, beta_n ~ U(0.05, 0.95), eta 1.55, isotropic directions (test_hair_batches_match_oracle_on_fresh_inputs)
  b  beta_m in {0.05, 0.1}
  c  beta_m within +-2 % of the three values at which v[0], v[1] = v[0] / 4, v[2] = 4 v[0] equal 0.1 (mp's switch), a lobe per row
  d  cos_theta_i cos_theta_o / v within +-10 % of 12 (log_i0's switch) for lobe 0 or lobe 1, alpha 0, near the specular cone
  e  phi - Phi(p) within 1e-3 of +-pi (np's wrap), a lobe per row
  f  beta_n = 0.05
  g  outgoing 1e-3 rad from the tangent and exactly along it, both signs, under an isotropic normal
  h  v in {0, 1, 1e-7, 0.9999999, 0.5}: h = -1, 1, ...
  i  sigma_a = 0 and eumelanin 8, alpha in {0, 10}, eta in {1.0, 1.3, 1.7}
  j  rn components in {0, 1 - 2^-24, 0.5}, de-interleaved halves 0 (the only value below the 1e-5 clamp), u[0][0] 1e-3 either side of
     each cumulative lobe pdf of the float64 lobe pdfs
  y  (2 048 rows) g with the normal made orthogonal to the tangent, so that the tangent is the frame's x axis: cos_theta_o is 0 or
     3.45e-4 in float and etap a division by zero. Float's sqrt(1 - x^2) has lost its digits there, on both sides: the oracle's own
     median error against float64 is 1.4e-4 (f; 1.2e-3 at the sampled direction) and its p99 O(1e3), so y is held to finiteness, to bar 1 and to the MEDIAN half of bar 3
  z  (512 rows) y with sigma_a = 0 and h = +-1, exactly along the strand: ap[3] is 0 / 0

Every stratum is evaluated at `incoming` and, in a second call, at the float64 restatement's sampled direction (the specular cone, where
a narrow lobe is not zero): columns f, pdf and f@s, pdf@s below.

Bars (none of them taken from what the device gives):
  1  quad-fast and lane-fast: all 15 floats of every row bit for bit, NaN pattern included;
  2  stratum a against the oracle: f and pdf at `incoming` and at the oracle's sampled direction, and the lobe pdfs, within REL_BSDF
     (1e-4, floor 1e-7), the sampled direction within ABS_DIR (5e-5). A row is set aside from the direction check only when its u[0][0] lies within 1e-5
     of a cumulative lobe pdf of the float64 lobe pdfs (a last-place difference picks another lobe there); at most 2e-4 of the rows,
     asserted on the inputs;
  3  strata b-j (and y: medians only) against float64: median and p99 of the relative error (floor 1e-7; per row the largest over the components) of f, pdf
     and the lobe pdfs, and of the absolute error of the sampled direction, at most K x max(the oracle's same statistic on the same
     rows, 1e-6): K = 2 for the exact arithmetic (the reference's IEEE operations, libm's last place apart), K = 4 for the default
     arithmetic (reciprocal, square root and asinf of 1 ulp for 0.5);
  4  every output finite wherever the oracle's and the restatement's are: every row of a-j and y; on z the non-finite mask is the oracle's;
  5  the outputs at `incoming` equal yh_hair_eval_batch / yh_hair_pdf_batch (device-derived material constants) within REL_BSDF;
  6  n in {1, 3, 4097}: each row equals the same row of the ROWS-row call bit for bit; the refusals of the entry point.
The CPU test holds the restatement to the oracle (and to the real reference where it is built): median relative difference of f and
pdf at `incoming` below 1e-5 on every stratum (the largest median measured on the CPU is 6e-7; a wrong formula gives O(1)), at the
sampled direction too (stratum b: 1e-4, CPU_MEDIAN_AT_SAMPLE), the oracle finite on every row of a-j and y.

What the bars catch, tried once on a copy of the library whose unit kernels were compiled from a dev_hair.h with two one-token errors:
mp's 0.6931f written 0.69315f (5e-5 of every lobe with v <= 0.1) fails bar 3 on strata c, d and i in every combination and on b, f, h and j
in the exact arithmetic, and no other bar — stratum a stays inside its 1e-4; hair_prepare<true> taking pdf0 from lane 0 instead of lane 2 fails bar 1 on every stratum.

MEASURED (2026-10-19, AMD Instinct MI355X, gfx950; also profiles/hair_unit/errors.txt): no assertion fails; quad-fast and lane-fast agree bit
for bit on every stratum.
median and p99 per stratum of the error against float64 (relative with a floor of 1e-7, per row the largest over the components;
direction: absolute), 8192 rows each (y: 2048; its p99 is held to no bar). reference = the oracle on the CPU; fast = quad-fast =
lane-fast (bit for bit); exact = quad-exact.
              f                   pdf                 f@s                 pdf@s               lobe pdfs           direction
  a
    reference 3.82e-07 1.49e-05   2.92e-07 1.37e-05   5.38e-07 4.29e-05   4.31e-07 4.17e-05   3.41e-07 4.12e-06   1.14e-07 1.09e-06
    fast      4.23e-07 1.61e-05   3.36e-07 1.46e-05   5.80e-07 4.36e-05   4.74e-07 4.19e-05   4.03e-07 3.93e-06   1.27e-07 1.10e-06
    exact     3.90e-07 1.56e-05   3.08e-07 1.42e-05   5.47e-07 4.35e-05   4.43e-07 4.17e-05   3.43e-07 4.12e-06   1.20e-07 1.10e-06
  b
    reference 1.62e-11 1.06e-04   3.38e-11 9.81e-05   1.74e-05 2.71e-04   1.69e-05 2.71e-04   3.42e-07 3.11e-06   1.81e-07 2.33e-06
    fast      1.72e-11 1.05e-04   3.78e-11 9.81e-05   1.75e-05 2.71e-04   1.69e-05 2.71e-04   3.92e-07 3.23e-06   1.93e-07 2.36e-06
    exact     1.67e-11 1.05e-04   3.56e-11 9.81e-05   1.74e-05 2.71e-04   1.69e-05 2.71e-04   3.43e-07 3.11e-06   1.85e-07 2.36e-06
  c
    reference 4.93e-07 1.18e-05   3.98e-07 1.12e-05   7.97e-07 1.66e-05   6.93e-07 1.63e-05   3.42e-07 4.01e-06   1.10e-07 9.34e-07
    fast      5.62e-07 1.28e-05   4.69e-07 1.19e-05   8.55e-07 1.64e-05   7.63e-07 1.59e-05   3.96e-07 3.92e-06   1.22e-07 9.50e-07
    exact     5.17e-07 1.23e-05   4.28e-07 1.16e-05   8.38e-07 1.61e-05   7.30e-07 1.57e-05   3.43e-07 4.01e-06   1.14e-07 9.54e-07
  d
    reference 8.04e-07 9.94e-06   6.69e-07 9.67e-06   6.50e-07 9.63e-06   5.86e-07 9.59e-06   3.41e-07 1.54e-06   1.04e-07 7.61e-07
    fast      8.83e-07 1.06e-05   7.24e-07 1.04e-05   7.13e-07 1.06e-05   6.38e-07 1.05e-05   3.85e-07 1.79e-06   1.15e-07 7.84e-07
    exact     8.40e-07 1.01e-05   6.85e-07 9.82e-06   6.82e-07 1.05e-05   6.22e-07 1.03e-05   3.41e-07 1.54e-06   1.08e-07 7.73e-07
  e
    reference 5.86e-07 4.16e-05   4.21e-07 3.81e-05   3.98e-07 4.26e-05   2.96e-07 4.20e-05   3.42e-07 3.68e-06   1.17e-07 1.15e-06
    fast      6.40e-07 4.17e-05   4.67e-07 3.77e-05   4.31e-07 4.29e-05   3.29e-07 4.21e-05   3.88e-07 3.75e-06   1.30e-07 1.15e-06
    exact     6.14e-07 4.20e-05   4.40e-07 3.81e-05   4.10e-07 4.26e-05   3.12e-07 4.21e-05   3.43e-07 3.68e-06   1.23e-07 1.16e-06
  f
    reference 7.92e-08 2.90e-05   7.41e-08 2.79e-05   3.80e-06 5.51e-05   3.77e-06 5.46e-05   3.46e-07 3.86e-06   1.03e-07 6.89e-07
    fast      8.98e-08 3.39e-05   8.31e-08 3.41e-05   4.41e-06 5.63e-05   4.36e-06 5.61e-05   3.91e-07 3.87e-06   1.15e-07 7.00e-07
    exact     8.01e-08 3.10e-05   7.50e-08 3.10e-05   4.12e-06 5.40e-05   4.10e-06 5.36e-05   3.46e-07 3.81e-06   1.08e-07 7.03e-07
  g
    reference 4.01e-07 4.04e-05   2.77e-07 2.79e-05   6.32e-07 5.43e-05   4.23e-07 4.46e-05   5.24e-07 4.57e-04   1.22e-07 2.42e-06
    fast      4.42e-07 4.00e-05   3.00e-07 2.84e-05   6.58e-07 5.41e-05   4.59e-07 4.44e-05   6.01e-07 4.57e-04   1.32e-07 2.41e-06
    exact     4.02e-07 4.00e-05   2.78e-07 2.81e-05   6.34e-07 5.43e-05   4.27e-07 4.44e-05   5.24e-07 4.57e-04   1.24e-07 2.42e-06
  h
    reference 2.77e-07 4.12e-05   2.41e-07 3.27e-05   4.28e-07 2.95e-05   4.00e-07 2.92e-05   2.81e-07 1.16e-04   1.23e-07 9.80e-07
    fast      3.02e-07 4.45e-05   2.63e-07 3.66e-05   4.61e-07 2.97e-05   4.37e-07 2.96e-05   2.92e-07 1.34e-04   1.26e-07 9.97e-07
    exact     2.92e-07 4.14e-05   2.53e-07 3.25e-05   4.52e-07 2.97e-05   4.21e-07 2.96e-05   2.80e-07 1.16e-04   1.26e-07 9.97e-07
  i
    reference 2.72e-07 1.39e-05   2.59e-07 2.37e-05   6.45e-07 8.25e-05   5.37e-07 1.02e-04   2.11e-07 6.19e-02   1.19e-07 1.42e-06
    fast      2.85e-07 1.41e-05   2.79e-07 2.38e-05   7.18e-07 8.22e-05   6.22e-07 1.04e-04   2.35e-07 7.12e-02   1.26e-07 1.42e-06
    exact     2.81e-07 1.39e-05   2.67e-07 2.41e-05   6.86e-07 8.22e-05   5.91e-07 1.03e-04   2.12e-07 6.19e-02   1.23e-07 1.44e-06
  j
    reference 3.79e-07 1.65e-05   2.94e-07 1.58e-05   5.46e-07 4.44e-05   4.29e-07 4.18e-05   3.26e-07 3.44e-06   1.35e-07 1.63e-05
    fast      4.25e-07 1.69e-05   3.33e-07 1.63e-05   5.88e-07 4.44e-05   4.75e-07 4.20e-05   3.77e-07 3.81e-06   1.52e-07 2.02e-05
    exact     3.91e-07 1.65e-05   3.05e-07 1.58e-05   5.64e-07 4.44e-05   4.52e-07 4.18e-05   3.24e-07 3.44e-06   1.43e-07 2.02e-05
  y
    reference 1.39e-04 5.29e+03   4.35e-05 5.29e+03   1.22e-03 2.35e+00   1.12e-03 2.35e+00   5.83e-06 1.65e-01   8.83e-05 1.36e+00
    fast      1.39e-04 5.29e+03   4.29e-05 5.29e+03   1.22e-03 2.35e+00   1.13e-03 2.35e+00   5.86e-06 1.65e-01   8.83e-05 1.36e+00
    exact     1.39e-04 5.29e+03   4.38e-05 5.29e+03   1.22e-03 2.35e+00   1.13e-03 2.35e+00   5.83e-06 1.65e-01   8.83e-05 1.36e+00
stratum a against the oracle, largest difference over the rows (bars: f, pdf, lobe pdfs 1e-4; direction 5e-5):
    quad-fast  f 3.40e-05  pdf 3.38e-05  f@s 6.04e-05  pdf@s 5.98e-05  direction 1.08e-06  lobe pdfs 3.08e-06  (set aside 0 rows)
    lane-fast  f 3.40e-05  pdf 3.38e-05  f@s 6.04e-05  pdf@s 5.98e-05  direction 1.08e-06  lobe pdfs 3.08e-06  (set aside 0 rows)
    quad-exact f 3.63e-05  pdf 3.63e-05  f@s 5.96e-05  pdf@s 5.96e-05  direction 1.08e-06  lobe pdfs 6.46e-07  (set aside 0 rows)
stratum z: 512 of 512 rows non-finite in the oracle, 0 rows with another mask (the three combinations alike)
rows that differ at all between the host's material row and the device-derived one: 2494 of 8192; largest 3.62e-05 (f) 3.62e-05 (pdf)
The 68 tests of the module take 1.57 s together.
"""
import types

import numpy as np
import pytest

import hair_f64 as h64
import oracle_capi as oc
from test_gpu_parity import ABS_DIR, REL_BSDF, _rel

ROWS = 8192
F = np.float32
BELOW1 = np.nextafter(F(1), F(0))  # 1 - 2^-24
COMBOS = [("quad-fast", 0, 0), ("lane-fast", 1, 0), ("quad-exact", 0, 1)]  # (id, form, exact)
K_BAR = {0: 4.0, 1: 2.0}  # by `exact`
E_FLOOR = 1e-6
U_ASIDE, ASIDE_CAP = 1e-5, 2e-4
STRATA = "abcdefghij"
SEEDS = {s: 1100 + k for k, s in enumerate(STRATA + "zy")}
# The CPU test's bar on the median difference between the oracle and the restatement: 1e-5, at the sampled direction too — but for
# stratum b there. At the sampled direction every row sits in the specular cone, and with beta_m = 0.05 mp's exponent sums three terms
# of magnitude 1 / v[1] = 2 720, each rounded to float: three roundings of 2 720 x 2^-24 / sqrt(12) rms each are 8e-5 of the value.
CPU_MEDIAN = 1e-5
CPU_MEDIAN_AT_SAMPLE = {"b": 1e-4}
QUANTITIES = ("f", "pdf", "f@s", "pdf@s", "lobe pdfs", "direction")


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _v0(beta):
    return (0.726 * beta + 0.812 * beta ** 2 + 3.7 * beta ** 20) ** 2


def _beta_for_v0(v0):
    """beta_m with v[0] = v0: the root of the (monotone) polynomial of eval_hair_brdf, by bisection."""
    lo, hi = np.zeros_like(np.asarray(v0, np.float64)), np.ones_like(np.asarray(v0, np.float64))
    for _ in range(60):
        mid = (lo + hi) / 2
        up = _v0(mid) < v0
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    return (lo + hi) / 2


def _local(theta, phi):
    return np.stack([np.sin(theta), np.cos(theta) * np.cos(phi), np.cos(theta) * np.sin(phi)], axis=1)


def _base(rng, n):
    """Today's domain, drawn as test_hair_batches_match_oracle_on_fresh_inputs draws it."""
    mats = np.zeros((n, 12), F)
    mats[:, 3:5] = rng.uniform(0.05, 0.95, (n, 2))
    mats[:, 5] = rng.uniform(0, 4, n)
    mats[:, 6] = 1.55
    mats[:, 10] = rng.uniform(0, 8, n)
    v = rng.uniform(0, 1, n).astype(F)
    d = lambda: _unit(rng.normal(size=(n, 3))).astype(F)  # noqa: E731
    tng, wo, wi, nrm = d(), d(), d(), d()
    rn = np.minimum(rng.uniform(0, 1, (n, 2)).astype(F), BELOW1)
    return types.SimpleNamespace(mats=mats, v=v, nrm=nrm, tng=tng, wo=wo, wi=wi, rn=rn)


def _inputs(name, oracle):
    n = {"z": 512, "y": 2048}.get(name, ROWS)
    rng = np.random.default_rng(SEEDS[name])
    s = _base(rng, n)
    row = np.arange(n)
    brdf = lambda: h64.Brdf(oracle.hair_brdf(s.mats, s.v, s.nrm, s.tng))  # noqa: E731
    if name == "b":
        s.mats[:, 3] = np.where(row % 2 == 0, F(0.05), F(0.1))
    elif name == "c":
        star = _beta_for_v0(np.array([0.1, 0.4, 0.025]))  # v[0] = 0.1, v[1] = v[0] / 4 = 0.1, v[2] = 4 v[0] = 0.1
        s.lobe = row % 3
        s.mats[:, 3] = star[s.lobe] * rng.uniform(0.98, 1.02, n)
    elif name == "d":
        s.lobe = row % 2
        vp = rng.uniform(0.03, 0.07, n)
        s.mats[:, 3] = _beta_for_v0(np.where(s.lobe == 0, vp, 4 * vp))
        s.mats[:, 5] = 0
        B = brdf()
        t = 12 * B.v[np.arange(n), s.lobe] * rng.uniform(0.9, 1.1, n)
        e, sg = rng.uniform(-0.03, 0.03, n), rng.choice([-1.0, 1.0], n)
        theta_o, theta_i = sg * np.arccos(np.sqrt(t) * np.exp(e)), -sg * np.arccos(np.sqrt(t) * np.exp(-e))
        s.wo = B.to_world(_local(theta_o, rng.uniform(-np.pi, np.pi, n))).astype(F)
        s.wi = B.to_world(_local(theta_i, rng.uniform(-np.pi, np.pi, n))).astype(F)
    elif name == "e":
        s.lobe = row % 3
        s.mats[:, 4] = rng.uniform(0.3, 0.95, n)
        B = brdf()
        sin_o, cos_o, phi_o = h64._outgoing(B, s.wo)
        _, gamma_t = h64.transmittance(B, sin_o, cos_o)
        s.delta = rng.uniform(-0.9e-3, 0.9e-3, n)
        phi_i = phi_o + h64.phi_fn(s.lobe, B.gamma_o, gamma_t) + rng.choice([-1.0, 1.0], n) * np.pi + s.delta
        theta_i = np.clip(-np.arcsin(sin_o) + rng.normal(0, 0.2, n), -1.5, 1.5)
        s.wi = B.to_world(_local(theta_i, phi_i)).astype(F)
    elif name == "f":
        s.mats[:, 4] = 0.05
    elif name in ("g", "y", "z"):
        # g measures the angle from the tangent as it is given, under an isotropic normal: the frame's x axis is the tangent
        # orthonormalised against the normal, so theta_o stays away from +-pi / 2. y and z have the normal made orthogonal to the
        # tangent, so that the tangent IS the x axis and cos_theta_o comes out as 0 or 3.45e-4 (etap: a division by zero). There
        # float's sqrt(1 - x^2) has lost its digits, in the oracle as on the device.
        orth = name != "g"
        t64, n64 = s.tng.astype(np.float64), s.nrm.astype(np.float64)
        if orth:
            s.nrm = _unit(n64 - t64 * np.sum(n64 * t64, axis=1, keepdims=True)).astype(F)
        if name == "z":
            s.mats[:, 10] = 0  # sigma_a = 0: no colour, no melanin
            s.v = np.where(row % 4 < 2, F(0), F(1))
            ang, sg = np.zeros(n), np.where(row % 2 == 0, 1.0, -1.0)
        else:
            ang, sg = np.where(row % 2 == 0, 0.0, 1e-3), np.where((row // 2) % 2 == 0, 1.0, -1.0)
        s.ang, s.sg = ang, sg
        B = brdf()
        along = np.asarray(B.M[:, :, 0]) if orth else t64  # the frame's x axis (a float32 vector), or the tangent as given
        side = _unit(np.cross(along, rng.normal(size=(n, 3))))
        wo = _unit(np.cos(ang)[:, None] * along + np.sin(ang)[:, None] * side)
        s.wo = (sg[:, None] * np.where((ang == 0)[:, None], along, wo)).astype(F)
    elif name == "h":
        s.v = np.array([0, 1, 1e-7, 0.9999999, 0.5], F)[row % 5]
    elif name == "i":
        s.mats[:, 10] = np.where(row % 2 == 0, 0, 8)
        s.mats[:, 5] = np.where((row // 2) % 2 == 0, 0, 10)
        s.mats[:, 6] = np.array([1.0, 1.3, 1.7], F)[(row // 4) % 3]
    elif name == "j":
        s.mats[:900, 10] = 0.2  # light hair under the edge values: the last lobe's pdf is a few per cent, and 1 - 2^-24 (u[0][0] = 0.99976) selects it
        B = brdf()
        c = h64.boundaries(h64.lobe_pdfs(B, s.wo))
        edge = np.array([F(0), BELOW1, F(0.5)])
        k = row[:900]
        s.rn[k, 0], s.rn[k, 1] = edge[k % 3], edge[(k // 3) % 3]
        r12 = lambda m: rng.integers(0, 4096, m).astype(np.uint64) << np.uint64(4)  # noqa: E731
        k = row[900:1800]
        zero = np.zeros(len(k), np.uint64)
        s.rn[k, 1] = h64.mux_float(zero, np.where(k % 2 == 0, r12(len(k)), zero))      # u[1][0] = 0 (below the 1e-5 clamp)
        s.rn[k, 0] = h64.mux_float(r12(len(k)), np.where(k % 3 == 0, zero, r12(len(k))))  # ... and u[0][1] = 0 on a third
        k = row[1800:4800]
        side = np.where(k % 2 == 0, 1.0, -1.0)
        target = c[k, (k // 2) % 3] + side * 1e-3
        grid = np.where(side > 0, np.ceil(target * 4096), np.floor(target * 4096))
        ok = (grid >= 0) & (grid <= 4095)
        s.rn[k[ok], 0] = h64.mux_float(grid[ok].astype(np.uint64) << np.uint64(4), r12(int(ok.sum())))
        s.placed = k[ok]
    for key in ("mats", "v", "nrm", "tng", "wo", "wi", "rn"):
        setattr(s, key, np.ascontiguousarray(getattr(s, key), F))
    return s


def _row_err(got, want, absolute=False):
    """Per row the largest error over the components: relative with a floor of 1e-7, or absolute."""
    got, want = np.asarray(got, np.float64).reshape(len(want), -1), np.asarray(want, np.float64).reshape(len(want), -1)
    with np.errstate(invalid="ignore"):
        return np.max(np.abs(got - want) if absolute else _rel(got, want, 1e-7), axis=1)


def _stat(err):
    return float(np.median(err)), float(np.percentile(err, 99))


_CACHE = {}


def _stratum(name, oracle):
    """Inputs, the float64 values, the oracle's values and the oracle's errors against float64 (E50_ref, E99_ref), made once."""
    if name in _CACHE:
        return _CACHE[name]
    s = _inputs(name, oracle)
    s.name, s.n = name, len(s.v)
    s.brdf = oracle.hair_brdf(s.mats, s.v, s.nrm, s.tng)
    B = h64.Brdf(s.brdf)
    s.f64 = types.SimpleNamespace()
    s.f64.f, s.f64.pdf = h64.eval_pdf(B, s.wo, s.wi)
    s.f64.q = h64.lobe_pdfs(B, s.wo)
    s.f64.dir, s.f64.lobe = h64.sample(B, s.wo, s.rn)
    with np.errstate(invalid="ignore"):
        s.wi_s = np.ascontiguousarray(s.f64.dir, F)  # the second call's `incoming`
    s.f64.f_s, s.f64.pdf_s = h64.eval_pdf(B, s.wo, s.wi_s)
    u00, _ = h64.demux_float(s.rn[:, 0])
    with np.errstate(invalid="ignore"):
        s.aside = np.any(np.abs(u00[:, None] - h64.boundaries(s.f64.q)) <= U_ASIDE, axis=1)
    s.orc = types.SimpleNamespace(f=oracle.hair_eval(s.brdf, s.wo, s.wi), pdf=oracle.hair_pdf(s.brdf, s.wo, s.wi),
                                  q=oracle.hair_lobe_pdfs(s.brdf, s.wo), dir=oracle.hair_sample(s.brdf, s.wo, s.rn),
                                  f_s=oracle.hair_eval(s.brdf, s.wo, s.wi_s), pdf_s=oracle.hair_pdf(s.brdf, s.wo, s.wi_s))
    s.e_ref = _errors(s, s.orc.f, s.orc.pdf, s.orc.f_s, s.orc.pdf_s, s.orc.q, s.orc.dir) if name != "z" else None
    s.mat_rows = None
    _CACHE[name] = s
    return s


def _errors(s, f, pdf, f_s, pdf_s, q, direction):
    """(median, p99) against float64 for each of QUANTITIES."""
    keep = ~s.aside
    return {"f": _stat(_row_err(f, s.f64.f)), "pdf": _stat(_row_err(pdf, s.f64.pdf)), "f@s": _stat(_row_err(f_s, s.f64.f_s)),
            "pdf@s": _stat(_row_err(pdf_s, s.f64.pdf_s)), "lobe pdfs": _stat(_row_err(q, s.f64.q)),
            "direction": _stat(_row_err(direction[keep], s.f64.dir[keep], absolute=True))}


def _all_finite(*arrays):
    return all(np.isfinite(a).all() for a in arrays)


# ---------------------------------------------------------------------------------------------------------------
# CPU: the restatement is the oracle's function; the strata are what they claim to be
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(STRATA) + ["y"])
def test_float64_restatement_is_the_oracles_function(oracle, name):
    s = _stratum(name, oracle)
    o, r = s.orc, s.f64
    assert _all_finite(o.f, o.pdf, o.q, o.dir, o.f_s, o.pdf_s), "the oracle is not finite on every row"
    assert _all_finite(r.f, r.pdf, r.q, r.dir, r.f_s, r.pdf_s), "the restatement is not finite on every row"
    assert s.aside.mean() <= ASIDE_CAP, f"{s.aside.sum()} rows within {U_ASIDE} of a lobe boundary"
    print(f"stratum {name}: oracle against float64 (median, p99): " + "  ".join(f"{q} {a:.2e} {b:.2e}" for q, (a, b) in s.e_ref.items()))
    if name == "y":
        return  # float arithmetic has no digits of cos_theta_o left here: finite on both sides is what the CPU can ask
    bar = {"f": CPU_MEDIAN, "pdf": CPU_MEDIAN, "f@s": CPU_MEDIAN_AT_SAMPLE.get(name, CPU_MEDIAN), "pdf@s": CPU_MEDIAN_AT_SAMPLE.get(name, CPU_MEDIAN)}
    for q in bar:
        assert s.e_ref[q][0] < bar[q], (q, s.e_ref[q])
    for api in [oc.Ref()] if oc.have_ref() else []:  # the real reference, where it is built
        f, pdf, d = api.hair_eval(s.brdf, s.wo, s.wi), api.hair_pdf(s.brdf, s.wo, s.wi), api.hair_sample(s.brdf, s.wo, s.rn)
        f_s, pdf_s = api.hair_eval(s.brdf, s.wo, s.wi_s), api.hair_pdf(s.brdf, s.wo, s.wi_s)
        assert _all_finite(f, pdf, d, f_s, pdf_s)
        for q, e in (("f", _row_err(f, r.f)), ("pdf", _row_err(pdf, r.pdf)), ("f@s", _row_err(f_s, r.f_s)), ("pdf@s", _row_err(pdf_s, r.pdf_s))):
            assert np.median(e) < bar[q], ("reference", q, _stat(e))
        assert np.median(_row_err(d[~s.aside], r.dir[~s.aside], absolute=True)) < 1e-5


def test_strata_reach_the_edges_they_name(oracle):
    le = lambda s: np.asarray(s.brdf[:, 6:10]) <= F(0.1)  # noqa: E731
    c = _stratum("c", oracle)
    for p in range(3):  # each side of each lobe's v <= 0.1 switch gets at least a third of that lobe's rows
        side = le(c)[c.lobe == p, p]
        assert 1 / 3 <= side.mean() <= 2 / 3, (p, side.mean())
    d = _stratum("d", oracle)
    B = h64.Brdf(d.brdf)
    _, cos_o, _ = h64._outgoing(B, d.wo)
    sin_i = B.to_local(d.wi)[:, 0]
    a = np.sqrt(1 - sin_i ** 2) * cos_o / B.v[np.arange(d.n), d.lobe]
    assert (np.abs(a / 12 - 1) <= 0.1).mean() >= 0.5 and (a > 12).mean() >= 0.25 and (a <= 12).mean() >= 0.25
    assert le(d)[np.arange(d.n), d.lobe].all()  # ... in the form of mp that calls log_i0
    e = _stratum("e", oracle)
    B = h64.Brdf(e.brdf)
    sin_o, cos_o, phi_o = h64._outgoing(B, e.wo)
    _, gamma_t = h64.transmittance(B, sin_o, cos_o)
    li = B.to_local(e.wi)
    dphi = np.arctan2(li[:, 2], li[:, 1]) - phi_o - h64.phi_fn(e.lobe, B.gamma_o, gamma_t)
    wrapped = np.abs((dphi + np.pi) % (2 * np.pi) - np.pi)  # |dphi| in [0, pi]
    assert (np.pi - wrapped <= 1e-3).all()
    for p in range(3):
        assert (e.lobe == p).mean() >= 0.33
    g, y = _stratum("g", oracle), _stratum("y", oracle)
    for t in (g, y):
        sin_o = h64._outgoing(h64.Brdf(t.brdf), t.wo)[0]
        assert ((sin_o > 0) == (t.sg > 0)).all()
        for a in (0, 1e-3):
            for sg in (-1, 1):
                assert ((t.ang == a) & (t.sg == sg)).sum() == t.n // 4
        if t is g:
            dot = np.sum(g.wo.astype(np.float64) * g.tng, axis=1)
            assert np.array_equal(g.wo[g.ang == 0], (g.sg[:, None] * g.tng)[g.ang == 0].astype(F))  # the tangent itself
            assert (np.abs(np.arccos(np.clip(np.abs(dot[g.ang > 0]), 0, 1)) - 1e-3) < 1e-4).all()  # 1e-3 rad from it
        else:
            assert (np.abs(sin_o[y.ang == 0]) > 1 - 1e-10).all()  # along the x axis of the frame
            assert (np.abs(1 - np.abs(sin_o[y.ang > 0]) - 5e-7) < 1e-7).all()  # 1e-3 rad from it: cos_theta_o = 1e-3
    h = _stratum("h", oracle)
    assert set(np.unique(h.brdf[:, 5])) >= {F(-1), F(1), F(0)}
    i = _stratum("i", oracle)
    assert (i.brdf[0::2, 0:3] == 0).all() and (i.brdf[1::2, 0:3] > 3).all()
    assert len(set(map(tuple, np.column_stack([i.brdf[:, 0] > 0, i.brdf[:, 3], i.brdf[:, 4]]).tolist()))) == 12
    j = _stratum("j", oracle)
    u00, u01 = h64.demux_float(j.rn[:, 0])
    u10, _ = h64.demux_float(j.rn[:, 1])
    assert (u10 == 0).sum() >= 400 and (u01 == 0).sum() >= 300 and (j.rn == BELOW1).any() and (j.rn == 0).any()
    c = h64.boundaries(j.f64.q)
    k = j.placed
    gap = np.abs(u00[k] - c[k, (k // 2) % 3])
    assert len(k) >= 2000 and (gap >= 1e-3).all() and (gap <= 1e-3 + 1 / 4096).all()
    for lobe in range(4):  # every lobe is sampled
        assert (j.f64.lobe == lobe).sum() > 50
    z = _stratum("z", oracle)
    assert (~np.isfinite(z.orc.f)).any() and (~np.isfinite(z.orc.pdf)).any()


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
_DEV = {}


def _mat_rows(s, yh):
    if s.mat_rows is None:
        s.mat_rows = yh.hair_material_rows(s.mats)
    return s.mat_rows


def _device(ctx, yh, s, combo):
    """The two calls of a stratum in one combination: at `incoming` and at the restatement's sampled direction."""
    key = (s.name, combo)
    if key not in _DEV:
        _, form, exact = next(c for c in COMBOS if c[0] == combo)
        m = _mat_rows(s, yh)
        _DEV[key] = (ctx.hair_shade(form, exact, m, s.v, s.nrm, s.tng, s.wo, s.wi, s.rn),
                     ctx.hair_shade(form, exact, m, s.v, s.nrm, s.tng, s.wo, s.wi_s, s.rn))
    return _DEV[key]


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STRATA) + ["y", "z"])
def test_quad_and_lane_forms_agree_bit_for_bit(ctx, yh, oracle, name):
    s = _stratum(name, oracle)
    for q, l in zip(_device(ctx, yh, s, "quad-fast"), _device(ctx, yh, s, "lane-fast")):
        differ = np.flatnonzero((q.view(np.uint32) != l.view(np.uint32)).any(axis=1))
        assert len(differ) == 0, f"{len(differ)} rows differ between the forms, first {differ[:5]}: {q[differ[:2]]} {l[differ[:2]]}"


@pytest.mark.gpu
@pytest.mark.parametrize("combo", [c[0] for c in COMBOS])
def test_stated_bars_hold_on_todays_domain(ctx, yh, oracle, combo):
    s = _stratum("a", oracle)
    assert s.aside.mean() <= ASIDE_CAP  # on the inputs, before the device is looked at
    _, form, exact = next(c for c in COMBOS if c[0] == combo)
    out = _device(ctx, yh, s, combo)[0]
    wi_o = np.ascontiguousarray(s.orc.dir, F)  # the oracle's sampled direction
    at_s = ctx.hair_shade(form, exact, _mat_rows(s, yh), s.v, s.nrm, s.tng, s.wo, wi_o, s.rn)
    of_s, op_s = oracle.hair_eval(s.brdf, s.wo, wi_o), oracle.hair_pdf(s.brdf, s.wo, wi_o)
    assert _all_finite(out, at_s, of_s, op_s)
    fig = {"f": np.max(_rel(out[:, 0:3], s.orc.f, 1e-7)), "pdf": np.max(_rel(out[:, 3], s.orc.pdf, 1e-7)),
           "f@s": np.max(_rel(at_s[:, 0:3], of_s, 1e-7)), "pdf@s": np.max(_rel(at_s[:, 3], op_s, 1e-7)),
           "direction": np.max(np.abs(out[:, 4:7] - s.orc.dir)[~s.aside]), "lobe pdfs": np.max(_rel(out[:, 11:15], s.orc.q, 1e-7))}
    print(f"stratum a {combo}: largest difference from the oracle: " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items())
          + f"  (set aside {int(s.aside.sum())} rows)")
    for k in ("f", "pdf", "f@s", "pdf@s", "lobe pdfs"):
        assert fig[k] <= REL_BSDF, (k, fig[k])
    assert fig["direction"] <= ABS_DIR


@pytest.mark.gpu
@pytest.mark.parametrize("combo", [c[0] for c in COMBOS])
@pytest.mark.parametrize("name", list(STRATA) + ["y"])
def test_error_against_float64_is_the_references_own(ctx, yh, oracle, name, combo):
    s = _stratum(name, oracle)
    assert s.aside.mean() <= ASIDE_CAP  # on the inputs, before the device is looked at
    out, at_s = _device(ctx, yh, s, combo)
    assert _all_finite(out, at_s), f"{(~np.isfinite(out)).any(axis=1).sum()} rows with a non-finite value"
    e_dev = _errors(s, out[:, 0:3], out[:, 3], at_s[:, 0:3], at_s[:, 3], out[:, 11:15], out[:, 4:7])
    k = K_BAR[next(c for c in COMBOS if c[0] == combo)[2]]
    print(f"stratum {name} {combo} (median, p99 | reference's):  "
          + "  ".join(f"{q} {e_dev[q][0]:.2e} {e_dev[q][1]:.2e} | {s.e_ref[q][0]:.2e} {s.e_ref[q][1]:.2e}" for q in QUANTITIES))
    if name == "a":
        return  # stratum a is held to the stated bars (test_stated_bars_hold_on_todays_domain); its figures are printed for the table
    # y: the median alone. Its p99 is the oracle's O(1) to O(1e3) error where cos_theta_o has no digits left, and bounds nothing
    stats = (0,) if name == "y" else (0, 1)
    bad = [(q, i, e_dev[q][i], s.e_ref[q][i]) for q in QUANTITIES for i in stats if not e_dev[q][i] <= k * max(s.e_ref[q][i], E_FLOOR)]
    assert not bad, f"(quantity, 0 median / 1 p99, device, reference) beyond {k} x max(reference, {E_FLOOR}): {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("combo", [c[0] for c in COMBOS])
def test_non_finite_values_are_the_oracles(ctx, yh, oracle, combo):
    s = _stratum("z", oracle)
    out, _ = _device(ctx, yh, s, combo)
    o = s.orc
    wi_o = np.ascontiguousarray(o.dir, F)
    # columns 7-10: the device evaluates at ITS sampled direction, the oracle at the oracle's. On z the sampled direction is NaN
    # on both sides (asserted through columns 4-6), so both evaluations are NaN and the masks can be compared.
    with np.errstate(invalid="ignore"):
        want = np.column_stack([o.f, o.pdf, o.dir, oracle.hair_eval(s.brdf, s.wo, wi_o), oracle.hair_pdf(s.brdf, s.wo, wi_o), o.q])
    bad = np.flatnonzero((np.isfinite(out) != np.isfinite(want)).any(axis=1))
    print(f"stratum z {combo}: {int((~np.isfinite(want)).any(axis=1).sum())} of {s.n} rows non-finite in the oracle, {len(bad)} rows with another mask")
    assert len(bad) == 0, (bad[:5], out[bad[:2]], want[bad[:2]])


@pytest.mark.gpu
def test_host_material_row_is_the_row_under_test(ctx, yh, oracle):
    s = _stratum("a", oracle)
    out = _device(ctx, yh, s, "quad-fast")[0]
    f, pdf = ctx.hair_eval(s.brdf, s.wo, s.wi), ctx.hair_pdf(s.brdf, s.wo, s.wi)  # material constants derived on the device
    differ = int(((out[:, 0:3] != f).any(axis=1) | (out[:, 3] != pdf)).sum())
    print(f"rows that differ at all between the host's material row and the device-derived one: {differ} of {s.n}; largest "
          f"{np.max(_rel(out[:, 0:3], f, 1e-7)):.2e} (f) {np.max(_rel(out[:, 3], pdf, 1e-7)):.2e} (pdf)")
    assert np.max(_rel(out[:, 0:3], f, 1e-7)) <= REL_BSDF and np.max(_rel(out[:, 3], pdf, 1e-7)) <= REL_BSDF
    assert np.max(_rel(f, s.orc.f, 1e-7)) <= REL_BSDF and np.max(_rel(pdf, s.orc.pdf, 1e-7)) <= REL_BSDF  # each against the oracle
    assert np.max(_rel(out[:, 0:3], s.orc.f, 1e-7)) <= REL_BSDF and np.max(_rel(out[:, 3], s.orc.pdf, 1e-7)) <= REL_BSDF


@pytest.mark.gpu
@pytest.mark.parametrize("combo", [c[0] for c in COMBOS])
def test_batch_shape_does_not_change_a_row(ctx, yh, oracle, combo):
    s = _stratum("a", oracle)
    _, form, exact = next(c for c in COMBOS if c[0] == combo)
    whole = _device(ctx, yh, s, combo)[0]
    for n in (1, 3, 4097):  # one row, a ragged quad, a ragged last block
        part = ctx.hair_shade(form, exact, s.mats[:n], s.v[:n], s.nrm[:n], s.tng[:n], s.wo[:n], s.wi[:n], s.rn[:n])
        assert _same_bits(part, whole[:n]), n


@pytest.mark.gpu
def test_refusals(ctx, yh, oracle):
    s = _stratum("a", oracle)
    n = 8
    m = yh.hair_material_rows(s.mats[:n])
    out = np.full((n, yh.HAIR_SHADE_FLOATS), 7, F)
    rows = [np.ascontiguousarray(x[:n]) for x in (s.v, s.nrm, s.tng, s.wo, s.wi, s.rn)]
    ptrs = [yh.fptr(x) for x in rows] + [yh.fptr(out)]
    call = ctx.lib.yh_hair_shade_batch
    assert call(ctx.h, 0, 0, n, m, *ptrs) == yh.YH_OK and not (out == 7).any()
    assert call(ctx.h, 1, 1, n, m, *ptrs) == yh.YH_E_INVALID  # the exact arithmetic has the quad form alone
    for form, exact in ((2, 0), (-1, 0), (0, 2), (0, -1)):
        assert call(ctx.h, form, exact, n, m, *ptrs) == yh.YH_E_INVALID
    assert call(ctx.h, 0, 0, -1, m, *ptrs) == yh.YH_E_INVALID
    assert call(None, 0, 0, n, m, *ptrs) == yh.YH_E_INVALID
    assert call(ctx.h, 0, 0, n, None, *ptrs) == yh.YH_E_INVALID
    for k in range(len(ptrs)):
        assert call(ctx.h, 0, 0, n, m, *[None if i == k else p for i, p in enumerate(ptrs)]) == yh.YH_E_INVALID
    for form, exact in ((0, 0), (1, 0), (0, 1)):
        assert call(ctx.h, form, exact, 0, None, *[None] * len(ptrs)) == yh.YH_OK
