"""The non-hair surface lobes and their mixture on the device (yh_surface_lobe_batch, yh_surface_bsdf_batch: csrc/dev_surface.h as the
sample loops call it) at the edges of their domain: grazing angles, a zero halfway vector, the specular peak at the smallest
roughness, total internal reflection and the ior_is_one switch, degenerate metals, the random numbers' edges and the mixture's
lobe-selection boundaries.

References: the oracle (float arithmetic, the reference's operations; held to the real reference bit for bit on these strata by
tests/test_oracle_vs_ref.py and tests/test_oracle_golden.py: lobes_edges.npz) and tests/surface_f64.py, the same formulas in float64.
Strata (tests/surface_cases.py; ROWS rows each, fixed seeds), each through all nine lobes and through the mixture: a the existing
goldens' domain, b grazing, c special incoming directions, d roughness and the specular peak, e ior and the critical angle,
f metals, g the random numbers' edges (the mixture: rnl on each cumulative lobe pdf of the oracle and its two float neighbours).

Bars (none of them taken from what the device gives):
  2  the mixture's 22 leading floats (lobe weights, roughness, opacity, lobe pdfs) bit for bit on every stratum; on g the device's
     sampled direction is the oracle's (within ABS_DIR) on every row, nothing set aside: it picked the oracle's lobe;
  3  stratum a against the oracle: f and pdf within REL_BSDF (1e-4, floor 1e-7), the direction within ABS_DIR (5e-5);
  4  strata b-g against float64: median and p99 of the relative error (floor 1e-7; per row the largest over the components) of f and
     pdf and of the absolute error of the direction at most K = 2 x max(the oracle's same statistic on the same rows, 1e-6);
  5  the non-finite mask equals the oracle's on every row of every stratum, every lobe and the mixture;
  6  set aside from the direction comparison only: rows of the two refraction lobes (and of the mixture where rnl selects
     refraction) whose rnl lies within 1e-5 of the float64 Fresnel value that decides reflect-or-refract; decided on the inputs, at
     most 2e-4 of a stratum's rows, asserted on the CPU too. Statistics run over the rows whose float64 and oracle values are finite.
The CPU test holds the restatement to the oracle: on every stratum, for every lobe and the mixture, the median relative difference
of f and pdf below 1e-5.

What the bars catch, tried once on copies of the library whose kernels were compiled from a dev_surface.h with one one-token error each:
  1 / ior and ior swapped in sample_microfacet_refraction's refract: bar 2 on stratum g (the mixture's direction is not the oracle's), bar 3
    (the refraction lobe's direction, 1.15 against 5e-5) and bar 4 on every stratum b-g (the refraction lobe's direction: p99 0.86 to 0.99
    against 3e-7 to 2e-5; the mixture's on b, c, d, e and g);
  (sample_phasefunction's 1e-3f written 1e-2f and iclamp((int)(rl * 3), 0, 2) written with 0, 1 are volume code: caught by
  tests/test_volume_unit.py, no surface bar.)

MEASURED (2026-10-19, AMD Instinct MI355X, gfx950; also profiles/surface_volume_unit/errors.txt): no assertion fails.
median and p99 per stratum of the error against float64 (relative with a floor of 1e-7, per row the largest over the components;
direction: absolute), 8192 rows each, per lobe (yh_surface_lobe_batch) and for the mixture (yh_surface_bsdf_batch). reference = the oracle.
                              f                   pdf                 direction
  a
    diffuse         reference 0.00e+00 2.51e-07   0.00e+00 2.51e-07   1.70e-08 1.88e-07
                    device    0.00e+00 2.51e-07   0.00e+00 2.51e-07   1.65e-08 1.88e-07
    specular        reference 0.00e+00 2.00e-04   0.00e+00 2.74e-04   1.29e-08 2.67e-07
                    device    0.00e+00 2.00e-04   0.00e+00 2.74e-04   1.31e-08 2.74e-07
    metal           reference 0.00e+00 3.05e-04   0.00e+00 2.74e-04   1.29e-08 2.67e-07
                    device    0.00e+00 3.05e-04   0.00e+00 2.74e-04   1.31e-08 2.74e-07
    transmission    reference 0.00e+00 2.72e-04   0.00e+00 2.72e-04   1.51e-08 2.79e-07
                    device    0.00e+00 2.72e-04   0.00e+00 2.72e-04   1.57e-08 2.84e-07
    refraction      reference 7.55e-08 5.07e-04   1.83e-07 5.68e-04   4.03e-08 4.04e-07
                    device    7.55e-08 5.07e-04   1.83e-07 5.68e-04   4.03e-08 4.14e-07
    d-specular      reference 0.00e+00 9.77e-05   0.00e+00 0.00e+00   8.52e-09 1.23e-07
                    device    0.00e+00 9.77e-05   0.00e+00 0.00e+00   8.52e-09 1.23e-07
    d-metal         reference 0.00e+00 2.97e-06   0.00e+00 0.00e+00   8.52e-09 1.23e-07
                    device    0.00e+00 2.97e-06   0.00e+00 0.00e+00   8.52e-09 1.23e-07
    d-transmission  reference 0.00e+00 0.00e+00   0.00e+00 0.00e+00   0.00e+00 0.00e+00
                    device    0.00e+00 0.00e+00   0.00e+00 0.00e+00   0.00e+00 0.00e+00
    d-refraction    reference 0.00e+00 6.49e-07   0.00e+00 6.53e-07   1.76e-08 1.27e-07
                    device    0.00e+00 6.49e-07   0.00e+00 6.53e-07   1.76e-08 1.27e-07
    mixture         reference 0.00e+00 3.59e-04   0.00e+00 2.38e-04   1.26e-08 2.50e-07
                    device    0.00e+00 3.59e-04   0.00e+00 2.38e-04   1.28e-08 2.50e-07
  b
    diffuse         reference 0.00e+00 1.30e-08   0.00e+00 1.30e-08   0.00e+00 1.81e-07
                    device    0.00e+00 1.30e-08   0.00e+00 1.30e-08   0.00e+00 1.81e-07
    specular        reference 0.00e+00 3.86e-07   0.00e+00 2.21e-07   0.00e+00 2.08e-07
                    device    0.00e+00 3.86e-07   0.00e+00 2.21e-07   0.00e+00 2.28e-07
    metal           reference 0.00e+00 1.12e-06   0.00e+00 2.21e-07   0.00e+00 2.08e-07
                    device    0.00e+00 1.12e-06   0.00e+00 2.21e-07   0.00e+00 2.28e-07
    transmission    reference 0.00e+00 2.46e-07   0.00e+00 2.33e-07   0.00e+00 2.08e-07
                    device    0.00e+00 2.46e-07   0.00e+00 2.33e-07   0.00e+00 2.28e-07
    refraction      reference 0.00e+00 4.21e-06   3.70e-11 1.64e-05   2.85e-08 1.91e-05
                    device    0.00e+00 4.21e-06   3.70e-11 1.64e-05   2.87e-08 1.91e-05
    d-specular      reference 0.00e+00 1.00e+07   0.00e+00 0.00e+00   0.00e+00 0.00e+00
                    device    0.00e+00 1.00e+07   0.00e+00 0.00e+00   0.00e+00 0.00e+00
    d-metal         reference 0.00e+00 1.33e-07   0.00e+00 0.00e+00   0.00e+00 0.00e+00
                    device    0.00e+00 1.33e-07   0.00e+00 0.00e+00   0.00e+00 0.00e+00
    d-transmission  reference 0.00e+00 0.00e+00   0.00e+00 0.00e+00   0.00e+00 0.00e+00
                    device    0.00e+00 0.00e+00   0.00e+00 0.00e+00   0.00e+00 0.00e+00
    d-refraction    reference 0.00e+00 2.30e-01   0.00e+00 2.30e-01   0.00e+00 0.00e+00
                    device    0.00e+00 2.30e-01   0.00e+00 2.30e-01   0.00e+00 0.00e+00
    mixture         reference 0.00e+00 3.64e-01   0.00e+00 3.25e-07   0.00e+00 3.89e-07
                    device    0.00e+00 3.64e-01   0.00e+00 3.25e-07   0.00e+00 4.02e-07
  c
    diffuse         reference 0.00e+00 2.33e-07   0.00e+00 2.40e-07   1.24e-08 1.78e-07
                    device    0.00e+00 2.33e-07   0.00e+00 2.40e-07   1.25e-08 1.81e-07
    specular        reference 0.00e+00 8.75e-02   0.00e+00 1.13e-01   8.90e-09 2.76e-07
                    device    0.00e+00 8.75e-02   0.00e+00 1.13e-01   9.04e-09 2.84e-07
    metal           reference 0.00e+00 1.14e-01   0.00e+00 1.13e-01   8.90e-09 2.76e-07
                    device    0.00e+00 1.14e-01   0.00e+00 1.13e-01   9.04e-09 2.84e-07
    transmission    reference 0.00e+00 1.70e-01   0.00e+00 1.70e-01   1.06e-08 2.95e-07
                    device    0.00e+00 1.70e-01   0.00e+00 1.70e-01   1.06e-08 2.97e-07
    refraction      reference 3.17e-07 3.25e-01   3.57e-07 3.28e-01   3.91e-08 3.64e-07
                    device    3.17e-07 3.25e-01   3.57e-07 3.28e-01   3.94e-08 3.77e-07
    d-specular      reference 0.00e+00 8.39e-05   0.00e+00 0.00e+00   5.77e-09 1.21e-07
                    device    0.00e+00 8.39e-05   0.00e+00 0.00e+00   5.77e-09 1.21e-07
    d-metal         reference 0.00e+00 2.69e-06   0.00e+00 0.00e+00   5.77e-09 1.21e-07
                    device    0.00e+00 2.69e-06   0.00e+00 0.00e+00   5.77e-09 1.21e-07
    d-transmission  reference 0.00e+00 0.00e+00   0.00e+00 0.00e+00   0.00e+00 0.00e+00
                    device    0.00e+00 0.00e+00   0.00e+00 0.00e+00   0.00e+00 0.00e+00
    d-refraction    reference 0.00e+00 6.02e-07   0.00e+00 6.10e-07   1.76e-08 1.37e-07
                    device    0.00e+00 6.02e-07   0.00e+00 6.10e-07   1.76e-08 1.37e-07
    mixture         reference 0.00e+00 2.20e-01   0.00e+00 1.83e-01   1.04e-08 2.52e-07
                    device    0.00e+00 2.20e-01   0.00e+00 1.83e-01   1.05e-08 2.55e-07
  d
    diffuse         reference 0.00e+00 2.06e-07   0.00e+00 2.06e-07   0.00e+00 1.79e-07
                    device    0.00e+00 2.06e-07   0.00e+00 2.06e-07   0.00e+00 1.81e-07
    specular        reference 0.00e+00 6.83e-01   0.00e+00 8.32e-01   0.00e+00 2.61e-07
                    device    0.00e+00 6.83e-01   0.00e+00 8.32e-01   0.00e+00 2.68e-07
    metal           reference 0.00e+00 8.32e-01   0.00e+00 8.32e-01   0.00e+00 2.61e-07
                    device    0.00e+00 8.32e-01   0.00e+00 8.32e-01   0.00e+00 2.68e-07
    transmission    reference 0.00e+00 9.54e-01   0.00e+00 9.54e-01   0.00e+00 2.92e-07
                    device    0.00e+00 9.54e-01   0.00e+00 9.54e-01   0.00e+00 2.94e-07
    refraction      reference 6.20e-08 9.94e-01   8.00e-08 9.94e-01   3.81e-08 3.71e-07
                    device    6.20e-08 9.94e-01   8.00e-08 9.94e-01   3.84e-08 3.58e-07
    d-specular      reference 0.00e+00 7.17e-05   0.00e+00 0.00e+00   0.00e+00 1.19e-07
                    device    0.00e+00 7.17e-05   0.00e+00 0.00e+00   0.00e+00 1.19e-07
    d-metal         reference 0.00e+00 3.65e-06   0.00e+00 0.00e+00   0.00e+00 1.19e-07
                    device    0.00e+00 3.65e-06   0.00e+00 0.00e+00   0.00e+00 1.19e-07
    d-transmission  reference 0.00e+00 0.00e+00   0.00e+00 0.00e+00   0.00e+00 0.00e+00
                    device    0.00e+00 0.00e+00   0.00e+00 0.00e+00   0.00e+00 0.00e+00
    d-refraction    reference 0.00e+00 5.84e-07   0.00e+00 5.85e-07   1.79e-08 1.29e-07
                    device    0.00e+00 5.84e-07   0.00e+00 5.85e-07   1.79e-08 1.29e-07
    mixture         reference 0.00e+00 3.53e-01   0.00e+00 3.42e-01   1.52e-08 2.53e-07
                    device    0.00e+00 3.53e-01   0.00e+00 3.42e-01   1.52e-08 2.65e-07
  e
    diffuse         reference 0.00e+00 1.93e-07   0.00e+00 1.94e-07   0.00e+00 1.76e-07
                    device    0.00e+00 1.93e-07   0.00e+00 1.94e-07   0.00e+00 1.77e-07
    specular        reference 0.00e+00 3.58e-05   0.00e+00 1.21e-06   0.00e+00 2.39e-07
                    device    0.00e+00 3.58e-05   0.00e+00 1.21e-06   0.00e+00 2.56e-07
    metal           reference 0.00e+00 9.67e-06   0.00e+00 1.21e-06   0.00e+00 2.39e-07
                    device    0.00e+00 9.67e-06   0.00e+00 1.21e-06   0.00e+00 2.56e-07
    transmission    reference 0.00e+00 3.68e-06   0.00e+00 1.62e-06   0.00e+00 2.69e-07
                    device    0.00e+00 3.68e-06   0.00e+00 1.62e-06   0.00e+00 2.74e-07
    refraction      reference 0.00e+00 7.76e-05   4.85e-09 6.88e-05   9.39e-08 1.21e-05
                    device    0.00e+00 7.76e-05   4.85e-09 6.88e-05   9.60e-08 1.21e-05
    d-specular      reference 0.00e+00 3.08e-04   0.00e+00 0.00e+00   0.00e+00 1.04e-07
                    device    0.00e+00 3.08e-04   0.00e+00 0.00e+00   0.00e+00 1.04e-07
    d-metal         reference 0.00e+00 5.95e-07   0.00e+00 0.00e+00   0.00e+00 1.04e-07
                    device    0.00e+00 5.95e-07   0.00e+00 0.00e+00   0.00e+00 1.04e-07
    d-transmission  reference 0.00e+00 0.00e+00   0.00e+00 0.00e+00   0.00e+00 0.00e+00
                    device    0.00e+00 0.00e+00   0.00e+00 0.00e+00   0.00e+00 0.00e+00
    d-refraction    reference 0.00e+00 2.09e-03   0.00e+00 2.09e-03   4.92e-10 6.82e-06
                    device    0.00e+00 2.09e-03   0.00e+00 2.09e-03   4.92e-10 6.82e-06
    mixture         reference 0.00e+00 9.68e-04   0.00e+00 6.49e-04   3.21e-08 6.51e-06
                    device    0.00e+00 9.68e-04   0.00e+00 6.49e-04   3.21e-08 6.51e-06
  f
    diffuse         reference 0.00e+00 3.81e-07   0.00e+00 3.84e-07   0.00e+00 1.84e-07
                    device    0.00e+00 3.81e-07   0.00e+00 3.84e-07   0.00e+00 1.83e-07
    specular        reference 0.00e+00 2.11e-01   0.00e+00 2.17e-01   0.00e+00 2.78e-07
                    device    0.00e+00 2.11e-01   0.00e+00 2.17e-01   0.00e+00 2.89e-07
    metal           reference 0.00e+00 1.11e+01   0.00e+00 2.17e-01   0.00e+00 2.78e-07
                    device    0.00e+00 1.11e+01   0.00e+00 2.17e-01   0.00e+00 2.89e-07
    transmission    reference 0.00e+00 9.32e-05   0.00e+00 9.33e-05   0.00e+00 2.95e-07
                    device    0.00e+00 9.32e-05   0.00e+00 9.33e-05   0.00e+00 3.05e-07
    refraction      reference 4.76e-07 4.36e-01   6.42e-07 4.84e-01   4.05e-08 3.41e-07
                    device    4.76e-07 4.36e-01   6.42e-07 4.84e-01   4.05e-08 3.53e-07
    d-specular      reference 0.00e+00 1.07e-04   0.00e+00 0.00e+00   0.00e+00 1.21e-07
                    device    0.00e+00 1.07e-04   0.00e+00 0.00e+00   0.00e+00 1.21e-07
    d-metal         reference 0.00e+00 3.09e-01   0.00e+00 0.00e+00   0.00e+00 1.21e-07
                    device    0.00e+00 3.09e-01   0.00e+00 0.00e+00   0.00e+00 1.21e-07
    d-transmission  reference 0.00e+00 0.00e+00   0.00e+00 0.00e+00   0.00e+00 0.00e+00
                    device    0.00e+00 0.00e+00   0.00e+00 0.00e+00   0.00e+00 0.00e+00
    d-refraction    reference 0.00e+00 6.61e-07   0.00e+00 6.68e-07   1.86e-08 1.38e-07
                    device    0.00e+00 6.61e-07   0.00e+00 6.68e-07   1.86e-08 1.38e-07
    mixture         reference 0.00e+00 5.91e+00   0.00e+00 2.26e-02   0.00e+00 2.41e-07
                    device    0.00e+00 5.91e+00   0.00e+00 2.26e-02   0.00e+00 2.53e-07
  g
    diffuse         reference 0.00e+00 4.81e-07   0.00e+00 4.79e-07   7.36e-08 1.01e-04
                    device    0.00e+00 4.81e-07   0.00e+00 4.79e-07   7.36e-08 1.01e-04
    specular        reference 0.00e+00 3.36e-05   0.00e+00 3.39e-05   7.71e-08 2.98e-07
                    device    0.00e+00 3.36e-05   0.00e+00 3.39e-05   8.14e-08 3.09e-07
    metal           reference 0.00e+00 6.68e-05   0.00e+00 3.39e-05   7.71e-08 2.98e-07
                    device    0.00e+00 6.68e-05   0.00e+00 3.39e-05   8.14e-08 3.09e-07
    transmission    reference 2.57e-10 3.85e-05   7.23e-11 3.76e-05   8.98e-08 3.14e-07
                    device    2.57e-10 3.85e-05   7.23e-11 3.76e-05   9.35e-08 3.21e-07
    refraction      reference 6.53e-08 3.39e-05   1.23e-07 3.53e-05   4.68e-08 2.54e-07
                    device    6.53e-08 3.39e-05   1.23e-07 3.53e-05   4.75e-08 2.62e-07
    d-specular      reference 0.00e+00 3.55e-07   0.00e+00 0.00e+00   4.24e-08 1.44e-07
                    device    0.00e+00 3.55e-07   0.00e+00 0.00e+00   4.24e-08 1.44e-07
    d-metal         reference 0.00e+00 2.62e-05   0.00e+00 0.00e+00   4.24e-08 1.44e-07
                    device    0.00e+00 2.62e-05   0.00e+00 0.00e+00   4.24e-08 1.44e-07
    d-transmission  reference 0.00e+00 0.00e+00   0.00e+00 0.00e+00   0.00e+00 0.00e+00
                    device    0.00e+00 0.00e+00   0.00e+00 0.00e+00   0.00e+00 0.00e+00
    d-refraction    reference 4.34e-08 3.55e-07   3.06e-08 3.55e-07   3.49e-08 1.20e-07
                    device    4.34e-08 3.55e-07   3.06e-08 3.55e-07   3.49e-08 1.20e-07
    mixture         reference 5.14e-08 4.04e-05   1.15e-08 1.73e-05   6.02e-08 1.00e-04
                    device    5.14e-08 4.04e-05   1.15e-08 1.73e-05   6.15e-08 1.00e-04
stratum g mixture: 3643 rows on a lobe boundary; largest direction difference from the oracle 4.77e-07
stratum a diffuse: largest difference from the oracle: f 0.00e+00  pdf 0.00e+00  direction 1.19e-07  (set aside 0 rows)
stratum a specular: largest difference from the oracle: f 0.00e+00  pdf 0.00e+00  direction 4.77e-07  (set aside 0 rows)
stratum a metal: largest difference from the oracle: f 0.00e+00  pdf 0.00e+00  direction 4.77e-07  (set aside 0 rows)
stratum a transmission: largest difference from the oracle: f 0.00e+00  pdf 0.00e+00  direction 5.36e-07  (set aside 0 rows)
stratum a refraction: largest difference from the oracle: f 0.00e+00  pdf 0.00e+00  direction 1.81e-06  (set aside 0 rows)
stratum a d-specular: largest difference from the oracle: f 0.00e+00  pdf 0.00e+00  direction 0.00e+00  (set aside 0 rows)
stratum a d-metal: largest difference from the oracle: f 0.00e+00  pdf 0.00e+00  direction 0.00e+00  (set aside 0 rows)
stratum a d-transmission: largest difference from the oracle: f 0.00e+00  pdf 0.00e+00  direction 0.00e+00  (set aside 0 rows)
stratum a d-refraction: largest difference from the oracle: f 0.00e+00  pdf 0.00e+00  direction 0.00e+00  (set aside 0 rows)
stratum a mixture: largest difference from the oracle: f 0.00e+00  pdf 0.00e+00  direction 4.77e-07  (set aside 0 rows)
the mixture's 22 leading floats equal the oracle's bit for bit on every stratum (a NaN for a NaN; rows with one: a 0, b 399, c 0, d 0, e 0, f 0, g 0)
The GPU tests of the module: 15 passed, 8 deselected in 1.86s
"""
import types

import numpy as np
import pytest

import surface_cases as sc
import surface_f64 as s64
from test_gpu_parity import ABS_DIR, REL_BSDF, _rel

F = np.float32
ROWS = sc.ROWS
K_BAR = 2.0
E_FLOOR = 1e-6
U_ASIDE, ASIDE_CAP = 1e-5, 2e-4
CPU_MEDIAN = 1e-5
KINDS = list(range(9))
KIND_NAMES = ("diffuse", "specular", "metal", "transmission", "refraction", "d-specular", "d-metal", "d-transmission", "d-refraction")
QUANTITIES = ("f", "pdf", "direction")
COLS = {"f": slice(0, 3), "pdf": slice(3, 4), "direction": slice(4, 7)}


def _row_err(got, want, absolute=False):
    got, want = np.asarray(got, np.float64).reshape(len(want), -1), np.asarray(want, np.float64).reshape(len(want), -1)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.max(np.abs(got - want) if absolute else _rel(got, want, 1e-7), axis=1)


def _stat(err):
    return (float(np.median(err)), float(np.percentile(err, 99))) if len(err) else (0.0, 0.0)


def _finite_rows(a):
    return np.isfinite(np.asarray(a, np.float64).reshape(len(a), -1)).all(axis=1)


def _errors(t, out):
    """(median, p99) against float64 of f, pdf and the direction (columns f[3] pdf w[3]) over the rows where float64 and the oracle are finite."""
    e = {}
    for q in QUANTITIES:
        want = t.f64[:, COLS[q]]
        keep = _finite_rows(want) & _finite_rows(t.orc[:, COLS[q]]) & (~t.aside if q == "direction" else True)
        e[q] = _stat(_row_err(out[keep][:, COLS[q]], want[keep], absolute=q == "direction"))
    return e


def _near_fresnel(rnl, fresnel):
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(rnl, np.float64) - fresnel) <= U_ASIDE


_CACHE = {}


def _stratum(name, oracle, yh):
    """Inputs and, per lobe and for the mixture, float64's values, the oracle's and the oracle's errors against float64, made once."""
    if name in _CACHE:
        return _CACHE[name]
    s = sc.inputs(name)
    s.rows = sc.material_rows(yh, s.mats)
    args = (s.nrm, s.wo, s.wi)
    p64, n64, o64 = s.params.astype(np.float64), s.nrm.astype(np.float64), s.wo.astype(np.float64)
    rough_F = s64.refraction_fresnel(p64[:, 0], p64[:, 1], n64, o64, s.rn[:, 1].astype(np.float64), s.rn[:, 2].astype(np.float64))[0]
    delta_F = s64.delta_refraction_fresnel(p64[:, 0], n64, o64)
    s.lobe = {}
    for kind in KINDS:
        t = types.SimpleNamespace(kind=kind)
        f, pdf, w = s64.lobe(kind, s.params, *args, s.rn)
        t.f64 = np.column_stack([f, pdf, w])
        t.orc = oracle.surface_lobe(kind, s.params, *args, s.rn)
        t.aside = {s64.REFRACTION: _near_fresnel(s.rn[:, 0], rough_F),
                   s64.DELTA_REFRACTION: _near_fresnel(s.rn[:, 0], delta_F) & ~s64.ior_is_one(s.params[:, 0])}.get(kind, np.zeros(s.n, bool))
        t.e_ref = _errors(t, t.orc)
        s.lobe[kind] = t
    # the mixture: on g, rnl goes onto the oracle's cumulative lobe pdfs (which do not depend on the random numbers)
    m = types.SimpleNamespace(rn=s.rn.copy())
    lead = oracle.surface_bsdf(s.rows, *args, m.rn)[:, :22]
    if name == "g":
        _, cdf = s64.selected_lobe(lead, m.rn[:, 0])
        row = np.arange(s.n)
        k = (row // 3) % 5
        for _ in range(5):  # the next lobe that has a boundary
            k = np.where(np.isnan(cdf[row, k]), (k + 1) % 5, k)
        c = cdf[row, k]
        ok = np.isfinite(c) & (c < 1)
        step = row % 3
        placed = np.where(step == 0, np.nextafter(c, F(0)), np.where(step == 1, c, np.nextafter(c, F(2)))).astype(F)
        m.rn[ok, 0] = np.minimum(placed[ok], sc.BELOW1)
        m.placed, m.boundary = ok, k
    m.orc = oracle.surface_bsdf(s.rows, *args, m.rn)
    assert np.array_equal(m.orc[:, :22].view(np.uint32), lead.view(np.uint32))
    f, pdf, w, m.selected = s64.mixture(lead, s.mats[:, 8], s.mats[:, 0:3], *args, m.rn)
    m.f64 = np.column_stack([f, pdf, w])
    delta = lead[:, 15] == 0
    mix_F = np.where(delta, s64.delta_refraction_fresnel(s.mats[:, 8].astype(np.float64), n64, o64),
                     s64.refraction_fresnel(s.mats[:, 8].astype(np.float64), lead[:, 15].astype(np.float64), n64, o64,
                                            m.rn[:, 1].astype(np.float64), m.rn[:, 2].astype(np.float64))[0])
    m.aside = (m.selected == 4) & _near_fresnel(m.rn[:, 0], mix_F) & ~(delta & s64.ior_is_one(s.mats[:, 8]))
    m.lead = lead
    mt = types.SimpleNamespace(f64=m.f64, orc=m.orc[:, 22:], aside=m.aside)
    m.view = mt
    m.e_ref = _errors(mt, mt.orc)
    s.mix = m
    _CACHE[name] = s
    return s


def _fmt(e):
    return "  ".join(f"{q} {a:.2e} {b:.2e}" for q, (a, b) in e.items())


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.STRATA))
def test_float64_restatement_is_the_oracles_function(oracle, yh, name):
    s = _stratum(name, oracle, yh)
    for t in list(s.lobe.values()) + [s.mix.view]:
        label = KIND_NAMES[t.kind] if hasattr(t, "kind") else "mixture"
        assert t.aside.mean() <= ASIDE_CAP, f"{label}: {t.aside.sum()} rows within {U_ASIDE} of the Fresnel value"
        e = s.mix.e_ref if label == "mixture" else t.e_ref
        print(f"stratum {name} {label}: oracle against float64 (median, p99): {_fmt(e)}")
        for q in ("f", "pdf"):
            assert e[q][0] < CPU_MEDIAN, (label, q, e[q])
        assert e["direction"][0] < 1e-5, (label, e["direction"])


def test_strata_reach_the_edges_they_name(oracle, yh):
    b = _stratum("b", oracle, yh)
    assert len(set(zip(b.no.tolist(), b.ni.tolist()))) == 49
    assert np.array_equal(np.sum(b.nrm * b.wo, axis=1), b.no.astype(F)) and np.array_equal(np.sum(b.nrm * b.wi, axis=1), b.ni.astype(F))
    c = _stratum("c", oracle, yh)
    assert np.array_equal(c.wi[c.case == 0], -c.wo[c.case == 0]) and np.array_equal(c.wi[c.case == 1], c.wo[c.case == 1])
    h = s64.normalize(c.wi[c.case == 2].astype(np.float64) + c.wo[c.case == 2])
    assert (np.abs(np.abs(s64.dot(h, c.nrm[c.case == 2].astype(np.float64))) - 1) < 1e-6).all()  # the mirror: halfway = +-normal
    d = _stratum("d", oracle, yh)
    assert set(np.unique(d.params[:, 1])) == set(sc.ROUGHNESS_EDGES.tolist()) and (d.case <= 2).mean() == pytest.approx(0.5, abs=0.01)
    e = _stratum("e", oracle, yh)
    assert set(np.unique(e.params[:, 0])) == set(sc.IOR_EDGES.tolist())
    one = s64.ior_is_one(e.params[:, 0])
    assert one[np.isin(np.arange(e.n) % 8, (0, 1, 4, 5))].all() and not one[np.isin(np.arange(e.n) % 8, (2, 3, 6, 7))].any()
    total = s64.delta_refraction_fresnel(e.params[:, 0].astype(np.float64), e.nrm.astype(np.float64), e.wo.astype(np.float64)) == 1
    steep = e.theta_c < 1.5  # (ior 1 +- 1e-3: the critical angle is 87 degrees and more, and the clip holds the direction short of grazing)
    assert total[steep & (e.offset > 0)].all() and not total[steep & (e.offset < 0)].any() and (steep & (np.abs(e.offset) == 1e-4)).sum() > 1000
    f = _stratum("f", oracle, yh)
    assert (f.params[f.case == 1, 2:8] == [1, 1, 1, 0, 0, 0]).all() and (f.params[f.case == 2, 5:8] == 10).all() and (f.params[f.case == 3, 2:5] == F(0.1)).all()
    g = _stratum("g", oracle, yh)
    assert len(set(map(tuple, g.rn.tolist()))) == 27 and g.mix.placed.mean() > 0.4  # (a boundary of 1 cannot be placed)
    for k in range(3):  # diffuse | specular | metal | transmission or refraction: each inner boundary is visited from both sides (the last lobe's is the sum: 1 in float, or just short of it)
        on = g.mix.placed & (g.mix.boundary == k)
        assert on.sum() > 100 and (g.mix.selected[on] == k).any() and (g.mix.selected[on] != k).any(), k
    short = g.mix.placed & (g.mix.boundary >= 3)
    print(f"stratum g: {int(short.sum())} rows whose lobe pdfs sum to less than 1 in float; {int((g.mix.selected == -1).sum())} rows select no lobe")


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
_DEV = {}


def _device(ctx, s, kind):
    key = (s.name, kind)
    if key not in _DEV:
        _DEV[key] = (ctx.surface_bsdf(s.rows, s.nrm, s.wo, s.wi, s.mix.rn) if kind == "mixture"
                     else ctx.surface_lobe(kind, s.params, s.nrm, s.wo, s.wi, s.rn))
    return _DEV[key]


def _views(ctx, s):
    """(label, reference view, device rows in the columns f[3] pdf w[3]) for the nine lobes and the mixture."""
    for kind in KINDS:
        yield KIND_NAMES[kind], s.lobe[kind], _device(ctx, s, kind)
    yield "mixture", s.mix.view, _device(ctx, s, "mixture")[:, 22:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.STRATA))
def test_mixture_set_up_and_non_finite_masks_are_the_oracles(ctx, yh, oracle, name):
    s = _stratum(name, oracle, yh)
    out = _device(ctx, s, "mixture")
    nan = np.isnan(s.mix.orc[:, :22])  # (a NaN's sign and payload are the platform's: a NaN for a NaN, every other float bit for bit)
    same = np.where(nan, np.isnan(out[:, :22]), out[:, :22].view(np.uint32) == s.mix.orc[:, :22].view(np.uint32))
    differ = np.flatnonzero(~same.all(axis=1))
    print(f"stratum {name} mixture: {int(nan.any(axis=1).sum())} rows with a NaN among the oracle's 22 leading floats")
    assert len(differ) == 0, (differ[:5], out[differ[:2], :22], s.mix.orc[differ[:2], :22])
    for label, t, dev in _views(ctx, s):
        bad = np.flatnonzero((np.isfinite(dev) != np.isfinite(t.orc)).any(axis=1))
        assert len(bad) == 0, (label, bad[:5], dev[bad[:2]], t.orc[bad[:2]])
    if name == "g":  # the lobe the oracle picks, on every row: nothing set aside
        t, dev = s.mix.view, out[:, 22:]
        keep = _finite_rows(t.orc[:, 4:7])
        worst = np.max(np.abs(dev[keep, 4:7] - t.orc[keep, 4:7]), axis=1)
        print(f"stratum g mixture: {int(s.mix.placed.sum())} rows on a lobe boundary; largest direction difference from the oracle {worst.max():.2e}")
        assert keep.mean() > 0.99 and worst.max() <= ABS_DIR, np.flatnonzero(worst > ABS_DIR)[:5]


@pytest.mark.gpu
def test_stated_bars_hold_on_todays_domain(ctx, yh, oracle):
    s = _stratum("a", oracle, yh)
    for label, t, dev in _views(ctx, s):
        assert t.aside.mean() <= ASIDE_CAP  # on the inputs, before the device is looked at
        fig = {}
        for q in QUANTITIES:
            keep = _finite_rows(t.orc[:, COLS[q]]) & (~t.aside if q == "direction" else True)
            fig[q] = float(np.max(_row_err(dev[keep][:, COLS[q]], t.orc[keep][:, COLS[q]], absolute=q == "direction")))
        print(f"stratum a {label}: largest difference from the oracle: " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items())
              + f"  (set aside {int(t.aside.sum())} rows)")
        for q in QUANTITIES:
            assert fig[q] <= (ABS_DIR if q == "direction" else REL_BSDF), (label, q, fig[q])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(sc.STRATA))
def test_error_against_float64_is_the_references_own(ctx, yh, oracle, name):
    s = _stratum(name, oracle, yh)
    bad = []
    for label, t, dev in _views(ctx, s):
        assert t.aside.mean() <= ASIDE_CAP  # on the inputs, before the device is looked at
        e_dev, e_ref = _errors(t, dev), (s.mix.e_ref if label == "mixture" else t.e_ref)
        print(f"stratum {name} {label} (median, p99 | reference's):  "
              + "  ".join(f"{q} {e_dev[q][0]:.2e} {e_dev[q][1]:.2e} | {e_ref[q][0]:.2e} {e_ref[q][1]:.2e}" for q in QUANTITIES)
              + f"  (set aside {int(t.aside.sum())} rows)")
        if name != "a":  # stratum a is held to the stated bars; its figures are printed for the table
            bad += [(label, q, i, e_dev[q][i], e_ref[q][i]) for q in QUANTITIES for i in (0, 1) if not e_dev[q][i] <= K_BAR * max(e_ref[q][i], E_FLOOR)]
    assert not bad, f"(lobe, quantity, 0 median / 1 p99, device, reference) beyond {K_BAR} x max(reference, {E_FLOOR}): {bad}"
