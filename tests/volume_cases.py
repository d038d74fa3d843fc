"""The input strata of the unit-level volume tests (tests/test_volume_unit.py) and of their golden vectors
(oracle/make_golden.py: volumes_unit.npz): ROWS rows each, fixed seeds, numpy only.

A row: mats (10: color[3], transmission, thin, trdepth, scattering[3], anisotropy), nrm, wo, wi (3 each), tex (4: the colour
texture's value[3], the emission texture's x), rn (5: rl, rd, max_distance, rx, ry).

  a  today's domain: colour ~ U(0.05, 0.95), trdepth in {0.01, 0.1, 1}, g ~ U(-0.8, 0.8), isotropic directions (7 rows of 8 with
     `incoming` on the far side of the surface), max_distance ~ 10^U(-3, 1), texture values ~ U(0.2, 1)
  b  g in {0, +-the floats either side of 1e-3f, +-1e-3f, +-2e-3, +-0.99, +-0.9999}; for |g| >= 0.99 `incoming` within 1e-3 rad of
     -outgoing (the forward peak)
  c  density per channel: a colour channel of exactly 1 (density 0: flt_max when rl picks it), colour (1, 1, 1) (is_zero), a channel
     at 0, at 1e-4, at 1e-5 (below the clamp), trdepth 1e-4, and channels 1e3 to 1e5 apart with the distance drawn from the thinnest
     so that the middle channel's expf lands between 2^-122 and 2^-152 and the densest's below everything
  d  rl in {0, 1/3 and 2/3 as floats and their neighbours either way, 1 - 2^-24} x rd in {0, 2^-24, 0.5, 1 - 2^-24}; three
     well-separated densities, no max_distance in the way
  e  max_distance with the float64 free-flight distance at 1 +- 1e-3 of it, and 1e-6, 1e30, flt_max
  f  outgoing = +-z exactly, with z = -0.0 and +0.0, 1e-4 rad off +-z, of length 0.5 and 3; ry in {0, 1 - 2^-24}, rx in
     {0, 0.25, 1 - 2^-24}
  g  the crossing: n.o and n.i in {0, +-1e-7, +-0.5}, all 25 pairs, under four materials: thin, transmission 0, both, and a closed
     transmissive one (the only one that can enter a medium)
Strata b-g have texture values of 1, so that both forms (tex 0 / 1) see the edges they name.
"""
import types

import numpy as np

import volume_f64 as v64

ROWS = 8192
F = np.float32
BELOW1 = np.nextafter(F(1), F(0))  # 1 - 2^-24
FLT_MAX = np.finfo(F).max
STRATA = "abcdefg"
SEEDS = {s: 2100 + k for k, s in enumerate(STRATA)}
G_EDGES = np.array([0] + [sg * x for x in (np.nextafter(F(1e-3), F(0)), np.nextafter(F(1e-3), F(1)), F(1e-3), F(2e-3), F(0.99), F(0.9999))
                          for sg in (1, -1)], F)
THIRD, TWO_THIRDS = F(1) / F(3), F(2) / F(3)
RL_EDGES = np.array([0, np.nextafter(THIRD, F(0)), THIRD, np.nextafter(THIRD, F(1)), np.nextafter(TWO_THIRDS, F(0)), TWO_THIRDS,
                     np.nextafter(TWO_THIRDS, F(1)), BELOW1], F)
RD_EDGES = np.array([0, 2.0 ** -24, 0.5, BELOW1], F)
DOTS = np.array([0, 1e-7, -1e-7, 0.5, -0.5])


def unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _across(nrm, wo, wi, keep=None):
    """`wi` mirrored where needed so that it lies on the other side of the surface from `wo` (rows of `keep` stay as drawn)."""
    same = np.sum(nrm * wo, axis=1) * np.sum(nrm * wi, axis=1) > 0
    if keep is not None:
        same &= ~keep
    return np.where(same[:, None], wi - 2 * np.sum(nrm * wi, axis=1, keepdims=True) * nrm, wi)


def _base(rng, n):
    mats = np.zeros((n, 10), F)
    mats[:, 0:3] = rng.uniform(0.05, 0.95, (n, 3))
    mats[:, 3] = rng.uniform(0.2, 1.0, n)
    mats[:, 5] = rng.choice([0.01, 0.1, 1.0], n)
    mats[:, 6:9] = rng.uniform(0, 1, (n, 3))
    mats[:, 9] = rng.uniform(-0.8, 0.8, n)
    nrm, wo, wi = (unit(rng.normal(size=(n, 3))) for _ in range(3))
    wi = _across(nrm, wo, wi, keep=np.arange(n) % 8 == 7)
    tex = rng.uniform(0.2, 1.0, (n, 4))
    rn = np.minimum(rng.uniform(0, 1, (n, 5)).astype(F), BELOW1)
    rn[:, 2] = 10 ** rng.uniform(-3, 1, n)
    return types.SimpleNamespace(mats=mats, nrm=nrm, wo=wo, wi=wi, tex=tex, rn=rn)


def _near(rng, axis, angle):
    """Unit vectors `angle` radians from `axis` (unit rows)."""
    side = unit(np.cross(axis, rng.normal(size=axis.shape)))
    return np.cos(angle)[:, None] * axis + np.sin(angle)[:, None] * side


def inputs(name, n=ROWS):
    rng = np.random.default_rng(SEEDS[name])
    s = _base(rng, n)
    row = np.arange(n)
    if name != "a":
        s.tex[:] = 1
    if name == "b":
        s.mats[:, 9] = G_EDGES[row % len(G_EDGES)]
        peak = np.abs(s.mats[:, 9]) >= 0.99
        s.wi = np.where(peak[:, None], _near(rng, -s.wo, rng.uniform(0, 1e-3, n)), s.wi)
    elif name == "c":
        case, ch = row % 8, (row // 8) % 3
        s.case = case
        pick = lambda k: (case == k)[:, None] & (np.arange(3)[None, :] == ch[:, None])  # noqa: E731
        col = s.mats[:, 0:3]
        col[pick(0)] = 1
        s.rn[(case == 0) & (row // 24 % 2 == 0), 0] = ((ch + 0.5) / 3)[(case == 0) & (row // 24 % 2 == 0)]  # rl picks the empty channel
        col[case == 1] = 1
        col[pick(2)], col[pick(3)], col[pick(4)] = 0, 1e-4, 1e-5
        s.mats[case == 5, 5] = 1e-4
        wide = case >= 6
        thin_c, mid_c, dense_c = ch, (ch + 1) % 3, (ch + 2) % 3
        k = np.flatnonzero(wide)
        col[k, thin_c[k]] = 1 - rng.uniform(1e-4, 2e-4, len(k))
        col[k, mid_c[k]] = rng.uniform(0.8, 0.9, len(k))
        col[k, dense_c[k]] = rng.uniform(1e-4, 2e-4, len(k))
        s.mats[:, 0:3] = col
        d = -np.log(np.clip(s.mats[k, 0:3].astype(np.float64), v64.CLAMP_LO, 1)) / s.mats[k, 5:6]
        t = rng.uniform(85, 105, len(k))  # the middle channel's exponent: expf's denormal range is 87.3 to 103.3
        s.rn[k, 0] = (thin_c[k] + 0.5) / 3
        s.rn[k, 1] = -np.expm1(-t * d[np.arange(len(k)), thin_c[k]] / d[np.arange(len(k)), mid_c[k]])
        s.rn[k, 2] = 1e30
        s.exponent = np.full(n, np.nan)
        s.exponent[k] = t
    elif name == "d":
        lo, mid, hi = rng.uniform(0.1, 0.3, n), rng.uniform(0.4, 0.6, n), rng.uniform(0.7, 0.9, n)
        order = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]])[(row // 32) % 6]
        s.mats[:, 0:3] = np.take_along_axis(np.stack([lo, mid, hi], axis=1), order, axis=1)
        s.rn[:, 0] = RL_EDGES[row % 8]
        s.rn[:, 1] = RD_EDGES[(row // 8) % 4]
        s.rn[:, 2] = 1e30
    elif name == "e":
        case = row % 8
        s.case = case
        s.wi = _across(s.nrm, s.wo, s.wi)  # every row inside
        s.rn[:, 1] = np.minimum(rng.uniform(0.02, 0.98, n).astype(F), BELOW1)
        for key in ("mats", "nrm", "wo", "wi", "tex", "rn"):
            setattr(s, key, np.ascontiguousarray(getattr(s, key), F))
        r = v64.batch(0, s.mats, s.nrm, s.wo, s.wi, s.tex, s.rn)
        side = np.where(np.isin(case, (0, 1, 7)), 1.0, -1.0)
        s.rn[:, 2] = r.unclamped / (1 + side * 1e-3)
        s.rn[case == 4, 2], s.rn[case == 5, 2], s.rn[case == 6, 2] = 1e-6, 1e30, FLT_MAX
    elif name == "f":
        case = row % 8
        s.case = case
        z = np.array([0.0, 0.0, 1.0])[None, :] * np.where(case % 2 == 0, 1.0, -1.0)[:, None]
        flat = unit(np.column_stack([rng.normal(size=(n, 2)), np.zeros(n)]))
        flat[:, 2] = np.where(case == 2, -0.0, 0.0)
        off = _near(rng, z, np.full(n, 1e-4))
        s.wo = np.where((case < 2)[:, None], z, np.where((case < 4)[:, None], flat, np.where((case < 6)[:, None], off, s.wo)))
        s.wo = s.wo.astype(F).astype(np.float64)
        s.wo[case == 6] *= 0.5
        s.wo[case == 7] *= 3
        s.wi = _across(s.nrm, s.wo, s.wi)
        e = (row // 8) % 12
        ry, rx = np.array([0, BELOW1, np.nan], F)[e % 3], np.array([0, 0.25, BELOW1, np.nan], F)[e // 3]
        s.rn[:, 4] = np.where(np.isnan(ry), s.rn[:, 4], ry)
        s.rn[:, 3] = np.where(np.isnan(rx), s.rn[:, 3], rx)
    elif name == "g":
        combo = row % 100
        no, ni, kind = DOTS[combo % 5], DOTS[(combo // 5) % 5], combo // 25
        s.no, s.ni, s.kind = no, ni, kind
        axis = (row // 100) % 3
        along = lambda c: np.column_stack([np.sqrt(1 - c * c), np.zeros(n), c])  # noqa: E731  (n = +z: n.o = c exactly)
        roll = lambda v: np.stack([np.roll(v[i], axis[i] + 1) for i in range(n)])  # noqa: E731
        s.nrm, s.wo, s.wi = roll(np.tile([0.0, 0.0, 1.0], (n, 1))), roll(along(no)), roll(along(ni))
        s.mats[:, 4] = np.isin(kind, (0, 2))
        s.mats[np.isin(kind, (1, 2)), 3] = 0
    for key in ("mats", "nrm", "wo", "wi", "tex", "rn"):
        setattr(s, key, np.ascontiguousarray(getattr(s, key), F))
    s.name, s.n = name, n
    return s


# The rows of each stratum whose reference outputs are committed (tests/golden/volumes_unit.npz, oracle/make_golden.py): the first of
# each (the strata's cases repeat with periods of at most 100 rows).
GOLDEN_ROWS = {"a": 1024, "b": 512, "c": 512, "d": 512, "e": 512, "f": 512, "g": 512}


def reference_view(orc):
    """The oracle's rows (yo_volume_batch) in the layout of ref_volume_batch (oracle/ref_shim.cpp: the reference's public volume
    functions on a given medium) and the rows that layout covers: those with a medium, where eval_scattering's pdf IS the phase
    function. Returns (n, 12) and the mask."""
    view = np.column_stack([orc[:, 8:16], orc[:, 19], orc[:, 19], orc[:, 23], orc[:, 23]])
    return view, (orc[:, 1:4] != 0).any(axis=1)
