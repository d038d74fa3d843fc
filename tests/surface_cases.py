"""The input strata of the unit-level surface tests (tests/test_surface_unit.py) and of their golden vectors
(oracle/make_golden.py: lobes_edges.npz): ROWS rows each, fixed seeds, numpy only.

A row: params (8: ior, roughness [brdf.roughness, already squared], eta[3], etak[3]), nrm, wo, wi (3 each), rn (3: rnl, rn.x,
rn.y) for yh_surface_lobe_batch — every stratum goes through all nine lobes — and mats (10: color[3], specular, metallic, roughness,
transmission, thin, ior, opacity) for yh_surface_bsdf_batch on the same directions and random numbers.

  a  the existing goldens' domain (oracle/make_golden.py: lobe_inputs; tests/test_gpu_parity.py: the random materials)
  b  grazing: n.o and n.i in {0, +-1e-7, +-1e-4, +-1e-2} independently, all 49 pairs, exact in float (an axis as the normal)
  c  incoming = -outgoing (a zero halfway vector), = outgoing, = the exact mirror, = the float64 refraction direction
  d  roughness in {1e-6, 1e-4, 9e-4, 1}; half of the rows with `incoming` at a float64 specular peak (the mirror, -outgoing, the
     refraction direction), so that the halfway vector equals the normal to the last place
  e  ior in {1, the floats either side of 1 +- 1e-3, 1.0005, 1 / 1.5, 2.4}; outgoing on the side that can be totally reflected, at the
     float64 critical angle +- 1e-4 rad and +- 0.05 rad
  f  metals: etak = 0; eta = 1 with etak = 0; etak = 10; eta = 0.1 (the mixture: metallic 1 with colours 0, 0.99, 1 and random)
  g  rn components in {0, 0.5, 1 - 2^-24}; for the mixture rnl is placed by the test on each cumulative lobe pdf of the oracle and
     its two float neighbours (test_surface_unit.py: the oracle's bits are needed for that)
rnl is drawn from U(0.001, 0.999) in b-f, so that no row sits on a Fresnel value of exactly 0 or 1 (ior 1, total reflection).
"""
import types

import numpy as np

import surface_f64 as s64

ROWS = 8192
F = np.float32
BELOW1 = np.nextafter(F(1), F(0))
STRATA = "abcdefg"
SEEDS = {s: 3100 + k for k, s in enumerate(STRATA)}
GRAZING = np.array([0, 1e-7, -1e-7, 1e-4, -1e-4, 1e-2, -1e-2])
ROUGHNESS_EDGES = np.array([1e-6, 1e-4, 9e-4, 1], F)
IOR_EDGES = np.array([1, np.nextafter(F(1.001), F(0)), np.nextafter(F(1.001), F(2)), np.nextafter(F(0.999), F(0)), np.nextafter(F(0.999), F(2)),
                      1.0005, F(1) / F(1.5), 2.4], F)
GOLDEN_ROWS = 256  # the first rows of each stratum whose reference outputs are committed (tests/golden/lobes_edges.npz); the cases' periods are at most 147 rows


def unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _base(rng, n):
    """The existing goldens' domain (oracle/make_golden.py: lobe_inputs) and the random materials of test_gpu_parity.py."""
    nn, wo, wi = (unit(rng.normal(size=(n, 3))) for _ in range(3))
    k = n // 4
    wi[:k] = -wo[:k] + 2 * np.sum(nn[:k] * wo[:k], 1, keepdims=True) * nn[:k] + rng.normal(0, 0.05, (k, 3))
    wi[k:2 * k] = -wo[k:2 * k] + rng.normal(0, 0.05, (k, 3))
    wi = unit(wi)
    p = np.zeros((n, 8), F)
    p[:, 0] = rng.choice([1.0, 1.0005, 1.33, 1.5, 2.4], n)
    p[:, 1] = rng.choice([0.0009, 0.01, 0.04, 0.25, 1.0], n)
    p[:, 2:5] = rng.uniform(0.1, 3.5, (n, 3))
    p[:, 5:8] = rng.choice([0, 1], n)[:, None] * rng.uniform(0, 4, (n, 3))
    rn = np.minimum(rng.uniform(0, 1, (n, 3)).astype(F), BELOW1)
    mats = np.zeros((n, 10), F)
    mats[:, 0:3] = np.where((rng.uniform(size=n) < 0.3)[:, None], rng.choice([0.0, 0.3, 0.9], (n, 3)), rng.uniform(0, 1, (n, 3)))
    mats[:, 3] = rng.choice([0, 0.5, 1], n)
    mats[:, 4] = rng.choice([0, 0, 0.4, 1], n)
    mats[:, 5] = rng.choice([0, 0, 0.05, 0.3, 1], n)
    mats[:, 6] = rng.choice([0, 0, 0.6, 1], n)
    mats[:, 7] = rng.choice([1, 1, 0], n)
    mats[:, 8] = rng.choice([1.0, 1.33, 1.5], n)
    mats[:, 9] = rng.choice([1, 1, 0.9995, 0.5], n)
    return types.SimpleNamespace(params=p, nrm=nn, wo=wo, wi=wi, rn=rn, mats=mats)


def _about_axis(rng, n, axis, cosine):
    """Float vectors whose dot with the axis `axis` (0, 1, 2 per row) is float(cosine) exactly: the other two components random."""
    phi = rng.uniform(0, 2 * np.pi, n)
    s = np.sqrt(1 - cosine * cosine)
    v = np.column_stack([s * np.cos(phi), s * np.sin(phi), cosine])
    return np.stack([np.roll(v[i], axis[i] + 1) for i in range(n)])


def _mirror(n, o):
    return -o + 2 * np.sum(n * o, axis=1, keepdims=True) * n


def _refracted(ior, n, o):
    entering, up, rel = s64._side(np.asarray(ior, np.float64), n, o)
    r = s64.refract(o, up, 1 / rel)
    return np.where((r == 0).all(axis=1)[:, None], -o, r)  # (total reflection: straight through instead)


def inputs(name, n=ROWS):
    rng = np.random.default_rng(SEEDS[name])
    s = _base(rng, n)
    row = np.arange(n)
    if name not in "ag":
        s.rn[:, 0] = rng.uniform(0.001, 0.999, n)
    f32 = lambda x: np.asarray(x, F).astype(np.float64)  # noqa: E731
    if name == "b":
        axis = (row // 49) % 3
        s.no, s.ni = GRAZING[row % 7], GRAZING[(row // 7) % 7]
        s.nrm = np.stack([np.roll([0.0, 0.0, 1.0], a + 1) for a in axis])
        s.wo, s.wi = _about_axis(rng, n, axis, s.no), _about_axis(rng, n, axis, s.ni)
    elif name == "c":
        s.case = row % 4
        nn, wo = f32(s.nrm), f32(s.wo)
        s.wi = np.where((s.case == 0)[:, None], -wo, np.where((s.case == 1)[:, None], wo,
                        np.where((s.case == 2)[:, None], _mirror(nn, wo), _refracted(s.params[:, 0], nn, wo))))
    elif name == "d":
        s.params[:, 1] = ROUGHNESS_EDGES[row % 4]
        s.mats[:, 5] = np.sqrt(ROUGHNESS_EDGES.astype(np.float64))[row % 4]
        s.case = (row // 4) % 6
        nn, wo = f32(s.nrm), f32(s.wo)
        s.wi = np.where((s.case == 0)[:, None], _mirror(nn, wo), np.where((s.case == 1)[:, None], -wo,
                        np.where((s.case == 2)[:, None], _refracted(s.params[:, 0], nn, wo), s.wi)))
    elif name == "e":
        s.params[:, 0] = IOR_EDGES[row % 8]
        s.mats[:, 8] = s.params[:, 0]
        s.mats[:, 6], s.mats[:, 7] = np.where(row % 3 == 0, 0.6, 1.0), 0  # a closed transmissive material: the refraction lobe
        ior = s.params[:, 0].astype(np.float64)
        s.case = (row // 8) % 4
        offset = np.array([1e-4, -1e-4, 0.05, -0.05])[s.case]
        sin_c = np.minimum(np.where(ior >= 1, 1 / ior, ior), 1.0)  # the side with rel_ior < 1 is reflected totally beyond asin(rel_ior)
        theta = np.clip(np.arcsin(sin_c) + offset, 1e-3, np.pi / 2 - 1e-6)
        s.theta_c, s.offset = np.arcsin(sin_c), offset
        side = np.where(ior >= 1, -1.0, 1.0)  # ior > 1: leaving (n.o < 0)
        nn = f32(s.nrm)
        tangent = unit(np.cross(nn, rng.normal(size=(n, 3))))
        s.wo = side[:, None] * np.cos(theta)[:, None] * nn + np.sin(theta)[:, None] * tangent
    elif name == "f":
        s.case = row % 4
        s.params[s.case <= 1, 5:8] = 0
        s.params[s.case == 1, 2:5] = 1
        s.params[s.case == 2, 5:8] = 10
        s.params[s.case == 3, 2:5] = 0.1
        s.mats[:, 4] = 1
        edge = np.array([0, 0.99, 1, np.nan], F)[(row // 4) % 4]
        s.mats[:, 0:3] = np.where(np.isnan(edge)[:, None], s.mats[:, 0:3], edge[:, None])
        s.wi = np.where((row % 8 < 4)[:, None], _mirror(f32(s.nrm), f32(s.wo)), s.wi)
    elif name == "g":
        edge = np.array([0, 0.5, BELOW1], F)
        s.rn[:, 0], s.rn[:, 1], s.rn[:, 2] = edge[row % 3], edge[(row // 3) % 3], edge[(row // 9) % 3]
        s.params[:, 0] = np.where(row % 2 == 0, 1.33, 1.5)
        s.mats[:, 8] = s.params[:, 0]
        nn = f32(s.nrm)
        flip = np.sum(nn * s.wo, axis=1) < 0
        s.wo = np.where(flip[:, None], -s.wo, s.wo)  # entering, away from grazing: the Fresnel value stays off 0 and 1
        s.wo = unit(s.wo + 0.3 * nn)
    for key in ("params", "nrm", "wo", "wi", "rn", "mats"):
        setattr(s, key, np.ascontiguousarray(getattr(s, key), F))
    s.name, s.n = name, n
    return s


def material_rows(yh, mats10):
    """(n, 10) rows [color3 specular metallic roughness transmission thin ior opacity] -> ctypes array of yh_material."""
    arr = (yh.Material * len(mats10))()
    for i, r in enumerate(np.asarray(mats10, F)):
        m = arr[i]
        m.color[:] = r[0:3].tolist()
        m.specular, m.metallic, m.roughness, m.transmission = (float(x) for x in r[3:7])
        m.thin, m.ior, m.opacity = int(r[7] != 0), float(r[8]), float(r[9])
        m.trdepth = 0.01
    return arr
