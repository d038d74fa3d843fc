"""The cases of tests/test_oracle_vs_ref.py: seeded inputs run through either side of the comparison — the CPU oracle
(oracle_capi.Oracle) or the real reference (oracle_capi.Ref, only where oracle/_ref has been built) — and their outputs.

The reference is not built everywhere the suite runs, so its outputs are also stored, as digests, in
tests/golden/ref_digests.json (written by oracle/make_ref_digests.py from the reference): the oracle is held to them
bit for bit on every machine, and to the live reference as well where there is one.
"""
import hashlib
import json
import os

import numpy as np

import oracle_capi as oc

yh = oc.yh
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_digests.json")

IMAGE_CASES = [
    ("sphere-hairblock", dict(scale=0.1, zoom=True), 80, 4),
    ("hair-curls", dict(scale=0.1), 80, 4),
    ("straight-hair", dict(scale=0.1, beta_m=0.6), 80, 4),
    ("lobes", dict(scale=0.1), 160, 8),
    ("volumes", dict(scale=0.1), 160, 8),
    ("sphere-hairblock", dict(scale=0.1, dof=True), 120, 4),
    ("textured", dict(scale=0.1), 160, 8),
    ("crowd", dict(scale=0.1), 128, 4),
    # the light and environment tables at their edges (tools/make_scenes.py: make_envs_unit)
    ("envs-unit", dict(scale=0.05, variant="rot"), 80, 4),
    ("envs-unit", dict(scale=0.05, variant="lookat"), 80, 4),
    ("envs-unit", dict(scale=0.05, variant="multi"), 96, 4),
    ("envs-unit", dict(scale=0.05, variant="tex-65x64"), 72, 4),
    ("envs-unit", dict(scale=0.05, variant="tex-16x8"), 64, 4),
    ("envs-unit", dict(scale=0.05, variant="lights-4"), 80, 4),
]
SHADERS = ["naive", "eyelight", "normal"]
SHADER_CASES = [
    ("hair-curls", dict(scale=0.1), 64, 4),
    ("lobes", dict(scale=0.1), 128, 4),
    ("volumes", dict(scale=0.1), 96, 4),
    ("textured", dict(scale=0.1), 96, 4),
]


# The `maps` scene and its one-map variants (tools/make_scenes.py: make_maps), as tests/golden/maps.npz holds them
# (tools/make_map_goldens.py): (prefix of the fixture's keys, scene keywords, the fixture's key of the resolution, shaders).
MAP_KINDS = ["specular", "metallic", "roughness", "opacity", "normal"]
MAPS_CASES = [("", {}, "res", ["path", "naive", "eyelight", "normal"])] + [
    (f"only-{kind}/", dict(only=kind), "vres", ["path", "naive", "eyelight"]) for kind in MAP_KINDS]


def maps_entries(api, scene_path, g, prefix, kw, res_key, shaders):
    """What `api` renders for every `*_1`, `*_8` and `*_8_s777` entry of the maps fixture `g` under `prefix`, and `rng_8`."""
    out = {}
    for shader in shaders:
        for suffix, spp, seed in (("_1", 1, None), ("_8", 8, None), ("_8_s777", 8, int(g["seeds"][1]))):
            key = f"{prefix}{shader}{suffix}"
            if key not in g.files:
                continue
            r = render(api, scene_path, "maps", kw, int(g[res_key]), spp, shader, seed)
            out[key] = r["image"]
            if key == "path_8":
                out["rng_8"] = r["rng"]
    return out


def digest(a):
    """sha256 of an array, with np.array_equal(..., equal_nan=True)'s notion of equality: every NaN alike, -0 == +0."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = np.where(np.isnan(a), a.dtype.type(np.nan), a + a.dtype.type(0))
    h = hashlib.sha256(f"{a.dtype.str}{a.shape}".encode())
    h.update(a.tobytes())
    return h.hexdigest()


def stored(key):
    return json.load(open(DIGESTS))[key]


def _dirs(rng, n):
    x = rng.normal(size=(n, 3))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def bsdf_random_inputs(api):
    rng = np.random.default_rng(99)
    n = 20000
    mats = np.zeros((n, 12), np.float32)
    mats[:, 3:5] = rng.uniform(0.02, 0.98, (n, 2))
    mats[:, 5] = rng.uniform(0, 6, n)
    mats[:, 6] = rng.uniform(1.2, 1.8, n)
    mats[:, 10:12] = rng.uniform(0, 8, (n, 2))
    mats[: n // 3, 7:10] = rng.uniform(0.01, 0.99, (n // 3, 3))
    v = rng.uniform(0, 1, n).astype(np.float32)
    tng, wo, wi = _dirs(rng, n), _dirs(rng, n), _dirs(rng, n)
    nrm = _dirs(rng, n)
    rn = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    b = api.hair_brdf(mats, v, nrm, tng)
    return {"hair_brdf": b, "hair_eval": api.hair_eval(b, wo, wi), "hair_pdf": api.hair_pdf(b, wo, wi),
            "hair_sample": api.hair_sample(b, wo, rn)}


def surface_lobes_random_inputs(api):
    rng = np.random.default_rng(100)
    n = 20000
    nn, wo, wi = _dirs(rng, n), _dirs(rng, n), _dirs(rng, n)
    p = np.zeros((n, 8), np.float32)
    p[:, 0] = rng.choice([1.0, 1.0005, 1.33, 1.5, 2.4], n)
    p[:, 1] = rng.choice([0.0009, 0.01, 0.04, 0.25, 1.0], n)
    p[:, 2:5] = rng.uniform(0, 4, (n, 3))
    p[:, 5:8] = rng.choice([0, 1], n)[:, None] * rng.uniform(0, 4, (n, 3))
    rn = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    out = {"fresnel": api.fresnel(p, nn, wo)}
    for kind in range(yh.LOBE_COUNT):
        out[f"surface_lobe_{kind}"] = api.surface_lobe(kind, p, nn, wo, wi, rn)
    return out


def curve_conversion_random_inputs(api):
    rng = np.random.default_rng(101)
    n = 30000
    P = rng.normal(size=(n, 12)).astype(np.float32)
    w0, w1 = rng.uniform(0.001, 0.1, n).astype(np.float32), rng.uniform(0.0005, 0.05, n).astype(np.float32)
    return dict(zip(("positions", "normals", "radius", "lines"), api.curves_to_lines(P, w0, w1, 3)))


def render(api, scene_path, name, kw, res, spp, shader="path", seed=None):
    """The image and the per-pixel RNG states after `spp` samples of the scene; scene_path(name, **kw) gives its JSON. The
    oracle gets the materials' maps the scene file names, as the reference's loader gives them to the reference."""
    path = scene_path(name, **kw)
    p = yh.TraceParams.default(resolution=res, shader=shader) if seed is None else yh.TraceParams.default(resolution=res, shader=shader, seed=seed)
    if isinstance(api, oc.Ref):
        sc, sf = api.scene(path), None
    else:
        sf = yh.SceneFile(path)
        sc = api.scene(sf.desc, sf.maps)
    img, rng = sc.render(p, spp, want_rng=True)
    sc.close()
    if sf is not None:
        sf.close()
    return {"image": img, "rng": rng}


def image_key(name, kw, res, spp, shader="path"):
    return "|".join([shader, name] + [f"{k}={v}" for k, v in sorted(kw.items())] + [str(res), str(spp)])
