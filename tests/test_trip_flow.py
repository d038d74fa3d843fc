"""The trip of the once-per-ray traversal (csrc/dev_trace.h: trace_ray_loop, ONCE) restated for the shape of its control flow: the
objects that wait are one count and a cull without a loop, one address form, one return per primitive test, leaf regions under one
mask, the surviving hit kept in the hit record. Nothing may change:

  * the closest hits of hits-unit's variants four, six, deep and ties through the 512-thread quad form and the octet form
    (yh_intersect_plain_batch forms 0 and 1: the traversal of launch shape 0 and of both halves of shape 5) are the oracle's bit for
    bit, in order and shuffled, at the row counts those variants have;
  * `enter-chain`, a scene of this file: four plates across the x axis in one scene leaf, each half of its own box, in three
    orders of entry. A ray along x passes all four padded boxes at its first tmax and hits some of the plates, and which of the objects that
    wait are entered and which are culled follows from where the plates lie along it. The CPU proves with the oracle's hits on each
    plate alone that every pattern asked for occurs with a wide margin before anything runs on the GPU: none, one and two objects
    culled in a row with the last one entered, all three culled and the ray done, and the later culls that leave nothing to enter;
  * 64 x 64, 4 spp of sphere-hairblock and of a four-object plain scene under launch shapes 0 and 5 are k_stream's bits (shape 3),
    pixels and RNG states."""
import os

import numpy as np
import pytest

import hit_cases as hc
import make_scenes
from conftest import SCENES, scene_path
from test_hits_unit import _same

pytestmark = pytest.mark.gpu
FORMS = {"plain-quad": 0, "plain-octet": 1}
F = np.float32


# ---------------------------------------------------------------------------------------------------------------------------------
# the rows of hits-unit
# ---------------------------------------------------------------------------------------------------------------------------------
def _variant_rays(variant):
    return hc.deep_rays() if variant == "deep" else hc.ties_rays() if variant == "ties" else hc.main_batch(variant)


@pytest.fixture(scope="module")
def rows(yh, oracle):
    """Per variant: the scene, its rows, a shuffle of them and the oracle's hits (hit_cases.oracle_hits: once per session)."""
    out = {}
    for k, v in enumerate(("four", "six", "deep", "ties")):
        rays = _variant_rays(v)
        out[v] = dict(sf=yh.SceneFile(scene_path("hits-unit", variant=v)), rays=rays, ref=hc.oracle_hits(v, yh, oracle, scene_path)[0],
                      perm=np.random.default_rng(40 + k).permutation(len(rays)))
    yield out
    for c in out.values():
        c["sf"].close()


@pytest.mark.parametrize("variant", ("four", "six", "deep", "ties"))
def test_rows_through_the_quad_and_the_octet_form(ctx, rows, variant):
    c = rows[variant]
    ctx.upload_scene(c["sf"].desc)
    assert ctx.scene_once() == (4 if variant == "four" else 0)  # (the others keep the in-loop scene level: their kernels are not to move either)
    names = hc.DEEP_NAMES if variant == "deep" else hc.TIES_NAMES if variant == "ties" else hc.NAMES
    for form, k in FORMS.items():
        _same(c["ref"], ctx.intersect_plain(k, c["rays"]), lambda r: hc.where(r, names), f"{variant}, {form}")
        _same([a[c["perm"]] for a in c["ref"]], ctx.intersect_plain(k, c["rays"][c["perm"]]), lambda r: hc.where(c["perm"][r], names) + " (shuffled)", f"{variant}, {form}")


# ---------------------------------------------------------------------------------------------------------------------------------
# enter-chain
# ---------------------------------------------------------------------------------------------------------------------------------
# Object k is the half of the square [-1, 1]^2 in the plane x = X[k] on one side of a diagonal: its box is the whole square, a ray
# through the other half passes the box and hits nothing. The four halves are the four sides of the two diagonals, so every point of
# the square lies on two plates and off two. Order "behind": a hit on the first object culls the second and the
# third, the fourth lies in front of it. Order "front": the first object is the nearest of a ray along +x, its hit culls all three.
# Order "mixed": the second lies behind the first and the third in front of it — one object culled, the next entered.
ORDERS = {"behind": (2.0, 3.0, 4.0, 1.0), "front": (1.0, 2.0, 3.0, 4.0), "mixed": (2.0, 3.0, 1.0, 4.0)}
_CORNERS = np.array([(-1.0, -1.0), (1.0, -1.0), (1.0, 1.0), (-1.0, 1.0)])
N_PER = 1408  # rays per order: 4 224 in all


def _plate(k, x):
    """The triangle of corners k - 1, k, k + 1 of the square, in the plane at x."""
    c = _CORNERS[[(k - 1) % 4, k, (k + 1) % 4]]
    return np.stack([np.full(3, x), c[:, 0], c[:, 1]], 1)


def _make_enter_chain(order, only=-1):
    """The scene file of an order of entry (only >= 0: that plate alone, for the hits on it)."""
    name = f"enter-chain-{order}" + (f"-only{only}" if only >= 0 else "")
    path = os.path.join(SCENES, name, name + ".json")
    if os.path.exists(path):
        return path
    d = make_scenes._prep(SCENES, name)
    objects = {}
    for k, x in enumerate(ORDERS[order]):
        if only >= 0 and k != only:
            continue
        make_scenes._write_f32_ply(os.path.join(d, "shapes", f"plate{k}.ply"), _plate(k, x), triangles=[(0, 1, 2)])
        objects[f"plate{k}"] = {"frame": make_scenes.IDENT, "shape": f"plate{k}", "material": "diffuse"}
    scene = {"asset": {"copyright": "synthetic (tests/test_trip_flow.py)"},
             "cameras": {"default": {"lens": 0.05, "aperture": 0.0, "aspect": 1.0, "lookat": [2.5, 0.5, 9.0, 2.5, 0.0, 0.0, 0, 1, 0]}},
             "environments": {"sky": {"emission": [1, 1, 1]}}, "objects": objects, "materials": {"diffuse": {"color": [0.8, 0.4, 0.05]}}}
    make_scenes._dump(scene, path)
    return path


def _chain_rays(seed):
    """N_PER rays: along +x from x = 0 and along -x from x = 5 through points of the square, tilted a little (they stay inside it
    over the plates' range); from between the plates, where a box or two lie behind the origin; with a finite tmax between two
    plates; and exactly along +-x (a zero direction component: the second pass)."""
    rng = np.random.default_rng(seed)
    n = N_PER
    y, z = rng.uniform(-0.8, 0.8, n), rng.uniform(-0.8, 0.8, n)
    fam = np.arange(n) % 8
    sign = np.where(fam % 2 == 0, 1.0, -1.0)
    x0 = np.where(sign > 0, 0.0, 5.0)
    between = (fam == 4) | (fam == 5)
    x0 = np.where(between, rng.choice([1.5, 2.5, 3.5], n), x0)
    tilt = rng.uniform(-0.03, 0.03, (n, 2))
    tilt[fam >= 6] = 0.0  # axis-parallel
    d = np.stack([sign, tilt[:, 0], tilt[:, 1]], 1) * rng.choice([0.5, 1.0, 2.0], n)[:, None]
    tmax = np.where(fam == 3, rng.choice([1.5, 2.5, 3.5], n) / np.abs(d[:, 0]), 3.4e38)
    rays = np.concatenate([np.stack([x0, y, z], 1), d, np.full((n, 1), 1e-4), tmax[:, None]], 1).astype(F)
    return rays


def _leaf_order(yh, boxes):
    """The order in which the scene leaf holds the objects (the host's builder on their boxes: one leaf node)."""
    lib = yh.load()
    b = np.ascontiguousarray(boxes, F)
    n = lib.yh_bvh_build(len(b), yh.fptr(b), None, None)
    nodes, prims = np.zeros((n, 8), F), np.zeros(len(b), np.int32)
    assert lib.yh_bvh_build(len(b), yh.fptr(b), yh.fptr(nodes), yh.iptr(prims)) == n == 1
    return [int(p) for p in prims]


def _patterns(order, rays, alone, leaf):
    """Per ray (those with four boxes on their way and nothing near a decision's edge): a letter per object that waits behind the
    first, in the order of entry — E entered, c culled — and the closest distance that leaves, for a check against the oracle's hit
    on the whole scene. alone[k]: the oracle's (object, element, uv, distance) on plate k alone. float64; the device's padded box is
    the plate's box and a sliver (1e-3 of its size), the plates lie a whole unit apart and a decision nearer than 0.05 is not counted."""
    X = np.array(ORDERS[order])
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    tmax0 = rays[:, 7].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = (X[None, :] - o[:, :1]) / d[:, :1]                      # where the ray meets each plate's plane = its flat box
    py, pz = o[:, 1:2] + tx * d[:, 1:2], o[:, 2:3] + tx * d[:, 2:3]
    inbox = (tx > 1e-4) & (np.abs(py) < 0.95) & (np.abs(pz) < 0.95) & (tx < tmax0[:, None] - 0.05)  # passes the box at the first tmax, clearly
    out, closest = [], []
    for r in range(len(rays)):
        entries = [k for k in leaf if inbox[r, k]]
        tmax, pat, sure = tmax0[r], "", True
        for j, k in enumerate(entries):
            if j > 0:
                if abs(tx[r, k] - tmax) < 0.05:
                    sure = False
                if tx[r, k] > tmax:
                    pat += "c"
                    continue
                pat += "E"
            hit_obj, dist = alone[k][0][r], float(alone[k][3][r])
            if hit_obj >= 0 and dist <= tmax:
                tmax = dist
        out.append((len(entries), pat) if sure else (0, "?"))
        closest.append(tmax if tmax < tmax0[r] else np.inf)
    return out, np.array(closest)


@pytest.fixture(scope="module")
def chain(yh, oracle):
    """Per order of entry: the scene, its rays and a shuffle, the oracle's hits on the whole scene and on each plate alone, and the
    cull patterns the CPU finds — all before a test sends anything to the GPU."""
    out = {}
    for s, order in enumerate(ORDERS):
        rays = _chain_rays(70 + s)
        sf = yh.SceneFile(_make_enter_chain(order))
        osc = oracle.scene(sf.desc)
        ref = osc.intersect(rays)
        osc.close()
        alone = []
        for k in range(4):
            one = yh.SceneFile(_make_enter_chain(order, only=k))
            o1 = oracle.scene(one.desc)
            alone.append(o1.intersect(rays))
            o1.close(), one.close()
        X = ORDERS[order]
        leaf = _leaf_order(yh, [(x, -1, -1, x, 1, 1) for x in X])
        pats, closest = _patterns(order, rays, alone, leaf)
        out[order] = dict(sf=sf, rays=rays, ref=ref, leaf=leaf, pats=pats, closest=closest, perm=np.random.default_rng(80 + s).permutation(len(rays)))
    yield out
    for c in out.values():
        c["sf"].close()


def test_enter_chain_every_cull_pattern_occurs_and_the_hits_are_the_oracles(ctx, chain):
    # on the CPU first: the walk above names the oracle's closest hit, and every pattern is there
    seen = {}
    for order, c in chain.items():
        assert c["leaf"] == [0, 1, 2, 3], "the scene leaf holds the plates in another order than the scene names them"
        hit = c["ref"][0] >= 0
        sure = np.array([p[1] != "?" for p in c["pats"]])
        assert np.array_equal(np.isfinite(c["closest"])[sure], hit[sure]) and sure.mean() > 0.9
        assert np.allclose(c["closest"][sure & hit], c["ref"][3][sure & hit], rtol=1e-5)
        for n, p in c["pats"]:
            seen.setdefault((order, n), set()).add(p)
        assert (c["rays"][:, 4:6] == 0).all(1).sum() >= N_PER // 8 and hit[(c["rays"][:, 4:6] == 0).all(1)].any()  # the axis-parallel rows, hits among them
    four = seen[("behind", 4)] | seen[("front", 4)] | seen[("mixed", 4)]
    # four boxes at the first tmax: none, one, two culled in a row and the next entered; all three culled; the later culls that empty the stack
    for want in ("EEE", "cE", "ccE", "ccc", "Ecc", "EEc", "EcE"):
        assert any(p.startswith(want) for p in four), (want, sorted(four))
    assert "ccE" in seen[("behind", 4)] and "ccc" in seen[("front", 4)] and "cEc" in seen[("mixed", 4)]
    fewer = lambda n: set().union(*(seen.get((order, n), set()) for order in ORDERS))  # noqa: E731  (an origin between the plates: three boxes, two)
    assert "cc" in fewer(3) and "c" in fewer(2)
    # then the device
    for order, c in chain.items():
        ctx.upload_scene(c["sf"].desc)
        assert ctx.scene_once() == 4
        for form, k in FORMS.items():
            _same(c["ref"], ctx.intersect_plain(k, c["rays"]), lambda r: f"row {r}", f"enter-chain ({order}), {form}")
            _same([a[c["perm"]] for a in c["ref"]], ctx.intersect_plain(k, c["rays"][c["perm"]]), lambda r: f"row {c['perm'][r]} (shuffled)", f"enter-chain ({order}), {form}")


# ---------------------------------------------------------------------------------------------------------------------------------
# renders
# ---------------------------------------------------------------------------------------------------------------------------------
def _render(ctx, yh, monkeypatch, shape, res=64, spp=4):
    monkeypatch.setenv("YHAIR_SHAPE", shape)
    ctx.init_state(yh.TraceParams.default(resolution=res, bounces=8))
    ctx.trace_samples(1), ctx.trace_samples(spp - 1)
    assert ctx.launch_shape() == int(shape)
    return np.ascontiguousarray(ctx.download()).view(np.uint32), ctx.download_rng()


@pytest.mark.parametrize("name,kw,once", [("sphere-hairblock", dict(scale=0.05), 2), ("scene-once", dict(variant="full"), 4)])
def test_shapes_0_and_5_render_k_streams_bits(ctx, yh, monkeypatch, name, kw, once):
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc)
    assert ctx.scene_once() == once
    want = _render(ctx, yh, monkeypatch, "3")
    assert want[0].view(F)[..., 3].max() > 0 and np.isfinite(want[0].view(F)).all()
    for shape in ("0", "5"):
        got = _render(ctx, yh, monkeypatch, shape)
        bad = np.flatnonzero((got[0] != want[0]).reshape(-1, 4).any(1))
        assert bad.size == 0, f"{name}, shape {shape} against shape 3: {bad.size} pixels differ, first {bad[0]}"
        assert np.array_equal(got[1], want[1]), f"{name}, shape {shape} against shape 3: RNG states differ"
    sf.close()
