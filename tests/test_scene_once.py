"""The scene level resolved once per ray (csrc/dev_trace.h: trace_ray_loop, ONCE): the plain 512-thread kernels — launch shape 0
and both halves of shape 5 — run the scene node's box test, the padded-box slabs and the ENTER arithmetic of every object ahead
of the traversal loop when the scene level is one leaf node, keep the result per (path, object) in LDS and cull an object at its
pop with the current tmax. Nothing may change: closest hits are the oracle's bit for bit at unit level (yh_intersect_plain_batch
runs the plain traversal, which no other unit-level entry reaches), images, RNG states and work counts are those of the dense
shape (1), which keeps the in-loop scene level. Every comparison is over all rays and all pixels."""
import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu
VARIANTS = ("one", "disjoint", "overlap", "tie", "full", "five")
N = 4096  # rays per set


def _boxes(desc):
    """World boxes of the scene's objects, from the description (hair radii included)."""
    out, desc = [], desc.contents
    for i in range(desc.num_objects):
        o, sh = desc.objects[i], desc.shapes[desc.objects[i].shape]
        p = np.ctypeslib.as_array(sh.positions, (sh.num_vertices, 3)).astype(np.float64)
        f = np.array(list(o.frame), np.float64).reshape(4, 3)
        w = p @ f[:3] + f[3]
        r = float(np.ctypeslib.as_array(sh.radius, (sh.num_vertices,)).max()) * 2 if sh.num_lines else 0.0
        out.append((w.min(0) - r, w.max(0) + r))
    return out


def _unit(v):
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-30)


def _rays(o, d, tmin=1e-4, tmax=3.4e38):
    n = len(o)
    return np.concatenate([o, d, np.full((n, 1), tmin), np.broadcast_to(np.asarray(tmax, np.float64).reshape(-1, 1), (n, 1))], axis=1).astype(np.float32)


def ray_sets(boxes, seed=3):
    """name -> (N, 8) rays: random ones and the targeted sets of the scene level's edges."""
    rng = np.random.default_rng(seed)
    lo, hi = np.min([b[0] for b in boxes], 0), np.max([b[1] for b in boxes], 0)
    # (the far-away lights of `full` / `five` would stretch the frame of the random rays over empty space: aim at the near objects)
    near = [b for b in boxes if np.all(b[1] < 3.5)] or boxes
    nlo, nhi = np.min([b[0] for b in near], 0), np.max([b[1] for b in near], 0)
    ctr, ext = (nlo + nhi) / 2, (nhi - nlo) / 2 + 1e-3
    sets = {}
    pt = lambda b, n: rng.uniform(b[0], b[1], (n, 3))
    o = ctr + rng.normal(0, 1.5, (N, 3)) * ext
    sets["random"] = _rays(o, _unit(rng.normal(size=(N, 3))))
    sets["towards"] = _rays(o, _unit(pt((nlo, nhi), N) - o))
    # miss every padded box: from above everything, upwards
    up = _unit(rng.normal(size=(N, 3)) * [1, 0, 1] + [0, 1, 0])
    sets["miss-all"] = _rays(pt((lo, hi), N) * [1, 0, 1] + [0, hi[1] + 1.0, 0], up)
    # origins inside the boxes (inside both where two overlap)
    a, b = near[0], near[-1]
    ilo, ihi = np.maximum(a[0], b[0]), np.minimum(a[1], b[1])
    inside = (ilo, ihi) if np.all(ilo < ihi) else a
    sets["inside"] = _rays(np.concatenate([pt(inside, N // 2), pt(b, N - N // 2)]), _unit(rng.normal(size=(N, 3))))
    sets["finite-tmax"] = _rays(o, _unit(pt((nlo, nhi), N) - o), tmax=rng.uniform(0.05, 8.0, N))
    # axis-parallel and zero-component directions, a zero direction: the second pass (the in-loop scene level, compare + select)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 1, 1], [1, 0, -1], [-1, 1, 0], [0, 0, 0]], np.float64)
    d = axes[rng.integers(0, len(axes), N)]
    d = np.where(np.arange(N)[:, None] % 3 == 0, d, d * rng.uniform(0.3, 2.0, (N, 1)))
    sets["axis-parallel"] = _rays(pt((nlo, nhi), N) - 3.0 * d, d)
    # through one object into the next, both ways: a hit in the first shrinks tmax below the second's box entry
    first, second = pt(a, N), pt(b, N)
    d = _unit(second - first + 1e-9)
    half = np.arange(N)[:, None] < N // 2
    sets["through"] = _rays(np.where(half, first - 4.0 * d, second + 4.0 * d), np.where(half, d, -d))
    # straight down and up onto the block's middle (in `tie`: onto the coincident quads, every hit of theirs an exact-t tie)
    tgt = pt((ctr - ext * [0.6, 0, 0.6], ctr + ext * [0.6, 0, 0.6]), N)
    src = tgt + rng.normal(0, 0.4, (N, 3)) * [1, 0, 1] + np.where(half, 3.0, -3.0) * np.array([0, 1, 0])
    sets["vertical"] = _rays(src, _unit(tgt - src))
    return sets


@pytest.fixture(scope="module")
def cases(yh, oracle):
    """Per variant: the loaded scene, its rays (the sets one after the other, then all of them shuffled: waves of one kind of ray
    and waves of every kind) and the oracle's closest hits for them — computed once, read by the tests."""
    out = {}
    for v in VARIANTS:
        sf = yh.SceneFile(scene_path("scene-once", variant=v))
        sets = ray_sets(_boxes(sf.desc))
        rays = np.concatenate(list(sets.values()))
        rays = np.concatenate([rays, rays[np.random.default_rng(9).permutation(len(rays))]])
        osc = oracle.scene(sf.desc)
        ref = osc.intersect(rays)
        osc.close()
        out[v] = dict(sf=sf, sets=sets, rays=rays, ref=ref)
    yield out
    for c in out.values():
        c["sf"].close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_form_is_taken_by_a_scene_level_of_one_leaf(ctx, yh, cases, variant):
    ctx.upload_scene(cases[variant]["sf"].desc)
    n = cases[variant]["sf"].desc.contents.num_objects
    assert ctx.scene_once() == (n if n <= 4 else 0)  # five objects: more than one scene node, the in-loop scene level stays


@pytest.mark.parametrize("form", [0, 1], ids=["quad", "octet"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_plain_traversal_closest_hits_are_the_oracles(ctx, yh, cases, variant, form):
    c = cases[variant]
    ctx.upload_scene(c["sf"].desc)
    got = ctx.intersect_plain(form, c["rays"])
    n = len(c["rays"]) // 2
    names = list(c["sets"])
    for what, a, b in zip(("object", "element", "uv", "distance"), c["ref"], got):
        same = (_bits(a) == _bits(b)).reshape(len(a), -1).all(1)
        bad = np.flatnonzero(~same)
        assert bad.size == 0, f"{what} differs on {bad.size} rays, first {bad[0]} (set {names[(bad[0] % n) // N] if bad[0] < n else 'shuffled'}): oracle {a[bad[0]]} device {b[bad[0]]}"
    # the sets are what they are meant to be
    obj = c["ref"][0][:n].reshape(len(names), N)
    hitrate = dict(zip(names, (obj >= 0).mean(1)))
    assert hitrate["miss-all"] == 0 and hitrate["towards"] > 0.2 and hitrate["through"] > 0.5
    if variant != "one":
        through = obj[names.index("through")]
        assert len(np.unique(through[through >= 0])) >= 2  # closest hits in the first object and in the second
    if variant == "tie":  # the later of the two coincident quads wins every tie (math.h:3450), the earlier is never the closest hit
        ids = set(np.unique(c["ref"][0]))
        assert 2 in ids and 1 not in ids


def test_general_scenes_are_refused(ctx, yh):
    sf = yh.SceneFile(scene_path("lobes", scale=0.05))
    ctx.upload_scene(sf.desc)
    assert ctx.scene_once() == 0
    with pytest.raises(yh.YhError, match="GENERAL"):
        ctx.intersect_plain(0, np.zeros((4, 8), np.float32))
    sf.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_shapes_0_and_5_render_the_dense_shapes_bits(ctx, yh, cases, variant, monkeypatch):
    """Launch shapes 0 and 5 (the prologue form where the scene takes it) against shape 1 (256 x 5: the in-loop scene level): images, final
    RNG states and, for the instrumented shape 0, the work counts."""
    ctx.upload_scene(cases[variant]["sf"].desc)
    p = yh.TraceParams.default(resolution=40, bounces=8)
    res, counts = {}, {}
    for shape in ("1", "0", "5"):
        monkeypatch.setenv("YHAIR_SHAPE", shape)
        ctx.init_state(p)
        ctx.trace_samples(1), ctx.trace_samples(3)
        res[shape] = (ctx.download(), ctx.download_rng())
        if shape != "5":  # (side by side has no instrumented build)
            ctx.init_state(p)
            counts[shape] = ctx.trace_samples_counted(4).as_dict()
    assert res["1"][0][..., 3].max() > 0
    for shape in ("0", "5"):
        assert np.array_equal(_bits(res[shape][0]), _bits(res["1"][0])), f"shape {shape} renders different pixels"
        assert np.array_equal(res[shape][1], res["1"][1]), f"shape {shape} leaves different RNG states"
    for k in ("samples", "rays", "nodes", "seg_tests", "tri_tests", "hair_shades", "surf_shades", "env_lookups", "env_samples"):
        assert counts["0"][k] == counts["1"][k], (k, counts["0"][k], counts["1"][k])
    assert counts["1"]["samples"] == 40 * 40 * 4
