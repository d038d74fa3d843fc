"""Closest hits on the device at the edges of segments, triangles and boxes. The rays are the strata of tests/hit_cases.py on the scene
hits-unit (tools/make_scenes.py); tests/test_hit_cases.py proves on the CPU that they are what they claim, tests/test_oracle_vs_ref.py
holds the oracle to the live reference on every one of them.

    stratum  aims at                                                    decision points of csrc/dev_trace.h, csrc/dev_lane.h
    a        the objects, from outside and inside their boxes           today's domain; the float64 bar's cap
    b        p0, p1, joints; distance r, r +- 1 ulp; r = 0 tips; the    the clamp of s; d2 > r * r; det == 0; the leaf's accept rule
             zero-length segment; the twin strand; along the x strand   (the later primitive wins a bit-equal t); intersect_line's three forms
    c        vertices, shared edges at dyadic parameters, the grid's    u < 0, u > 1, v < 0, u + v > 1; det == 0; ties between neighbours
             plane, the sliver, the coincident pair                     and of the pair
    d        t == tmax, t == tmin and their float neighbours, a         t against tmin and tmax, both inclusive; (quad-only batch: tmin =
             finite tmax about the first and the second hit             0, 2^-10, 1)
    e        faces and planes of the flat box and of leaf boxes,        the redo on finite3(1 / d); compare + select against the hardware
             tiny and denormal direction components, box corners        min / max; t0 == t1 under 1.00000024f
    f        b and c in the sheared, rotated, mirrored, scaled frames;  dot(ld, ld) != 1; the padded world box at ENTER
             the faces of the objects' world boxes
    g        128 hit rows of b, 64 times each, the last 16 an ulp off   the cooperative leaves: the step's first tmax, the running re-check;
                                                                        lane_hit_retest
    h        through one object into another just behind, both ways     the pop-time cull of the once-per-ray scene level

The bars, per variant (four: a scene level of one leaf, the once-per-ray form; six: a scene tree; far: six at 2^12 ... 2^16) and per
form (yh_intersect_batch's one-lane kernel and, with YHAIR_INTERSECT=quad, its quad kernel; yh_intersect_plain_batch forms 0 and 1):
    1  object, element, uv and distance are the oracle's on every row, as bits — in stratum order and shuffled
    2  the same against the reference's committed rows (tests/golden/hits_unit.npz)
    3  the float64 restatement (tests/hit_f64.py) names the same hit on every row above its margin
    4  every launch shape renders `four` and `six` to the same bits (the sixteen-lane kernels, leaf pairs and leaf groups)
What an error of one token in the device's tests does to bar 1: profiles/hits_unit/mutations.txt.

What these rows found in the exact second pass, and what was changed for it: DESIGN.md and profiles/hits_unit/exact_pass_ab.txt. The
sixteen-lane and octet forms of that change are reached by bar 4 alone, whose camera rays never lie on a box face: they are held by
reading, not by a row here. The stacks past their windows: tests/test_hits_deep.py. Run time on an MI355X: profiles/hits_unit/gpu_time.txt."""
import numpy as np
import pytest

import hit_cases as hc
import hit_f64
from conftest import golden, scene_path

pytestmark = pytest.mark.gpu
VARIANTS = ("four", "six", "far")
FORMS = ("lanes", "quad", "plain-quad", "plain-octet")
FIELDS = ("object", "element", "uv", "distance")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _run(ctx, form, rays, monkeypatch):
    if form == "lanes":
        monkeypatch.delenv("YHAIR_INTERSECT", raising=False)
        assert len(rays) >= 65536 and (rays[:, 6] == hc.TMIN).all()  # what yh_intersect_batch sends through k_intersect_lanes
        return ctx.intersect(rays)
    if form == "quad":
        monkeypatch.setenv("YHAIR_INTERSECT", "quad")
        got = ctx.intersect(rays)
        monkeypatch.delenv("YHAIR_INTERSECT")
        return got
    return ctx.intersect_plain(FORMS.index(form) - 2, rays)


@pytest.fixture(scope="module")
def cases(yh, oracle):
    """Per variant: the scene, the main batch and its shuffle, the quad-only batch, and the oracle's hits of each (computed once)."""
    out = {}
    _UPLOADED.clear()
    for v in VARIANTS:
        sf = yh.SceneFile(scene_path("hits-unit", variant=v))
        main, quad = hc.main_batch(v), hc.quad_only(v).rays
        ref_main, ref_quad = hc.oracle_hits(v, yh, oracle, scene_path)
        perm = np.random.default_rng(9).permutation(len(main))
        out[v] = dict(sf=sf, main=main, quad=quad, ref_main=ref_main, ref_quad=ref_quad, perm=perm, device={})
    yield out
    for c in out.values():
        c["sf"].close()


def _same(ref, got, where, what):
    for field, a, b in zip(FIELDS, ref, got):
        same = (_bits(a) == _bits(b)).reshape(len(a), -1).all(1)
        bad = np.flatnonzero(~same)
        assert bad.size == 0, f"{what}: {field} differs on {bad.size} rows, first {where(bad[0])}: oracle {a[bad[0]]} device {b[bad[0]]}"


_UPLOADED = {}  # "variant": the variant of this module that the context holds


def _upload(ctx, cases, variant):
    """The variant's scene in the context: uploaded on entry of a test unless the test before it left that very scene there."""
    if _UPLOADED.get("variant") != variant:
        ctx.upload_scene(cases[variant]["sf"].desc)
        _UPLOADED["variant"] = variant


@pytest.fixture(scope="module", params=VARIANTS)
def uploaded(request, cases):
    """(variant, its case). Module-scoped so that pytest runs a variant's tests together and the scene is uploaded once for them;
    the tests do not rely on that order: each calls _upload on entry."""
    return request.param, cases[request.param]


def _device(ctx, c, form, monkeypatch):
    """The device's hits on the variant's main batch through `form`: one run, read by the three bars."""
    if form not in c["device"]:
        c["device"][form] = _run(ctx, form, c["main"], monkeypatch)
    return c["device"][form]


@pytest.mark.parametrize("form", FORMS)
def test_every_row_is_the_oracles(ctx, uploaded, form, monkeypatch):
    """Bar 1 on the main batch, in stratum order and shuffled (waves of one kind of ray, waves of every kind)."""
    variant, c = uploaded
    _upload(ctx, {variant: c}, variant)
    assert ctx.scene_once() == (4 if variant == "four" else 0)
    _same(c["ref_main"], _device(ctx, c, form, monkeypatch), hc.where, f"{variant}, {form}")
    shuffled = _run(ctx, form, c["main"][c["perm"]], monkeypatch)
    _same([a[c["perm"]] for a in c["ref_main"]], shuffled, lambda r: hc.where(c["perm"][r]) + " (shuffled)", f"{variant}, {form}")


@pytest.mark.parametrize("form", FORMS)
def test_the_references_committed_rows(ctx, uploaded, form, monkeypatch):
    """Bar 2: the first rows of every stratum against what the reference said (tests/golden/hits_unit.npz; the oracle may be rebuilt
    where this runs, the committed rows are not)."""
    variant, c = uploaded
    _upload(ctx, {variant: c}, variant)
    got, g = _device(ctx, c, form, monkeypatch), golden("hits_unit.npz")
    for k, name in enumerate(hc.NAMES):
        n = len(g[f"{variant}_{name}_rays"])
        assert np.array_equal(_bits(g[f"{variant}_{name}_rays"]), _bits(c["main"][k * hc.N:k * hc.N + n]))
        _same([g[f"{variant}_{name}_{f}"] for f in FIELDS], [a[k * hc.N:k * hc.N + n] for a in got], lambda r: f"stratum {name} row {r}", f"{variant}, {form}, committed rows")


@pytest.mark.parametrize("form", FORMS)
def test_float64_names_the_same_hit(ctx, uploaded, form, monkeypatch):
    """Bar 3: no tree, box or cull of the device loses a hit that float64 finds with a margin (tests/hit_f64.py)."""
    variant, c = uploaded
    _upload(ctx, {variant: c}, variant)
    hit_f64.compare(variant, _device(ctx, c, form, monkeypatch), f"the device ({form})")


@pytest.mark.parametrize("form", FORMS[1:])
def test_rows_with_another_tmin(ctx, uploaded, form, monkeypatch):
    """The quad-only batch (tmin = 0, 2^-10, 1: t == tmin and t == tmax on the edge) through the three quad forms."""
    variant, c = uploaded
    _upload(ctx, {variant: c}, variant)
    _same(c["ref_quad"], _run(ctx, form, c["quad"], monkeypatch), lambda r: f"quad-only row {r}", f"{variant}, {form}")


@pytest.mark.parametrize("variant", ("four", "six"))
def test_every_launch_shape_renders_the_same_bits(ctx, yh, cases, variant, monkeypatch):
    """Bar 4: 64 x 64, the eyelight shader, 4 + 3 samples under every YHAIR_SHAPE — the only way the sixteen-lane kernels, leaf pairs
    and leaf groups meet flat boxes, ties and zero-radius tips."""
    _upload(ctx, cases, variant)
    p = yh.TraceParams.default(resolution=64, shader="eyelight")
    images = {}
    for shape in ("0", "1", "3", "4", "5", "6", "7", "8"):
        monkeypatch.setenv("YHAIR_SHAPE", shape)
        ctx.init_state(p)
        ctx.trace_samples(4), ctx.trace_samples(3)
        images[shape] = (ctx.download(), ctx.download_rng())
    monkeypatch.delenv("YHAIR_SHAPE")
    base = images["0"]
    assert (base[0][..., 3] > 0).mean() > 0.05
    for k, (img, rng) in images.items():
        assert np.array_equal(_bits(img), _bits(base[0])), f"shape {k} renders different pixels"
        assert np.array_equal(rng, base[1]), f"shape {k} leaves different RNG states"
