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
form — yh_intersect_batch's one-lane kernel and, with YHAIR_INTERSECT=quad, its quad kernel; yh_intersect_plain_batch forms 0 and 1 (512
threads), forms 2-6 (the traversal of launch shapes 1, 4, 7, 6 and 8 at their 256 threads: the dense quad, the octet, the octet with
leaf pairs, the sixteen, the sixteen with leaf groups) and forms 3-6 with the scene level read from memory, as the GENERAL variants of
those shapes read it: thirteen in all (FORMS):
    1  object, element, uv and distance are the oracle's on every row, as bits — in stratum order and shuffled
    2  the same against the reference's committed rows (tests/golden/hits_unit.npz)
    3  the float64 restatement (tests/hit_f64.py) names the same hit on every row above its margin
    4  every launch shape renders `four` and `six` to the same bits
Variant `ties` (four and shapes whose primitives are there 4 to 64 times over, hit_cases.ties): bit-equal hits in different leaves, in
different slots of one 8-wide and one 16-wide node, leaf runs of 0, 1, 2 and more entries on top of the stack — what the visiting order
across slots, the rank arithmetic and the key merge across a group's leaves decide; bars 1-3 through the thirteen forms.
What an error of one token in the device's tests does to bar 1: profiles/hits_unit/mutations.txt (the sixteen-lane step of the exact
pass, the leaf-group key and the 16-wide rank among them: each moves rows in the forms that run it and in no other).

What these rows found in the exact second pass, and what was changed for it: DESIGN.md and profiles/hits_unit/exact_pass_ab.txt. Its
sixteen-lane and octet forms, the leaf pairs and the leaf groups are now held row by row (forms 3-6). Still held by bar 4 and by reading
alone: the once-per-ray scene level under a wide MODE (no launch shape runs it) and the side-by-side kernel's own hand-out. The stacks
past their windows: tests/test_hits_deep.py. The 4-wide scene level from memory under eight and sixteen lanes: tests/test_instances.py.
Run time on an MI355X: profiles/hits_unit/gpu_time.txt."""
import numpy as np
import pytest

import hit_cases as hc
import hit_f64
from conftest import golden, scene_path

pytestmark = pytest.mark.gpu
VARIANTS = ("four", "six", "far")
# yh_intersect_plain_batch's form per name: 0 and 1 at 512 threads; 2-6 the traversal of launch shapes 1, 4, 7, 6 and 8 at their 256 threads;
# mem-*: forms 3-6 with the scene level read from memory (YH_INTERSECT_TABLE_IN_MEMORY = 16), as the GENERAL variants of those shapes read it
PLAIN = {"plain-quad": 0, "plain-octet": 1, "dense-quad": 2, "octet": 3, "octet-pairs": 4, "sixteen": 5, "sixteen-groups": 6,
         "mem-octet": 16 | 3, "mem-octet-pairs": 16 | 4, "mem-sixteen": 16 | 5, "mem-sixteen-groups": 16 | 6}
FORMS = ("lanes", "quad") + tuple(PLAIN)
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
    return ctx.intersect_plain(PLAIN[form], rays)


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


@pytest.fixture(scope="module")
def ties(yh, oracle):
    """Variant `ties`: the scene, its one batch (hit_cases.ties_rays) and the oracle's hits of it."""
    sf = yh.SceneFile(scene_path("hits-unit", variant="ties"))
    rays, ref = hc.ties_rays(), hc.oracle_hits("ties", yh, oracle, scene_path)[0]
    yield dict(sf=sf, rays=rays, ref=ref, perm=np.random.default_rng(12).permutation(len(rays)))
    sf.close()


@pytest.mark.parametrize("form", FORMS)
def test_ties_across_leaves_go_to_the_copy_the_oracle_names(ctx, ties, form, monkeypatch):
    """Variant `ties` — primitives that are there many times over, their copies in different leaves, slots and wide nodes
    (tests/test_hit_cases.py proves it on the CPU), so that the visiting order across slots and the merge across a group's leaves decide
    who wins — through every form: bar 1 in order and shuffled, bar 2 on the reference's committed rows, bar 3 (float64 knows the copies
    of a primitive as one, tests/hit_f64.py). The 8 192 rows are sent eight times over where the one-lane kernel wants 65 536."""
    if _UPLOADED.get("variant") != "ties":
        ctx.upload_scene(ties["sf"].desc)
        _UPLOADED["variant"] = "ties"
    assert ctx.scene_once() == 0
    n = len(ties["rays"])
    rep = 8 if form == "lanes" else 1
    where = lambda r: hc.where(r % n, hc.TIES_NAMES)  # noqa: E731
    got = _run(ctx, form, np.tile(ties["rays"], (rep, 1)), monkeypatch)
    _same([np.concatenate([a] * rep) for a in ties["ref"]], got, where, f"ties, {form}")
    g = golden("hits_unit.npz")
    m = len(g["ties_t_rays"])
    assert np.array_equal(_bits(g["ties_t_rays"]), _bits(ties["rays"][:m]))
    _same([g[f"ties_t_{f}"] for f in FIELDS], [a[:m] for a in got], lambda r: f"row {r}", f"ties, {form}, committed rows")
    hit_f64.compare("ties", [a[:n] for a in got], f"the device ({form})")
    perm = ties["perm"] if rep == 1 else np.random.default_rng(13).permutation(rep * n)
    shuffled = _run(ctx, form, np.tile(ties["rays"], (rep, 1))[perm], monkeypatch)
    _same([np.concatenate([a] * rep)[perm] for a in ties["ref"]], shuffled, lambda r: where(perm[r]) + " (shuffled)", f"ties, {form}")


def test_an_unknown_form_is_refused(ctx, yh, uploaded):
    """Every form outside PLAIN is YH_E_INVALID on an uploaded scene, the memory-table flag on forms 0-2 among them; every form of PLAIN answers."""
    variant, c = uploaded
    _upload(ctx, {variant: c}, variant)
    known = set(PLAIN.values())
    assert yh.INTERSECT_TABLE_IN_MEMORY == 16 and known == set(range(yh.INTERSECT_FORMS)) | {16 | k for k in (3, 4, 5, 6)}
    for form in list(range(-2, 40)) + [16 | 7, 32 | 3, 48 | 3, 1 << 30]:
        if form in known:
            assert len(ctx.intersect_plain(form, c["main"][:4])[0]) == 4
        else:
            with pytest.raises(yh.YhError):
                ctx.intersect_plain(form, c["main"][:4])


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
