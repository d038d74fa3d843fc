"""The shading point of a hit on the device as the sample loops make it (yh_point_batch: unit/point_shade.h), at unit level and at its
edges: eval_hit / eval_hit_fetch_first, eval_texcoord, eval_maps, eval_normalmap, eval_hit_maps, the shading-normal rule and the head
of path_step / shade_step up to surface_brdf (csrc/dev_path.h) with eval_texture (csrc/dev_surface.h), then medium_crossing straight
through the surface, on two uploaded scenes built in memory (tests/point_cases.py): PLAIN, where form 0 runs the rows from LDS and
eval_hit_fetch_first, and GENERAL with textures, maps and volumes. Forms: 0 launch shape 0 on the scene (a quad per row), 1 k_stream (a
lane per row), 2 the 256-thread shape and shade_step (a quad per row, rows from memory, the mixture for every material).

References: the oracle's yo_scene_point_batch (float arithmetic, the reference's operations; its maps are held to the reference's
images bit for bit by tests/test_oracle_golden.py::test_material_maps_bit_exact, its rows on these strata to
tests/golden/points_unit.npz) and tests/point_f64.py, the same formulas in float64.
Strata (ROWS rows each, fixed seeds): a today's domain, b uv edges, c texcoords, d normals, e the rule, f normal maps, g scalar maps
and textures.

Quantities: position (error relative to the scene's diagonal), normal and shading_normal (absolute), texcoord (relative with a floor
of 1: it is consumed through fmod, so its absolute place in texel space counts), color_tex, emission_tex (with its linear x),
scattering_tex, emission, weights (the five lobes), roughness, opacity, pdfs, density, scatter, anisotropy (relative, floor 1e-7; per
row the largest over the components).

Bars (none of them taken from what the device gives):
  1  forms 0, 1 and 2 give every float of every row bit for bit, NaN pattern included, on both scenes and every stratum. One sign is
     left out: on a row whose material is plain, forms 0 and 1 report the constants of the loop's diffuse-only path where form 2
     reports the mixture it made, and a zero lobe of that mixture may be -0 (0 x the negative rounding residue that
     fresnel_conductor leaves for eta = 1, a black colour): on those rows a zero METAL PDF counts as +0, and only there. The sign is
     the reference's: form 2 carries -0 on exactly the rows where the oracle does (asserted), in no other lobe column;
  2  exact against the oracle, every row of every stratum and form: texcoord where the shape has none; emission and diffuse weight
     of untextured plain materials; which rows flip the normal (triangles without a normal map: shading normal = -normal); which
     rows are delta (roughness 0); which rows have opacity exactly 1; the zero pattern of the five pdfs. The texcoord column is
     compared only where the loop evaluates it (a material with a texture or a map; else the loop keeps the element uv);
  3  stratum a against the oracle: values within REL_BSDF (1e-4), the directions (eval_normal, the shading normal) within ABS_DIR
     (5e-5), position within REL_BSDF x the scene's diagonal;
  4  strata b-g against float64: median and p99 of the per-row error of every quantity at most K = 2 x max(the oracle's same
     statistic on the same rows, 1e-6), over the rows where float64 and the oracle are finite;
  5  the non-finite mask equals the oracle's on every row;
  6  set aside from bar 4: rows whose float64 decision quantity — dot(n, outgoing) against 0, opacity against 0.999, div against 0,
     flip_v's dot against 0 — lies within 4 float ulps of its threshold without lying on it (decided on the inputs alone); at most
     2e-4 of a stratum's rows, asserted on the CPU too. (The texel index at a boundary is no such quantity here: the bilinear lookup
     with its wrap is continuous across every boundary, so those rows stay in.);
  7  n in {1, 3, 4097}: each row equals the same row of the ROWS-row call bit for bit; the refusals of the entry point.
The CPU tests hold the restatement to the oracle (median relative difference of every quantity below 1e-5 per stratum and scene) and
the strata to the edges they name.

What the bars catch: the module run once against three scratch copies of the library whose point kernels were compiled from a
csrc/dev_path.h with one one-token error each (nothing of them is committed; none moves an address):
  1  eval_normalmap's `dot(f.y, tgv) < 0` written `> 0`: 15 tests fail, general scene, all three forms, no other bar.
       bar 3 (stratum a): shading_normal 1.76 against 5e-5.
       bar 4 on strata b, d, e, f: shading_normal p99 0.41 to 1.86 against the reference's 4.4e-7 to 2.2e-6 (on f also the median, 3.9e-2
       against 4.8e-8), and with it weights (p99 5.9e-2 to 1.3e-1 against 5.2e-7 to 1.6e-5) and pdfs (p99 0.70 to 2.4 against 5.2e-6 to 7.0e-6).
  2  eval_maps' `0.999f` written `0.99f`: 24 tests fail, general scene, all three forms.
       bar 2 (which rows have opacity exactly 1) on strata a, b, f, g: the hair with an opacity map and the opacity-straddle object.
       bar 3 (stratum a): opacity 1.36e-3 against 1e-4.
       bar 4 on strata b, f, g: opacity p99 1.20e-3 to 1.27e-3 against the reference's 5.2e-8 to 9.6e-7.
  3  eval_hit_fetch_first reading n1 and n2 swapped: 21 tests fail, plain scene (the only place the function runs: form 0).
       bar 1 on every stratum: 204 to 1366 rows of form 0 differ from forms 1 and 2 in the normal and shading-normal columns.
       bar 2 (which rows flip the normal) on every stratum, form 0.
       bar 3 (stratum a, form 0): normal 1.53 against 5e-5.
       bar 4 on strata b-g, form 0: normal and shading_normal p99 0.35 to 1.5 against the reference's 8e-8 to 2e-7 (on d also the median,
       2.6e-2 against 2.9e-8).

MEASURED (2026-10-20, AMD Instinct MI355X, gfx950; the median / p99 table per stratum, scene and quantity: profiles/point_unit/errors.txt):
no assertion fails. The GPU tests of the module: 112 passed in 1.86 s (the slowest 0.13 s). Forms 0, 1 and 2 agree bit for bit on all
fourteen stratum x scene pairs. On stratum a the device equals the oracle bit for bit in every quantity but the density (logf: 2.2e-7
against 1e-4); on strata b-g its median and p99 against float64 equal the reference's to the printed digits in every quantity but the
density (general scene, stratum g: p99 1.03e-6 against the reference's 1.04e-6). No row is set aside on any stratum. The oracle's rows are finite on every
stratum and so are the device's. The sign bar 1 leaves out: a metal pdf of -0 on 4 / 20 / 0 / 0 / 10 / 61 / 12 plain rows of strata
a-g of the plain scene (the black material and the hair of colour 0), the same rows in the oracle and in form 2, in no other lobe column.
"""
import types

import numpy as np
import pytest

import point_cases as pc
import point_f64 as p64
from test_gpu_parity import ABS_DIR, REL_BSDF, _rel

F = np.float32
ROWS = pc.ROWS
FORMS = [("shape0", 0), ("stream", 1), ("shade", 2)]
SCENES = [("plain", False), ("general", True)]
K_BAR = 2.0
E_FLOOR = 1e-6
ASIDE_ULPS, ASIDE_CAP = 4, 2e-4
CPU_MEDIAN = 1e-5
QUANTITIES = tuple(p64.COLS)
COL = p64.COLS  # the quantities' columns (from the binding's POINT_COLUMNS)
METAL_PDF = COL["pdfs"].start + 2
ABSOLUTE = ("normal", "shading_normal")


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _row_err(sc, q, got, want):
    """Per row the largest error of quantity q over its components (see the module's docstring for the measure of each)."""
    if len(want) == 0:
        return np.zeros(0)
    got, want = np.asarray(got, np.float64).reshape(len(want), -1), np.asarray(want, np.float64).reshape(len(want), -1)
    with np.errstate(invalid="ignore", over="ignore"):
        if q == "position":
            return np.max(np.abs(got - want), axis=1) / sc.diagonal
        if q in ABSOLUTE:
            return np.max(np.abs(got - want), axis=1)
        return np.max(_rel(got, want, 1.0 if q == "texcoord" else 1e-7), axis=1)


def _stat(err):
    return (float(np.median(err)), float(np.percentile(err, 99))) if len(err) else (0.0, 0.0)


def _finite_rows(a):
    return np.isfinite(np.asarray(a, np.float64).reshape(len(a), -1)).all(axis=1)


_CACHE, _ORACLE_SCENES = {}, {}


def _oracle_scene(oracle, yh, general):
    if general not in _ORACLE_SCENES:
        _ORACLE_SCENES[general] = oracle.scene(*pc.scene(general).desc(yh))
    return _ORACLE_SCENES[general]


def _stratum(name, general, oracle, yh):
    """Inputs, the float64 values, the oracle's values and the oracle's errors against float64, made once."""
    key = (name, general)
    if key not in _CACHE:
        s = pc.inputs(name, _oracle_scene(oracle, yh, True))
        s.sc = pc.scene(general)
        s.f64 = p64.batch(s.sc, s.obj, s.elem, s.uv, s.wo, ulps=ASIDE_ULPS)
        s.orc = _oracle_scene(oracle, yh, general).point(s.obj, s.elem, s.uv, s.wo)
        s.e_ref = _errors(s, s.orc)
        _CACHE[key] = s
    return _CACHE[key]


def _errors(s, out):
    e = {}
    for q in QUANTITIES:
        c = p64.COLS[q]
        keep = _finite_rows(s.f64.out[:, c]) & _finite_rows(s.orc[:, c]) & ~s.f64.aside
        e[q] = _stat(_row_err(s.sc, q, out[keep][:, c], s.f64.out[keep][:, c]))
    return e


def _fmt(e):
    return "  ".join(f"{q} {a:.2e} {b:.2e}" for q, (a, b) in e.items())


def _plain_rows(s):
    """Rows whose material is plain (host/scene_upload.cpp: make_material, scene_materials): no lobe beyond diffuse / hair, no texture, no map."""
    m = [s.sc.materials[s.sc.objects[int(o)]["material"]] for o in s.obj]
    mp = [s.sc.maps[s.sc.objects[int(o)]["material"]] for o in s.obj]
    return np.array([a["specular"] == 0 and a["metallic"] == 0 and a["transmission"] == 0 and a["opacity"] == 1 and not (a["color_tex"] or a["emission_tex"] or a["scattering_tex"])
                     and not (s.sc.general and any(b.values())) for a, b in zip(m, mp)])


def _decisions(s, out):
    """What bar 2 compares: flags derived from a (n, POINT_FLOATS) output alone."""
    n3, s3 = out[:, p64.COLS["normal"]], out[:, p64.COLS["shading_normal"]]
    plain_tri = ~s.f64.mapped & ~np.array([s.sc.is_lines(int(o)) for o in s.obj])
    flips = plain_tri & (n3 != 0).any(axis=1) & (s3 == -n3).all(axis=1)
    return types.SimpleNamespace(flips=flips, delta=out[:, COL["roughness"]][:, 0] == 0, opaque=out[:, COL["opacity"]][:, 0] == 1,
                                 pdf_zero=out[:, COL["pdfs"]] == 0)


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", [x[0] for x in SCENES])
@pytest.mark.parametrize("name", list(pc.STRATA))
def test_float64_restatement_is_the_oracles_function(oracle, yh, name, scene):
    s = _stratum(name, dict(SCENES)[scene], oracle, yh)
    assert s.f64.aside.mean() <= ASIDE_CAP, f"{int(s.f64.aside.sum())} rows within {ASIDE_ULPS} ulps of a threshold"
    print(f"stratum {name} {scene}: oracle against float64 (median, p99): {_fmt(s.e_ref)}")
    for q in QUANTITIES:
        assert s.e_ref[q][0] < CPU_MEDIAN, (q, s.e_ref[q])
    d = _decisions(s, s.orc)
    plain_tri = ~s.f64.mapped & ~np.array([s.sc.is_lines(int(o)) for o in s.obj])
    assert np.array_equal(d.flips, s.f64.flips & plain_tri & (s.orc[:, COL["normal"]] != 0).any(axis=1))  # away from a threshold float64 decides as float does
    with np.errstate(invalid="ignore"):
        assert np.array_equal(d.opaque, ~(s.f64.opacity <= float(F(0.999))))


def test_strata_reach_the_edges_they_name(oracle, yh):
    g = lambda name: _stratum(name, True, oracle, yh)  # noqa: E731
    p = lambda name: _stratum(name, False, oracle, yh)  # noqa: E731
    sc = pc.scene(True)
    kinds = {o["frame_kind"] for o in sc.objects}
    assert kinds == {"identity", "rigid", "sheared", "mirrored"}
    assert min(np.linalg.det(o["frame"][:9].reshape(3, 3).astype(np.float64)) for o in sc.objects) < 0
    assert 200 < sum(sc.num_elements(k) for k in range(len(sc.objects))) < 1500
    assert {(t["w"], t["h"], bool(t["is_byte"])) for t in sc.textures} >= {(w, h, b) for w, h in ((1, 1), (1, 7), (5, 3), (32, 32)) for b in (False, True)}
    assert all({0, 10, 11, 255} <= set(np.unique(t["px"])) for t in sc.textures if t["is_byte"] and t["name"] in ("b1x7", "b5x3", "b32x32"))
    assert max(t["px"].max() for t in sc.textures if not t["is_byte"]) > 1 and (sc.textures[sc.tex["nm0"] - 1]["px"] == 0.5).all()
    a = g("a")
    assert len(np.unique(a.obj)) >= 20 and not np.isin(a.obj, [pc.OBJ[f] for f in pc.FRAGILE]).any()
    b = g("b")
    assert set(pc.UV_EDGES.tolist()) <= set(np.unique(b.uv).tolist()) and (b.uv[:, 0] + b.uv[:, 1] == 1).sum() > ROWS // 8
    c = g("c")
    tc = np.isin(c.obj, [pc.OBJ[f"tc{k}"] for k in range(8)])
    got = set(np.unique(c.orc[tc, COL["texcoord"]]).tolist())
    assert set(pc.TC_VALUES.tolist()) <= got, sorted(set(pc.TC_VALUES.tolist()) - got)  # the table's values arrive exactly, -0 and 1e6 among them
    assert len(np.unique(c.obj[tc])) == 8 and (~tc).sum() > ROWS // 8
    tu = c.orc[:, COL["texcoord"]][:, 0]
    tiny = (tu < 0) & (tu > -7e-8)
    assert tiny.sum() >= 8  # s + sx rounds to sx there
    d = g("d")
    cancel = d.case < 2
    assert ((d.orc[cancel, COL["normal"]] == 0).all(axis=1)).sum() >= 8 and (np.abs(d.f64.out[cancel, COL["normal"]]).max(axis=1) > 0.9).sum() > 20
    zero_area = np.isin(d.case, (6, 7))
    assert (d.orc[zero_area & (d.obj == pc.OBJ["bare"])][:, COL["normal"]] == 0).all() and zero_area.sum() > ROWS // 8
    e = g("e")
    assert (e.f64.dot_no == 0).sum() >= 40 and np.signbit(e.wo[e.f64.dot_no == 0]).any()
    axis = e.obj == pc.OBJ["axis"]
    assert ((e.orc[axis, COL["shading_normal"]] == 0).all(axis=1)).sum() >= 8  # outgoing parallel to the tangent: orthonormalize gives 0
    length = np.linalg.norm(e.wo.astype(np.float64), axis=1)
    assert (np.abs(length - 0.5) < 1e-3).sum() > ROWS // 5 and (np.abs(length - 3) < 1e-3).sum() > ROWS // 5
    tri = ~np.array([sc.is_lines(int(o)) for o in e.obj])
    thin = np.array([bool(sc.materials[sc.objects[int(o)]["material"]]["thin"]) for o in e.obj])
    facing = np.sum(e.f64.out[:, COL["normal"]] * e.wo.astype(np.float64), axis=1) >= 0
    for is_thin in (True, False):  # thin and closed, facing and facing away; only thin and away flips
        for faces in (True, False):
            rows = tri & (thin == is_thin) & (facing == faces)
            assert rows.sum() > ROWS // 20, (is_thin, faces, int(rows.sum()))
            assert e.f64.flips[rows].all() if (is_thin and not faces) else not e.f64.flips[rows].any(), (is_thin, faces)
    f = g("f")
    assert (f.f64.div == 0).sum() > ROWS // 12 and (f.f64.flip_dot < 0).sum() > ROWS // 20 and (f.f64.flip_dot > 0).sum() > ROWS // 20
    zero = f.obj == pc.OBJ["special_nm0"]
    assert (f.orc[zero, COL["shading_normal"]] == 0).all() and zero.sum() > ROWS // 8  # nm = 0 exactly: the shading normal is normalize(0) = 0
    assert f.f64.mapped.mean() > 0.6 and (f.obj == pc.OBJ["hair_nm"]).sum() > ROWS // 12 and not f.f64.mapped[f.obj == pc.OBJ["hair_nm"]].any()
    no_tc = f.obj == pc.OBJ["no_tc_nm"]  # zero tangents: the mapped normal is +-normal
    assert (np.abs(np.abs(np.sum(f.orc[no_tc, COL["normal"]] * f.orc[no_tc, COL["shading_normal"]], axis=1)) - 1) < 1e-5).all()
    s = g("g")
    op = s.f64.opacity[s.obj == pc.OBJ["opacity"]]
    assert (op > 0.999).mean() > 0.2 and (op < 0.999).mean() > 0.2 and np.abs(op - 0.999).max() < 1e-3
    assert (s.orc[s.obj == pc.OBJ["hair"], COL["opacity"]] < 1).all()
    rough = s.orc[s.obj == pc.OBJ["rough0"], COL["roughness"]]
    assert (rough == 0).sum() > 10 and (rough > 0).sum() > 10
    vol = s.obj == pc.OBJ["volume"]
    dens = s.orc[vol, COL["density"]]
    clamp = -np.log(F(0.0001)) / F(0.1)
    assert (dens != 0).any(axis=1).mean() > 0.9 and (np.abs(dens / clamp - 1) < 1e-6).any(axis=1).sum() > 20
    assert (s.orc[vol, COL["scatter"]] != 0).any(axis=1).mean() > 0.9
    # the plain scene is plain: no mixture, no texture, no map
    for name in pc.STRATA:
        q = p(name)
        textures = slice(COL["color_tex"].start, COL["scattering_tex"].stop)
        assert (q.orc[:, textures] == 1).all() and (q.orc[:, COL["weights"]][:, 3:] == 0).all() and (q.orc[:, COL["roughness"]] == 1).all()
        assert (q.orc[:, COL["opacity"]] == 1).all() and (q.orc[:, COL["density"].start:] == 0).all()


def test_golden_fixture_is_small():
    """tests/golden/points_unit.npz (oracle/make_golden.py; its rows are compared bit for bit in tests/test_oracle_golden.py) stays within
    the size of a committed file."""
    import os
    from conftest import GOLD
    assert os.path.getsize(os.path.join(GOLD, "points_unit.npz")) < 1 << 20


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
_DEV = {}
_UPLOADED = [None]


def _upload(ctx, yh, general):
    if _UPLOADED[0] != (id(ctx), general):
        ctx.upload_scene(*pc.scene(general).desc(yh))
        _UPLOADED[0] = (id(ctx), general)


def _device(ctx, yh, s, general, form):
    key = (s.name, general, form)
    if key not in _DEV:
        _upload(ctx, yh, general)
        _DEV[key] = ctx.point(form, s.obj, s.elem, s.uv, s.wo)
    return _DEV[key]


@pytest.mark.gpu
def test_the_scenes_run_the_variants_they_are_meant_for(ctx, yh):
    rays = pc.rays(1, 64)
    _upload(ctx, yh, False)
    ctx.intersect_plain(0, rays)  # a plain scene: form 0 reads its rows from LDS and fetches the record first
    _upload(ctx, yh, True)
    with pytest.raises(yh.YhError):
        ctx.intersect_plain(0, rays)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", [x[0] for x in SCENES])
@pytest.mark.parametrize("name", list(pc.STRATA))
def test_forms_agree_bit_for_bit(ctx, yh, oracle, name, scene):
    general = dict(SCENES)[scene]
    s = _stratum(name, general, oracle, yh)
    plain = _plain_rows(s)

    def canonical(out):  # (bar 1: the sign of a zero metal pdf on a plain row)
        out = out.copy()
        pdf = out[plain, METAL_PDF]
        out[plain, METAL_PDF] = np.where(pdf == 0, F(0), pdf)
        return out

    # the one sign bar 1 leaves out is the reference's: form 2's mixture carries -0 exactly where the oracle's does
    minus = lambda a: (a[:, METAL_PDF] == 0) & np.signbit(a[:, METAL_PDF])  # noqa: E731
    shade = _device(ctx, yh, s, general, 2)
    assert np.array_equal(minus(shade), minus(s.orc)) and not minus(_device(ctx, yh, s, general, 0))[plain].any()
    print(f"stratum {name} {scene}: metal pdf -0 on {int(minus(s.orc).sum())} rows of the oracle and of form 2 ({int((minus(s.orc) & plain).sum())} of them plain rows: objects "
          f"{np.unique(s.obj[minus(s.orc) & plain]).tolist()}); -0 in no other lobe column: {not ((s.orc[:, COL['weights'].start:COL['pdfs'].stop] == 0) & np.signbit(s.orc[:, COL['weights'].start:COL['pdfs'].stop]))[:, [c for c in range(22) if c != METAL_PDF - COL['weights'].start]].any()}")
    base = canonical(_device(ctx, yh, s, general, 0))
    for form in (1, 2):
        out = canonical(_device(ctx, yh, s, general, form))
        differ = np.flatnonzero((base.view(np.uint32) != out.view(np.uint32)).any(axis=1))
        cols = np.flatnonzero((base.view(np.uint32) != out.view(np.uint32)).any(axis=0))
        assert len(differ) == 0, f"form {form}: {len(differ)} rows differ from form 0's in columns {cols}, first rows {differ[:5]} (objects {s.obj[differ[:5]]})"


@pytest.mark.gpu
@pytest.mark.parametrize("form", [f[0] for f in FORMS])
@pytest.mark.parametrize("scene", [x[0] for x in SCENES])
@pytest.mark.parametrize("name", list(pc.STRATA))
def test_decisions_are_the_oracles(ctx, yh, oracle, name, scene, form):
    general = dict(SCENES)[scene]
    s = _stratum(name, general, oracle, yh)
    out = _device(ctx, yh, s, general, dict(FORMS)[form])
    no_tc = np.array([s.sc.shapes[s.sc.objects[int(o)]["shape"]]["tc"] is None for o in s.obj])
    assert _same_bits(out[no_tc][:, COL["texcoord"]], s.orc[no_tc][:, COL["texcoord"]]) and _same_bits(out[no_tc][:, COL["texcoord"]], s.uv[no_tc]), "texcoord of a shape without texcoords"
    plain = _plain_rows(s)  # (strata c, f and g of the general scene have none)
    assert _same_bits(out[plain][:, COL["emission"]], s.orc[plain][:, COL["emission"]]), "emission of an untextured plain material"
    diffuse = slice(COL["weights"].start, COL["weights"].start + 3)
    assert _same_bits(out[plain][:, diffuse], s.orc[plain][:, diffuse]), "diffuse weight of an untextured plain material"
    got, want = _decisions(s, out), _decisions(s, s.orc)
    for what in ("flips", "delta", "opaque", "pdf_zero"):
        a, b = getattr(got, what), getattr(want, what)
        rows = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
        assert len(rows) == 0, f"{what}: rows {rows[:5]} (objects {s.obj[rows[:5]]}) decide otherwise than the oracle"
    bad = np.flatnonzero((np.isfinite(out) != np.isfinite(s.orc)).any(axis=1))
    print(f"stratum {name} {scene} {form}: {int((~np.isfinite(s.orc)).any(axis=1).sum())} of {s.n} rows non-finite in the oracle, {len(bad)} rows with another mask; "
          f"flips {int(want.flips.sum())} delta {int(want.delta.sum())} opacity 1 on {int(want.opaque.sum())}")
    assert len(bad) == 0, (bad[:5], s.obj[bad[:5]])


def _compared(s, q):
    """The rows of quantity q that are compared with a reference: the texcoord only where the loop evaluates it."""
    return s.f64.uses_texcoord if q == "texcoord" else np.ones(s.n, bool)


@pytest.mark.gpu
@pytest.mark.parametrize("form", [f[0] for f in FORMS])
@pytest.mark.parametrize("scene", [x[0] for x in SCENES])
def test_stated_bars_hold_on_todays_domain(ctx, yh, oracle, scene, form):
    general = dict(SCENES)[scene]
    s = _stratum("a", general, oracle, yh)
    out = _device(ctx, yh, s, general, dict(FORMS)[form])
    fig = {}
    for q in QUANTITIES:
        c = p64.COLS[q]
        keep = _finite_rows(s.orc[:, c]) & _compared(s, q)
        fig[q] = float(np.max(_row_err(s.sc, q, out[keep][:, c], s.orc[keep][:, c]))) if keep.any() else 0.0
    print(f"stratum a {scene} {form}: largest difference from the oracle: " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    for q in QUANTITIES:
        assert fig[q] <= (ABS_DIR if q in ABSOLUTE else REL_BSDF), (q, fig[q])


@pytest.mark.gpu
@pytest.mark.parametrize("form", [f[0] for f in FORMS])
@pytest.mark.parametrize("scene", [x[0] for x in SCENES])
@pytest.mark.parametrize("name", list(pc.STRATA))
def test_error_against_float64_is_the_references_own(ctx, yh, oracle, name, scene, form):
    general = dict(SCENES)[scene]
    s = _stratum(name, general, oracle, yh)
    assert s.f64.aside.mean() <= ASIDE_CAP  # on the inputs, before the device is looked at
    out = _device(ctx, yh, s, general, dict(FORMS)[form])
    e_dev, e_ref = {}, {}
    for q in QUANTITIES:
        c = p64.COLS[q]
        keep = _finite_rows(s.f64.out[:, c]) & _finite_rows(s.orc[:, c]) & ~s.f64.aside & _compared(s, q)
        e_dev[q] = _stat(_row_err(s.sc, q, out[keep][:, c], s.f64.out[keep][:, c]))
        e_ref[q] = _stat(_row_err(s.sc, q, s.orc[keep][:, c], s.f64.out[keep][:, c]))
    print(f"stratum {name} {scene} {form} (median, p99 | reference's):  "
          + "  ".join(f"{q} {e_dev[q][0]:.2e} {e_dev[q][1]:.2e} | {e_ref[q][0]:.2e} {e_ref[q][1]:.2e}" for q in QUANTITIES)
          + f"  (set aside {int(s.f64.aside.sum())} rows)")
    if name == "a":
        return  # stratum a is held to the stated bars (test_stated_bars_hold_on_todays_domain); its figures are printed for the table
    bad = [(q, i, e_dev[q][i], e_ref[q][i]) for q in QUANTITIES for i in (0, 1) if not e_dev[q][i] <= K_BAR * max(e_ref[q][i], E_FLOOR)]
    assert not bad, f"(quantity, 0 median / 1 p99, device, reference) beyond {K_BAR} x max(reference, {E_FLOOR}): {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("form", [f[0] for f in FORMS])
@pytest.mark.parametrize("scene", [x[0] for x in SCENES])
def test_batch_shape_does_not_change_a_row(ctx, yh, oracle, scene, form):
    general = dict(SCENES)[scene]
    s = _stratum("g", general, oracle, yh)
    whole = _device(ctx, yh, s, general, dict(FORMS)[form])
    _upload(ctx, yh, general)
    for n in (1, 3, 4097):  # one row, a ragged quad, a ragged last block (the stratum's rows again from the top)
        k = np.arange(n) % ROWS
        part = ctx.point(dict(FORMS)[form], s.obj[k], s.elem[k], s.uv[k], s.wo[k])
        assert _same_bits(part, whole[k]), n


@pytest.mark.gpu
def test_refusals(ctx, yh, oracle):
    s = _stratum("a", True, oracle, yh)
    n = 8
    obj, elem, uv, wo = (np.ascontiguousarray(x[:n]) for x in (s.obj, s.elem, s.uv, s.wo))
    out = np.full((n, yh.POINT_FLOATS), 7, F)
    call = ctx.lib.yh_point_batch
    ptrs = [yh.iptr(obj), yh.iptr(elem), yh.fptr(uv), yh.fptr(wo), yh.fptr(out)]
    fresh = yh.Context(0)
    try:
        assert call(fresh.h, 0, n, *ptrs) == yh.YH_E_STATE and b"before yh_upload_scene" in fresh.lib.yh_last_error(fresh.h)
    finally:
        fresh.close()
    _upload(ctx, yh, True)
    for form in (0, 1, 2):
        out[:] = 7
        assert call(ctx.h, form, n, *ptrs) == yh.YH_OK and not (out == 7).all(axis=1).any()
    for form in (3, -1):
        assert call(ctx.h, form, n, *ptrs) == yh.YH_E_INVALID
    for bad_n in (0, -1):
        assert call(ctx.h, 0, bad_n, *ptrs) == yh.YH_E_INVALID
    assert call(None, 0, n, *ptrs) == yh.YH_E_INVALID
    for k in range(len(ptrs)):
        assert call(ctx.h, 0, n, *[None if i == k else p for i, p in enumerate(ptrs)]) == yh.YH_E_INVALID
    sc = pc.scene(True)
    for row, (o, e) in ((0, (len(sc.objects), 0)), (n - 1, (-1, 0)), (3, (int(obj[3]), sc.num_elements(int(obj[3])))), (5, (int(obj[5]), -1)), (2, (2 ** 30, 2 ** 30))):
        bo, be = obj.copy(), elem.copy()
        bo[row], be[row] = o, e
        out[:] = 7
        assert call(ctx.h, 0, n, yh.iptr(bo), yh.iptr(be), *ptrs[2:]) == yh.YH_E_INVALID and f"row {row} ".encode() in ctx.lib.yh_last_error(ctx.h)
        assert (out == 7).all()  # found before anything follows the index: nothing ran
    # ... and each refusal leaves a usable context
    assert _same_bits(ctx.point(0, obj, elem, uv, wo), _device(ctx, yh, s, True, 0)[:n])
