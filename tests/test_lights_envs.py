"""Lights and environments at unit level and at their edges: sample_lights, sample_lights_pdf and eval_environment
(csrc/dev_path.h; pt.cpp:536-547, 1283-1358) and the light / environment tables of host/scene_upload.cpp, through
yh_lights_batch (the integrators' own functions, form 0 = a quad per row, form 1 = a lane per row) against the oracle's
(yo_scene_lights_batch), and as images. The oracle is pinned to the reference on six of these scenes bit for bit
(tests/ref_cases.py: IMAGE_CASES).

Scenes (tools/make_scenes.py: make_envs_unit): a rotated sky, a sky placed with "lookat", four environments (one of them
no light, so light.environment != the environment's index; two textured ones, so texel_base and cdf_base are non-zero),
png environments of 65x63 (4095 texels: the cdf is searched through memory), 64x64 (4096: LDS index of stride 2), 65x64
(stride 3, 1387 entries, a last block of 2), 16x8 and 1x1, all with black rows (a flat cdf), and single emitters of 1, 3,
4 and 5 triangles around YH_SMALL_LIGHT_TRIS = 4 (4 has a triangle without area).

Bars (none of them taken from what the device gives):
  * directions sampled from area lights: bit for bit (+ - x / sqrt only, -ffp-contract=off);
  * directions sampled from environments: ABS_DIR (5e-5, the project's bar for directions through device sin / cos);
  * pdfs: REL_BSDF (1e-4) with a floor of 1e-7, non-finite values non-finite on both sides (_lobe_close). The pdf at the
    SAMPLED direction is compared with the oracle's pdf at the direction the device sampled. A row is left out of a pdf
    comparison only when the ORACLE ALONE puts the direction into another texel of a textured environment light after
    moving any of its components by +-4 ulp (26 moves); on the random rows that share must stay <= 1 %. The texel-edge
    rows (poles, seam, texel corners; their positions are far outside, so no area light is on the ray) accept either
    neighbouring texel's value, each taken from the oracle: its pdf at those 27 directions and at the eight directions
    1e-5 rad away in the map's own coordinates;
  * eval_environment: rel 1e-3 on >= 99 % of the rows (the bar of test_images_match_reference_statistically for escaping
    pixels); the two forms bit for bit;
  * images: the bars of test_light_sampling_matches_oracle_at_unit_level.

MEASURED (2026-10-17, AMD Instinct MI355X, gfx950; thirteen unit scenes x 4096 rows, both forms, which agree bit for bit):
  * directions from area lights: no row differs; from environments: at most 1.49e-7 (lookat; bar 5e-5);
  * pdf at the sampled direction: at most 2.65e-7 relative (multi; bar 1e-4); rows left out by the texel rule: 0.049 % (lookat),
    0.024 % (rot), none elsewhere;
  * pdf at the given direction: at most 2.54e-7 relative (tex-65x63); random rows left out: 0.025 % (rot), 0.026 % (multi), none
    elsewhere (bar 1 %; the same figures by the oracle alone on the CPU); of the texel-edge rows 0-11 per scene take a neighbouring
    texel's value (multi 11, tex-65x64 10; one row of rot, ty x height = 340.9999975, takes the texel the oracle reaches only
    through the 1e-5 rad directions);
  * eval_environment within 1e-3 on 100 % of the rows of every scene; no row is non-finite on either side;
  * images: RNG states equal and pixels within 1e-3 on 100 % of the pixels of all twelve scenes at bounces 2 and 8.
The 32 GPU tests take 4.6 s together.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from conftest import scene_path
from test_gpu_parity import ABS_DIR, REL_BSDF, _lobe_close, _rel

VARIANTS = ("rot", "lookat", "multi", "tex-65x63", "tex-64x64", "tex-65x64", "tex-16x8", "tex-1x1",
            "lights-1", "lights-3", "lights-4", "lights-5")
ENV_SCENES = [("envs-unit", dict(scale=0.05, variant=v)) for v in VARIANTS]
UNIT_SCENES = ENV_SCENES + [("lights-unit", dict(scale=0.05, biglight=True))]  # (an 18-triangle light under the identity-frame sky)
IDS = [kw.get("variant", "lights-unit-biglight") for _, kw in UNIT_SCENES]
ROWS = 4096
F = np.float32
BELOW1 = np.nextafter(F(1), F(0))  # the largest float below 1
MOVES = [m for m in itertools.product((0, -4, 4), repeat=3)]  # MOVES[0] = no move
EXCLUDED_MAX = 0.01
RANDOM, LIGHT_GEOMETRY, TEXEL_EDGE = 0, 1, 2  # classes of rows by their position / direction


def _ulps(a, k):
    a = np.array(a, F)
    for _ in range(abs(k)):
        a = np.nextafter(a, F(np.inf if k > 0 else -np.inf))
    return a


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _light_list(desc, osc):
    """The scene's lights in the oracle's order: dicts with the cdf and, for an area light, world vertices + triangles,
    for an environment its frame rows (x, y, z) and map size."""
    d, out = desc.contents, []
    for k in range(osc.num_lights()):
        obj, env, cdf = osc.light(k)
        L = dict(cdf=cdf, object=obj, environment=env)
        if obj >= 0:
            o = d.objects[obj]
            sh = d.shapes[o.shape]
            fr = np.array(o.frame[:], np.float64).reshape(4, 3)
            pos = np.ctypeslib.as_array(sh.positions, (sh.num_vertices * 3,)).reshape(-1, 3).astype(np.float64)
            L["verts"] = pos @ fr[:3] + fr[3]
            L["tris"] = np.ctypeslib.as_array(sh.triangles, (sh.num_triangles * 3,)).reshape(-1, 3).copy()
        else:
            e = d.environments[env]
            L["frame"] = np.array(e.frame[:], np.float64).reshape(4, 3)[:3]
            L["w"], L["h"] = (e.tex_width, e.tex_height) if e.texels else (0, 0)
        out.append(L)
    return out


def _rel_for_entry(cdf, idx):
    """rel values whose product with the cdf's last entry IS cdf[idx] in float arithmetic (sample_discrete_cdf's r lands
    on the entry), with their neighbours one ulp either side."""
    back, c = cdf[-1], cdf[idx]
    if not back > 0:
        return [F(0)]
    r0 = F(c) / F(back)
    cands = [_ulps(r0, k) for k in range(-3, 4)]
    on = [r for r in cands if F(r * back) == c and 0 <= r < 1]
    on = on[:1] or [np.clip(r0, F(0), BELOW1)]
    return [np.clip(v, F(0), BELOW1) for r in on for v in (r, _ulps(r, -1), _ulps(r, 1))]


def _cdf_entries(cdf, rng):
    m = len(cdf)
    idx = [0, 1, 2, m - 2, m - 1]
    ties = np.flatnonzero(np.diff(cdf) == 0) + 1  # entries equal to the one before: black texels, a triangle without area
    if len(ties):
        idx += list(ties[:3]) + list(ties[-3:]) + [ties[len(ties) // 2], ties[-1] + 1]
    hot = int(np.argmax(np.diff(cdf, prepend=F(0))))
    idx += [hot - 1, hot, hot + 1]
    if m >= 4096:  # the LDS index of scene_upload.cpp: blocks of S entries, the last one partial
        S = (m + 2047) // 2048
        K = (m + S - 1) // S
        for b in (1, 2, K // 2, K - 1):
            idx += [b * S - 1, b * S, b * S + 1]
        idx += [(K - 1) * S, m - 1]
    idx += list(rng.integers(0, m, 24))
    return sorted(set(int(np.clip(i, 0, m - 1)) for i in idx))


def _inputs(desc, osc, seed=17):
    """ROWS rows of (position, direction, rn) and their class: the issue's edge rows first, random rows after them."""
    rng = np.random.default_rng(seed)
    lights = _light_list(desc, osc)
    n = len(lights)
    P = (rng.uniform(-1, 1, (ROWS, 3)) * [3, 2, 3] + [0, 2.05, 0]).astype(F)
    D = _unit(rng.normal(size=(ROWS, 3))).astype(F)
    RN = rng.uniform(0, 1, (ROWS, 4)).astype(F)
    RN = np.minimum(RN, BELOW1)
    cls = np.zeros(ROWS, np.int32)
    edge_light = np.full(ROWS, -1, np.int32)  # a texel-edge row: the environment light whose map it is an edge of
    # ---- random numbers (on rows whose position and direction stay random) ----
    rn_rows = []
    for rl in [F(0), BELOW1] + [F(k) / F(n) for k in range(1, n)] + [_ulps(F(k) / F(n), -1) for k in range(1, n)]:
        rn_rows += [(rl, None, None, None), (rl, F(0), F(0), F(0)), (rl, BELOW1, BELOW1, BELOW1)]
    corners = [(F(0), F(0)), (BELOW1, BELOW1), (F(0), BELOW1), (BELOW1, F(0)), (None, None)]
    for k, L in enumerate(lights):
        rl = (F(k) + F(0.5)) / F(n)
        rels = [F(0), BELOW1]
        if len(L["cdf"]):
            for i in _cdf_entries(L["cdf"], rng):
                rels += _rel_for_entry(L["cdf"], i)
        for j, rel in enumerate(rels):
            rn_rows.append((rl, rel) + corners[j % len(corners)])
        rn_rows += [(rl, None) + c for c in corners[:4]]
    assert len(rn_rows) < ROWS // 2
    for i, row in enumerate(rn_rows):
        for c, v in enumerate(row):
            if v is not None:
                RN[i, c] = v
    # ---- positions and directions, from the end of the batch ----
    at = [ROWS]

    def put(p, d, c):
        at[0] -= 1
        P[at[0]], D[at[0]], cls[at[0]] = np.asarray(p, np.float64).astype(F), np.asarray(d, np.float64).astype(F), c

    for k, L in enumerate(lights):
        if L["environment"] >= 0 and L["w"]:
            W, H, M = L["w"], L["h"], L["frame"]
            local = [(0, 1, 0), (0, -1, 0), (1e-9, 1, 0), (0, -1, -1e-9)]  # the poles of the lat-long map
            for y in (0.0, 0.3, -0.8):  # its seam (atan2 = +-pi) and the tx < 0 wrap at +x
                local += [(-1, y, 0.0), (-1, y, -0.0), (-1, y, 1e-12), (-1, y, -1e-12), (1, y, 0.0), (1, y, -0.0), (1, y, -1e-12)]
            hot = int(np.argmax(np.diff(L["cdf"], prepend=F(0))))
            ij = [(i, j) for i in (0, 1, W // 2, W - 1, W) for j in (0, 1, H // 3, H - 1, H)]
            ij += [(hot % W + a, hot // W + b) for a in (0, 1) for b in (0, 1)]
            ij += [(int(rng.integers(0, W + 1)), int(rng.integers(0, H + 1))) for _ in range(16)]
            for i, j in ij:  # directions through texel corners
                tx, ty = 2 * np.pi * i / W, np.pi * j / H
                local.append((np.cos(tx) * np.sin(ty), np.cos(ty), np.sin(tx) * np.sin(ty)))
            for v in local:
                w = np.asarray(v, np.float64) @ M
                w = w / np.linalg.norm(w)
                if np.allclose(M, np.eye(3)):  # (an identity frame keeps the signed zeros of the local direction)
                    w = np.asarray(v, np.float64) / np.linalg.norm(v)
                put(1000 * w, w, TEXEL_EDGE)
                edge_light[at[0]] = k
    area = [L for L in lights if L["object"] >= 0]
    for L in area:
        V, T = L["verts"], L["tris"]
        cross = np.cross(V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]])
        t0 = int(np.argmax(np.linalg.norm(cross, axis=1)))
        nrm, ctr = _unit(cross[t0]), V[np.unique(T)].mean(axis=0)
        a, b, c = V[T[t0]]
        for s, t in ((0.3, 0.3), (1.5, -0.2), (-0.5, 0.5), (0.5, 0.5)):  # on the light's plane: inside, outside, on an edge
            p = a + s * (b - a) + t * (c - a)
            put(p, _unit(rng.normal(size=3)), LIGHT_GEOMETRY), put(p, _unit(b - a), LIGHT_GEOMETRY)  # ... and along the plane (grazing)
            put(p, nrm, LIGHT_GEOMETRY), put(p, -nrm, LIGHT_GEOMETRY)
        for side in (0.7, -0.7, 3.0, -3.0):  # in front of it and behind it
            p = ctr + side * nrm
            put(p, _unit(ctr - p), LIGHT_GEOMETRY), put(p, _unit(rng.normal(size=3)), LIGHT_GEOMETRY)
        edges = {}
        for tri in T:
            for e in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
                edges.setdefault(tuple(sorted(e)), []).append(1)
        shared = [e for e, c in edges.items() if len(c) > 1] or list(edges)
        for e in shared[:3]:  # through the edge two triangles share, and through its end
            for t in (0.5, 0.25, 0.0):
                target = V[e[0]] + t * (V[e[1]] - V[e[0]])
                for p in (rng.uniform(-2, 2, 3) * [1, 0, 1] + [0, 0.05, 0], ctr + 1.5 * nrm + rng.uniform(-1, 1, 3)):
                    put(p, _unit(target - p), LIGHT_GEOMETRY)
    if len(area) >= 2:  # on the line through both stacked lights: the pdf walk crosses both
        c1, c2 = (L["verts"][np.unique(L["tris"])].mean(axis=0) for L in area[:2])
        for t in (-0.5, 0.5, 1.5, -2.0, 3.0):
            p = c1 + t * (c2 - c1)
            put(p, _unit(c2 - c1), LIGHT_GEOMETRY), put(p, _unit(c1 - c2), LIGHT_GEOMETRY)
    assert at[0] > len(rn_rows), "the edge rows must leave room for random ones"
    return dict(P=P, D=D, RN=RN, cls=cls, edge_light=edge_light, lights=lights, rn_rows=len(rn_rows))


def _stability(osc, P, D, RN):
    """By the oracle alone: which rows' direction lands in another texel of a textured environment light when its
    components move by +-4 ulp, and the oracle's pdf at each of the 27 directions (27, n)."""
    base = None
    unstable = np.zeros(len(D), bool)
    pdfs = []
    for m in MOVES:
        Dm = np.stack([_ulps(D[:, c], m[c]) for c in range(3)], axis=1)
        out, tex = osc.lights(P, Dm, RN, want_texels=True)
        pdfs.append(out[:, 4])
        if base is None:
            base = tex
        unstable |= (tex != base).any(axis=1)
    return unstable, np.stack(pdfs)


NUDGE = 1e-5  # radians: far above the rounding of a float direction (1e-7), far below a texel of the largest map (3e-3)


def _edge_neighbours(osc, inp):
    """The oracle's pdf for each texel-edge row at the eight directions NUDGE away in the map's own (tx, ty): the values of
    the texels that meet at the edge, each taken from the oracle (8, n); rows of another class keep NaN."""
    out = np.full((8, ROWS), np.nan, F)
    for k, L in enumerate(inp["lights"]):
        rows = np.flatnonzero(inp["edge_light"] == k)
        if not len(rows):
            continue
        local = _unit(inp["D"][rows].astype(np.float64) @ L["frame"].T)
        tx, ty = np.arctan2(local[:, 2], local[:, 0]), np.arccos(np.clip(local[:, 1], -1, 1))
        steps = [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1) if a or b]
        for m, (a, b) in enumerate(steps):
            x, y = tx + a * NUDGE, ty + b * NUDGE
            w = np.stack([np.cos(x) * np.sin(y), np.cos(y), np.sin(x) * np.sin(y)], axis=1) @ L["frame"]
            out[m, rows] = osc.lights(inp["P"][rows], w.astype(F), inp["RN"][rows])[:, 4]
    return out


class _Reference:
    """A scene, its oracle, the inputs and everything the oracle says about them: computed once, shared, never changed."""

    def __init__(self, yh, oracle, name, kw):
        self.sf = yh.SceneFile(scene_path(name, **kw))
        self.desc = self.sf.desc
        self.osc = oracle.scene(self.desc)
        self.inp = _inputs(self.desc, self.osc)
        i = self.inp
        self.base = self.osc.lights(i["P"], i["D"], i["RN"])
        self.unstable, self.alts = _stability(self.osc, i["P"], i["D"], i["RN"])
        self.alts = np.concatenate([self.alts, _edge_neighbours(self.osc, i)])
        n = len(i["lights"])
        pick = np.clip((i["RN"][:, 0] * F(n)).astype(np.int32), 0, n - 1)  # sample_lights: the light of a row
        self.area_row = np.array([i["lights"][k]["object"] >= 0 for k in pick])
        for a in (self.base, self.unstable, self.alts, self.area_row, i["P"], i["D"], i["RN"], i["cls"]):
            a.setflags(write=False)


_REFS = {}


def _reference(yh, oracle, name, kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _REFS:
        _REFS[key] = _Reference(yh, oracle, name, kw)
    return _REFS[key]


def _pdf_ok(got, want):
    """_lobe_close on one column of pdfs: within REL_BSDF (floor 1e-7), or non-finite on both sides."""
    g, w = np.zeros((len(got), 7), F), np.zeros((len(got), 7), F)
    g[:, 3], w[:, 3] = got, want
    nonfinite = ~np.isfinite(got) & ~np.isfinite(want)
    return _lobe_close(g, w)[1] | nonfinite


def _worst_rel(got, want, rows):
    ok = rows & np.isfinite(got) & np.isfinite(want)
    return float(np.max(_rel(got[ok], want[ok], 1e-7))) if ok.any() else 0.0


# ---------------------------------------------------------------------------------------------
# CPU: the loader, and the oracle on the edge inputs
# ---------------------------------------------------------------------------------------------
def test_environment_lookat_and_frames_load_as_the_reader_says(yh):
    """An environment's "lookat" gives lookat_frame(eye, center, up) with x and z negated (scene_io.cpp: the inv_xz variant;
    the frame the reference-pinned render of this scene implies) and overrides a "frame" next to it; a "frame" alone is
    taken as it stands; environments load in name order, a textured one with emission 0 included."""
    import make_scenes
    eye, ctr, up = (np.array(make_scenes.ENV_LOOKAT[k:k + 3], F) for k in (0, 3, 6))
    nz = lambda v: (v / np.sqrt(np.dot(v, v))).astype(F)  # noqa: E731
    w = nz(eye - ctr)
    u = nz(np.cross(up, w).astype(F))
    v = nz(np.cross(w, u).astype(F))
    want = np.concatenate([-u, v, -w, eye])
    sf = yh.SceneFile(scene_path("envs-unit", scale=0.05, variant="lookat"))  # ("frame": ENV_ROT and "lookat" together)
    d = sf.desc.contents
    assert d.num_environments == 1
    got = np.array(d.environments[0].frame[:], F)
    assert np.allclose(got, want, rtol=0, atol=2e-7), (got, want)
    assert not np.allclose(got[:9], np.array(make_scenes.ENV_ROT[:9], F), atol=1e-2), "lookat must override frame"
    assert (d.environments[0].tex_width, d.environments[0].tex_height) == (2048, 1024)
    sf.close()
    sf = yh.SceneFile(scene_path("envs-unit", scale=0.05, variant="rot"))
    assert np.array_equal(np.array(sf.desc.contents.environments[0].frame[:], F), np.array(make_scenes.ENV_ROT, F))
    sf.close()
    sf = yh.SceneFile(scene_path("envs-unit", scale=0.05, variant="multi"))
    d = sf.desc.contents
    assert d.num_environments == 4
    e = [d.environments[k] for k in range(4)]
    assert [(x.tex_width, x.tex_height) for x in e] == [(0, 0), (67, 63), (2048, 1024), (67, 63)]
    assert [tuple(x.emission[:]) for x in e] == [(F(0.3), F(0.4), F(0.5)), (0, 0, 0), (1.5, 1.5, 1.5), (2, 2, 2)]
    assert np.array_equal(np.array(e[3].frame[:], F), np.array(make_scenes.ENV_ROT_SMALL, F))
    px = np.ctypeslib.as_array(e[3].texels, (63 * 67 * 3,)).reshape(63, 67, 3)
    assert not px[:21].any() and px[21:].min() > 0 and px.max() == 1.0  # 8-bit texels through srgb_to_rgb: black rows, one texel at 255
    sf.close()


LIGHT_COUNTS = {"rot": 3, "lookat": 3, "multi": 5, "tex-65x63": 3, "tex-64x64": 3, "tex-65x64": 3, "tex-16x8": 3, "tex-1x1": 3,
                "lights-1": 2, "lights-3": 2, "lights-4": 2, "lights-5": 2, "lights-unit-biglight": 3}


@pytest.mark.parametrize("name,kw", UNIT_SCENES, ids=IDS)
def test_oracle_on_the_edge_inputs(yh, oracle, name, kw):
    """The reference side of the GPU tests on its own: the lights the oracle makes of each scene, no NaN in what it says about
    the edge inputs (a direction that grazes a light's plane gives an infinite pdf at most, the documented non-finite rows),
    the rows the texel rule leaves out of the pdf comparison (<= 1 % of the random rows), and the inputs themselves."""
    ref = _reference(yh, oracle, name, kw)
    i, tag = ref.inp, kw.get("variant", "lights-unit-biglight")
    assert len(i["lights"]) == LIGHT_COUNTS[tag]
    assert (i["cls"] == TEXEL_EDGE).sum() + (i["cls"] == LIGHT_GEOMETRY).sum() + i["rn_rows"] < ROWS * 3 // 4
    assert np.all(i["RN"] < 1) and np.all(i["RN"] >= 0)
    assert not np.isnan(ref.base).any(), np.flatnonzero(np.isnan(ref.base).any(axis=1))
    assert np.isfinite(ref.base[:, [0, 1, 2, 5, 6, 7]]).all()
    inf_rows = ~np.isfinite(ref.base[:, 3:5]).all(axis=1)
    assert not inf_rows[i["cls"] != LIGHT_GEOMETRY].any(), "only a ray along a light's plane may have an infinite pdf"
    random = i["cls"] == RANDOM
    share = float(ref.unstable[random].mean())
    print(f"{tag}: excluded share of the {random.sum()} random rows {share:.4%}, infinite-pdf rows {int(inf_rows.sum())}")
    assert share <= EXCLUDED_MAX
    textured = [L for L in i["lights"] if L["environment"] >= 0 and L["w"]]
    if tag == "multi":  # the second textured environment light: environment 3 behind a skipped one, its cdf behind the sky's
        assert [(L["environment"], len(L["cdf"])) for L in textured] == [(2, 2048 * 1024), (3, 67 * 63)]
    for L in textured:
        if L["w"] * L["h"] > 2:
            assert (np.diff(L["cdf"]) == 0).any() == (L["h"] >= 3), "black rows make a flat stretch of the cdf"
    if tag == "lights-4":
        assert (np.diff(i["lights"][0]["cdf"]) == 0).sum() == 1, "one triangle without area"


# ---------------------------------------------------------------------------------------------
# GPU: the unit batch
# ---------------------------------------------------------------------------------------------
def _check_batch(ref, got, label):
    """Holds one form's (n, 8) output to the oracle; returns the measured figures."""
    i, base, osc = ref.inp, ref.base, ref.osc
    cls = i["cls"]
    fig = {}
    # sampled directions: area lights bit for bit, environments within ABS_DIR
    w_got, w_ref = got[:, :3], base[:, :3]
    same = ((w_got == w_ref) | (np.isnan(w_got) & np.isnan(w_ref))).all(axis=1)
    g7, r7 = np.zeros((len(got), 7), F), np.zeros((len(got), 7), F)
    g7[:, 4:], r7[:, 4:] = w_got, w_ref
    close = _lobe_close(g7, r7)[2]
    env_row = ~ref.area_row
    with np.errstate(invalid="ignore"):
        fig["dir_env_max_abs"] = float(np.nanmax(np.abs(w_got - w_ref)[env_row], initial=0.0))
    fig["dir_area_differ"] = int((~same & ref.area_row).sum())
    # pdf at the sampled direction: the oracle's pdf at the direction the device sampled, the texel rule by the oracle on it
    at_w = osc.lights(i["P"], w_got, i["RN"])[:, 4]
    unstable_w, _ = _stability(osc, i["P"], w_got, i["RN"])
    ok_w = _pdf_ok(got[:, 3], at_w)
    fig["pdf_sampled_excluded"] = float(unstable_w.mean())
    fig["pdf_sampled_max_rel"] = _worst_rel(got[:, 3], at_w, ~unstable_w)
    # pdf at the given direction
    edge = cls == TEXEL_EDGE
    ok_d = _pdf_ok(got[:, 4], base[:, 4])
    ok_edge = np.any([_pdf_ok(got[:, 4], alt) for alt in ref.alts], axis=0)
    fig["pdf_given_excluded_random"] = float(ref.unstable[cls == RANDOM].mean())
    fig["pdf_given_max_rel"] = _worst_rel(got[:, 4], base[:, 4], ~ref.unstable & ~edge)
    fig["pdf_edge_rows_off_base"] = int((edge & ~ok_d).sum())
    # eval_environment
    e_got, e_ref = got[:, 5:8], base[:, 5:8]
    e_close = ((e_got == e_ref) | (_rel(e_got, e_ref) < 1e-3)).all(axis=1)
    fig["env_share"] = float(e_close.mean())
    fig["env_share_random"] = float(e_close[cls == RANDOM].mean())
    print(label, " ".join(f"{k}={v:.3g}" for k, v in fig.items()))
    assert (same | ~ref.area_row).all(), f"{label}: directions sampled from area lights differ in rows {np.flatnonzero(~same & ref.area_row)[:8]}"
    assert close[env_row].all(), f"{label}: directions sampled from environments off by {fig['dir_env_max_abs']:.3g} (rows {np.flatnonzero(~close & env_row)[:8]})"
    assert unstable_w.mean() <= EXCLUDED_MAX
    bad = ~ok_w & ~unstable_w
    assert not bad.any(), f"{label}: pdf at the sampled direction, rows {np.flatnonzero(bad)[:8]}: {got[bad, 3][:8]} vs {at_w[bad][:8]}"
    assert ref.unstable[cls == RANDOM].mean() <= EXCLUDED_MAX
    bad = ~edge & ~ref.unstable & ~ok_d
    assert not bad.any(), f"{label}: pdf at the given direction, rows {np.flatnonzero(bad)[:8]}: {got[bad, 4][:8]} vs {base[bad, 4][:8]}"
    bad = edge & ~ok_edge
    assert not bad.any(), f"{label}: pdf on texel-edge rows {np.flatnonzero(bad)[:8]}: {got[bad, 4][:8]} is neither neighbour's value ({base[bad, 4][:8]})"
    assert e_close.mean() >= 0.99, f"{label}: eval_environment within 1e-3 on {e_close.mean():.4f} of the rows"
    return fig


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", UNIT_SCENES, ids=IDS)
def test_light_functions_match_the_oracle_row_by_row(ctx, oracle, yh, name, kw):
    """sample_lights, sample_lights_pdf (at the sampled and at a given direction) and eval_environment of the uploaded
    scene, 4096 rows, in the quad form (the plain variant with its tables in LDS; the GENERAL one, reading big lights
    through memory, for lights-5 and the 18-triangle light) and in the one-lane form of the streaming kernel: each against
    the oracle with the module's bars, and the two forms bit for bit."""
    ref = _reference(yh, oracle, name, kw)
    ctx.upload_scene(ref.desc)
    i, tag = ref.inp, kw.get("variant", "lights-unit-biglight")
    got = [ctx.lights(form, i["P"], i["D"], i["RN"]) for form in (0, 1)]
    for form in (0, 1):
        _check_batch(ref, got[form], f"{tag} form {form}:")
    differ = ~((got[0] == got[1]) | (np.isnan(got[0]) & np.isnan(got[1]))).all(axis=1)
    assert not differ.any(), f"{tag}: the quad form and the one-lane form differ in rows {np.flatnonzero(differ)[:8]}"


@pytest.mark.gpu
def test_empty_and_invalid_light_batches(ctx, yh):
    c2 = yh.Context(0)
    z3, z4, o8 = np.zeros((1, 3), F), np.zeros((1, 4), F), np.zeros((1, 8), F)
    assert c2.lib.yh_lights_batch(c2.h, 0, 1, yh.fptr(z3), yh.fptr(z3), yh.fptr(z4), yh.fptr(o8)) == yh.YH_E_STATE  # no scene yet
    assert b"before" in c2.lib.yh_last_error(c2.h)
    c2.close()
    sf = yh.SceneFile(scene_path("envs-unit", scale=0.05, variant="tex-1x1"))
    ctx.upload_scene(sf.desc)
    for form in (0, 1):
        assert ctx.lights(form, np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros((0, 4), F)).shape == (0, 8)
        assert ctx.lib.yh_lights_batch(ctx.h, form, 0, None, None, None, None) == yh.YH_OK
        assert ctx.lib.yh_lights_batch(ctx.h, form, -1, None, None, None, None) == yh.YH_E_INVALID
        assert ctx.lib.yh_lights_batch(ctx.h, form, 1, yh.fptr(z3), yh.fptr(z3), yh.fptr(z4), None) == yh.YH_E_INVALID
        assert ctx.lib.yh_lights_batch(ctx.h, form, 1, None, yh.fptr(z3), yh.fptr(z4), yh.fptr(o8)) == yh.YH_E_INVALID
        assert ctx.lib.yh_lights_batch(None, form, 1, yh.fptr(z3), yh.fptr(z3), yh.fptr(z4), yh.fptr(o8)) == yh.YH_E_INVALID
    for form in (-1, 2):
        assert ctx.lib.yh_lights_batch(ctx.h, form, 1, yh.fptr(z3), yh.fptr(z3), yh.fptr(z4), yh.fptr(o8)) == yh.YH_E_INVALID
    sf.close()


@pytest.mark.gpu
def test_a_fifth_environment_is_refused(ctx, yh):
    """The ABI holds four environments (YH_MAX_ENVS): a description with five is refused with YH_E_INVALID, one with four uploads."""
    sf = yh.SceneFile(scene_path("envs-unit", scale=0.05, variant="multi"))
    d = sf.desc.contents
    envs = (yh.Environment * 5)()
    for k in range(5):
        C.memmove(C.byref(envs[k]), C.byref(d.environments[min(k, 3)]), C.sizeof(yh.Environment))
    five = yh.SceneDesc()
    C.memmove(C.byref(five), C.byref(d), C.sizeof(yh.SceneDesc))
    five.num_environments, five.environments = 5, envs
    assert ctx.lib.yh_upload_scene(ctx.h, C.byref(five)) == yh.YH_E_INVALID
    assert b"environments" in ctx.lib.yh_last_error(ctx.h)
    five.num_environments = 4
    assert ctx.lib.yh_upload_scene(ctx.h, C.byref(five)) == yh.YH_OK
    sf.close()


# ---------------------------------------------------------------------------------------------
# GPU: images
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", ENV_SCENES, ids=IDS[:len(ENV_SCENES)])
def test_images_of_the_light_scenes_follow_the_oracle(ctx, oracle, yh, name, kw):
    """Every scene of make_envs_unit as an image, with the bars of test_light_sampling_matches_oracle_at_unit_level: diffuse-only
    paths follow the oracle draw for draw, so the RNG states agree on more than 99.5 % of the pixels and more than 99 % of
    the pixels are within 1e-3."""
    ref = _reference(yh, oracle, name, kw)
    ctx.upload_scene(ref.desc)
    for bounces, spp in ((2, 4), (8, 4)):
        p = yh.TraceParams.default(resolution=80, bounces=bounces)
        ctx.init_state(p)
        ctx.trace_samples(spp)
        img, rng = ctx.download(), ctx.download_rng()
        want, rwant = ref.osc.render(p, spp, want_rng=True)
        same_rng = float(np.mean(rng[:, 0] == rwant[:, 0]))
        close = _rel(img[..., :3], want[..., :3]).max(axis=2) < 1e-3
        print(f"{kw['variant']} bounces {bounces}: rng {same_rng:.4f} close {close.mean():.4f}")
        assert same_rng > 0.995
        assert close.mean() > 0.99, f"bounces {bounces}: {close.mean():.4f}"
        assert (want[..., 3] > 0).mean() > 0.3


SHAPE_SCENES = [("envs-unit", dict(scale=0.05, variant=v)) for v in ("multi", "tex-65x64", "lights-5")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", SHAPE_SCENES, ids=[kw["variant"] for _, kw in SHAPE_SCENES])
def test_launch_shapes_render_the_light_scenes_identically(ctx, yh, name, kw, monkeypatch):
    """As test_launch_shapes_and_kernels_render_identical_pixels: every launch shape renders the same pixels and leaves the same
    RNG states — with two textured environments (one behind the LDS index, one searched through memory), with an index whose
    last block is partial, and with a five-triangle light (the GENERAL variants)."""
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=72)
    images = {}
    for shape in ("0", "1", "3", "4", "5", "6", "7", "8"):
        monkeypatch.setenv("YHAIR_SHAPE", shape)
        ctx.init_state(p)
        ctx.trace_samples(3), ctx.trace_samples(2)
        images[shape] = (ctx.download(), ctx.download_rng())
    monkeypatch.delenv("YHAIR_SHAPE")
    base = images["0"]
    assert base[0][..., 3].max() > 0
    for k, (img, rng) in images.items():
        assert np.array_equal(img, base[0]), f"shape {k} renders different pixels"
        assert np.array_equal(rng, base[1]), f"shape {k} leaves different RNG states"
    sf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["multi", "tex-65x64"])
def test_host_and_device_uploads_render_the_light_scenes_identically(ctx, yh, variant, monkeypatch):
    """YHAIR_BVH=host and YHAIR_BVH=device (the small lights' records read back from the device) render the same pixels."""
    sf = yh.SceneFile(scene_path("envs-unit", scale=0.05, variant=variant))
    got = {}
    for mode in ("host", "device"):
        monkeypatch.setenv("YHAIR_BVH", mode)
        ctx.upload_scene(sf.desc)
        ctx.init_state(yh.TraceParams.default(resolution=64))
        ctx.trace_samples(4)
        got[mode] = (ctx.download(), ctx.download_rng())
    monkeypatch.delenv("YHAIR_BVH")
    assert got["host"][0][..., 3].max() > 0
    assert np.array_equal(got["host"][0], got["device"][0]) and np.array_equal(got["host"][1], got["device"][1])
    sf.close()
