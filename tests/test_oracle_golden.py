"""Pins the CPU oracle (oracle/yh_oracle.cpp) against golden vectors produced by the REAL
reference (oracle/make_golden.py -> tests/golden/*.npz), bit for bit: RNG streams, the hair BSDF
(brdf / eval / sample / pdf), ray-line / ray-triangle / ray-bbox tests, closest hits and whole
rendered images on small synthetic scenes. CPU only."""
import numpy as np
import pytest

from conftest import GOLDEN_SCENES, golden, scene_path, scene_tag


def test_rng_streams(oracle):
    g = golden("rng.npz")
    keys = [k[len("state_"):] for k in g.files if k.startswith("state_")]
    assert len(keys) == 5
    for k in keys:
        seed, seq = (int(x) for x in k.split("_"))
        (st, inc), fl = oracle.rng_stream(seed, seq, 64)
        assert (st, inc) == tuple(int(x) for x in g["state_" + k])
        assert np.array_equal(fl, g["floats_" + k])
    # SURVEY.md 8c sanity values (make_rng(961748941, 1))
    (st, inc), fl = oracle.rng_stream(961748941, 1, 4)
    assert st == 0xefe4fedd9474c793 and inc == 3
    assert np.allclose(fl, [0.893633127, 0.246839881, 0.458433747, 0.477094531], rtol=0, atol=1e-9)
    assert np.array_equal(oracle.pixel_seqs(64 * 64), g["pixel_seqs"])
    assert oracle.pixel_seqs(6).tolist() == [725124800, 678759815, 790335339, 839039096, 650700596, 307940000]


def test_hair_bsdf_bit_exact(oracle):
    g = golden("hair_bsdf.npz")
    brdf = oracle.hair_brdf(g["mats"], g["v"], g["normal"], g["tangent"])
    # -0.0 vs 0.0 in the frame origin is not a difference
    assert np.array_equal(brdf + 0.0, g["brdf"] + 0.0)
    assert np.array_equal(oracle.hair_eval(g["brdf"], g["wo"], g["wi"]), g["f"], equal_nan=True)
    assert np.array_equal(oracle.hair_pdf(g["brdf"], g["wo"], g["wi"]), g["pdf"], equal_nan=True)
    wis = oracle.hair_sample(g["brdf"], g["wo"], g["rn"])
    assert np.array_equal(wis, g["wi_sampled"], equal_nan=True)
    assert np.array_equal(oracle.hair_eval(g["brdf"], g["wo"], wis), g["f_sampled"], equal_nan=True)
    assert np.array_equal(oracle.hair_pdf(g["brdf"], g["wo"], wis), g["pdf_sampled"], equal_nan=True)


def test_hair_bsdf_survey_sanity_row(oracle):
    """The hand-checked row of SURVEY.md 8(c): eumelanin 1.3, defaults, v = 0.7."""
    g = golden("hair_bsdf.npz")
    b = g["brdf"][-1]
    assert np.allclose(b[0:3], [0.544699967, 0.906099975, 1.7809999], rtol=1e-7)
    assert np.isclose(b[5], 0.399999976) and np.isclose(b[17], 0.411516815)
    assert np.allclose(b[6:10], [0.0846111849, 0.0211527962, 0.33844474, 0.33844474], rtol=1e-7)
    assert np.isclose(b[10], 0.117159814)
    assert np.allclose(b[11:14], [0.0348994955, 0.0697564706, 0.139173105], rtol=1e-7)
    assert np.allclose(g["f"][-1], [0.0072593037, 0.00171589118, 0.000117730997], rtol=1e-6)
    assert np.isclose(g["pdf"][-1], 0.0127097657, rtol=1e-6)
    assert np.allclose(g["wi_sampled"][-1], [-0.336120844, -0.789911628, -0.512896121], rtol=1e-6)
    assert np.allclose(g["f_sampled"][-1], [1.45676994, 0.697069347, 0.117038034], rtol=1e-6)
    assert np.isclose(g["pdf_sampled"][-1], 3.73515105, rtol=1e-6)
    # colour row: color (0.8, 0.4, 0.05), beta_n 0.3
    assert np.allclose(g["brdf"][-2][0:3], [0.00143605738, 0.0242141783, 0.258826762], rtol=1e-6)


def test_volume_functions_bit_exact(oracle, yh):
    """The free flight and the scatter in a homogeneous medium (yocto_math.h:4758-4813) on the strata of tests/volume_cases.py:
    the oracle's rows against the reference's own outputs on the same medium, bit for bit; the committed inputs are the strata's."""
    import volume_cases as vc
    g = golden("volumes_unit.npz")
    for name, k in vc.GOLDEN_ROWS.items():
        s = vc.inputs(name)
        orc = oracle.volume(0, s.mats[:k], s.nrm[:k], s.wo[:k], s.wi[:k], s.tex[:k], s.rn[:k])
        for key, got in (("density", orc[:, 1:4]), ("anisotropy", orc[:, 7]), ("wo", s.wo[:k]), ("wi", s.wi[:k]), ("rn", s.rn[:k])):
            assert np.array_equal(got, g[f"{name}_{key}"]), (name, key)
        view, covered = vc.reference_view(orc)
        assert covered.mean() > (0.05 if name == "g" else 0.7), name
        differ = np.flatnonzero(~((view == g[f"{name}_ref"]) | (np.isnan(view) & np.isnan(g[f"{name}_ref"]))).all(axis=1) & covered)
        assert len(differ) == 0, (name, differ[:5], view[differ[:2]], g[f"{name}_ref"][differ[:2]])


def test_shading_points_bit_exact(oracle, yh):
    """yo_scene_point_batch on the strata of tests/point_cases.py (general scene: stratum a whole, GOLDEN_ROWS rows of each edge
    stratum) against the committed rows, bit for bit; the committed inputs are the strata's."""
    import point_cases as pc
    g = golden("points_unit.npz")
    osc = oracle.scene(*pc.scene(True).desc(yh))
    for name in pc.STRATA:
        s = pc.inputs(name, osc)
        k = pc.ROWS if name == "a" else pc.GOLDEN_ROWS
        for key, got in (("object", s.obj[:k]), ("element", s.elem[:k]), ("uv", s.uv[:k]), ("outgoing", s.wo[:k])):
            assert np.array_equal(got, g[f"{name}_{key}"]), (name, key)
        got, want = osc.point(s.obj[:k], s.elem[:k], s.uv[:k], s.wo[:k]), g[f"{name}_point"]
        assert want.shape == (k, yh.POINT_FLOATS)
        differ = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
        assert len(differ) == 0, (name, differ[:5])
    osc.close()


@pytest.mark.parametrize("variant", ("four", "six", "far"))
def test_hits_unit_bit_exact(oracle, yh, variant):
    """yo_scene_intersect on the first rows of every stratum of tests/hit_cases.py against the reference's committed closest hits
    (oracle/make_golden.py: hits_unit), bit for bit; the committed rays are the strata's."""
    import hit_cases as hc
    g = golden("hits_unit.npz")
    got = hc.oracle_hits(variant, yh, oracle, scene_path)[0]
    for k, name in enumerate(hc.NAMES):
        rays = g[f"{variant}_{name}_rays"]
        n = len(rays)
        assert n == 512 and np.array_equal(rays.view(np.uint32), hc.strata(variant)[name].rays[:n].view(np.uint32)), (variant, name)
        for what, a in zip(("object", "element", "uv", "distance"), got):
            a, want = a[k * hc.N:k * hc.N + n], g[f"{variant}_{name}_{what}"]
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), want.view(np.uint32)), (variant, name, what)


def test_hits_unit_ties_bit_exact(oracle, yh):
    """The same on variant `ties`: the first rows of hit_cases.ties_rays, where who wins among a primitive's copies is the visiting order's."""
    import hit_cases as hc
    g = golden("hits_unit.npz")
    got = hc.oracle_hits("ties", yh, oracle, scene_path)[0]
    rays = g["ties_t_rays"]
    n = len(rays)
    assert n == 512 and np.array_equal(rays.view(np.uint32), hc.ties_rays()[:n].view(np.uint32))
    assert len(np.unique(g["ties_t_element"][g["ties_t_object"] == hc.TIES_OBJECTS["stack"]])) >= 3  # (more than one copy wins on the committed rows)
    for what, a in zip(("object", "element", "uv", "distance"), got):
        assert np.array_equal(np.ascontiguousarray(a[:n]).view(np.uint32), g[f"ties_t_{what}"].view(np.uint32)), what


def test_surface_lobes_bit_exact(oracle, yh):
    """Fresnel terms and the nine surface lobes (yocto_math.h:4215-4755)
    — value * |cos|, pdf and sampled direction — against vectors made by the reference."""
    g = golden("lobes.npz")
    args = (g["params"], g["normal"], g["wo"], g["wi"], g["rn"])
    assert np.array_equal(oracle.fresnel(g["params"], g["normal"], g["wo"]), g["fresnel"], equal_nan=True)
    for kind in range(yh.LOBE_COUNT):
        want = g[f"lobe_{kind}"]
        assert np.array_equal(oracle.surface_lobe(kind, *args), want, equal_nan=True), kind
        # the fixture really exercises the lobe: non-zero values, non-zero samples, finite
        assert np.isfinite(want).all()
        assert (want[:, :3] != 0).any(axis=1).mean() > 0.15, kind
        assert (want[:, 4:] != 0).any(axis=1).mean() > 0.4, kind


def test_surface_lobes_at_their_edges_bit_exact(oracle, yh):
    """The Fresnel terms and the nine lobes on the edge strata of tests/surface_cases.py (grazing, a zero halfway vector, the
    specular peak at roughness 1e-6, the critical angle, degenerate metals, the random numbers' edges) against the reference's own
    outputs; the committed inputs are the strata's."""
    import surface_cases as sc
    g = golden("lobes_edges.npz")
    for name in sc.STRATA:
        s, k = sc.inputs(name), sc.GOLDEN_ROWS
        args = (s.params[:k], s.nrm[:k], s.wo[:k], s.wi[:k], s.rn[:k])
        for key, got in zip(("params", "normal", "wo", "wi", "rn"), args):
            assert np.array_equal(got, g[f"{name}_{key}"]), (name, key)
        assert np.array_equal(oracle.fresnel(*args[:3]), g[f"{name}_fresnel"], equal_nan=True), name
        for kind in range(yh.LOBE_COUNT):
            assert np.array_equal(oracle.surface_lobe(kind, *args), g[f"{name}_lobe_{kind}"], equal_nan=True), (name, kind)


def test_curve_conversion_bit_exact(oracle):
    """pbrt curve -> five-vertex strand (yocto_pbrt.h:1751-1797)."""
    g = golden("curves.npz")
    pos, nrm, rad, lines = oracle.curves_to_lines(g["P"], g["width0"], g["width1"], int(g["base_vertex"]))
    assert np.array_equal(pos, g["positions"]) and np.array_equal(nrm, g["normals"], equal_nan=True)
    assert np.array_equal(rad, g["radius"]) and np.array_equal(lines, g["lines"])
    assert lines.min() == 100 and lines.max() == 100 + 5 * len(g["P"]) - 1
    assert np.array_equal(pos[0::5], g["P"][:, 0:3]) and np.array_equal(pos[4::5], g["P"][:, 9:12])


def test_primitive_tests_bit_exact(oracle):
    g = golden("intersect.npz")
    h, uv, d = oracle.intersect_line(g["rays"], g["p0"], g["p1"], g["r0"], g["r1"])
    assert np.array_equal(h, g["line_hit"]) and np.array_equal(uv, g["line_uv"]) and np.array_equal(d, g["line_dist"])
    assert 0.05 < h.mean() < 0.95
    # SURVEY.md 8c sanity ray
    assert h[0] == 1 and np.allclose(uv[0], [0.524203897, 0.946916103], rtol=1e-6) and np.isclose(d[0], 1.00201702)
    h, uv, d = oracle.intersect_triangle(g["rays"], g["p0"], g["p1"], g["p2"])
    assert np.array_equal(h, g["tri_hit"]) and np.array_equal(uv, g["tri_uv"]) and np.array_equal(d, g["tri_dist"])
    assert np.array_equal(oracle.intersect_bbox(g["rays"], g["bbox"]), g["bbox_hit"])


@pytest.mark.parametrize("name,kw", GOLDEN_SCENES, ids=[f"{n}-{'-'.join(map(str, k.values()))}" for n, k in GOLDEN_SCENES])
def test_scene_hits_and_images_bit_exact(oracle, yh, name, kw):
    g = golden(f"scene_{scene_tag(name, kw)}.npz")
    sf = yh.SceneFile(scene_path(name, **kw))
    sc = oracle.scene(sf.desc)
    assert sc.num_lights() == int(g["num_lights"])
    obj, elem, uv, dist = sc.intersect(g["rays"])
    assert np.array_equal(obj, g["object"]) and np.array_equal(elem, g["element"])
    assert np.array_equal(uv, g["uv"]) and np.array_equal(dist, g["distance"])
    res = g["img_1"].shape[0]
    p = yh.TraceParams.default(resolution=res)
    for spp in (1, 16):
        img, rng = sc.render(p, spp, want_rng=True)
        assert np.array_equal(img, g[f"img_{spp}"], equal_nan=True)
        assert np.array_equal(rng, g[f"rng_{spp}"])
    # single-threaded == multi-threaded (the reference is thread-count independent)
    assert np.array_equal(sc.render(p, 16, nthreads=1), g["img_16"])
    assert np.array_equal(sc.render(yh.TraceParams.default(resolution=res, seed=12345), 16), g["img_16_seed12345"])
    sc.close()
    sf.close()


def test_other_shaders_bit_exact(oracle, yh):
    """trace_naive / trace_eyelight / trace_normal (pt.cpp:1514-1672) against the reference's images."""
    g = golden("shaders.npz")
    tags = sorted({k.split("|")[0] for k in g.files})
    by_tag = {scene_tag(n, k): (n, k) for n, k in GOLDEN_SCENES}
    assert len(tags) == 4
    for tag in tags:
        name, kw = by_tag[tag]
        sf = yh.SceneFile(scene_path(name, **kw))
        sc = oracle.scene(sf.desc)
        for shader in ("naive", "eyelight", "normal"):
            p = yh.TraceParams.default(resolution=g[f"{tag}|{shader}|1"].shape[0], shader=shader)
            assert np.array_equal(sc.render(p, 1), g[f"{tag}|{shader}|1"], equal_nan=True)
            img, rng = sc.render(p, 8, want_rng=True)
            assert np.array_equal(img, g[f"{tag}|{shader}|8"], equal_nan=True)
            assert np.array_equal(rng, g[f"{tag}|{shader}|rng8"])
        sc.close(), sf.close()
    # an unknown shader is an error, as in get_trace_shader_func (pt.cpp:1669)
    sf = yh.SceneFile(scene_path(by_tag[tags[0]][0], **by_tag[tags[0]][1]))
    sc = oracle.scene(sf.desc)
    with pytest.raises(Exception):
        sc.render(yh.TraceParams.default(resolution=16, shader=9), 1)
    sc.close(), sf.close()


def _maps_ids():
    import ref_cases as rc
    return rc.MAPS_CASES


@pytest.mark.parametrize("prefix,kw,res_key,shaders", _maps_ids(), ids=[c[0].strip("/") or "maps" for c in _maps_ids()])
def test_material_maps_bit_exact(oracle, yh, prefix, kw, res_key, shaders):
    """The materials' maps (eval_normalmap and eval_element_tangents, pt.cpp:314-347; the scalar maps of eval_brdf, :413-424; the
    opacity rule): the oracle's renders of the `maps` scene and of its five one-map variants against EVERY `*_1`, `*_8` and
    `*_8_s777` image the reference rendered of them (tests/golden/maps.npz) — path, naive, eyelight and normal — and the
    pixels' RNG states after path_8, bit for bit. The reference's eval_* are static, so this fixture is what holds the
    restatement to it."""
    import ref_cases as rc
    g = golden("maps.npz")
    got = rc.maps_entries(oracle, scene_path, g, prefix, kw, res_key, shaders)
    want = [k for k in g.files if k.startswith(prefix) and "/" not in k[len(prefix):] and k != "rng_8" and k.split("_")[-1] in ("1", "8", "s777")]
    assert sorted(k for k in got if k != "rng_8") == sorted(want) and len(want) == (11 if not prefix else 9)
    for k in want:
        assert np.array_equal(got[k], g[k], equal_nan=True), (k, int((got[k] != g[k]).any(axis=2).sum()))
    if not prefix:
        assert np.array_equal(got["rng_8"], g["rng_8"])


REF_SCENE_NAMES = ["sloth", "bold-man", "straight-hair", "curly-hair", "hair-curls", "sphere-hairblock"]


@pytest.mark.parametrize("which", REF_SCENE_NAMES)
def test_reference_scene_files_bit_exact(oracle, yh, which):
    """The reference's own scene descriptions (tests/golden/ref_scenes/*.json, verbatim; stand-in
    geometry from tools/make_scenes.py) read by THIS build's loader and rendered by the oracle,
    against images the reference rendered from the same files through its own loader."""
    g = golden("refscenes.npz")
    sf = yh.SceneFile(scene_path("ref-" + which, scale=0.05))
    sc = oracle.scene(sf.desc)
    assert sc.num_lights() == int(g[f"{which}|lights"])
    p = yh.TraceParams.default(resolution=48)
    assert np.array_equal(sc.render(p, 1), g[f"{which}|1"], equal_nan=True)
    img, rng = sc.render(p, 8, want_rng=True)
    assert np.array_equal(img, g[f"{which}|8"], equal_nan=True) and np.array_equal(rng, g[f"{which}|rng8"])
    sc.close(), sf.close()


def test_selftests_pass_on_oracle(oracle):
    """The four Monte-Carlo self-tests of the reference (ext.cpp:555-693) restated; the two
    cheap ones run here, all four run against the GPU in test_gpu_parity.py."""
    for which in (2, 3):
        ok, worst = oracle.selftest(which)
        assert ok, (which, worst)


def test_reference_work_counts_fixture(oracle, yh):
    """the N_* of the algorithmic-bytes formula are counts of the REFERENCE algorithm
    (binary BVH, <= 4 primitives per leaf) made by the instrumented oracle and committed per config
    (tests/golden/workcounts.json, oracle/make_workcounts.py). C0 is re-counted here exactly; the
    formula's bytes/sample of every config is re-derived from its committed counts."""
    import json
    import os
    from conftest import GOLD
    fx = json.load(open(os.path.join(GOLD, "workcounts.json")))
    assert {"C0", "C1", "C2-beta_m0.1", "C2-beta_m0.25", "C2-beta_m0.6", "C3", "C4"} <= set(fx)
    for name, c in fx.items():
        p = c["per_sample"]
        b = (32 * p["nodes"] + 44 * p["seg_tests"] + 52 * p["tri_tests"] + 104 * p["hair_shades"] +
             (48 * p["env_lookups"] if c["env_textured"] else 0) + 88 * p["env_samples"] + 32.0 / c["spp_per_launch_assumed"])  # env texels: textured environments only
        assert abs(b - c["algorithmic_bytes_per_sample"]) < 0.6, name
    c0 = fx["C0"]
    sf = yh.SceneFile(scene_path("sphere-hairblock"))
    osc = oracle.scene(sf.desc)
    _, wc = osc.render(yh.TraceParams.default(resolution=c0["resolution"]), c0["spp_counted"], want_counts=True)
    got = {k: round(v / wc.samples, 4) for k, v in wc.as_dict().items() if k in c0["per_sample"]}
    assert got == c0["per_sample"]
    osc.close(), sf.close()
