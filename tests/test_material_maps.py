"""Scalar material textures and normal maps (yh_material_maps, yh_upload_scene_maps): the `maps` scene of tools/make_scenes.py
against the REFERENCE's own images of it (tests/golden/maps.npz, tools/make_map_goldens.py). The CPU oracle knows the maps too
(yo_scene_create_maps) and renders these very images bit for bit (tests/test_oracle_golden.py::test_material_maps_bit_exact); row by
row the maps are held to it at unit level in tests/test_point_unit.py.

CPU: the scene reader's keys and indices, the mirror's setters with texture arguments, the fixture against a live render of the
reference where oracle/_ref is built. GPU: the four shaders against the reference with the bars of the other shader tests, the
map-by-map variants, the RNG draws, every launch shape and kernel, the command line, and that a NULL map table or a transmission
map changes no bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden, scene_path

BAR_1SPP = 0.90


def _rel(a, b, floor=1e-6):
    return np.abs(a - b) / np.maximum(np.abs(b), floor)


def _relrmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3] - b[..., :3]) ** 2)) / max(1e-12, np.mean(b[..., :3])))


def _maps_of(yh, sf):
    d = sf.desc.contents
    names = [f for f, _ in yh.MaterialMaps._fields_]
    return [{k: getattr(sf.maps[i], k) for k in names} for i in range(d.num_materials)]


def _write_scene(tmp_path, material, textures=("spec",)):
    """A one-material scene next to the maps scene's textures (a plain quad, an area light)."""
    import json
    import shutil
    src = os.path.dirname(scene_path("maps"))
    d = tmp_path / "s"
    shutil.copytree(os.path.join(src, "shapes"), d / "shapes")
    shutil.copytree(os.path.join(src, "textures"), d / "textures")
    scene = {"cameras": {"default": {"lens": 0.05, "aspect": 1.0, "lookat": [0, 0, 3, 0, 0, 0, 0, 1, 0]}},
             "objects": {"q": {"shape": "plainquad", "material": "m"}},
             "materials": {"m": material}}
    (d / "s.json").write_text(json.dumps(scene))
    return str(d / "s.json")


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_maps_scene_loads_with_its_map_indices(yh):
    """The scene reader takes the map keys of sceneio.cpp:1298-1317 (it refused them before) and hands them out through
    yh_scene_get_maps, 1-based into the scene's textures: one index per map, the same file under one index."""
    sf = yh.SceneFile(scene_path("maps"))
    d = sf.desc.contents
    mats = {}
    import json
    names = sorted(json.load(open(scene_path("maps")))["materials"])  # materials are numbered alphabetically
    for name, m in zip(names, _maps_of(yh, sf)):
        mats[name] = m
    assert d.num_materials == len(names) == 8
    a = mats["allmaps"]
    assert all(a[k] > 0 for k in a), a
    assert a["roughness_tex"] == a["transmission_tex"]  # both "rough": stored once
    assert mats["specmap"]["specular_tex"] == a["specular_tex"] and sum(mats["specmap"].values()) == a["specular_tex"]
    assert mats["metalmap"]["metallic_tex"] == a["metallic_tex"] and sum(mats["metalmap"].values()) == a["metallic_tex"]
    assert mats["roughmap"]["roughness_tex"] == a["roughness_tex"] and sum(mats["roughmap"].values()) == a["roughness_tex"]
    assert mats["hairop"]["opacity_tex"] == a["opacity_tex"] and sum(mats["hairop"].values()) == a["opacity_tex"]
    for n in ("normalmap", "flatnormal"):
        assert mats[n]["normal_tex"] == a["normal_tex"] and sum(mats[n].values()) == a["normal_tex"]
    assert sum(mats["arealight"].values()) == 0
    ids = {a[k] for k in a}
    assert ids == set(range(1, d.num_textures + 1)) and d.num_textures == 5
    tex = {k: d.textures[a[k] - 1] for k in a}
    assert all(t.width == t.height == 32 and t.is_byte for t in tex.values())
    # a scalar map is grey RGB; metal.png is an RGB file, read as grey with stb's weights as the reference's scalar loader does
    px = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint8 * (32 * 32 * 3)).from_address(tex["metallic_tex"].pixels)).reshape(-1, 3)
    assert (px == px[:, :1]).all() and px.std() > 0
    sf.close()


def test_ignored_and_checked_map_keys(yh, tmp_path):
    """coat_tex / spectint_tex are not read by the reference's loader: accepted and ignored (even naming no file).
    translucency_tex / displacement_tex are loaded: a missing file is the usual error."""
    p = _write_scene(tmp_path, {"color": [0.5, 0.5, 0.5], "coat_tex": "nothing", "spectint_tex": "nothing",
                                "translucency_tex": "spec", "displacement_tex": "rough"})
    sf = yh.SceneFile(p)
    assert sf.desc.contents.num_textures == 0  # loaded, used by nothing
    assert sum(_maps_of(yh, sf)[0].values()) == 0
    sf.close()
    for key in ("translucency_tex", "displacement_tex", "opacity_tex", "normal_tex"):
        p = _write_scene(tmp_path / key, {"color": [0.5, 0.5, 0.5], key: "missing"})
        with pytest.raises(yh.YhError, match="file not found"):
            yh.SceneFile(p)


def test_fixture_is_the_reference_live(tmp_path):
    """Two entries of tests/golden/maps.npz re-rendered with the real reference are bit-equal (where oracle/_ref is built)."""
    import oracle_capi as oc
    import yhair_capi as yh
    import make_map_goldens as mg
    if not oc.have_ref():
        pytest.skip("oracle/_ref/libyh_ref.so is not built here (make -C oracle ref)")
    g = golden("maps.npz")
    ref = oc.Ref()
    assert np.array_equal(mg.render(ref, scene_path("maps"), int(g["res"]), "path", 1), g["path_1"])
    assert np.array_equal(mg.render(ref, scene_path("maps", only="normal"), int(g["vres"]), "eyelight", 8), g["only-normal/eyelight_8"])


def test_fixture_is_small_and_complete():
    g = golden("maps.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "maps.npz")) < 1 << 20
    for k in ("path_1", "path_8", "path_8_s777", "rng_8", "normal_1", "normal_8", "naive_8_s777", "eyelight_8_s777"):
        assert k in g.files, k
    assert g["path_1"][..., 3].mean() > 0.4  # the objects fill the frame


def test_mirror_takes_the_reference_setters(tmp_path):
    """A C++ caller that uses the reference's material setters with texture arguments, set_normalmap and scalar set_texture
    compiles against the mirror (host/yhair_pathtrace.h) with g++ and builds the scene it means."""
    exe = str(tmp_path / "mirror_maps")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "yocto-hair_amd", "host"), "-Wno-class-memaccess",
                           os.path.join(ROOT, "tests", "cpp", "test_mirror_maps.cpp"), "-c", "-o", exe + ".o"])


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def _render(ctx, yh, path, res, shader, spp, seed=961748941, maps=True, rng=False):
    sf = yh.SceneFile(path)
    ctx.upload_scene(sf.desc, sf.maps if maps else None)
    ctx.set_shard(0, 1)
    ctx.init_state(yh.TraceParams.default(resolution=res, seed=seed, shader=shader))
    ctx.trace_samples(spp)
    img = ctx.download()
    r = ctx.download_rng() if rng else None
    sf.close()
    return (img, r) if rng else img


def _check_shader(ctx, yh, g, path, res, prefix, shader):
    img1 = _render(ctx, yh, path, res, shader, 1)
    ref1 = g[prefix + shader + "_1"]
    assert np.array_equal(img1[..., 3] > 0, ref1[..., 3] > 0)
    close = _rel(img1[..., :3], ref1[..., :3]).max(axis=2) < 1e-3
    assert close.mean() >= BAR_1SPP, f"{prefix}{shader}: only {close.mean():.3f} of pixels within rel 1e-3 at 1 spp"
    img8, ref8 = _render(ctx, yh, path, res, shader, 8), g[prefix + shader + "_8"]
    err, floor = _relrmse(img8, ref8), _relrmse(g[prefix + shader + "_8_s777"], ref8)
    assert err <= 0.5 * floor, f"{prefix}{shader}: relRMSE {err:.4f} vs 0.5 x seed floor {floor:.4f}"


@pytest.mark.gpu
@pytest.mark.parametrize("shader", ["path", "naive", "eyelight"])
def test_maps_render_like_the_reference(ctx, yh, shader):
    g = golden("maps.npz")
    _check_shader(ctx, yh, g, scene_path("maps"), int(g["res"]), "", shader)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["specular", "metallic", "roughness", "opacity", "normal"])
@pytest.mark.parametrize("shader", ["path", "naive", "eyelight"])
def test_each_map_renders_like_the_reference(ctx, yh, kind, shader):
    g = golden("maps.npz")
    _check_shader(ctx, yh, g, scene_path("maps", only=kind), int(g["vres"]), f"only-{kind}/", shader)


@pytest.mark.gpu
def test_normal_shader_shows_the_mapped_normals(ctx, yh):
    g = golden("maps.npz")
    res = int(g["res"])
    img1, ref1 = _render(ctx, yh, scene_path("maps"), res, "normal", 1), g["normal_1"]
    assert np.array_equal(img1[..., 3], ref1[..., 3])
    close = _rel(img1[..., :3], ref1[..., :3]).max(axis=2) < 1e-3
    assert close.mean() >= 0.97, close.mean()
    assert np.abs(img1 - ref1).max() < 2e-2
    assert _relrmse(_render(ctx, yh, scene_path("maps"), res, "normal", 8), g["normal_8"]) < 2e-3
    # without the maps the normals differ: the test sees them
    assert not np.array_equal(_render(ctx, yh, scene_path("maps"), res, "normal", 1, maps=False), img1)


@pytest.mark.gpu
def test_rng_draws_follow_the_reference(ctx, yh):
    """The opacity draws (pt.cpp:1429) line up with the reference's: the pixels' RNG states after 8 spp."""
    g = golden("maps.npz")
    _, rng = _render(ctx, yh, scene_path("maps"), int(g["res"]), "path", 8, rng=True)
    same = (rng.reshape(-1, 2) == g["rng_8"].reshape(-1, 2)).all(axis=1)
    assert same.mean() >= 0.90, same.mean()


@pytest.mark.gpu
def test_transmission_map_changes_no_pixel(ctx, yh):
    a = _render(ctx, yh, scene_path("maps"), 48, "path", 4, rng=True)
    b = _render(ctx, yh, scene_path("maps", notrans=True), 48, "path", 4, rng=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", [("textured", dict(scale=0.05)), ("lobes", dict(scale=0.05))])
def test_null_map_table_is_the_plain_upload(ctx, yh, name, kw):
    """yh_upload_scene(c, d) is yh_upload_scene_maps(c, d, NULL), bit for bit."""
    sf = yh.SceneFile(scene_path(name, **kw))
    p = yh.TraceParams.default(resolution=64)
    out = []
    for call in (lambda: ctx.lib.yh_upload_scene(ctx.h, sf.desc), lambda: ctx.lib.yh_upload_scene_maps(ctx.h, sf.desc, None),
                 lambda: ctx.lib.yh_upload_scene_maps(ctx.h, sf.desc, sf.maps)):
        ctx._chk(call())
        ctx.set_shard(0, 1)
        ctx.init_state(p)
        ctx.trace_samples(4)
        out.append((ctx.download(), ctx.download_rng()))
    for img, rng in out[1:]:
        assert np.array_equal(img, out[0][0]) and np.array_equal(rng, out[0][1])
    sf.close()


@pytest.mark.gpu
def test_bad_map_index_keeps_the_previous_scene(ctx, yh):
    sf = yh.SceneFile(scene_path("maps"))
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    ctx.init_state(yh.TraceParams.default(resolution=32))
    ctx.trace_samples(2)
    before = ctx.download()
    n = sf.desc.contents.num_materials
    bad = (yh.MaterialMaps * n)()
    bad[n - 1].normal_tex = sf.desc.contents.num_textures + 1
    with pytest.raises(yh.YhError, match="missing texture"):
        ctx.upload_scene(sf.desc, bad)
    ctx.init_state(yh.TraceParams.default(resolution=32))
    ctx.trace_samples(2)
    assert np.array_equal(ctx.download(), before)
    sf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["default", "hair_exact"])
def test_every_launch_shape_renders_maps_identically(ctx, yh, monkeypatch, exact):
    """Every launch shape that takes GENERAL scenes (k_trace's quad forms, the wide forms, side by side, k_stream) renders the
    same bits on `maps`; so does k_trace_exact against itself."""
    sf = yh.SceneFile(scene_path("maps"))
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    p = yh.TraceParams.default(resolution=88, hair_exact=exact)
    images = {}
    for shape in ("0", "1", "3", "4", "5", "6", "7", "8"):
        monkeypatch.setenv("YHAIR_SHAPE", shape)
        ctx.init_state(p)
        ctx.trace_samples(3), ctx.trace_samples(5)
        images[shape] = (ctx.download(), ctx.download_rng())
    monkeypatch.delenv("YHAIR_SHAPE")
    base = images["0"]
    assert base[0][..., 3].max() > 0
    for k, (img, rng) in images.items():
        assert np.array_equal(img, base[0]), f"shape {k} renders different pixels"
        assert np.array_equal(rng, base[1]), f"shape {k} leaves different RNG states"
    sf.close()


@pytest.mark.gpu
def test_cli_renders_maps_like_the_library(ctx, yh, tmp_path):
    """yscenetrace builds the scene through the mirror (set_* with texture arguments, set_normalmap, yh_upload_scene_maps):
    the same bits as the scene-file route through the library."""
    exe = os.path.join(ROOT, "yocto-hair_amd", "yscenetrace")
    scene = scene_path("maps")
    out = str(tmp_path / "cli.pfm")
    r = subprocess.run([exe, scene, "-r", "48", "-s", "6", "-o", out, "--spp-per-launch", "4"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    head = b"PF\n48 48\n-1\n"
    raw = open(out, "rb").read()
    assert raw.startswith(head)
    cli = np.frombuffer(raw[len(head):], np.float32).reshape(48, 48, 3)
    assert np.array_equal(cli, _render(ctx, yh, scene, 48, "path", 6)[..., :3])
