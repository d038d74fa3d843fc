"""Edits of an uploaded scene that keep its trees — yh_update_camera, yh_update_materials, yh_update_environments — the display
download (yh_download_display), the C++ mirror passing set_* edits on at init_state, and `ysceneitraces --turntable`.

The yardstick of every edit is a FRESH context that got yh_upload_scene_maps of the edited description (the existing upload, pinned
against the oracle elsewhere): images, RNG states, yh_lights_batch, yh_intersect_batch and yh_scene_once must be the same bits.
The camera edits are also held against the oracle on the edited description (alpha of every pixel at 1 spp).

The display bytes are compared with a float64 numpy restatement of tonemap + float_to_byte (yocto_math.h:3820-3829, 3721-3729)
applied to yh_download's floats: a byte may differ, and then by exactly 1, only where the restated value x 256 lies within
256 * 1e-5 * max(value, 1e-3) of an integer (float32 against float64 through exp2 / pow: a few 1e-7 relative; 1e-5 leaves two
orders of magnitude); such bytes must be at most 1 % of the image, counted on the numpy side alone — and on the CPU with the
oracle's render of the same image (test_display_image_has_few_bytes_near_a_step).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path

RES, F = 64, np.float32
PKG = os.path.join(ROOT, "yocto-hair_amd")
DISPLAY_SETTINGS = [(0.0, 0, 1), (1.5, 1, 1), (-2.0, 0, 0)]  # (exposure, filmic, srgb)
DISPLAY_SCENE = ("textured", dict(scale=0.05))
# The image: a close-up of the scene's emissive, textured, half-transparent ball. Under the scene's own camera a third of the pixels
# are the constant sky, 0.5, which exposure -2 turns into 0.125 x 256 = 32 exactly, and some are black floor texels, 0 exactly: bytes
# that sit ON a step by the rule below (and come out equal all the same) would be a third of the image. The ball emits everywhere.
DISPLAY_EYE, DISPLAY_CENTER, DISPLAY_LENS = (0.7, 1.2, 2.8), (0.7, 0.35, 0.3), 0.15
NEAR_STEP_MAX = 0.01


# ---------------------------------------------------------------------------------------------
# descriptions and their edited copies
# ---------------------------------------------------------------------------------------------
class Edited:
    """A copy of a scene description with its own camera, material and environment arrays (the geometry is shared)."""

    def __init__(self, yh, desc):
        src = desc.contents if hasattr(desc, "contents") else desc
        self.d = yh.SceneDesc.from_buffer_copy(src)
        self.materials = (yh.Material * src.num_materials)(*[yh.Material.from_buffer_copy(src.materials[i]) for i in range(src.num_materials)])
        self.envs = (yh.Environment * max(1, src.num_environments))(*[yh.Environment.from_buffer_copy(src.environments[i]) for i in range(src.num_environments)])
        self.d.materials = C.cast(self.materials, C.POINTER(yh.Material))
        self.d.environments = C.cast(self.envs, C.POINTER(yh.Environment))
        self.n_envs = src.num_environments

    @property
    def ptr(self):
        return C.pointer(self.d)

    @property
    def camera(self):
        return self.d.camera

    def env_array(self, yh):
        return (yh.Environment * self.n_envs)(*[self.envs[i] for i in range(self.n_envs)])


def _lookat(eye, center, up=(0, 1, 0)):
    """lookat_frame (yocto_math.h:3229-3239) as 12 floats x, y, z, o."""
    eye, center, up = (np.asarray(v, np.float64) for v in (eye, center, up))
    w = (eye - center) / np.linalg.norm(eye - center)
    u = np.cross(up, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    return [float(F(x)) for x in np.concatenate([u, v / np.linalg.norm(v), w, eye])]


def _rot_y(frame12, degrees):
    f = np.array(frame12, np.float64).reshape(4, 3)
    a = np.radians(degrees)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    return [float(F(x)) for x in (f @ R.T).reshape(-1)]


def _row_of(desc, lines):
    """The material row of the first object whose shape is made of lines (True) / triangles (False)."""
    d = desc.contents if hasattr(desc, "contents") else desc
    for i in range(d.num_objects):
        if (d.shapes[d.objects[i].shape].num_lines > 0) == lines:
            return d.objects[i].material
    raise AssertionError("no such object")


def _render(c, yh, spp=4, res=RES, first=0):
    """init_state, `first` samples, then `spp`: (image, RNG states)."""
    c.set_shard(0, 1)
    c.init_state(yh.TraceParams.default(resolution=res))
    if first:
        c.trace_samples(first)
    c.trace_samples(spp)
    return c.download(), c.download_rng()


def _fresh(yh, desc, maps=None, **kw):
    """The yardstick: a new context, the upload of `desc`, the same render."""
    c = yh.Context(0)
    try:
        c.upload_scene(desc, maps)
        return _render(c, yh, **kw) + (c.scene_once(),)
    finally:
        c.close()


def _same(got, want, what):
    assert want[0][..., 3].max() > 0, what
    assert got[0].shape == want[0].shape, f"{what}: image size {got[0].shape} against {want[0].shape}"
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), f"{what}: pixels differ from a fresh upload's"
    assert np.array_equal(got[1], want[1]), f"{what}: RNG states differ from a fresh upload's"


def _rays_at_the_hairblock_scene(n=4096, seed=0):
    """From around sphere-hairblock's camera towards the box that holds its sphere (at (-0.5, 0, 0)) and its hair block (at (0.5, 1, -0.5))."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1, 1, (n, 3)) * [1.5, 0.8, 0.5] + [-0.5, 1.5, 5.0]
    d = rng.uniform([-1.5, -1.0, -1.5], [1.5, 2.0, 0.5], (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d, np.full((n, 1), 1e-4), np.full((n, 1), 3.4e38)], axis=1).astype(F)


# ---------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------
NEW_ENTRIES = ("yh_update_camera", "yh_update_materials", "yh_update_environments", "yh_download_display")


def test_library_exports_and_header_declares_the_entry_points(yh):
    lib = yh.load()
    header = open(os.path.join(ROOT, "include", "yhair.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libyhair.so")], capture_output=True, text=True, check=True).stdout
    for name in NEW_ENTRIES:
        assert hasattr(lib, name) and f" T {name}\n" in exported, name
        assert f"int {name}(yh_context*" in header, name
        assert name in yh.EXPORTS
    for method in ("update_camera", "update_materials", "update_environments", "download_display"):
        assert callable(getattr(yh.Context, method))


def _compile_mirror_test(tmp_path):
    exe = str(tmp_path / "mirror_edits")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host"), "-Wno-class-memaccess", os.path.join(ROOT, "tests", "cpp", "test_mirror_edits.cpp"),
                           "-o", exe, "-L" + PKG, "-lyhair", "-Wl,-rpath," + PKG, "-lpthread"])
    return exe


def test_mirror_classifies_edits_without_a_device(built, tmp_path):
    """The mirror's classification of what changed since the last upload is a pure function over two flattened descriptions
    (detail::classify_edit): camera only, material only, an emission toggle, an object frame, a shape pointer and their
    neighbours, checked by the C++ program itself. It compiles and links without a GPU; asked to render without one it ends
    with the library's message."""
    import torch
    exe = _compile_mirror_test(tmp_path)
    r = subprocess.run([exe, "--classify"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    if not torch.cuda.is_available():
        r = subprocess.run([exe, scene_path("sphere-hairblock", scale=0.02)], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "no HIP device available" in r.stdout + r.stderr, (r.returncode, r.stdout, r.stderr)


def _restate_display(img, exposure, filmic, srgb):
    """tonemap + float_to_byte in float64 on (H, W, 4) float32 pixels: the values before the byte conversion and the bytes."""
    v = img.astype(np.float64)
    rgb = v[..., :3]
    if exposure != 0:
        rgb = rgb * 2.0 ** exposure
    if filmic:
        h = rgb * 0.6
        rgb = np.maximum(0.0, (h * h * 2.51 + h * 0.03) / (h * h * 2.43 + h * 0.59 + 0.14))
    if srgb:
        with np.errstate(invalid="ignore"):
            rgb = np.where(rgb <= 0.0031308, 12.92 * rgb, (1 + 0.055) * np.power(np.maximum(rgb, 0.0), 1 / 2.4) - 0.055)
    v = np.concatenate([rgb, v[..., 3:]], axis=2)
    s = v * 256
    with np.errstate(invalid="ignore"):
        b = np.where(~np.isfinite(s) | (s <= 0), 0, np.where(s >= 255, 255, np.floor(np.where(np.isfinite(s), s, 0))))
    return v, b.astype(np.uint8)


def _display_description(yh, sf):
    e = Edited(yh, sf.desc)
    e.camera.frame[:] = _lookat(DISPLAY_EYE, DISPLAY_CENTER)
    e.camera.lens = DISPLAY_LENS
    return e


def _near_step(v):
    """Where value x 256 lies within 256 * 1e-5 * max(value, 1e-3) of an integer: the bytes that may differ by 1."""
    s = v * 256
    return np.isfinite(s) & (np.abs(s - np.rint(s)) <= 256 * 1e-5 * np.maximum(np.abs(v), 1e-3))


def test_display_image_has_few_bytes_near_a_step(yh, oracle):
    """The image of the display test, rendered by the oracle: under each of the three settings at most 1 % of its bytes lie
    near a step of float_to_byte, so the GPU test's allowance cannot swallow the image."""
    sf = yh.SceneFile(scene_path(*DISPLAY_SCENE[:1], **DISPLAY_SCENE[1]))
    osc = oracle.scene(_display_description(yh, sf).ptr)
    img = osc.render(yh.TraceParams.default(resolution=RES), 4)
    osc.close(), sf.close()
    assert np.isfinite(img).all() and img[..., 3].max() > 0
    for exposure, filmic, srgb in DISPLAY_SETTINGS:
        v, b = _restate_display(img, exposure, filmic, srgb)
        share = _near_step(v)[..., :3].mean()  # (alpha bytes must be exact: no allowance to count)
        print(f"display {exposure, filmic, srgb}: {share:.4%} of the oracle image's bytes lie near a step; bytes span {b.min()}..{b.max()}")
        assert share <= NEAR_STEP_MAX, (exposure, filmic, srgb, share)
        assert len(np.unique(b[..., :3])) > 32  # an image, not a flat field


# ---------------------------------------------------------------------------------------------
# on the GPU: the camera
# ---------------------------------------------------------------------------------------------
def _camera_case(yh, sf, which):
    """(base description, edited description) of a camera edit."""
    base, new = Edited(yh, sf.desc), Edited(yh, sf.desc)
    if which == "frame":
        new.camera.frame[:] = _lookat((1.5, 2.2, 4.2), (0.25, 0.5, 0))
    elif which == "tall":  # the film flips the image from wide to tall: yh_image_size changes
        base.camera.film[:] = [0.036, 0.024]
        new.camera.film[:] = [0.024, 0.036]
    elif which == "dof":
        new.camera.aperture, new.camera.focus = 0.1, 4.0
    return base, new


@pytest.fixture(scope="module")
def hairblock(yh):
    sf = yh.SceneFile(scene_path("sphere-hairblock", scale=0.02))
    yield sf
    sf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["frame", "tall", "dof"])
def test_camera_edit_renders_as_a_fresh_upload(ctx, yh, oracle, hairblock, which):
    base, new = _camera_case(yh, hairblock, which)
    ctx.upload_scene(base.ptr)
    before = _render(ctx, yh, spp=2)
    ctx.update_camera(new.camera)
    got = _render(ctx, yh, spp=4)
    want = _fresh(yh, new.ptr, spp=4)
    _same(got, want, which)
    assert ctx.scene_once() == want[2]
    if which == "tall":
        assert before[0].shape[:2] == (43, 64) and got[0].shape[:2] == (64, 43)
    else:
        assert not np.array_equal(_render(ctx, yh, spp=2)[0], before[0]), "the edit changed nothing"
    # against the oracle on the edited description: primary visibility, every pixel
    p = yh.TraceParams.default(resolution=RES)
    ctx.init_state(p)
    ctx.trace_samples(1)
    osc = oracle.scene(new.ptr)
    ref = osc.render(p, 1)
    osc.close()
    assert np.array_equal(ctx.download()[..., 3], ref[..., 3]), f"{which}: alpha differs from the oracle's"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["0", "1", "3"])
def test_camera_edit_under_forced_launch_shapes(ctx, yh, hairblock, shape, monkeypatch):
    """The table the quad kernels stage in LDS and the table copy k_stream's callees read must both be the edited one."""
    base, new = _camera_case(yh, hairblock, "frame")
    monkeypatch.setenv("YHAIR_SHAPE", shape)
    ctx.upload_scene(base.ptr)
    _render(ctx, yh, spp=2)
    ctx.update_camera(new.camera)
    got = _render(ctx, yh, spp=4)
    assert ctx.launch_shape() == int(shape)
    want = _fresh(yh, new.ptr, spp=4)
    monkeypatch.delenv("YHAIR_SHAPE")
    _same(got, want, f"shape {shape}")


# ---------------------------------------------------------------------------------------------
# materials
# ---------------------------------------------------------------------------------------------
def _edit_hair(m):
    m.beta_m, m.eumelanin, m.pheomelanin = 0.6, 0.4, 0.3
    m.sigma_a[:] = [0.0, 0.0, 0.0]


def _edit_hair_sigma(m):
    m.beta_m = 0.1
    m.sigma_a[:] = [0.25, 0.5, 1.0]


def _steps_hair(d):
    r = _row_of(d, True)
    return [(r, 1, lambda ms: _edit_hair(ms[r])), (r, 1, lambda ms: _edit_hair_sigma(ms[r]))]


def _steps_general_and_back(d):
    r = _row_of(d, False)
    return [(r, 1, lambda ms: setattr(ms[r], "specular", 0.5)), (r, 1, lambda ms: setattr(ms[r], "specular", 0.0))]


def _steps_volume(d):
    r = next(i for i in range(d.num_materials) if d.materials[i].transmission != 0 and not d.materials[i].thin)
    return [(r, 1, lambda ms: setattr(ms[r], "thin", 1)), (r, 1, lambda ms: setattr(ms[r], "thin", 0))]


def _steps_textured_colour(d):
    r = next(i for i in range(d.num_materials) if d.materials[i].color_tex and not d.materials[i].transmission and not d.materials[i].specular)

    def edit(ms):
        ms[r].color[:] = [0.9, 0.3, 0.2]
    return [(r, 1, edit)]


def _steps_rows_1_3(d):
    def edit(ms):
        ms[1].eumelanin, ms[1].beta_n = 0.2, 0.5
        ms[1].color[:] = [ms[1].color[0] * 0.5, ms[1].color[1], ms[1].color[2]]
        ms[2].roughness, ms[2].color[2] = 0.4, 0.33
    return [(1, 2, edit)]


MATERIAL_CASES = {
    "hair-plain-to-plain": ("sphere-hairblock", dict(scale=0.02), _steps_hair),
    "sphere-general-and-back": ("sphere-hairblock", dict(scale=0.02), _steps_general_and_back),
    "volume-lost-and-gained": ("volumes", dict(scale=0.05), _steps_volume),
    "colour-under-a-texture": ("textured", dict(scale=0.05), _steps_textured_colour),
    "rows-1-3": ("volumes", dict(scale=0.05), _steps_rows_1_3),
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["0", "1", "3"])
@pytest.mark.parametrize("case", list(MATERIAL_CASES))
def test_material_edit_renders_as_a_fresh_upload(ctx, yh, case, shape, monkeypatch):
    name, kw, steps_of = MATERIAL_CASES[case]
    sf = yh.SceneFile(scene_path(name, **kw))
    monkeypatch.setenv("YHAIR_SHAPE", shape)
    ctx.upload_scene(sf.desc)
    once0 = ctx.scene_once()
    _render(ctx, yh, spp=2)
    new = Edited(yh, sf.desc)
    onces = []
    for first, count, edit in steps_of(sf.desc.contents):
        edit(new.materials)
        ctx.update_materials(first, (yh.Material * count)(*[new.materials[first + i] for i in range(count)]))
        got = _render(ctx, yh, spp=3)
        want = _fresh(yh, new.ptr, spp=3)
        _same(got, want, f"{case}, shape {shape}")
        assert ctx.scene_once() == want[2]
        onces.append(ctx.scene_once())
    monkeypatch.delenv("YHAIR_SHAPE")
    if case == "sphere-general-and-back":  # the once-per-ray form goes n -> 0 -> n where it was n
        assert onces == [0, once0]
    if case == "hair-plain-to-plain":
        assert onces == [once0, once0]
    sf.close()


# ---------------------------------------------------------------------------------------------
# environments; the geometry stays
# ---------------------------------------------------------------------------------------------
def _light_rows(n=1024, seed=29):
    rng = np.random.default_rng(seed)
    P = (rng.uniform(-1, 1, (n, 3)) * [3, 2, 3] + [0, 2.05, 0]).astype(F)
    D = rng.normal(size=(n, 3))
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(F)
    RN = np.minimum(rng.uniform(0, 1, (n, 4)).astype(F), np.nextafter(F(1), F(0)))
    return P, D, RN


@pytest.mark.gpu
def test_environment_edit_renders_and_samples_as_a_fresh_upload(ctx, yh):
    sf = yh.SceneFile(scene_path("envs-unit", scale=0.05, variant="multi"))
    assert sf.desc.contents.num_environments == 4
    ctx.upload_scene(sf.desc)
    rows = _light_rows()
    before = [ctx.lights(form, *rows) for form in (0, 1)]
    _render(ctx, yh, spp=2)
    new = Edited(yh, sf.desc)
    new.envs[2].frame[:] = _rot_y(new.envs[2].frame[:], 70)  # the sky, turned
    new.envs[3].emission[:] = [3.0, 2.5, 1.0]                 # the small map, scaled
    ctx.update_environments(new.env_array(yh))
    got = _render(ctx, yh, spp=4)
    got_lights = [ctx.lights(form, *rows) for form in (0, 1)]
    fresh = yh.Context(0)
    fresh.upload_scene(new.ptr)
    _same(got, _render(fresh, yh, spp=4), "environments")
    for form in (0, 1):
        want = fresh.lights(form, *rows)
        assert np.array_equal(got_lights[form].view(np.uint32), want.view(np.uint32)), f"yh_lights_batch form {form} differs from a fresh upload's"
        assert not np.array_equal(got_lights[form], before[form]), "the edit changed nothing"
    fresh.close(), sf.close()


@pytest.mark.gpu
def test_edits_leave_closest_hits_alone(ctx, yh, hairblock):
    rays = _rays_at_the_hairblock_scene()
    ctx.upload_scene(hairblock.desc)
    before = ctx.intersect(rays)
    assert (before[0] >= 0).mean() > 0.2 and len(np.unique(before[0])) == 3  # misses, the sphere, the hair
    new = Edited(yh, hairblock.desc)
    _edit_hair(new.materials[_row_of(hairblock.desc, True)])
    ctx.update_materials(0, new.materials)
    after_material = ctx.intersect(rays)
    new.envs[0].emission[:] = [0.2, 0.7, 1.1]
    new.envs[0].frame[:] = _rot_y(new.envs[0].frame[:], 33)
    ctx.update_environments(new.env_array(yh))
    after_env = ctx.intersect(rays)
    for after in (after_material, after_env):
        for a, b in zip(before, after):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def _refusals(yh, sf):
    """name -> a call on (lib, handle) that must return YH_E_INVALID, and the entry its message names."""
    d = sf.desc.contents
    sphere, n = _row_of(sf.desc, False), d.num_materials
    emitter = next(i for i in range(n) if any(d.materials[i].emission[:]))

    def material(row, **fields):
        m = yh.Material.from_buffer_copy(d.materials[row])
        for k, v in fields.items():
            if isinstance(v, list):
                getattr(m, k)[:] = v
            else:
                setattr(m, k, v)
        return (yh.Material * 1)(m)

    def env(count, **fields):
        e = (yh.Environment * count)(*[yh.Environment.from_buffer_copy(d.environments[0]) for _ in range(count)])
        for k, v in fields.items():
            getattr(e[0], k)[:] = v
        return e

    cam = yh.Camera.from_buffer_copy(d.camera)
    rows = (yh.Material * n)(*[yh.Material.from_buffer_copy(d.materials[i]) for i in range(n)])
    buf = (C.c_uint8 * 16)()
    return {
        "camera-null": (lambda lib, h: lib.yh_update_camera(h, None), "yh_update_camera"),
        "materials-null": (lambda lib, h: lib.yh_update_materials(h, 0, 1, None), "yh_update_materials"),
        "environments-null": (lambda lib, h: lib.yh_update_environments(h, 1, None), "yh_update_environments"),
        "display-null": (lambda lib, h: lib.yh_download_display(h, 0.0, 0, 1, None), "yh_download_display"),
        "first-negative": (lambda lib, h: lib.yh_update_materials(h, -1, 1, rows), "yh_update_materials"),
        "first-behind-the-table": (lambda lib, h: lib.yh_update_materials(h, n + 1, 0, rows), "yh_update_materials"),
        "count-negative": (lambda lib, h: lib.yh_update_materials(h, 0, -1, rows), "yh_update_materials"),
        "count-past-the-end": (lambda lib, h: lib.yh_update_materials(h, n - 1, 2, rows), "yh_update_materials"),
        "count-huge": (lambda lib, h: lib.yh_update_materials(h, 1, 2**31 - 1, rows), "yh_update_materials"),
        "environment-count": (lambda lib, h: lib.yh_update_environments(h, 2, env(2)), "yh_update_environments"),
        "environment-count-zero": (lambda lib, h: lib.yh_update_environments(h, 0, env(1)), "yh_update_environments"),
        "material-emission-on": (lambda lib, h: lib.yh_update_materials(h, sphere, 1, material(sphere, emission=[0.0, 2.0, 0.0])), "yh_update_materials"),
        "material-emission-off": (lambda lib, h: lib.yh_update_materials(h, emitter, 1, material(emitter, emission=[0.0, 0.0, 0.0])), "yh_update_materials"),
        "environment-emission-off": (lambda lib, h: lib.yh_update_environments(h, 1, env(1, emission=[0.0, 0.0, 0.0])), "yh_update_environments"),
        "color-tex": (lambda lib, h: lib.yh_update_materials(h, sphere, 1, material(sphere, color_tex=1)), "yh_update_materials"),
        "emission-tex": (lambda lib, h: lib.yh_update_materials(h, sphere, 1, material(sphere, emission_tex=1)), "yh_update_materials"),
        "scattering-tex": (lambda lib, h: lib.yh_update_materials(h, sphere, 1, material(sphere, scattering_tex=1)), "yh_update_materials"),
        "second-row-of-two": (lambda lib, h: lib.yh_update_materials(h, 0, n, (yh.Material * n)(*[rows[i] if i != emitter else material(emitter, emission=[0.0, 0.0, 0.0])[0] for i in range(n)])), "yh_update_materials"),
    }, (cam, buf)


REFUSALS = ["camera-null", "materials-null", "environments-null", "display-null", "first-negative", "first-behind-the-table", "count-negative",
            "count-past-the-end", "count-huge", "environment-count", "environment-count-zero", "material-emission-on", "material-emission-off",
            "environment-emission-off", "color-tex", "emission-tex", "scattering-tex", "second-row-of-two"]


@pytest.fixture(scope="module")
def refusal_baseline(yh, hairblock):
    """2 + 2 samples on the untouched scene, from a context of its own: what every refused context must go on rendering."""
    return _fresh(yh, hairblock.desc, spp=2, first=2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", REFUSALS)
def test_refused_edits_leave_the_context_rendering(ctx, yh, hairblock, refusal_baseline, name):
    calls, _keep = _refusals(yh, hairblock)
    call, entry = calls[name]
    ctx.upload_scene(hairblock.desc)
    ctx.set_shard(0, 1)
    ctx.init_state(yh.TraceParams.default(resolution=RES))
    ctx.trace_samples(2)
    assert call(ctx.lib, ctx.h) == yh.YH_E_INVALID, name
    assert entry in ctx.lib.yh_last_error(ctx.h).decode(), ctx.lib.yh_last_error(ctx.h)
    ctx.trace_samples(2)  # the image state is still there, and the scene is the earlier one
    _same((ctx.download(), ctx.download_rng()), refusal_baseline, name)
    assert ctx.scene_once() == refusal_baseline[2]


@pytest.mark.gpu
def test_call_order(yh, hairblock):
    d = hairblock.desc.contents
    cam = yh.Camera.from_buffer_copy(d.camera)
    rows = (yh.Material * 1)(yh.Material.from_buffer_copy(d.materials[0]))
    envs = (yh.Environment * 1)(yh.Environment.from_buffer_copy(d.environments[0]))
    buf = np.zeros((RES, RES, 4), np.uint8)
    c = yh.Context(0)
    lib = c.lib
    u8 = buf.ctypes.data_as(C.POINTER(C.c_uint8))
    # before an upload
    assert lib.yh_update_camera(c.h, C.byref(cam)) == yh.YH_E_STATE
    assert lib.yh_update_materials(c.h, 0, 1, rows) == yh.YH_E_STATE
    assert lib.yh_update_environments(c.h, 1, envs) == yh.YH_E_STATE
    assert lib.yh_download_display(c.h, 0.0, 0, 1, u8) == yh.YH_E_STATE
    c.upload_scene(hairblock.desc)
    assert lib.yh_download_display(c.h, 0.0, 0, 1, u8) == yh.YH_E_STATE  # before yh_init_state
    p = yh.TraceParams.default(resolution=RES)
    for edit in (lambda: c.update_camera(cam), lambda: c.update_materials(0, rows), lambda: c.update_environments(envs)):
        c.init_state(p)
        c.trace_samples(1)
        edit()  # (an edit that changes no value is an edit all the same)
        assert lib.yh_trace_samples(c.h, 1) == yh.YH_E_STATE
        assert lib.yh_download_display(c.h, 0.0, 0, 1, u8) == yh.YH_E_STATE
    c.close()


# ---------------------------------------------------------------------------------------------
# the display download
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def display_image(yh):
    """The 4 spp image of the display tests on a context of its own, which the tests go on using."""
    sf = yh.SceneFile(scene_path(*DISPLAY_SCENE[:1], **DISPLAY_SCENE[1]))
    c = yh.Context(0)
    c.upload_scene(_display_description(yh, sf).ptr)
    yield c
    c.close(), sf.close()


def _check_display(got, img, exposure, filmic, srgb, owned=None):
    v, want = _restate_display(img, exposure, filmic, srgb)
    near = _near_step(v)
    share = near[..., :3].mean() if owned is None else near[owned][:, :3].mean()  # (a shard: of its own pixels; the others are zero, on both sides)
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"display {exposure, filmic, srgb}: {share:.4%} of the bytes near a step, {np.count_nonzero(diff)} differ, largest difference {diff.max()}")
    assert share <= NEAR_STEP_MAX
    assert np.array_equal(got[..., 3], want[..., 3]), "alpha bytes"
    assert diff.max() <= 1 and not (diff[~near] != 0).any(), f"{np.count_nonzero(diff[~near])} bytes differ away from a step, largest difference {diff.max()}"


@pytest.mark.gpu
@pytest.mark.parametrize("exposure,filmic,srgb", DISPLAY_SETTINGS)
def test_display_bytes_are_the_tone_mapped_image(display_image, yh, exposure, filmic, srgb):
    c = display_image
    c.set_shard(0, 1)
    c.init_state(yh.TraceParams.default(resolution=RES))
    c.trace_samples(4)
    img = c.download()
    assert np.isfinite(img).all() and img[..., 3].max() > 0
    got = c.download_display(exposure, bool(filmic), bool(srgb))
    assert got.shape == (RES, RES, 4) and len(np.unique(got[..., :3])) > 32
    _check_display(got, img, exposure, filmic, srgb)
    assert np.array_equal(c.download(), img)  # the image itself is untouched


@pytest.mark.gpu
def test_display_of_a_shard_leaves_other_pixels_zero(display_image, yh):
    c = display_image
    c.set_shard(1, 2)
    c.init_state(yh.TraceParams.default(resolution=RES))
    c.trace_samples(4)
    img, got = c.download(), c.download_display(0.0, False, True)
    c.set_shard(0, 1)
    j, i = np.mgrid[0:RES, 0:RES]
    owned = ((j // 8) * (RES // 8) + i // 8) % 2 == 1
    assert not got[~owned].any() and got[owned][:, :3].any()
    _check_display(got, img, 0.0, 0, 1, owned)


# ---------------------------------------------------------------------------------------------
# the mirror and the command line
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mirror_passes_edits_on_at_init_state(built, tmp_path):
    """set_frame on the camera and a hair setter on a material after an init_state: one upload, the edits through the update
    calls, pixels those of a scene built that way from the start; set_frame on an object: a second upload."""
    exe = _compile_mirror_test(tmp_path)
    r = subprocess.run([exe, scene_path("sphere-hairblock", scale=0.02)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)


@pytest.mark.gpu
def test_turntable_command_line(built, tmp_path):
    cli, scene = os.path.join(PKG, "ysceneitraces"), scene_path("sphere-hairblock", scale=0.02)
    common = [cli, scene, "-r", "32", "-s", "2"]
    r = subprocess.run(common + ["--turntable", "3", "-o", str(tmp_path / "x.pfm")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    plain = subprocess.run(common + ["-o", str(tmp_path / "y.pfm")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, (plain.stdout, plain.stderr)
    steps = [open(tmp_path / f"x-{k:03d}.pfm", "rb").read() for k in range(3)]
    assert sorted(os.listdir(tmp_path)) == ["x-000.pfm", "x-001.pfm", "x-002.pfm", "y.pfm"]
    assert steps[0] == open(tmp_path / "y.pfm", "rb").read()
    assert len(set(steps)) == 3
    assert r.stdout.count("edit to preview:") == 2 and r.stdout.count("the camera alone was passed on") == 2, r.stdout
    assert "edit to preview" not in plain.stdout and "-000" not in plain.stdout
