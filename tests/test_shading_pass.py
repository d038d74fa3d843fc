"""The shading pass of the plain 512-thread kernels (launch shape 0 and both halves of shape 5; csrc/dev_path.h: path_step, TRIM and CENV).

Those kernels fetch a hit's record in one round trip whatever its kind, spread the remaining divisions by a common denominator over the
quad, read the camera in 16-byte pieces and — for a scene whose lights are constant environments only (yh_lights_const_env) — take light
sampling, the light pdf and the environment lookup from the kernel argument. Nothing may change: every image and every final RNG state
here is compared bit for bit with what launch shape 3 (k_stream, one lane per path: none of that code) renders of the same scene, over
all pixels. Scenes are made here, through the C ABI: a block of slanted hair strands (256 segments) in front of a diffuse sphere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F = np.float32
EYE, LENS, FILM = (0.0, 0.0, 5.0), 0.14, 0.036


def _lookat(eye, center, up=(0, 1, 0)):
    """lookat_frame (yocto_math.h:3229-3239) as 12 floats x, y, z, o."""
    eye, center, up = (np.asarray(v, np.float64) for v in (eye, center, up))
    w = (eye - center) / np.linalg.norm(eye - center)
    u = np.cross(up, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    return [float(F(x)) for x in np.concatenate([u, v / np.linalg.norm(v), w, eye])]


def _strands(count=32, segments=8, half=0.5, z=1.5, radius=0.006):
    """`count` strands of `segments` segments across [-half, half]^2 at depth z, each slanted and bent a little."""
    t = np.linspace(-1.0, 1.0, segments + 1)
    pos, lines = [], []
    for s in range(count):
        x0 = -half + (s + 0.5) * 2 * half / count
        x = x0 + 0.11 * t + 0.01 * np.sin(3.0 * t + s)
        p = np.stack([x, half * t, z + 0.05 * np.cos(2.0 * t + 0.7 * s)], 1)
        base = len(pos) * (segments + 1)
        pos.append(p)
        lines += [[base + k, base + k + 1] for k in range(segments)]
    pos = np.concatenate(pos)
    tan = np.gradient(pos.reshape(count, segments + 1, 3), axis=1).reshape(-1, 3)
    tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    return pos.astype(F), tan.astype(F), np.full(len(pos), radius, F), np.asarray(lines, np.int32)


def _sphere(n_lon=24, n_lat=12):
    th, ph = np.linspace(0, np.pi, n_lat + 1), np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    nrm = np.array([[np.sin(a) * np.cos(b), np.cos(a), np.sin(a) * np.sin(b)] for a in th for b in ph])
    tri = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, b = i * n_lon + j, i * n_lon + (j + 1) % n_lon
            tri += [[a, a + n_lon, b + n_lon], [a, b + n_lon, b]]
    return nrm.astype(F), nrm.astype(F), np.asarray(tri, np.int32)


class Made:
    """A scene description and the arrays it points at. envs: emissions of the constant environments; lamp: a two-triangle area light."""

    def __init__(self, yh, envs, lamp=False):
        self.keep = []
        hp, ht, hr, hl = _strands()
        sp, sn, st = _sphere()
        shapes = [dict(positions=hp, normals=ht, radius=hr, lines=hl), dict(positions=sp, normals=sn, triangles=st)]
        if lamp:
            q = np.array([[-1, 3, -1], [1, 3, -1], [1, 3, 1], [-1, 3, 1]], F)
            shapes.append(dict(positions=q, normals=np.tile(F([0, -1, 0]), (4, 1)), triangles=np.array([[0, 1, 2], [0, 2, 3]], np.int32)))
        self.shapes = (yh.Shape * len(shapes))()
        for s, a in zip(self.shapes, shapes):
            for k in a:
                a[k] = np.ascontiguousarray(a[k])
            self.keep.append(a)
            s.num_vertices = len(a["positions"])
            s.positions, s.normals = yh.fptr(a["positions"]), yh.fptr(a["normals"])
            if "lines" in a:
                s.radius, s.num_lines, s.lines = yh.fptr(a["radius"]), len(a["lines"]), yh.iptr(a["lines"])
            else:
                s.num_triangles, s.triangles = len(a["triangles"]), yh.iptr(a["triangles"])
        n = len(shapes)
        self.materials = (yh.Material * n)()
        hair = yh.hair_material_rows([[0.25, 0.5, 0.9, 0.3, 0.3, 2.0, 1.55, 0, 0, 0, 0, 0]])[0]
        C.memmove(C.byref(self.materials[0]), C.byref(hair), C.sizeof(yh.Material))
        for m in list(self.materials)[1:]:
            m.opacity, m.ior, m.thin, m.trdepth, m.roughness = 1.0, 1.5, 1, 0.01, 1.0
        self.materials[1].color[:] = [0.7, 0.6, 0.5]
        if lamp:
            self.materials[2].emission[:] = [12.0, 11.0, 10.0]
        self.objects = (yh.Object * n)()
        for i, o in enumerate(self.objects):
            o.frame[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
            o.shape, o.material = i, i
        self.envs = (yh.Environment * len(envs))()
        for e, em in zip(self.envs, envs):
            e.frame[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
            e.emission[:] = list(em)
        d = self.d = yh.SceneDesc()
        d.num_shapes, d.shapes, d.num_materials, d.materials = n, self.shapes, n, self.materials
        d.num_objects, d.objects, d.num_environments, d.environments = n, self.objects, len(envs), self.envs
        d.camera.frame[:] = _lookat(EYE, (0, 0, 0))
        d.camera.lens, d.camera.focus, d.camera.aperture = LENS, 5.0, 0.0
        d.camera.film[:] = [FILM, FILM]

    @property
    def desc(self):
        return C.pointer(self.d)


SCENES = {"a": dict(envs=[(0.9, 1.0, 1.1)]), "b": dict(envs=[(0.5, 0.6, 0.7), (0.4, 0.3, 0.2)]), "c": dict(envs=[(0.3, 0.3, 0.4)], lamp=True)}
CONST_ENV = {"a": 1, "b": 1, "c": 0}


@pytest.fixture(scope="module")
def made(yh):
    return {k: Made(yh, **kw) for k, kw in SCENES.items()}


def _render(ctx, yh, monkeypatch, shape, res, spp):
    """Pixels (as uint32) and final RNG states of `spp` samples in two launches under launch shape `shape`."""
    monkeypatch.setenv("YHAIR_SHAPE", shape)
    ctx.init_state(yh.TraceParams.default(resolution=res, bounces=8))
    ctx.trace_samples(1), ctx.trace_samples(spp - 1)
    assert ctx.launch_shape() == int(shape)
    return np.ascontiguousarray(ctx.download()).view(np.uint32), ctx.download_rng()


def _same(got, want, what):
    bad = np.flatnonzero((got[0] != want[0]).reshape(-1, 4).any(1))
    assert bad.size == 0, f"{what}: {bad.size} pixels differ, first {bad[0]}"
    assert np.array_equal(got[1], want[1]), f"{what}: RNG states differ"


def _as_k_stream(ctx, yh, monkeypatch, what, res=64, spp=4):
    want = _render(ctx, yh, monkeypatch, "3", res, spp)
    assert want[0].view(F)[..., 3].max() > 0 and np.isfinite(want[0].view(F)).all()
    for shape in ("0", "5"):
        _same(_render(ctx, yh, monkeypatch, shape, res, spp), want, f"{what}, shape {shape} against shape 3")
    return want


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scenes_take_the_variant_they_should_and_render_k_streams_bits(ctx, yh, made, name, monkeypatch):
    ctx.upload_scene(made[name].desc)
    assert ctx.lights_const_env() == CONST_ENV[name]
    assert len(ctx.light_list()) == len(SCENES[name]["envs"]) + (1 if SCENES[name].get("lamp") else 0)
    _as_k_stream(ctx, yh, monkeypatch, f"scene ({name})")


@pytest.mark.parametrize("name", ["a", "b"])
def test_an_emission_edit_is_followed(ctx, yh, made, name, monkeypatch):
    """yh_update_environments with other emissions: the variant stays, the image is the edited scene's (the emissions are read from the
    kernel argument at every launch, nothing of them is kept aside)."""
    ctx.upload_scene(made[name].desc)
    before = _as_k_stream(ctx, yh, monkeypatch, f"scene ({name})")
    edited = Made(yh, envs=[tuple(2.0 * c + 0.25 for c in em) for em in SCENES[name]["envs"]])
    ctx.update_environments(edited.envs)
    assert ctx.lights_const_env() == 1
    after = _as_k_stream(ctx, yh, monkeypatch, f"scene ({name}) after the edit")
    assert not np.array_equal(after[0], before[0])
    ctx.upload_scene(edited.desc)  # a fresh upload of the edited description
    _same(_render(ctx, yh, monkeypatch, "0", 64, 4), after, "the edited scene against its fresh upload")


def test_the_flag_follows_a_light_switched_off_and_on(ctx, yh, made, monkeypatch):
    """Scene (c) with its lamp switched off is a scene of constant environments; with the lamp on again it is not. Scene (b) with one
    environment turned black keeps the flag: the black one is no light, and adds its zero to the lookup."""
    ctx.set_light_edits(True)
    try:
        ctx.upload_scene(made["c"].desc)
        assert ctx.lights_const_env() == 0
        lit = _as_k_stream(ctx, yh, monkeypatch, "scene (c)")
        off = Made(yh, **SCENES["c"])
        off.materials[2].emission[:] = [0, 0, 0]
        ctx.update_materials(2, [off.materials[2]])
        assert ctx.lights_const_env() == 1 and len(ctx.light_list()) == 1
        dark = _as_k_stream(ctx, yh, monkeypatch, "scene (c), lamp off")
        assert not np.array_equal(dark[0], lit[0])
        ctx.update_materials(2, [made["c"].materials[2]])
        assert ctx.lights_const_env() == 0 and len(ctx.light_list()) == 2
        _same(_as_k_stream(ctx, yh, monkeypatch, "scene (c), lamp on again"), lit, "scene (c) after off and on")
        ctx.upload_scene(made["b"].desc)
        one = Made(yh, envs=[SCENES["b"]["envs"][0], (0, 0, 0)])
        ctx.update_environments(one.envs)
        assert ctx.lights_const_env() == 1 and len(ctx.light_list()) == 1
        _as_k_stream(ctx, yh, monkeypatch, "scene (b), second environment black")
    finally:
        ctx.set_light_edits(False)


def test_shapes_0_5_and_the_octet_shape_agree(ctx, yh, made, monkeypatch):
    ctx.upload_scene(made["a"].desc)
    want = _render(ctx, yh, monkeypatch, "0", 64, 16)
    for shape in ("5", "4"):
        _same(_render(ctx, yh, monkeypatch, shape, 64, 16), want, f"shape {shape} against shape 0")


def test_quadrants_that_see_both_kinds_of_hit(ctx, yh, made, monkeypatch):
    """32 x 32: every 4 x 4 quadrant — one wave's sixteen paths — has first hits on the sphere and on hair, so the merged record fetch runs
    with both kinds in the wave from the first bounce on."""
    for name in ("a", "c"):
        ctx.upload_scene(made[name].desc)
        monkeypatch.setenv("YHAIR_SHAPE", "0")
        ctx.init_state(yh.TraceParams.default(resolution=32, bounces=8))
        obj = ctx.trace_gbuffer("centre", planes=["object"])["object"]
        blocks = obj.reshape(8, 4, 8, 4).transpose(0, 2, 1, 3).reshape(64, 16)
        assert all((b == 0).any() and (b == 1).any() for b in blocks), "a quadrant sees one kind of hit only"
        _as_k_stream(ctx, yh, monkeypatch, f"scene ({name}) at 32 x 32", res=32, spp=8)
