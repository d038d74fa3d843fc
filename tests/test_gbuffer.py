"""yh_trace_gbuffer / yh_trace_gbuffer_device (unit/gbuffer.hip): the first-hit feature pass — per pixel the camera ray's closest hit and
what the `normal` shader evaluates there — with the Python binding, the C++ mirror's trace_gbuffer and `yscenetrace --features`.

The yardsticks: the CPU oracle's and yh_intersect_batch's closest hits on the pass's own rays (bit for bit), the `normal` shader's next
sample (bit for bit), float64 numpy restatements of the camera (pt.cpp:211-229) and of the shading point (pt.cpp:232-311, 405-412) from
the scene description, and a fresh upload of an edited description.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_scene_edits import Edited
from test_object_edits import CROWD, HAIRBLOCK, Moved, _compose, _rotation, _translation
from test_shape_edits import Reshaped, _edited, _sway
from test_shape_refit import TIE_PIXELS
from point_f64 import _texture64  # eval_texture in float64 (shared with the shading-point tests)
from test_instances import GOLDEN_KW as FIELD_KW  # 339 objects: the scene level is walked as 4-wide nodes

F = np.float32
PKG = os.path.join(ROOT, "yocto-hair_amd")
FLT_MAX = np.finfo(F).max
PLANES = ("object", "element", "material", "uv", "distance", "position", "normal", "tangent", "texcoord", "albedo", "ray")
MODES = ("centre", "next")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _same_planes(got, want, what, names=PLANES):
    for n in names:
        assert got[n].shape == want[n].shape and np.array_equal(_bits(got[n]), _bits(want[n])), f"{what}: plane {n} differs"


@pytest.fixture(scope="module")
def scenes(yh):
    """Scene files by (name, options), loaded once."""
    held = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in held:
            held[key] = yh.SceneFile(scene_path(name, **kw))
        return held[key]
    yield get
    for sf in held.values():
        sf.close()


def _begin(ctx, yh, sf, res, shader="path", desc=None):
    ctx.upload_scene(desc if desc is not None else sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    return ctx.init_state(yh.TraceParams.default(resolution=res, shader=shader))


def _rays_of(g):
    n = g["object"].size
    return np.concatenate([g["ray"].reshape(n, 6), np.full((n, 1), 1e-4, F), np.full((n, 1), FLT_MAX, F)], axis=1).astype(F)


def _hits_of(g):
    n = g["object"].size
    return g["object"].ravel(), g["element"].ravel(), g["uv"].reshape(n, 2), g["distance"].ravel()


# ---------------------------------------------------------------------------------------------
# 1. the hits against the oracle and yh_intersect_batch
# ---------------------------------------------------------------------------------------------
HIT_SCENES = {"hairblock": ("sphere-hairblock", dict(scale=0.02), 64), "crowd": ("crowd", dict(scale=0.05), 64), "fur-field": ("fur-field", FIELD_KW, 64),
              "scene-once": ("scene-once", {}, 48), "lobes": ("lobes", dict(scale=0.05), 64)}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(HIT_SCENES))
def test_hits_are_the_oracles_and_the_ray_batchs(ctx, oracle, yh, scenes, case, mode):
    """object, element, uv and distance are, bit for bit, what the oracle and yh_intersect_batch find along the pass's own `ray` plane (no
    tie rule: tests/test_gpu_parity.py allows the closest hits none), and material is the description's objects[object].material."""
    name, kw, res = HIT_SCENES[case]
    sf = scenes(name, **kw)
    _begin(ctx, yh, sf, res)
    g = ctx.trace_gbuffer(mode)
    rays, got = _rays_of(g), _hits_of(g)
    osc = oracle.scene(sf.desc)
    want = osc.intersect(rays)
    osc.close()
    batch = ctx.intersect(rays)
    hit = got[0] >= 0
    print(f"{case} {mode}: {ctx.width}x{ctx.height}, {hit.mean():.3f} of the pixels hit, {len(set(got[0][hit]))} objects")
    assert 0.05 < hit.mean() <= 1.0
    for k, what in enumerate(("object", "element", "uv", "distance")):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), f"{what} differs from the oracle's on {np.count_nonzero(_bits(got[k]) != _bits(want[k]))} entries"
        assert np.array_equal(_bits(got[k]), _bits(batch[k])), f"{what} differs from yh_intersect_batch's"
    d = sf.desc.contents
    mats = np.array([d.objects[i].material for i in range(d.num_objects)], np.int32)
    assert np.array_equal(g["material"].ravel()[hit], mats[got[0][hit]]) and np.all(g["material"].ravel()[~hit] == -1)


# ---------------------------------------------------------------------------------------------
# 2. next-sample mode against the `normal` shader
# ---------------------------------------------------------------------------------------------
NORMAL_SCENES = {"hairblock-dof": ("sphere-hairblock", dict(scale=0.05, dof=True)), "maps": ("maps", {}), "lobes": ("lobes", dict(scale=0.05)),
                 "textured": ("textured", dict(scale=0.05)), "fur-field": ("fur-field", FIELD_KW)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(NORMAL_SCENES))
def test_next_sample_is_what_the_normal_shader_renders(ctx, yh, scenes, case):
    """After the pass in next-sample mode, one sample of the `normal` shader is float32(normal) * 0.5 + 0.5 with alpha 1 on every hit pixel,
    bit for bit (the product by 0.5 is exact, so fused or not the expression rounds once); the pass leaves the pixels' streams as they
    were, and the image is the one rendered without the pass."""
    name, kw = NORMAL_SCENES[case]
    sf = scenes(name, **kw)
    _begin(ctx, yh, sf, 64, "normal")
    if case == "hairblock-dof":
        assert sf.desc.contents.camera.aperture != 0
    ctx.trace_samples(1)
    plain = ctx.download()
    ctx.init_state(yh.TraceParams.default(resolution=64, shader="normal"))
    rng0 = ctx.download_rng()
    g = ctx.trace_gbuffer("next")
    assert np.array_equal(ctx.download_rng(), rng0), "the pass moved a pixel's stream"
    ctx.trace_samples(1)
    img = ctx.download()
    assert np.array_equal(_bits(img), _bits(plain)), "a render with the pass in between differs from one without"
    hit = g["object"] >= 0
    want = g["normal"] * F(0.5) + F(0.5)
    print(f"{case}: {hit.mean():.3f} of the pixels hit")
    assert 0.05 < hit.mean()
    assert np.array_equal(_bits(img[hit][:, :3]), _bits(want[hit])), f"{np.count_nonzero((_bits(img[hit][:, :3]) != _bits(want[hit])).any(-1))} hit pixels differ"
    assert np.all(img[hit][:, 3] == 1)
    if case in ("maps", "textured"):  # the pass meets normal maps / texture coordinates there
        assert np.any(g["texcoord"][hit] != g["uv"][hit])


# ---------------------------------------------------------------------------------------------
# 3., 4. centre mode: the ray
# ---------------------------------------------------------------------------------------------
def _with_camera(yh, sf, **fields):
    e = Edited(yh, sf.desc)
    for k, v in fields.items():
        if k in ("film", "frame"):
            getattr(e.d.camera, k)[:] = [float(x) for x in v]
        else:
            setattr(e.d.camera, k, v)
    return e


def _camera_rays64(cam, w, h):
    """pt.cpp:211-229 in float64 at the pixel centres with the lens point at zero: directions (h, w, 3)."""
    i, j = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    u, v = (i + 0.5) / w, (j + 0.5) / h
    q = np.stack([cam.film[0] * (0.5 - u), cam.film[1] * (v - 0.5), np.full_like(u, cam.lens)], -1)
    dc = -q / np.linalg.norm(q, axis=-1, keepdims=True)
    p = dc * cam.focus / np.abs(dc[..., 2:3])
    d = p / np.linalg.norm(p, axis=-1, keepdims=True)
    fr = np.array(cam.frame[:], np.float64).reshape(4, 3)
    out = d[..., 0:1] * fr[0] + d[..., 1:2] * fr[1] + d[..., 2:3] * fr[2]
    return out / np.linalg.norm(out, axis=-1, keepdims=True)


@pytest.mark.gpu
def test_centre_ray_is_the_pinhole_ray_through_the_pixel_centre(ctx, yh, scenes):
    """On a 100 x 75 image (a non-square film, no multiple of the 8 x 8 tile): the origin is the camera frame's, every direction component
    within 1e-6 of the float64 camera — a dozen float32 roundings of 6e-8 on components of at most 1 — and an aperture changes no bit."""
    sf = scenes(*HAIRBLOCK[:1], **HAIRBLOCK[1])
    pin = _with_camera(yh, sf, film=(0.036, 0.027), aperture=0.0)
    lens = _with_camera(yh, sf, film=(0.036, 0.027), aperture=0.25, focus=3.0)
    pin.d.camera.focus = 3.0
    assert _begin(ctx, yh, sf, 100, desc=pin.ptr) == (100, 75)
    g = ctx.trace_gbuffer("centre")
    cam = pin.d.camera
    assert np.array_equal(g["ray"][..., :3], np.broadcast_to(np.array(cam.frame[9:12], F), (75, 100, 3)))
    err = np.abs(g["ray"][..., 3:].astype(np.float64) - _camera_rays64(cam, 100, 75))
    print(f"direction: max error {err.max():.3g} against the float64 camera")
    assert err.max() <= 1e-6
    hit = g["object"] >= 0
    assert 0.05 < hit.mean() < 0.999
    assert _begin(ctx, yh, sf, 100, desc=lens.ptr) == (100, 75)
    _same_planes(ctx.trace_gbuffer("centre"), g, "with an aperture")
    dof = ctx.trace_gbuffer("next")  # ... which the next sample's ray does see
    assert not np.array_equal(dof["ray"][..., :3], g["ray"][..., :3])


def _bbox(d, objects=None):
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for k in (range(d.num_objects) if objects is None else objects):
        o = d.objects[k]
        s = d.shapes[o.shape]
        p = np.ctypeslib.as_array(s.positions, (s.num_vertices, 3)).astype(np.float64)
        fr = np.array(o.frame[:], np.float64).reshape(4, 3)
        w = p @ fr[:3] + fr[3]
        lo, hi = np.minimum(lo, w.min(0)), np.maximum(hi, w.max(0))
    return lo, hi


@pytest.mark.gpu
def test_axis_parallel_centre_ray_takes_the_exact_redo(ctx, oracle, yh, scenes):
    """An axis-aligned camera frame and an odd resolution: the centre pixel's ray is exactly -z, which the traversal hands to the exact
    form (an infinite 1 / d). Its hit, and every other pixel's, is the oracle's."""
    sf = scenes(*HAIRBLOCK[:1], **HAIRBLOCK[1])
    d = sf.desc.contents
    ball = [k for k in range(d.num_objects) if d.shapes[d.objects[k].shape].num_triangles > 0][0]
    lo, hi = _bbox(d, [ball])
    c = (lo + hi) / 2  # (the camera looks down -z of its frame, at the middle of the sphere)
    e = _with_camera(yh, sf, frame=[1, 0, 0, 0, 1, 0, 0, 0, 1, c[0], c[1], hi[2] + 3.0], film=(0.036, 0.036))
    assert _begin(ctx, yh, sf, 75, desc=e.ptr) == (75, 75)
    g = ctx.trace_gbuffer("centre")
    assert np.array_equal(g["ray"][37, 37, 3:], np.array([0, 0, -1], F)), g["ray"][37, 37]
    osc = oracle.scene(e.ptr)
    want = osc.intersect(_rays_of(g))
    osc.close()
    k = 37 * 75 + 37
    assert want[0][k] >= 0, "the centre ray meets nothing: aim the camera elsewhere"
    for a, b, what in zip(_hits_of(g), want, ("object", "element", "uv", "distance")):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"centre pixel: {what} {a[k]} against the oracle's {b[k]}"
        assert np.array_equal(_bits(a), _bits(b)), what


# ---------------------------------------------------------------------------------------------
# 5. the derived planes against float64 numpy
# ---------------------------------------------------------------------------------------------
def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


# lobes-inside: the camera in the middle of a ball with a thin material, so that every normal it sees faces away and is flipped
DERIVED = {"hairblock": ("sphere-hairblock", dict(scale=0.02)), "lobes": ("lobes", dict(scale=0.05)), "lobes-inside": ("lobes", dict(scale=0.05)),
           "textured": ("textured", dict(scale=0.05))}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(DERIVED))
def test_derived_planes_follow_the_description(ctx, yh, scenes, case):
    """position and texcoord within 1e-5 x the scene's diagonal (a few float32 roundings of quantities it bounds), tangent within 2e-5 per
    component, albedo the material's colour bits (untextured) or within 1e-5 of the float64 bilinear lookup, normal of unit length within
    1e-5 and, on a strand, orthogonal to the tangent within 1e-5 and facing the ray's origin, on a triangle the interpolated vertex normal
    within 2e-5, flipped where a thin material faces away; a miss is -1 in the id planes and 0 elsewhere."""
    name, kw = DERIVED[case]
    sf = scenes(name, **kw)
    d = sf.desc.contents
    desc = None
    if case == "lobes-inside":
        ball = [k for k in range(d.num_objects) if d.shapes[d.objects[k].shape].num_triangles > 100 and d.materials[d.objects[k].material].thin][0]
        lo, hi = _bbox(d, [ball])
        desc = _with_camera(yh, sf, frame=[1, 0, 0, 0, 1, 0, 0, 0, 1] + list((lo + hi) / 2)).ptr
    _begin(ctx, yh, sf, 75, desc=desc)
    g = {k: v.reshape(-1, *v.shape[2:]) for k, v in ctx.trace_gbuffer("centre").items()}
    lo, hi = _bbox(d)
    diag = np.linalg.norm(hi - lo)
    hit = g["object"] >= 0
    for k in ("element", "material"):
        assert np.all(g[k][~hit] == -1)
    for k in ("uv", "distance", "position", "normal", "tangent", "texcoord", "albedo"):
        assert not g[k][~hit].any(), f"{k} of a miss"
    assert 0.05 < hit.mean() and (hit.mean() < 1.0 or case == "lobes-inside")
    assert np.abs(np.linalg.norm(g["normal"][hit].astype(np.float64), axis=-1) - 1).max() <= 1e-5
    kinds, flipped, textured = set(), 0, 0
    for ob in np.unique(g["object"][hit]):
        px = np.flatnonzero(g["object"] == ob)
        o = d.objects[int(ob)]
        s, m = d.shapes[o.shape], d.materials[o.material]
        fr = np.array(o.frame[:], np.float64).reshape(4, 3)
        lines = s.num_lines > 0
        idx = np.ctypeslib.as_array(s.lines, (s.num_lines, 2)) if lines else np.ctypeslib.as_array(s.triangles, (s.num_triangles, 3))
        e, u, v = idx[g["element"][px]], g["uv"][px, 0:1].astype(np.float64), g["uv"][px, 1:2].astype(np.float64)
        wts = [1 - u, u] if lines else [1 - u - v, u, v]

        def interp(ptr, cols):
            a = np.ctypeslib.as_array(ptr, (s.num_vertices, cols)).astype(np.float64)
            return sum(a[e[:, k]] * wts[k] for k in range(len(wts)))
        pos = interp(s.positions, 3) @ fr[:3] + fr[3]
        assert np.abs(g["position"][px] - pos).max() <= 1e-5 * diag, f"object {ob}: position"
        tc = interp(s.texcoords, 2) if s.texcoords else g["uv"][px].astype(np.float64)
        assert np.abs(g["texcoord"][px] - tc).max() <= 1e-5 * diag, f"object {ob}: texcoord"
        if m.color_tex == 0:
            assert np.array_equal(_bits(g["albedo"][px]), np.broadcast_to(_bits(np.array(m.color[:], F)), (len(px), 3))), f"object {ob}: albedo"
        else:
            textured += 1
            want = np.array(m.color[:], np.float64) * _texture64(d.textures[m.color_tex - 1], g["texcoord"][px, 0].astype(np.float64), g["texcoord"][px, 1].astype(np.float64))
            assert np.abs(g["albedo"][px] - want).max() <= 1e-5, f"object {ob}: albedo {np.abs(g['albedo'][px] - want).max():.3g} off the lookup"
        pts = np.ctypeslib.as_array(s.positions, (s.num_vertices, 3)).astype(np.float64)
        if s.normals:
            nrm = _unit(_unit(interp(s.normals, 3)) @ fr[:3])
        elif lines:
            nrm = _unit(_unit(pts[e[:, 1]] - pts[e[:, 0]]) @ fr[:3])
        else:
            nrm = _unit(_unit(np.cross(pts[e[:, 1]] - pts[e[:, 0]], pts[e[:, 2]] - pts[e[:, 0]])) @ fr[:3])
        out = -g["ray"][px, 3:].astype(np.float64)
        n = g["normal"][px].astype(np.float64)
        kinds.add(lines)
        if lines:
            assert np.abs(g["tangent"][px] - nrm).max() <= 2e-5, f"object {ob}: tangent"
            assert np.abs((n * g["tangent"][px]).sum(-1)).max() <= 1e-5 and ((n * out).sum(-1) >= 0).all(), f"object {ob}: strand normal"
        else:
            assert not g["tangent"][px].any()
            away = (nrm * out).sum(-1) < 0
            if m.thin:
                flipped += int(away.sum())
                nrm = np.where(away[:, None], -nrm, nrm)
            assert np.abs(n - nrm).max() <= 2e-5, f"object {ob}: normal"
    print(f"{case}: {hit.mean():.3f} hit, lines and triangles {sorted(kinds)}, {flipped} normals flipped, {textured} textured objects")
    assert kinds == {False, True} if case == "hairblock" else False in kinds
    assert case != "textured" or textured > 0
    assert case != "lobes-inside" or flipped > 1000


# ---------------------------------------------------------------------------------------------
# 6. plane skipping and the device form
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_single_planes_and_the_device_form(ctx, yh, scenes, mode):
    """Every plane asked for alone is the plane of a full request; the device form writes the same bits into torch tensors, and a tensor one
    row larger keeps its guard row."""
    import torch
    sf = scenes("textured", scale=0.05)
    w, h = _begin(ctx, yh, sf, 61)
    full = ctx.trace_gbuffer(mode)
    assert (full["object"] >= 0).mean() > 0.05
    for name in PLANES:
        alone = ctx.trace_gbuffer(mode, planes=[name])
        assert list(alone) == [name]
        _same_planes(alone, full, f"{name} alone", names=[name])
    comps = {n: c for n, _, c in yh.GBUFFER_PLANES}
    dev = {n: torch.full((h + 1, w, comps[n]), -7, dtype=torch.int32 if full[n].dtype == np.int32 else torch.float32, device="cuda") for n in PLANES}
    ctx.trace_gbuffer_device(mode, **dev)
    for n in PLANES:
        t = dev[n].cpu().numpy()
        assert np.all(t[h] == -7), f"{n}: the guard row was written"
        assert np.array_equal(_bits(t[:h].reshape(full[n].shape)), _bits(full[n])), f"{n}: the device form differs from the host form"
    one = torch.full((h + 1, w), -7, dtype=torch.float32, device="cuda")
    ctx.trace_gbuffer_device(mode, distance=one)
    assert np.array_equal(_bits(one.cpu().numpy()[:h]), _bits(full["distance"])) and bool((one[h] == -7).all())
    ms, launches = ctx.last_trace_ms()
    assert ms > 0 and launches == 1


# ---------------------------------------------------------------------------------------------
# 7. after edits
# ---------------------------------------------------------------------------------------------
def _fresh_pass(yh, desc, maps, res, mode):
    c = yh.Context(0)
    try:
        c.upload_scene(desc, maps)
        c.init_state(yh.TraceParams.default(resolution=res))
        return c.trace_gbuffer(mode)
    finally:
        c.close()


@pytest.mark.gpu
def test_pass_after_camera_and_object_edits_is_the_pass_on_a_fresh_upload(ctx, yh, scenes):
    sf = scenes(*CROWD[:1], **CROWD[1])
    _begin(ctx, yh, sf, 64)
    before = ctx.trace_gbuffer("centre")
    new = Moved(yh, sf.desc)
    f = np.array(new.d.camera.frame[:], np.float64)
    f[9:12] += 0.35 * f[0:3] + 0.2 * f[3:6]
    new.d.camera.frame[:] = [float(x) for x in f.astype(F)]
    new.d.camera.aperture = 0.05
    ctx.update_camera(new.d.camera)
    o = new.index(lines=False, emissive=False)[3]  # one of the balls
    new.set_frames([_compose(_translation(0.3, 0.2, 0.1), _compose(new.frames()[o], _rotation((0, 1, 0), 25.0)))], first=o)
    ctx.update_objects(o, new.rows(yh, o, 1))
    assert ctx.lib.yh_trace_gbuffer(ctx.h, 0, C.byref(yh.GBuffer())) == yh.YH_E_STATE  # (an edit takes the image state with it)
    ctx.init_state(yh.TraceParams.default(resolution=64))
    for mode in MODES:
        got = ctx.trace_gbuffer(mode)
        _same_planes(got, _fresh_pass(yh, new.ptr, sf.maps, 64, mode), f"after the edits, {mode}")
    assert not np.array_equal(got["object"], before["object"])


@pytest.mark.gpu
def test_pass_after_a_refit_has_the_distances_of_a_fresh_upload(ctx, yh, scenes):
    """After yh_refit_shape of a swayed hair block the refitted tree is another tree over the same primitives (tests/test_shape_refit.py):
    distances are the same bits, and object, element and uv may differ only where two primitives lie at the bit-equal closest distance — on
    at most TIE_PIXELS of the 48 x 48 pixels, that test's cap."""
    sf = scenes(*HAIRBLOCK[:1], **HAIRBLOCK[1])
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    new = _edited(yh, sf.desc, s, _sway(base.arrays(s), 0.1))
    _begin(ctx, yh, sf, 48)
    before = ctx.trace_gbuffer("centre")
    ctx.refit_shape(s, new.shapes[s])
    ctx.init_state(yh.TraceParams.default(resolution=48))
    for mode in MODES:
        got, want = ctx.trace_gbuffer(mode), _fresh_pass(yh, new.ptr, sf.maps, 48, mode)
        _same_planes(got, want, f"after the refit, {mode}", names=["distance", "ray", "material"])
        other = (got["object"] != want["object"]) | (got["element"] != want["element"]) | (_bits(got["uv"]) != _bits(want["uv"])).any(-1)
        print(f"{mode}: {np.count_nonzero(other)} of {other.size} pixels differ in object, element or uv at a bit-equal distance")
        assert other.size == 2304 and np.count_nonzero(other) <= TIE_PIXELS
    assert not np.array_equal(_bits(got["distance"]), _bits(before["distance"]))


# ---------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_the_context_rendering(yh, scenes):
    sf = scenes(*HAIRBLOCK[:1], **HAIRBLOCK[1])
    c = yh.Context(0)
    dist = np.zeros(64 * 64, F)
    g = yh.GBuffer()
    g.distance = yh.fptr(dist)
    for fn in (c.lib.yh_trace_gbuffer, c.lib.yh_trace_gbuffer_device):
        assert fn(c.h, 0, C.byref(g)) == yh.YH_E_STATE and b"before yh_upload_scene" in c.lib.yh_last_error(c.h)
    c.upload_scene(sf.desc)
    for fn in (c.lib.yh_trace_gbuffer, c.lib.yh_trace_gbuffer_device):
        assert fn(c.h, 0, C.byref(g)) == yh.YH_E_STATE and b"before yh_init_state" in c.lib.yh_last_error(c.h)
    p = yh.TraceParams.default(resolution=64)
    c.init_state(p)
    c.trace_samples(2)
    want, want_rng = c.download(), c.download_rng()
    c.init_state(p)
    c.trace_samples(1)
    for fn in (c.lib.yh_trace_gbuffer, c.lib.yh_trace_gbuffer_device):
        for mode in (-1, 2, 77):
            assert fn(c.h, mode, C.byref(g)) == yh.YH_E_INVALID and b"unknown mode" in c.lib.yh_last_error(c.h)
        assert fn(c.h, 0, None) == yh.YH_E_INVALID
        assert fn(c.h, 0, C.byref(yh.GBuffer())) == yh.YH_E_INVALID and b"every plane is NULL" in c.lib.yh_last_error(c.h)
    assert not dist.any()
    c.trace_samples(1)
    assert np.array_equal(_bits(c.download()), _bits(want)) and np.array_equal(c.download_rng(), want_rng)
    assert c.lib.yh_trace_gbuffer(c.h, 0, C.byref(g)) == yh.YH_OK and dist.any()
    c.close()


# ---------------------------------------------------------------------------------------------
# the mirror and the command line
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mirror_returns_the_planes_of_the_c_abi(built, tmp_path):
    exe = str(tmp_path / "mirror_gbuffer")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host"), "-Wno-class-memaccess", os.path.join(ROOT, "tests", "cpp", "test_mirror_gbuffer.cpp"),
                           "-o", exe, "-L" + PKG, "-lyhair", "-Wl,-rpath," + PKG, "-lpthread"])
    r = subprocess.run([exe, scene_path(*HAIRBLOCK[:1], **HAIRBLOCK[1])], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)


def _read_hdr(path):
    """A flat RGBE file as yh_save_image writes it: mantissa * 2^(e - 136) per channel (stb_image.h:6726-6751), (h, w, 3) float64."""
    raw = open(path, "rb").read()
    head, _, rest = raw.partition(b"\n\n")
    assert head.startswith(b"#?RADIANCE")
    dims, _, data = rest.partition(b"\n")
    _, h, _, w = dims.split()
    px = np.frombuffer(data, np.uint8).reshape(int(h), int(w), 4).astype(np.float64)
    return np.where(px[..., 3:] > 0, px[..., :3] * np.exp2(px[..., 3:] - 136), 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("cli", ["yscenetrace", "ysceneitraces"])
def test_command_lines_write_the_features(ctx, yh, scenes, tmp_path, cli):
    """--features PREFIX writes PREFIX.{normal,albedo,depth,ids}.hdr. RGBE keeps, per pixel, floor(v * 256 / 2^e) of each channel with 2^e
    the power of two above the largest channel m: a decoded channel is off by less than 2^(e - 8) <= m / 128. The files hold the planes'
    normal * 0.5 + 0.5, albedo and distance within that."""
    scene = scene_path(*HAIRBLOCK[:1], **HAIRBLOCK[1])
    prefix = str(tmp_path / "f")
    r = subprocess.run([os.path.join(PKG, cli), scene, "-r", "64", "-s", "1", "-o", str(tmp_path / "img.hdr"), "--features", prefix],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert sorted(os.listdir(tmp_path)) == ["f.albedo.hdr", "f.depth.hdr", "f.ids.hdr", "f.normal.hdr", "img.hdr"]
    _begin(ctx, yh, scenes(*HAIRBLOCK[:1], **HAIRBLOCK[1]), 64)
    g = ctx.trace_gbuffer("centre")
    hit = g["object"] >= 0
    want = {"normal": np.where(hit[..., None], g["normal"] * F(0.5) + F(0.5), 0), "albedo": g["albedo"], "depth": np.repeat(g["distance"][..., None], 3, -1)}
    for name, v in want.items():
        got, v = _read_hdr(prefix + f".{name}.hdr"), v.astype(np.float64)
        assert got.shape == v.shape
        assert np.all(np.abs(v - got) <= v.max(-1, keepdims=True) / 128), f"{name}: {np.abs(v - got).max():.3g} off the plane"
    ids = _read_hdr(prefix + ".ids.hdr")
    assert ids.shape == (64, 64, 3) and np.all(ids[~hit] == 0) and ids[hit].max() > 0
