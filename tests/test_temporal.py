"""The temporal stage on the device (unit/reproject.hip, host/temporal.cpp): yh_reproject_gpu against the host's form, the context entries
yh_temporal_accumulate / _device / _display over camera and object edits against the host's form on the downloaded render, the planes of
yh_trace_gbuffer and the previous step's result, what keeps and what drops the history, what the calls leave alone, what they refuse, the
sign conventions of the projection, and the quality condition.

The yardstick of the arithmetic is yh_reproject, which tests/test_temporal_cpu.py holds bit for bit to the numpy restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

import reproject_f32
import reproject_f64
from conftest import scene_path
from temporal_cases import SIZES, STRATA, arguments, bits, make_case
from test_object_edits import Moved, _compose, _rotation, _translation
from test_scene_edits import _near_step, _restate_display
from test_shape_edits import Reshaped, _edited, _sway

F = np.float32
SCENES = {"hairblock": ("sphere-hairblock", dict(scale=0.05, zoom=True)), "textured": ("textured", dict(scale=0.05)), "lobes": ("lobes", dict(scale=0.05)),
          "crowd": ("crowd", dict(scale=0.05))}
RES, SPP, REFERENCE_SPP = 64, 4, 1024
EDGE = (7, 8, 9, 17)  # widths and heights around the 8 x 8 tile: partly empty tiles


def _params(yh, P):
    return yh.TemporalParams(P["max_history"], P["sigma_position"], P["match_object"])


def _check_display(got, img, exposure, filmic, srgb):
    """The bytes are the tone map of `img` (tests/test_scene_edits.py's restatement): alpha exactly, colour within one step and only where the
    float value sits near a step of the byte."""
    v, want = _restate_display(img, exposure, filmic, srgb)
    near = _near_step(v)
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"display {exposure, filmic, srgb}: {near[..., :3].mean():.4%} of the bytes near a step, {np.count_nonzero(diff)} differ, largest difference {diff.max()}")
    assert np.array_equal(got[..., 3], want[..., 3]), "alpha bytes"
    assert diff.max() <= 1 and not (diff[~near] != 0).any(), f"{np.count_nonzero(diff[~near])} bytes differ away from a step, largest difference {diff.max()}"
    assert near[..., :3].mean() < 0.05, "the comparison away from the steps covers the image"


def _same(got, want, what):
    diff = bits(got) != bits(want)
    assert not diff.any(), f"{what}: {np.count_nonzero(diff)} of {diff.size} entries differ, first at {np.argwhere(diff)[0]}"


# ---------------------------------------------------------------------------------------------
# 1. the unit pair
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("stratum", STRATA)
def test_device_form_is_the_host_form_bit_for_bit(ctx, yh, stratum):
    for size in SIZES + tuple((w, h) for w in EDGE for h in EDGE):
        case = make_case(stratum, *size)
        p, args = _params(yh, case["P"]), arguments(case)
        want, want_len = yh.reproject(p, *args)
        got, got_len = ctx.reproject_gpu(p, *args)
        _same(got, want, f"{stratum} {size}")
        _same(got_len, want_len, f"{stratum} {size}: lengths")
        assert ctx.last_trace_ms()[1] == 2
    args[4] = None  # the seed of a first frame
    want, want_len = yh.reproject(p, *args)
    got, got_len = ctx.reproject_gpu(p, *args)
    _same(got, want, f"{stratum}: no history")
    _same(got_len, want_len, f"{stratum}: no history, lengths")


# ---------------------------------------------------------------------------------------------
# 2. the context entries over edits
# ---------------------------------------------------------------------------------------------
def _camera_floats(cam):
    return np.frombuffer(bytes(cam), F).copy()


def _orbit(new, degrees):
    """The description's camera turned about the vertical through the point it focuses on."""
    f = np.array(new.d.camera.frame[:], np.float64)
    centre = f[9:12] - new.d.camera.focus * f[6:9]
    new.d.camera.frame[:] = _compose(_rotation((0, 1, 0), degrees, centre), list(f))


def _render(ctx, yh, seed):
    ctx.init_state(yh.TraceParams.default(resolution=RES, seed=seed))
    ctx.trace_samples(SPP)
    g = ctx.trace_gbuffer("centre", ("object", "position"))
    return ctx.download(), g["object"], g["position"]


def _accumulate(ctx, yh, entry, p, dp, render, ids, pos):
    """One step through `entry`; returns the accumulated image, or for `display` the bytes."""
    if entry == "device":
        out = torch.zeros((ctx.height, ctx.width, 4), device="cuda")
        ctx.temporal_accumulate_device(p, out)
        assert ctx.last_trace_ms()[1] == 2  # the feature pass and the kernel
        return out.cpu().numpy()
    if entry == "device-given":  # the render and the planes passed in, in place
        image, o, x = torch.from_numpy(render).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(pos).cuda()
        ctx.temporal_accumulate_device(p, image, rgba_in=image, samples=SPP, object=o, position=x)
        assert ctx.last_trace_ms()[1] == 1
        return image.cpu().numpy()
    if entry == "host":
        return ctx.temporal_accumulate(p)
    if entry == "host-given":
        return ctx.temporal_accumulate(p, render, SPP, ids, pos)
    if entry == "update-only":
        assert ctx.temporal_accumulate(p, want_image=False) is None
        return None
    assert entry == "display"
    return ctx.temporal_display(p, dp, 0.5, True, True)


ENTRIES = ("device", "device-given", "host", "host-given", "update-only", "display")


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", ("hairblock", "textured", "crowd"))
def test_context_steps_are_the_host_form_on_the_downloads(ctx, yh, case, entry):
    """A first frame and three edits — an orbit of 1 degree per step, on crowd three moves of a ball and of the hair — each followed by
    yh_init_state, 4 spp and one accumulate through `entry`: image and lengths are yh_reproject's on the downloaded render, the planes of
    yh_trace_gbuffer and the previous step's result, so every entry equals every other."""
    name, kw = SCENES[case]
    sf = yh.SceneFile(scene_path(name, **kw))
    new = Moved(yh, sf.desc)
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    p, dp = ctx.temporal_default_params(), None
    assert p.max_history == 4 and p.sigma_position > 0 and p.match_object == 1
    assert ctx.temporal_lengths() is None, "an upload drops the history"
    ball, hair = new.index(lines=False, emissive=False)[-1], new.index(lines=True)[0]
    hist = prev_cam = prev_frames = None
    for step in range(4):
        if step > 0 and case == "crowd":
            o = ball if step != 2 else hair
            new.set_frames([_compose(_translation(0.02 * step, 0.0, 0.015), _compose(new.frames()[o], _rotation((0, 1, 0), 4.0 * step)))], first=o)
            ctx.update_objects(o, new.rows(yh, o, 1))
        elif step > 0:
            _orbit(new, 1.0)
            ctx.update_camera(new.d.camera)
        render, ids, pos = _render(ctx, yh, 7 + step)
        cam, frames = _camera_floats(new.d.camera), np.array(new.frames(), F)
        want, want_len = yh.reproject(p, render, SPP, ids, pos, hist, cam, prev_cam, frames, prev_frames)
        if entry == "display":
            dp = ctx.denoise_default_params() if step != 1 else None
        got = _accumulate(ctx, yh, entry, p, dp, render, ids, pos)
        if entry == "display":
            image = want
            if dp is not None:
                g = ctx.trace_gbuffer("centre", ("object", "normal", "position", "albedo"))
                image = yh.atrous_filter(dp, want, g["object"], g["normal"], g["position"], g["albedo"])
            _check_display(got, image, 0.5, 1, 1)
        elif got is not None:
            _same(got, want, f"{case} step {step} through {entry}")
        _same(ctx.temporal_lengths(), want_len, f"{case} step {step} through {entry}: lengths")
        _same(ctx.download(), render, "the render itself is untouched")
        hit = ids >= 0
        if step > 0:
            took = want_len > SPP
            print(f"{case} step {step}: {took.sum()} of {hit.sum()} hit pixels reuse the history, longest {want_len.max()}")
            assert took.sum() > 0.5 * hit.sum()
        hist, prev_cam, prev_frames = (want, want_len, ids, pos), cam, frames
    assert want_len.max() == SPP + min(p.max_history, 3 * SPP)
    sf.close()


@pytest.mark.gpu
def test_a_still_view_with_two_seeds_accumulates_by_the_one_tap_rule(ctx, yh):
    name, kw = SCENES["textured"]
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    p = ctx.temporal_default_params()
    a, ids, pos = _render(ctx, yh, 21)
    first = ctx.temporal_accumulate(p)
    _same(first, a, "the first frame passes through")
    b, ids_b, pos_b = _render(ctx, yh, 22)
    _same(ids_b, ids, "ids")
    _same(pos_b, pos, "positions")
    got = ctx.temporal_accumulate(p)
    cam = _camera_floats(sf.desc.contents.camera)
    restated, restated_len = yh.reproject(p, b, SPP, ids, pos, (a, np.where((ids >= 0) & np.isfinite(a[..., :3]).all(-1), SPP, 0).astype(np.int32), ids, pos), cam, cam)
    live = restated_len == 2 * SPP  # (a strand's axis point may project off the image at its border: no history there)
    assert live.sum() > 0.99 * ((ids >= 0) & np.isfinite(a[..., :3]).all(-1) & np.isfinite(b[..., :3]).all(-1)).sum()
    want = b.copy()
    h, c = a[..., :3][live], b[..., :3][live]
    want[..., :3][live] = h + (c - h) * (F(SPP) / F(2 * SPP))  # the one tap (i, j) with weight 1: sum w c / sum w = c's bits
    _same(got, want, "a still view")
    assert live.sum() > 0.3 * live.size
    _same(got, restated, "... and yh_reproject's")
    _same(ctx.temporal_lengths(), restated_len, "lengths")
    sf.close()


@pytest.mark.gpu
def test_what_keeps_and_what_drops_the_history(ctx, yh):
    """A refit makes the shape's objects unusable for one step and keeps the rest; yh_update_materials, yh_temporal_reset, a yh_init_state
    of another size and an upload drop the history; a yh_init_state of the same size keeps it."""
    name, kw = SCENES["hairblock"]
    sf = yh.SceneFile(scene_path(name, **kw))
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    users = [o for o in range(base.n) if base.objects[o].shape == s]
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    p = ctx.temporal_default_params()
    cam, frames = _camera_floats(sf.desc.contents.camera), np.array(base.frames(), F)
    render, ids, pos = _render(ctx, yh, 3)
    out = ctx.temporal_accumulate(p)
    hist = (out, ctx.temporal_lengths(), ids, pos)
    # a refit
    new = _edited(yh, sf.desc, s, _sway(base.arrays(s), 0.02))
    ctx.refit_shape(s, new.shapes[s])
    assert ctx.temporal_lengths() is not None
    render, ids, pos = _render(ctx, yh, 4)
    usable = np.array([0 if o in users else 1 for o in range(base.n)], np.int32)
    want, want_len = yh.reproject(p, render, SPP, ids, pos, hist, cam, cam, frames, frames, usable)
    _same(ctx.temporal_accumulate(p), want, "after a refit")
    _same(ctx.temporal_lengths(), want_len, "after a refit: lengths")
    of_shape, live = np.isin(ids, users), (ids >= 0) & np.isfinite(render[..., :3]).all(-1)
    assert (of_shape & live).sum() > 100 and (want_len[of_shape & live] == SPP).all(), "the refitted shape's pixels start again"
    assert (~of_shape & live).sum() > 100 and (want_len[~of_shape & live] == 2 * SPP).mean() > 0.9, "the others go on"
    # ... and the flags last one step
    render, ids2, pos2 = _render(ctx, yh, 5)
    want2, want_len2 = yh.reproject(p, render, SPP, ids2, pos2, (want, want_len, ids, pos), cam, cam, frames, frames)
    _same(ctx.temporal_accumulate(p), want2, "the step after")
    _same(ctx.temporal_lengths(), want_len2, "the step after: lengths")
    assert (want_len2[np.isin(ids2, users) & live] == 2 * SPP).mean() > 0.9
    # the same size keeps, materials drop
    ctx.init_state(yh.TraceParams.default(resolution=RES))
    _same(ctx.temporal_lengths(), want_len2, "yh_init_state of the same size")
    ctx.update_materials(0, base.materials)
    assert ctx.temporal_lengths() is None, "yh_update_materials drops the history"
    render, ids, pos = _render(ctx, yh, 6)
    _same(ctx.temporal_accumulate(p), render, "... and the next accumulate starts afresh")
    live = (ids >= 0) & np.isfinite(render[..., :3]).all(-1)
    _same(ctx.temporal_lengths(), np.where(live, SPP, 0).astype(np.int32), "every pixel has length n")
    ctx.temporal_reset()
    assert ctx.temporal_lengths() is None
    ctx.temporal_accumulate(p, want_image=False)
    ctx.init_state(yh.TraceParams.default(resolution=RES // 2))
    assert ctx.temporal_lengths() is None, "yh_init_state of another size drops the history"
    ctx.trace_samples(1)
    ctx.temporal_accumulate(p, want_image=False)
    assert ctx.temporal_lengths().shape == (ctx.height, ctx.width)
    ctx.upload_scene(sf.desc, sf.maps)
    assert ctx.temporal_lengths() is None
    sf.close()


# ---------------------------------------------------------------------------------------------
# 3. what the calls leave alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_render_with_temporal_calls_in_between_is_the_render_without(ctx, yh):
    """Pixels, RNG states, launch shapes, pending trials and the trial record of 2 + 2 + 4 spp are those of the same launches with every
    temporal entry called in between."""
    sf = yh.SceneFile(scene_path(*SCENES["textured"][:1], **SCENES["textured"][1]))
    runs = []
    for with_calls in (False, True):
        ctx.upload_scene(sf.desc, sf.maps)
        ctx.set_shard(0, 1)
        ctx.init_state(yh.TraceParams.default(resolution=RES))
        shapes = []
        for n in (2, 2, 4):
            ctx.trace_samples(n)
            shapes.append(ctx.launch_shape())
            if with_calls:
                p = ctx.temporal_default_params()
                ctx.temporal_accumulate(p), ctx.temporal_display(p, ctx.denoise_default_params()), ctx.temporal_lengths()
                out = torch.zeros((ctx.height, ctx.width, 4), device="cuda")
                ctx.temporal_accumulate_device(p, out)
                ctx.temporal_reset()
                ctx.temporal_accumulate(p, ctx.download(), 3)
                assert ctx.launch_shape() == shapes[-1]
        runs.append((ctx.download(), ctx.download_rng(), shapes, ctx.trials_pending(), ctx.kernel_trials()))
    _same(runs[1][0], runs[0][0], "pixels")
    assert np.array_equal(runs[1][1], runs[0][1]), "rng states"
    assert runs[1][2:4] == runs[0][2:4], "launch shapes and pending trials"
    assert set(runs[1][4]) == set(runs[0][4]) and all(runs[1][4][k][1] == runs[0][4][k][1] for k in runs[0][4]), "the trial record"
    sf.close()


# ---------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_come_before_any_write(yh):
    lib = yh.load()
    sf = yh.SceneFile(scene_path("sphere-hairblock", scale=0.02))
    c = yh.Context(0)
    p = yh.temporal_default_params()
    host = np.full((RES, RES, 4), 7, F)
    u8 = np.full((RES, RES, 4), 7, np.uint8)
    dev = torch.full((RES, RES, 4), 7.0, device="cuda")
    image = np.ones((RES, RES, 4), F)

    def entries(params=p, rgba_in=None, samples=0, guides=None):
        pp = C.byref(params) if params is not None else None
        gp = C.byref(guides) if guides is not None else None
        calls = {"yh_temporal_accumulate": lambda: lib.yh_temporal_accumulate(c.h, pp, yh.fptr(rgba_in) if rgba_in is not None else None, samples, gp, yh.fptr(host)),
                 "yh_temporal_accumulate_device": lambda: lib.yh_temporal_accumulate_device(c.h, pp, None, samples, None, dev.data_ptr())}
        if rgba_in is None and guides is None:
            calls["yh_temporal_display"] = lambda: lib.yh_temporal_display(c.h, pp, None, 0.0, 0, 1, u8.ctypes.data_as(C.POINTER(C.c_uint8)))
        return calls

    def all_are(code, message, only=None, **kw):
        before = c.temporal_lengths() if c.h and lib.yh_temporal_lengths(c.h, None) >= 0 else None
        for name, call in entries(**kw).items():
            if only is not None and name not in only:
                continue
            rc = call()
            assert rc == code, (name, rc)
            err = lib.yh_last_error(c.h).decode()
            assert name in err and message in err, err
        after = c.temporal_lengths() if lib.yh_temporal_lengths(c.h, None) >= 0 else None
        assert (before is None and after is None) or np.array_equal(before, after), "a refused call changed the history"
        assert np.all(host == 7) and np.all(u8 == 7) and bool((dev == 7).all()), "a refused call wrote to its output"
    all_are(yh.YH_E_STATE, "before yh_upload_scene")
    c.upload_scene(sf.desc)
    all_are(yh.YH_E_STATE, "before yh_init_state")
    c.init_state(yh.TraceParams.default(resolution=RES))
    all_are(yh.YH_E_STATE, "no sample has been traced")
    c.trace_samples(2)
    assert c.temporal_lengths() is None
    c.temporal_accumulate(p, want_image=False)  # a history to compare
    assert c.temporal_lengths().max() == 2
    all_are(yh.YH_E_INVALID, "params is NULL", params=None)
    for bad in (0, -5):
        all_are(yh.YH_E_INVALID, "max_history", params=p.copy(max_history=bad))
    for bad in (0, -1):
        all_are(yh.YH_E_INVALID, "samples", only=("yh_temporal_accumulate",), rgba_in=image, samples=bad)
    ids, pos = np.zeros((RES, RES), np.int32), np.ones((RES, RES, 3), F)
    for missing in ("object", "position"):
        g = yh.GBuffer()
        if missing != "object":
            g.object = yh.iptr(ids)
        if missing != "position":
            g.position = yh.fptr(pos)
        all_are(yh.YH_E_INVALID, f"guide plane `{missing}`", only=("yh_temporal_accumulate",), guides=g)
    before = c.temporal_lengths()
    assert lib.yh_temporal_accumulate_device(c.h, C.byref(p), None, 0, None, dev.data_ptr() + 4) == yh.YH_E_INVALID and b"aligned" in lib.yh_last_error(c.h)
    assert lib.yh_temporal_accumulate_device(c.h, C.byref(p), dev.data_ptr() + 8, 2, None, None) == yh.YH_E_INVALID and b"aligned" in lib.yh_last_error(c.h)
    assert lib.yh_temporal_display(c.h, C.byref(p), None, 0.0, 0, 1, None) == yh.YH_E_INVALID
    assert lib.yh_temporal_display(c.h, C.byref(p), C.byref(yh.denoise_default_params().copy(iterations=7)), 0.0, 0, 1, u8.ctypes.data_as(C.POINTER(C.c_uint8))) == yh.YH_E_INVALID
    assert np.array_equal(c.temporal_lengths(), before)
    # an asynchronous launch pending
    c.trace_samples_async(1)
    for name, call in entries().items():
        assert call() == yh.YH_E_STATE and "asynchronous launch pending" in lib.yh_last_error(c.h).decode(), name
    assert lib.yh_temporal_lengths(c.h, None) == yh.YH_E_STATE
    c.synchronize()
    assert np.array_equal(c.temporal_lengths(), before)
    # a shard: the own render is part of the image; a gathered image passed in is taken
    c.set_shard(1, 2)
    c.init_state(yh.TraceParams.default(resolution=RES))
    c.trace_samples(2)
    all_are(yh.YH_E_STATE, "gather first")
    assert entries(rgba_in=image, samples=2)["yh_temporal_accumulate"]() == yh.YH_OK
    assert c.temporal_lengths().max() == 4 and not np.all(host == 7)
    c.close(), sf.close()


# ---------------------------------------------------------------------------------------------
# 5. the projection's sign conventions
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_position_plane_projects_onto_its_own_pixel(ctx, yh):
    """On the triangle-hit pixels of lobes the centre-mode position, projected into its own camera, lands on its own pixel index within
    the projection bar (4 x the float32 form's worst error against float64, profiles/temporal/errors.txt). Hair positions lie on the
    strand axis, not on the ray: they are left out."""
    name, kw = SCENES["lobes"]
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    ctx.init_state(yh.TraceParams.default(resolution=RES))
    g = ctx.trace_gbuffer("centre", ("object", "position", "tangent"))
    triangles = (g["object"] >= 0) & (g["tangent"] == 0).all(-1)
    assert triangles.sum() > 0.3 * triangles.size
    lz, fx, fy = reproject_f32.project(_camera_floats(sf.desc.contents.camera), g["position"], ctx.width, ctx.height)
    jj, ii = np.mgrid[0:ctx.height, 0:ctx.width]
    ex, ey = np.abs(fx - ii)[triangles].max(), np.abs(fy - jj)[triangles].max()
    bar = 4 * reproject_f64.recorded_worst()
    print(f"lobes: |fx - i| <= {ex:.3e}, |fy - j| <= {ey:.3e} pixels over {triangles.sum()} triangle-hit pixels (bar {bar:.3e})")
    assert (lz[triangles] < 0).all()
    assert ex <= bar and ey <= bar
    sf.close()


# ---------------------------------------------------------------------------------------------
# 6. quality
# ---------------------------------------------------------------------------------------------
def _mse(a, reference, hit):
    return float(((a[..., :3].astype(np.float64) - reference[..., :3]) ** 2)[hit].mean())


@pytest.mark.gpu
@pytest.mark.parametrize("case", ("hairblock", "textured", "lobes"))
def test_accumulating_an_orbit_beats_the_last_frame(ctx, yh, case):
    """An orbit of eight 1-degree steps at 4 spp: over the hit pixels of the last view, against its 1 024-spp render, the accumulated image
    is strictly closer than the last 4-spp render, and accumulated + denoised strictly closer than that render denoised.

    Measured on an MI355X with the defaults (max_history 4, sigma_position 0.2 x the diagonal), MSE ratios accumulated / render and
    accumulated + denoised / render + denoised: hairblock 0.291 and 0.989, textured 0.284 and 0.423, lobes 0.293 and 0.353. The hair block
    is the narrow one: the filter alone takes its 4-spp render to x 0.025, and a longer history (1.008 at 16) or a tighter position test
    (0.996 at 0.05 x the diagonal) ends at or above 1 there (profiles/temporal/quality.txt)."""
    name, kw = SCENES[case]
    sf = yh.SceneFile(scene_path(name, **kw))
    new = Moved(yh, sf.desc)
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    p, dp = ctx.temporal_default_params(), ctx.denoise_default_params()
    for step in range(9):
        if step > 0:
            _orbit(new, 1.0)
            ctx.update_camera(new.d.camera)
        render, ids, pos = _render(ctx, yh, 100 + step)
        acc = ctx.temporal_accumulate(p)
    hit = ids >= 0
    acc_dn, render_dn = ctx.denoise(dp, acc), ctx.denoise(dp, render)
    ctx.trace_samples(REFERENCE_SPP - SPP)
    reference = ctx.download().astype(np.float64)
    noisy, noisy_dn = _mse(render, reference, hit), _mse(render_dn, reference, hit)
    print(f"{case}: MSE of the last {SPP}-spp render {noisy:.4e}; accumulated / render = {_mse(acc, reference, hit) / noisy:.3f}; "
          f"accumulated + denoised / render + denoised = {_mse(acc_dn, reference, hit) / noisy_dn:.3f}; longest history {ctx.temporal_lengths().max()}")
    assert _mse(acc, reference, hit) < noisy
    assert _mse(acc_dn, reference, hit) < noisy_dn
    sf.close()
