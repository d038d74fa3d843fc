"""The variance stage on the device (unit/variance.hip through host/variance.cpp; include/yhair.h: VARIANCE): the _gpu forms against the
host's forms bit for bit on sizes around the 8 x 8 and 16 x 16 tiles, the context entries against the host's forms on the downloads, the
moment history's lifetime, what the calls leave alone, the refusals, a still view, and the quality condition."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import scene_path
from test_object_edits import Moved, _compose, _rotation, _translation
from test_temporal import RES, SCENES, SPP, REFERENCE_SPP, _camera_floats, _check_display, _mse, _orbit
from variance_cases import F_STRATA, M_STRATA, S_STRATA, bits, m_arguments, make_f_case, make_m_case, make_s_case, s_arguments

F = np.float32
EDGE = (7, 8, 9, 15, 16, 17, 33)  # partly empty 8 x 8 and 16 x 16 tiles, a halo that crosses two tiles, an image smaller than a halo
SIZES = tuple((w, h) for w in EDGE for h in EDGE) + ((47, 35),)
PLANES = ("object", "normal", "position", "albedo")


def _same(got, want, what):
    diff = bits(got) != bits(want)
    assert not diff.any(), f"{what}: {np.count_nonzero(diff)} of {diff.size} entries differ, first at {np.argwhere(diff)[0]}"


def _tparams(yh, P):
    return yh.TemporalParams(P["max_history"], P["sigma_position"], P["match_object"])


def _vparams(yh, V):
    return yh.VarianceParams(V["iterations"], V["sigma_luminance"], V["sigma_normal"], V["sigma_position"], V["demodulate"], V["match_object"], V["epsilon"],
                             V["min_steps"])


# ---------------------------------------------------------------------------------------------
# 1. the unit pairs
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("stratum", M_STRATA)
def test_stage_m_device_form_is_the_host_form(ctx, yh, stratum):
    for size in SIZES + ((64, 64),):
        case = make_m_case(stratum, *size)
        p, args = _tparams(yh, case["P"]), m_arguments(case)
        for k, (got, want) in enumerate(zip(ctx.reproject_moments_gpu(p, *args), yh.reproject_moments(p, *args))):
            _same(got, want, f"{stratum} {size}: output {k}")
        assert ctx.last_trace_ms()[1] == 1
    args[5] = args[6] = None  # the seed of a first frame
    for k, (got, want) in enumerate(zip(ctx.reproject_moments_gpu(p, *args), yh.reproject_moments(p, *args))):
        _same(got, want, f"{stratum}: no history, output {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("stratum", S_STRATA)
def test_stage_s_device_form_is_the_host_form(ctx, yh, stratum):
    for size in SIZES:
        case = make_s_case(stratum, *size)
        p, args = _tparams(yh, case["P"]), s_arguments(case)
        _same(ctx.variance_spatial_gpu(p, *args), yh.variance_spatial(p, *args), f"{stratum} {size}")


@pytest.mark.gpu
@pytest.mark.parametrize("form", (0, 1))
@pytest.mark.parametrize("stratum", F_STRATA)
def test_stage_f_device_forms_are_the_host_form(ctx, yh, stratum, form):
    """Five iterations: levels 0 - 4, so form 1 runs its three staged levels and the two unstaged ones."""
    for size in SIZES:
        V, *arrays = make_f_case(stratum, *size)
        for iterations in ((5,) if size != (47, 35) else (0, 1, 2, 3, 4, 5)):
            p = _vparams(yh, dict(V, iterations=iterations))
            want, want_var = yh.atrous_variance_filter(p, *arrays)
            got, got_var = ctx.atrous_variance_filter_gpu(form, p, *arrays)
            _same(got, want, f"{stratum} {size} x {iterations}, form {form}")
            _same(got_var, want_var, f"{stratum} {size} x {iterations}, form {form}: variance")


# ---------------------------------------------------------------------------------------------
# 2. the context entries
# ---------------------------------------------------------------------------------------------
def _render(ctx, yh, seed):
    ctx.init_state(yh.TraceParams.default(resolution=RES, seed=seed))
    ctx.trace_samples(SPP)
    return ctx.download(), ctx.trace_gbuffer("centre", PLANES)


def _host_chain(yh, tp, vp, render, g, hist, mom, cam, prev_cam, frames=None, prev_frames=None, usable=None):
    """Stages M, S and F with the host's forms; returns (accumulated, lengths, moments, steps, variance, filtered, filtered variance)"""
    out, length, m, s = yh.reproject_moments(tp, render, SPP, g["object"], g["position"], g["albedo"] if vp.demodulate else None, hist, mom, cam, prev_cam, frames,
                                             prev_frames, usable)
    var = yh.variance_spatial(tp, vp.min_steps, m, s, g["object"], g["position"])
    flt, flt_var = yh.atrous_variance_filter(vp, out, var, g["object"], g["normal"], g["position"], g["albedo"])
    return out, length, m, s, var, flt, flt_var


def _through(ctx, yh, entry, tp, vp, render, g):
    """M and S, then F, through `entry`; returns (accumulated, variance, filtered, filtered variance), or for `display` the bytes"""
    shape = (ctx.height, ctx.width)
    if entry in ("device", "device-given"):
        acc, var, flt, fvar = (torch.zeros(shape + (4,), device="cuda"), torch.zeros(shape, device="cuda"), torch.zeros(shape + (4,), device="cuda"),
                               torch.zeros(shape, device="cuda"))
        if entry == "device":
            ctx.temporal_accumulate_variance_device(tp, vp, acc, var)
            assert ctx.last_trace_ms()[1] == 3  # the feature pass, k_reproject_m, k_var_spatial
            ctx.denoise_variance_image_device(vp, flt, acc, None, fvar)
            assert ctx.last_trace_ms()[1] == 2 + vp.iterations
        else:
            d = {k: torch.from_numpy(g[k]).cuda() for k in PLANES}
            acc.copy_(torch.from_numpy(render))
            ctx.temporal_accumulate_variance_device(tp, vp, acc, var, rgba_in=acc, samples=SPP, object=d["object"], position=d["position"], albedo=d["albedo"])
            assert ctx.last_trace_ms()[1] == 2
            flt.copy_(acc)
            ctx.denoise_variance_image_device(vp, flt, flt, var, fvar, **d)  # in place
            assert ctx.last_trace_ms()[1] == 1 + vp.iterations
        return acc.cpu().numpy(), var.cpu().numpy(), flt.cpu().numpy(), fvar.cpu().numpy()
    if entry == "host":
        acc, var = ctx.temporal_accumulate_variance(tp, vp)
        return (acc, var) + ctx.denoise_variance_image(vp, acc)
    if entry == "host-given":
        acc, var = ctx.temporal_accumulate_variance(tp, vp, render, SPP, g["object"], g["position"], g["albedo"])
        return (acc, var) + ctx.denoise_variance_image(vp, acc, var, **{k: g[k] for k in PLANES})
    assert entry == "display"
    return ctx.svgf_display(tp, vp, 0.5, True, True)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ("device", "device-given", "host", "host-given", "display"))
@pytest.mark.parametrize("case", ("hairblock", "textured", "crowd"))
def test_context_steps_are_the_host_forms_on_the_downloads(ctx, yh, case, entry):
    """tests/test_temporal.py's four steps — a first frame and three edits, each followed by yh_init_state and 4 spp — through stages M, S and
    F of `entry`: images, variances, lengths and steps are the host forms' on the downloaded render and planes, so every entry equals every other."""
    name, kw = SCENES[case]
    sf = yh.SceneFile(scene_path(name, **kw))
    new = Moved(yh, sf.desc)
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    tp, vp = ctx.temporal_default_params(), ctx.variance_default_params()
    assert ctx.temporal_steps() is None, "an upload drops the moment history"
    ball, hair = new.index(lines=False, emissive=False)[-1], new.index(lines=True)[0]
    hist = mom = prev_cam = prev_frames = None
    for step in range(4):
        if step > 0 and case == "crowd":
            o = ball if step != 2 else hair
            new.set_frames([_compose(_translation(0.02 * step, 0.0, 0.015), _compose(new.frames()[o], _rotation((0, 1, 0), 4.0 * step)))], first=o)
            ctx.update_objects(o, new.rows(yh, o, 1))
        elif step > 0:
            _orbit(new, 1.0)
            ctx.update_camera(new.d.camera)
        render, g = _render(ctx, yh, 7 + step)
        cam, frames = _camera_floats(new.d.camera), np.array(new.frames(), F)
        acc, length, m, s, var, flt, fvar = _host_chain(yh, tp, vp, render, g, hist, mom, cam, prev_cam, frames, prev_frames)
        got = _through(ctx, yh, entry, tp, vp, render, g)
        what = f"{case} step {step} through {entry}"
        if entry == "display":
            _check_display(got, flt, 0.5, 1, 1)
        else:
            for a, b, n in zip(got, (acc, var, flt, fvar), ("accumulated", "variance", "filtered", "filtered variance")):
                _same(a, b, f"{what}: {n}")
        _same(ctx.temporal_lengths(), length, f"{what}: lengths")
        _same(ctx.temporal_steps(), s, f"{what}: steps")
        _same(ctx.download(), render, "the render itself is untouched")
        if step > 0:
            hit = g["object"] >= 0
            assert (s > 1).sum() > 0.5 * hit.sum(), "most hit pixels carry their moments on"
        hist, mom, prev_cam, prev_frames = (acc, length, g["object"], g["position"]), (m, s), cam, frames
    assert s.max() == 4
    sf.close()


@pytest.mark.gpu
def test_what_keeps_and_what_drops_the_moment_history(ctx, yh):
    """It lives and dies with the colour history; a plain accumulate in between advances the colour and marks the moments as none."""
    name, kw = SCENES["textured"]
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    tp, vp = ctx.temporal_default_params(), ctx.variance_default_params()
    cam = _camera_floats(sf.desc.contents.camera)
    render, g = _render(ctx, yh, 3)
    acc, var = ctx.temporal_accumulate_variance(tp, vp)
    live = (g["object"] >= 0) & np.isfinite(render[..., :3]).all(-1)
    _same(ctx.temporal_steps(), live.astype(np.int32), "the first frame: steps 1 on every live pixel")
    hist = (acc, ctx.temporal_lengths(), g["object"], g["position"])
    # a plain accumulate in between
    render, g = _render(ctx, yh, 4)
    plain = ctx.temporal_accumulate(tp)
    want, want_len = yh.reproject(tp, render, SPP, g["object"], g["position"], hist, cam, cam)
    _same(plain, want, "the plain step advances the colour as it does without the moments")
    assert ctx.temporal_steps() is None, "... and marks the moment history as none"
    lib = yh.load()
    out = np.zeros_like(render)
    assert lib.yh_denoise_variance_image(ctx.h, C.byref(vp), yh.fptr(render), None, None, yh.fptr(out), None) == yh.YH_E_STATE, "no variance is kept"
    hist = (plain, ctx.temporal_lengths(), g["object"], g["position"])
    render, g = _render(ctx, yh, 5)
    acc, length, m, s, var, _, _ = _host_chain(yh, tp, vp, render, g, hist, None, cam, cam)
    got, got_var = ctx.temporal_accumulate_variance(tp, vp)
    _same(got, acc, "the colour history went on"), _same(got_var, var, "the variance is the spatial estimate")
    _same(ctx.temporal_lengths(), length, "lengths"), _same(ctx.temporal_steps(), s, "steps")
    assert s.max() == 1 and length.max() > SPP
    # the same size keeps; a reset, another size, materials and an upload drop
    ctx.init_state(yh.TraceParams.default(resolution=RES))
    _same(ctx.temporal_steps(), s, "yh_init_state of the same size")
    ctx.temporal_reset()
    assert ctx.temporal_steps() is None and ctx.temporal_lengths() is None
    ctx.trace_samples(1)
    ctx.temporal_accumulate_variance(tp, vp)
    assert ctx.temporal_steps() is not None
    ctx.init_state(yh.TraceParams.default(resolution=RES // 2))
    assert ctx.temporal_steps() is None, "yh_init_state of another size"
    ctx.trace_samples(1)
    ctx.temporal_accumulate_variance(tp, vp)
    assert ctx.temporal_steps().shape == (ctx.height, ctx.width)
    ctx.upload_scene(sf.desc, sf.maps)
    assert ctx.temporal_steps() is None
    sf.close()


@pytest.mark.gpu
def test_render_with_variance_calls_in_between_is_the_render_without(ctx, yh):
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
                tp, vp = ctx.temporal_default_params(), ctx.variance_default_params()
                acc, var = ctx.temporal_accumulate_variance(tp, vp)
                ctx.denoise_variance_image(vp, acc), ctx.svgf_display(tp, vp), ctx.temporal_steps()
                out, v = torch.zeros((ctx.height, ctx.width, 4), device="cuda"), torch.zeros((ctx.height, ctx.width), device="cuda")
                ctx.temporal_accumulate_variance_device(tp, vp, out, v)
                ctx.denoise_variance_image_device(vp, out, out)
                assert ctx.launch_shape() == shapes[-1]
        runs.append((ctx.download(), ctx.download_rng(), shapes, ctx.trials_pending(), ctx.kernel_trials()))
    _same(runs[1][0], runs[0][0], "pixels")
    assert np.array_equal(runs[1][1], runs[0][1]), "rng states"
    assert runs[1][2:4] == runs[0][2:4], "launch shapes and pending trials"
    assert set(runs[1][4]) == set(runs[0][4]) and all(runs[1][4][k][1] == runs[0][4][k][1] for k in runs[0][4]), "the trial record"
    sf.close()


@pytest.mark.gpu
def test_refusals_come_before_any_write(yh):
    lib = yh.load()
    sf = yh.SceneFile(scene_path("sphere-hairblock", scale=0.02))
    c = yh.Context(0)
    tp, vp = yh.temporal_default_params(), yh.variance_default_params()
    host, hvar = np.full((RES, RES, 4), 7, F), np.full((RES, RES), 7, F)
    u8 = np.full((RES, RES, 4), 7, np.uint8)
    dev, dvar = torch.full((RES, RES, 4), 7.0, device="cuda"), torch.full((RES, RES), 7.0, device="cuda")
    image, variance = np.ones((RES, RES, 4), F), np.ones((RES, RES), F)
    f = lambda a: yh.fptr(a) if a is not None else None  # noqa: E731
    ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731

    def entries(t=tp, v=vp, rgba_in=None, samples=0, guides=None, variance_in=variance):
        calls = {"yh_temporal_accumulate_variance": lambda: lib.yh_temporal_accumulate_variance(c.h, ref(t), ref(v), f(rgba_in), samples, ref(guides), f(host), f(hvar)),
                 "yh_denoise_variance_image": lambda: lib.yh_denoise_variance_image(c.h, ref(v), f(image), f(variance_in), ref(guides), f(host), f(hvar))}
        if guides is None:
            calls["yh_temporal_accumulate_variance_device"] = lambda: lib.yh_temporal_accumulate_variance_device(c.h, ref(t), ref(v), None, samples, None,
                                                                                                               dev.data_ptr(), dvar.data_ptr())
            calls["yh_svgf_display"] = lambda: lib.yh_svgf_display(c.h, ref(t), ref(v), 0.0, 0, 1, u8.ctypes.data_as(C.POINTER(C.c_uint8)))
        return calls

    def all_are(code, message, only=None, skip=(), **kw):
        steps = lambda: c.temporal_steps() if lib.yh_temporal_steps(c.h, None) >= 0 else None  # noqa: E731
        before, seen = steps(), 0
        for name, call in entries(**kw).items():
            if (only is not None and name not in only) or name in skip:
                continue
            rc = call()
            assert rc == code, (name, rc)
            err = lib.yh_last_error(c.h).decode()
            assert name in err and message in err, err
            seen += 1
        after = steps()
        assert seen and ((before is None and after is None) or np.array_equal(before, after)), "a refused call changed the history"
        assert np.all(host == 7) and np.all(hvar == 7) and np.all(u8 == 7) and bool((dev == 7).all()) and bool((dvar == 7).all()), "a refused call wrote to its output"
    temporal = ("yh_temporal_accumulate_variance", "yh_temporal_accumulate_variance_device", "yh_svgf_display")
    all_are(yh.YH_E_STATE, "before yh_upload_scene", only=temporal)
    c.upload_scene(sf.desc)
    all_are(yh.YH_E_STATE, "before yh_init_state")
    c.init_state(yh.TraceParams.default(resolution=RES))
    all_are(yh.YH_E_STATE, "no sample has been traced", only=temporal)
    all_are(yh.YH_E_STATE, "keeps no variance", only=("yh_denoise_variance_image",), variance_in=None)
    c.trace_samples(2)
    c.temporal_accumulate_variance(tp, vp)  # a history to compare
    assert c.temporal_steps().max() == 1
    all_are(yh.YH_E_INVALID, "params", v=None)
    all_are(yh.YH_E_INVALID, "params is NULL", only=temporal, t=None)
    for bad in (0, -3):
        all_are(yh.YH_E_INVALID, "min_steps", v=vp.copy(min_steps=bad))
    for bad in (0.0, -1.0, float("nan")):
        all_are(yh.YH_E_INVALID, "epsilon", v=vp.copy(epsilon=bad))
    for bad in (-1, 7):
        all_are(yh.YH_E_INVALID, "iterations", v=vp.copy(iterations=bad))
    all_are(yh.YH_E_INVALID, "max_history", only=temporal, t=tp.copy(max_history=0))
    all_are(yh.YH_E_INVALID, "samples", only=("yh_temporal_accumulate_variance",), rgba_in=image, samples=0)
    ids, pl = np.zeros((RES, RES), np.int32), np.ones((RES, RES, 3), F)
    for missing in ("object", "normal", "position", "albedo"):
        g = yh.GBuffer()
        for n in ("object", "normal", "position", "albedo"):
            if n != missing:
                setattr(g, n, yh.iptr(ids) if n == "object" else yh.fptr(pl))
        on = vp.copy(sigma_position=1.0)
        only = ("yh_denoise_variance_image",) if missing == "normal" else None
        all_are(yh.YH_E_INVALID, f"guide plane `{missing}`", only=only, v=on, guides=g, rgba_in=image, samples=2)
    g = yh.GBuffer()
    g.object, g.position = yh.iptr(ids), yh.fptr(pl)
    assert lib.yh_temporal_accumulate_variance(c.h, C.byref(tp), C.byref(vp.copy(demodulate=0)), f(image), 2, C.byref(g), None, None) == yh.YH_OK, "no albedo without demodulate"
    before = c.temporal_steps()
    assert lib.yh_temporal_accumulate_variance_device(c.h, C.byref(tp), C.byref(vp), None, 0, None, dev.data_ptr() + 4, None) == yh.YH_E_INVALID and b"aligned" in lib.yh_last_error(c.h)
    assert lib.yh_denoise_variance_image_device(c.h, C.byref(vp), dev.data_ptr() + 8, None, None, dev.data_ptr(), None) == yh.YH_E_INVALID and b"aligned" in lib.yh_last_error(c.h)
    assert lib.yh_denoise_variance_image_device(c.h, C.byref(vp), None, None, None, dev.data_ptr(), None) == yh.YH_E_INVALID
    assert lib.yh_svgf_display(c.h, C.byref(tp), C.byref(vp), 0.0, 0, 1, None) == yh.YH_E_INVALID
    assert np.array_equal(c.temporal_steps(), before) and bool((dev == 7).all())
    c.trace_samples_async(1)
    for name, call in entries().items():
        assert call() == yh.YH_E_STATE and "asynchronous launch pending" in lib.yh_last_error(c.h).decode(), name
    assert lib.yh_temporal_steps(c.h, None) == yh.YH_E_STATE
    c.synchronize()
    c.set_shard(1, 2)
    c.init_state(yh.TraceParams.default(resolution=RES))
    c.trace_samples(2)
    all_are(yh.YH_E_STATE, "gather first", only=temporal)
    c.close(), sf.close()


@pytest.mark.gpu
def test_a_still_view_counts_its_steps_and_its_variance_falls(ctx, yh):
    name, kw = SCENES["hairblock"]
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    tp, vp = ctx.temporal_default_params().copy(max_history=1 << 20), ctx.variance_default_params().copy(min_steps=1)
    means = []
    for step in range(6):
        render, g = _render(ctx, yh, 40 + step)
        acc, var = ctx.temporal_accumulate_variance(tp, vp)
        flt, fvar = ctx.denoise_variance_image(vp, acc)
        steps, lengths = ctx.temporal_steps(), ctx.temporal_lengths()
        settled = lengths == SPP * (step + 1)  # (a strand's axis point may project off the image at its border: no history there)
        assert settled.sum() > 0.95 * (g["object"] >= 0).sum()
        assert (steps[settled] == step + 1).all(), f"steps count 1, 2, 3, ...: step {step}"
        means.append((float(var[settled].mean()), float(fvar[settled].mean())))
    print("still view, mean variance over the settled pixels per step (temporal estimate, after the filter): " + ", ".join(f"{a:.3e} / {b:.3e}" for a, b in means))
    assert means[0][0] == 0, "one sample of the moments has no temporal variance"
    assert all(a > 0 and b < a for a, b in means[1:]), "from the second step on there is a variance, and the filter lowers it"
    sf.close()


# ---------------------------------------------------------------------------------------------
# 3. quality
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ("hairblock", "textured", "lobes"))
def test_the_variance_guided_chain_beats_the_filtered_last_frame(ctx, yh, case):
    """tests/test_temporal.py's orbit of eight 1-degree steps at 4 spp: over the hit pixels of the last view, against its 1 024-spp render,
    accumulate with moments + the variance-guided filter (defaults) is strictly closer than the last 4-spp render through the fixed-sigma
    filter. The second ratio, against the same accumulated image through the fixed-sigma filter, is printed: it is a measurement
    (profiles/variance/quality.txt).

    Measured on an MI355X with the defaults, first and second ratio: hairblock 0.958 and 0.968, textured 0.278 and 0.656, lobes 0.349 and 0.988."""
    name, kw = SCENES[case]
    sf = yh.SceneFile(scene_path(name, **kw))
    new = Moved(yh, sf.desc)
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    tp, vp, dp = ctx.temporal_default_params(), ctx.variance_default_params(), ctx.denoise_default_params()
    for step in range(9):
        if step > 0:
            _orbit(new, 1.0)
            ctx.update_camera(new.d.camera)
        render, g = _render(ctx, yh, 100 + step)
        acc, var = ctx.temporal_accumulate_variance(tp, vp)
    hit = g["object"] >= 0
    new_chain, _ = ctx.denoise_variance_image(vp, acc)
    acc_dn, render_dn = ctx.denoise(dp, acc), ctx.denoise(dp, render)
    ctx.trace_samples(REFERENCE_SPP - SPP)
    reference = ctx.download().astype(np.float64)
    e = _mse(new_chain, reference, hit)
    print(f"{case}: variance-guided chain / render + fixed-sigma filter = {e / _mse(render_dn, reference, hit):.3f}; "
          f"/ accumulated + fixed-sigma filter = {e / _mse(acc_dn, reference, hit):.3f}; mean variance {float(var[hit].mean()):.3e}")
    assert e < _mse(render_dn, reference, hit)
    sf.close()
