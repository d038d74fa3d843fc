"""The denoiser on the device (unit/denoise.hip, host/denoise.cpp): yh_atrous_filter_gpu in both forms against the host's form, the
context entries yh_denoise / yh_denoise_image_device / yh_denoise_display on rendered scenes against each other and against the host's form
on the downloaded render and planes, what the calls leave alone, what they refuse, a gathered shard pair, and the quality condition.

The yardstick of the arithmetic is yh_atrous_filter, which tests/test_denoise_cpu.py holds bit for bit to the numpy restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import scene_path
from denoise_cases import ITERATIONS, SIZES, STRATA, bits, make_case
from test_scene_edits import _check_display

F = np.float32
TILE = 16  # the side of form 1's LDS tile (yhk_dn_tile)
SCENES = {"hairblock": ("sphere-hairblock", dict(scale=0.05, zoom=True)), "textured": ("textured", dict(scale=0.05)), "lobes": ("lobes", dict(scale=0.05))}
RES, SPP, REFERENCE_SPP = 64, 4, 1024
GUIDES = ("object", "normal", "position", "albedo")


def _params(yh, P, iterations):
    return yh.DenoiseParams(iterations, P["sigma_color"], P["sigma_normal"], P["sigma_position"], P["demodulate"], P["match_object"])


def _same(got, want, what):
    diff = bits(got) != bits(want)
    assert not diff.any(), f"{what}: {np.count_nonzero(diff)} of {diff.size} entries differ, first at {np.argwhere(diff)[0]}"


# ---------------------------------------------------------------------------------------------
# 1. the unit pair
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("stratum", STRATA)
def test_both_device_forms_are_the_host_form_bit_for_bit(ctx, yh, stratum):
    assert ctx.lib.yhk_dn_tile() == TILE
    for size in SIZES:
        P, *arrays = make_case(stratum, *size)
        for it in ITERATIONS:
            p = _params(yh, P, it)
            want = yh.atrous_filter(p, *arrays)
            for form in (0, 1):
                _same(ctx.atrous_filter_gpu(form, p, *arrays), want, f"{stratum} {size} x{it} form {form}")
                assert len(ctx.atrous_level_ms()) == 1 + it


@pytest.mark.gpu
@pytest.mark.parametrize("stratum", ("full", "misses", "non-finite"))
def test_device_forms_at_the_tile_edges(ctx, yh, stratum):
    """Image sizes of tile - 1, tile and tile + 1 in each dimension, for one tile and for two: a block's halo ends inside, at and past the
    image, and the last block of a row and of a column is partly empty."""
    for w in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        for h in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1):
            P, *arrays = make_case(stratum, w, h)
            for it in (1, 2, 3, 5):
                p = _params(yh, P, it)
                want = yh.atrous_filter(p, *arrays)
                for form in (0, 1):
                    _same(ctx.atrous_filter_gpu(form, p, *arrays), want, f"{stratum} {w}x{h} x{it} form {form}")


# ---------------------------------------------------------------------------------------------
# 2. the context entries on rendered scenes
# ---------------------------------------------------------------------------------------------
def _begin(ctx, yh, sf):
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    ctx.init_state(yh.TraceParams.default(resolution=RES))


def _device_planes(ctx, names=GUIDES):
    comps = dict(object=(torch.int32, 1), normal=(torch.float32, 3), position=(torch.float32, 3), albedo=(torch.float32, 3))
    planes = {n: torch.zeros((ctx.height, ctx.width, comps[n][1]), dtype=comps[n][0], device="cuda").squeeze(-1).contiguous() for n in names}
    ctx.trace_gbuffer_device("centre", **planes)
    return planes


def _mse_ratio(denoised, noisy, reference, hit):
    err = lambda a: float(((a[..., :3].astype(np.float64) - reference[..., :3]) ** 2)[hit].mean())
    return err(denoised) / err(noisy), err(noisy)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(SCENES))
def test_context_entries_on_a_render(ctx, yh, case):
    name, kw = SCENES[case]
    sf = yh.SceneFile(scene_path(name, **kw))
    _begin(ctx, yh, sf)
    ctx.trace_samples(SPP)
    p = ctx.denoise_default_params()
    assert p.iterations == 5 and p.sigma_position > 0
    render = ctx.download()
    g = ctx.trace_gbuffer("centre", GUIDES)
    hit = g["object"] >= 0
    assert 0.3 < hit.mean() <= 1.0 and np.isfinite(render).all()
    want = yh.atrous_filter(p, render, g["object"], g["normal"], g["position"], g["albedo"])

    # the device form with its own guides, with the planes of yh_trace_gbuffer_device, and with the render passed in
    out = torch.zeros((ctx.height, ctx.width, 4), device="cuda")
    ctx.denoise_image_device(p, out)
    ms, launches = ctx.last_trace_ms()
    assert launches == 1 + 1 + p.iterations and ms > 0  # the feature pass, the pack step, the levels
    own = out.cpu().numpy()
    _same(own, want, "own guides against the host form on the downloaded render and planes")
    planes = _device_planes(ctx)
    out.zero_()
    ctx.denoise_image_device(p, out, **planes)
    assert ctx.last_trace_ms()[1] == 1 + p.iterations
    _same(out.cpu().numpy(), own, "given guides against own guides")
    image = torch.from_numpy(render).cuda()
    ctx.denoise_image_device(p, image, rgba_in=image, **planes)  # in place
    _same(image.cpu().numpy(), own, "the render passed in, in place")
    # the host-pointer form
    _same(ctx.denoise(p), own, "yh_denoise against the device form")
    _same(ctx.denoise(p, render), own, "yh_denoise of the download against yh_denoise of the own render")
    # other parameter sets: no demodulation (no albedo plane is traced), one level, none
    for q in (p.copy(demodulate=0), p.copy(iterations=1), p.copy(sigma_normal=0.0, sigma_position=0.0, match_object=0)):
        _same(ctx.denoise(q), yh.atrous_filter(q, render, g["object"], g["normal"], g["position"], g["albedo"]), "another parameter set")
    _same(ctx.denoise(p.copy(iterations=0)), render, "iterations = 0")
    _same(own[~hit], render[~hit], "misses")
    assert (bits(own[hit][:, :3]) != bits(render[hit][:, :3])).mean() > 0.9

    # the display bytes
    for exposure, filmic, srgb in ((0.0, False, True), (1.5, True, True)):
        assert np.array_equal(ctx.denoise_display(p.copy(iterations=0), exposure, filmic, srgb), ctx.download_display(exposure, filmic, srgb))
        _check_display(ctx.denoise_display(p, exposure, filmic, srgb), own, exposure, int(filmic), int(srgb))
    assert ctx.last_trace_ms()[1] == 1 + 1 + p.iterations + 1
    _same(ctx.download(), render, "the render itself is untouched")

    # quality: against the 1 024-spp render of the same context, over the hit pixels, the denoised image is strictly closer than the 4-spp one
    ctx.trace_samples(REFERENCE_SPP - SPP)
    ratio, noisy = _mse_ratio(own, render, ctx.download().astype(np.float64), hit)
    print(f"{case}: MSE of the {SPP}-spp image {noisy:.4e}, denoised / noisy = {ratio:.3f}")
    assert ratio < 1.0
    sf.close()


@pytest.mark.gpu
def test_render_with_denoise_calls_in_between_is_the_render_without(ctx, yh):
    """Pixels, RNG states, item costs' launch shape and sample count of 2 + 2 + 4 spp are those of the same launches with every denoise
    entry called in between."""
    sf = yh.SceneFile(scene_path(*SCENES["textured"][:1], **SCENES["textured"][1]))
    runs = []
    for with_calls in (False, True):
        _begin(ctx, yh, sf)
        shapes = []
        for n in (2, 2, 4):
            ctx.trace_samples(n)
            shapes.append(ctx.launch_shape())
            if with_calls:
                p = ctx.denoise_default_params()
                ctx.denoise(p), ctx.denoise_display(p)
                out = torch.zeros((ctx.height, ctx.width, 4), device="cuda")
                ctx.denoise_image_device(p, out)
                ctx.denoise_image_device(p, out, **_device_planes(ctx))
        runs.append((ctx.download(), ctx.download_rng(), shapes, ctx.trials_pending()))
    _same(runs[1][0], runs[0][0], "pixels")
    assert np.array_equal(runs[1][1], runs[0][1]), "rng states"
    assert runs[1][2:] == runs[0][2:], "launch shapes and pending trials"
    sf.close()


# ---------------------------------------------------------------------------------------------
# 3. refusals and shards
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_come_before_any_write(yh):
    lib = yh.load()
    sf = yh.SceneFile(scene_path("sphere-hairblock", scale=0.02))
    c = yh.Context(0)
    p = yh.denoise_default_params()
    host = np.full((RES, RES, 4), 7, F)
    u8 = np.full((RES, RES, 4), 7, np.uint8)
    dev = torch.full((RES, RES, 4), 7.0, device="cuda")

    def entries(rgba_in=None, params=p):
        pp = C.byref(params)
        return {"yh_denoise": lambda: lib.yh_denoise(c.h, pp, yh.fptr(rgba_in) if rgba_in is not None else None, yh.fptr(host)),
                "yh_denoise_display": lambda: lib.yh_denoise_display(c.h, pp, 0.0, 0, 1, u8.ctypes.data_as(C.POINTER(C.c_uint8))),
                "yh_denoise_image_device": lambda: lib.yh_denoise_image_device(c.h, pp, None, None, dev.data_ptr())}

    def all_are(code, message, **kw):
        for name, call in entries(**kw).items():
            rc = call()
            assert rc == code, (name, rc)
            assert name in lib.yh_last_error(c.h).decode() and message in lib.yh_last_error(c.h).decode(), lib.yh_last_error(c.h)
    all_are(yh.YH_E_STATE, "before yh_upload_scene")
    c.upload_scene(sf.desc)
    all_are(yh.YH_E_STATE, "before yh_init_state")
    c.init_state(yh.TraceParams.default(resolution=RES))
    c.trace_samples(2)
    for it in (-1, 7):
        all_are(yh.YH_E_INVALID, "iterations", params=p.copy(iterations=it))
    assert lib.yh_denoise(c.h, None, None, yh.fptr(host)) == yh.YH_E_INVALID
    assert lib.yh_denoise(c.h, C.byref(p), None, None) == yh.YH_E_INVALID
    assert lib.yh_denoise_display(c.h, C.byref(p), 0.0, 0, 1, None) == yh.YH_E_INVALID
    assert lib.yh_denoise_image_device(c.h, C.byref(p), None, None, None) == yh.YH_E_INVALID
    assert lib.yh_denoise_image_device(c.h, C.byref(p), None, None, dev.data_ptr() + 4) == yh.YH_E_INVALID and b"aligned" in lib.yh_last_error(c.h)
    # a guide plane the parameters need
    planes = _device_planes(c)
    q = c.denoise_default_params()
    for missing in GUIDES:
        with pytest.raises(yh.YhError, match=f"guide plane `{missing}`"):
            c.denoise_image_device(q, dev, **{n: (None if n == missing else t) for n, t in planes.items()})
    c.denoise_image_device(q.copy(sigma_normal=0.0), dev.clone(), **{n: t for n, t in planes.items() if n != "normal"})  # ... and only those
    # an asynchronous launch pending
    c.trace_samples_async(1)
    all_are(yh.YH_E_STATE, "asynchronous launch pending")
    c.synchronize()
    # the unit entry: an unknown form, iterations, a missing plane, a NULL output
    P, *arrays = make_case("full", 5, 5)
    out = np.full((5, 5, 4), 7, F)
    good = _params(yh, P, 2)

    def unit(form=0, params=good, a=arrays, out_=out):
        ptr = lambda v, f: f(v) if v is not None else None
        return lib.yh_atrous_filter_gpu(c.h, form, 5, 5, C.byref(params), yh.fptr(a[0]), ptr(a[1], yh.iptr), ptr(a[2], yh.fptr), ptr(a[3], yh.fptr),
                                        ptr(a[4], yh.fptr), ptr(out_, yh.fptr))
    for form in (-1, 2):
        assert unit(form=form) == yh.YH_E_INVALID and b"unknown form" in lib.yh_last_error(c.h)
    assert unit(params=good.copy(iterations=7)) == yh.YH_E_INVALID
    assert unit(out_=None) == yh.YH_E_INVALID
    for k in (1, 2, 3, 4):
        assert unit(a=[None if i == k else v for i, v in enumerate(arrays)]) == yh.YH_E_INVALID
    # a shard
    c.set_shard(1, 2)
    c.init_state(yh.TraceParams.default(resolution=RES))
    c.trace_samples(2)
    all_are(yh.YH_E_STATE, "gather first")
    assert np.all(host == 7) and np.all(u8 == 7) and bool((dev == 7).all()) and np.all(out == 7), "a refused call wrote to its output"
    assert entries(rgba_in=np.zeros((RES, RES, 4), F))["yh_denoise"]() == yh.YH_OK  # ... with an image passed in, a shard denoises it
    c.close(), sf.close()


@pytest.mark.gpu
def test_gathered_shard_pair_denoises_to_the_unsharded_result(ctx, yh):
    name, kw = SCENES["hairblock"]
    sf = yh.SceneFile(scene_path(name, **kw))
    _begin(ctx, yh, sf)
    ctx.trace_samples(SPP)
    p = ctx.denoise_default_params()
    whole = ctx.denoise(p)
    pair = [yh.Context(0), yh.Context(0)]
    for rank, c in enumerate(pair):
        c.upload_scene(sf.desc, sf.maps)
        c.set_shard(rank, 2)
        c.init_state(yh.TraceParams.default(resolution=RES))
        c.trace_samples(SPP)
    gathered = yh.gather_framebuffer(pair)
    _same(gathered, ctx.download(), "the gathered render")
    q = pair[0].denoise_default_params()
    assert bytes(q) == bytes(p)
    _same(pair[0].denoise(q, gathered), whole, "the gathered image denoised on context 0")
    for c in pair:
        c.close()
    sf.close()
