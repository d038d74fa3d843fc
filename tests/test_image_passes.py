"""yh_temporal_display against its stages run one by one through the public device entries, on an image that is no multiple of any tile:
the one place where a wrong plane mask or plane index of the shared feature pass (yocto-hair_amd/host/image_planes.h, image_pass.h)
would pass every per-stage test."""
import numpy as np
import pytest
import torch

from conftest import scene_path
from test_denoise import SCENES, _device_planes
from test_temporal import _check_display, _same

W, H, SPP = 19, 13, 2  # neither a multiple of the filter's 16 x 16 tile nor of the 8 x 8 work tile
DISPLAY = (0.5, True, True)


def _staged(ctx, tp, dp, union):
    """One step of the sequence yh_temporal_display is said to be: yh_trace_gbuffer_device of the planes in `union`, yh_temporal_accumulate_device
    and yh_denoise_image_device with those guides. Returns the image and the launches of the parts."""
    planes = _device_planes(ctx, union)
    launches = [ctx.last_trace_ms()[1]]
    image = torch.zeros((H, W, 4), device="cuda")
    ctx.temporal_accumulate_device(tp, image, object=planes["object"], position=planes["position"])
    launches.append(ctx.last_trace_ms()[1])
    ctx.denoise_image_device(dp, image, rgba_in=image, **planes)  # in place, as the display entry filters
    launches.append(ctx.last_trace_ms()[1])
    return image.cpu().numpy(), launches


@pytest.mark.gpu
def test_temporal_display_is_its_stages_one_by_one(ctx, yh):
    """sphere-hairblock at 19 x 13 pixels, 2 spp. For the default filter parameters (the union of the two stages' planes: object, position,
    normal, albedo) and with sigma_normal = 0 and demodulate = 0 (object and position alone), two steps each after yh_temporal_reset — the
    second reprojects through the traced position plane — through yh_temporal_display and through the stages one by one. The history's
    lengths are the same bits; the launch count of the display entry is the sum of the stages' plus the tone map's one kernel. The tone
    map of a device image has no public entry of its own, so that arm cannot be run separately: the bytes are held to the tone map of the
    staged image as restated on the host (tests/test_temporal.py: _check_display — alpha exactly, colour exactly except within one step
    where the float value sits at a step of the byte)."""
    name, kw = SCENES["hairblock"]
    sf = yh.SceneFile(scene_path(name, **kw))
    film = sf.desc.contents.camera.film
    film[1] = film[0] * H / W
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    ctx.init_state(yh.TraceParams.default(resolution=W))
    assert (ctx.width, ctx.height) == (W, H)
    ctx.trace_samples(SPP)
    tp, full = ctx.temporal_default_params(), ctx.denoise_default_params()
    assert full.iterations == 5 and full.sigma_normal > 0 and full.sigma_position > 0 and full.demodulate == 1
    for dp, union in ((full, ("object", "position", "normal", "albedo")), (full.copy(sigma_normal=0.0, demodulate=0), ("object", "position"))):
        ctx.temporal_reset()
        staged = [(*_staged(ctx, tp, dp, union), ctx.temporal_lengths()) for step in range(2)]
        ctx.temporal_reset()
        for step, (image, launches, lengths) in enumerate(staged):
            got = ctx.temporal_display(tp, dp, *DISPLAY)
            print(f"{union} step {step}: launches of the stages {launches}, of the display entry {ctx.last_trace_ms()[1]}")
            assert launches == [1, 1, 1 + dp.iterations]
            assert ctx.last_trace_ms()[1] == sum(launches) + 1
            _same(ctx.temporal_lengths(), lengths, f"{union} step {step}: lengths")
            _check_display(got, image, DISPLAY[0], int(DISPLAY[1]), int(DISPLAY[2]))
        assert staged[1][2].max() > SPP, "the second step reuses the first"
    sf.close()
