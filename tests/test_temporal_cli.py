"""The temporal stage above the C ABI: the C++ mirror's accumulate_image (tests/cpp/test_mirror_temporal.cpp) and `--temporal FILE` of
ysceneitraces --turntable, whose file holds the last step's accumulated image (.pfm: rgb floats, top row first) — the image the same
steps give through the library — next to step images that are the ones written without the option."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_denoise_cli import _read_pfm
from test_object_edits import Moved

PKG = os.path.join(ROOT, "yocto-hair_amd")
SCENE = ("textured", dict(scale=0.05))
F = np.float32
STEPS, RES, SPP = 12, 64, 2  # a turn in 12 steps


@pytest.mark.gpu
def test_mirror_returns_the_image_of_the_host_form(built, tmp_path):
    exe = str(tmp_path / "mirror_temporal")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host"), "-Wno-class-memaccess", os.path.join(ROOT, "tests", "cpp", "test_mirror_temporal.cpp"),
                           "-o", exe, "-L" + PKG, "-lyhair", "-Wl,-rpath," + PKG, "-lpthread"])
    r = subprocess.run([exe, scene_path(*SCENE[:1], **SCENE[1])], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)


def _turntable(tmp_path, tag, *options):
    out = str(tmp_path / f"{tag}.pfm")
    r = subprocess.run([os.path.join(PKG, "ysceneitraces"), scene_path(*SCENE[:1], **SCENE[1]), "-r", str(RES), "-s", str(SPP), "-o", out,
                        "--turntable", str(STEPS), "--turntable-objects", *options], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    return r.stdout, [str(tmp_path / f"{tag}-{k:03d}.pfm") for k in range(STEPS)]


def _turned(frame, k):
    """ysceneitraces --turntable-objects, step k of STEPS: the frame's four columns turned about the world's y axis, in float32."""
    a = F(2) * F(3.14159265358979323846) * F(k) / F(STEPS)
    c, s = F(np.cos(np.float64(a))), F(np.sin(np.float64(a)))  # (std::cos / std::sin of a float: correctly rounded)
    f = np.array(frame, F).reshape(4, 3)
    return np.stack([c * f[:, 0] + s * f[:, 2], f[:, 1], c * f[:, 2] - s * f[:, 0]], 1).reshape(12)


@pytest.mark.gpu
def test_turntable_writes_the_accumulated_image(ctx, yh, tmp_path):
    """--temporal FILE, and --denoise FILE with it, under --turntable-objects: the files hold what yh_temporal_accumulate and yh_denoise make
    of the same steps through the library, bit for bit, and the step images are those of a run without the options."""
    acc, dn = str(tmp_path / "acc.pfm"), str(tmp_path / "acc_dn.pfm")
    stdout, steps = _turntable(tmp_path, "with", "--temporal", acc, "--denoise", dn)
    assert "save accumulated: " + acc in stdout and "save accumulated and denoised: " + dn in stdout, stdout
    assert stdout.count("save accumulated") == 2, "the last step alone is written"
    assert stdout.count("the objects alone were passed on") == STEPS - 1, stdout
    _, plain = _turntable(tmp_path, "plain")
    for a, b in zip(steps, plain):
        assert open(a, "rb").read() == open(b, "rb").read(), "the step images themselves are untouched"
    # the same steps through the library
    sf = yh.SceneFile(scene_path(*SCENE[:1], **SCENE[1]))
    new = Moved(yh, sf.desc)
    loaded = new.frames()
    turning = new.index(emissive=False)
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    for k in range(STEPS):
        if k > 0:
            for o in turning:
                new.objects[o].frame[:] = [float(x) for x in _turned(loaded[o], k)]
            ctx.update_objects(0, new.rows(yh))
        ctx.init_state(yh.TraceParams.default(resolution=RES))
        ctx.trace_samples(SPP)
        assert np.array_equal(_read_pfm(steps[k], RES), ctx.download()[..., :3]), f"step {k}"
        want = ctx.temporal_accumulate(ctx.temporal_default_params())  # (the defaults follow the scene's bounds, which turn with the floor)
    bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)  # noqa: E731
    assert np.array_equal(bits(_read_pfm(acc, RES)), bits(want[..., :3]))
    assert np.array_equal(bits(_read_pfm(dn, RES)), bits(ctx.denoise(ctx.denoise_default_params(), want)[..., :3]))
    lengths = ctx.temporal_lengths()
    print(f"{(lengths > SPP).sum()} of {(lengths > 0).sum()} pixels reuse the history at the last step, longest {lengths.max()}")
    assert (lengths > SPP).sum() > 0.1 * (lengths > 0).sum() and not np.array_equal(_read_pfm(acc, RES), _read_pfm(steps[-1], RES))
    sf.close()
