"""The variance stage above the C ABI: the C++ mirror's accumulate_image_variance (tests/cpp/test_mirror_variance.cpp), built and run as
tests/test_temporal_cli.py builds and runs the temporal stage's, and `--variance-guided` / `--variance FILE` of ysceneitraces --turntable
--temporal: the files hold what the same steps give through the library, next to step images that are the ones written without the flags."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_denoise_cli import _read_pfm
from test_object_edits import Moved
from test_temporal_cli import RES, SCENE, SPP, STEPS, _turned, _turntable

PKG = os.path.join(ROOT, "yocto-hair_amd")
F = np.float32


@pytest.mark.gpu
def test_mirror_returns_the_image_of_the_host_forms(built, tmp_path):
    exe = str(tmp_path / "mirror_variance")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host"), "-Wno-class-memaccess", os.path.join(ROOT, "tests", "cpp", "test_mirror_variance.cpp"),
                           "-o", exe, "-L" + PKG, "-lyhair", "-Wl,-rpath," + PKG, "-lpthread"])
    r = subprocess.run([exe, scene_path(*SCENE[:1], **SCENE[1])], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)


@pytest.mark.gpu
def test_turntable_filters_by_the_variance_and_writes_it(ctx, yh, tmp_path):
    acc, dn, var = str(tmp_path / "acc.pfm"), str(tmp_path / "acc_dn.pfm"), str(tmp_path / "var.pfm")
    stdout, steps = _turntable(tmp_path, "with", "--temporal", acc, "--denoise", dn, "--variance-guided", "--variance", var)
    assert "save accumulated: " + acc in stdout and "save accumulated and denoised: " + dn in stdout and "save variance: " + var in stdout, stdout
    assert stdout.count("save variance") == 1 and stdout.count("save accumulated") == 2, "the last step alone is written"
    _, plain = _turntable(tmp_path, "plain")
    for a, b in zip(steps, plain):
        assert open(a, "rb").read() == open(b, "rb").read(), "the step images themselves are untouched"
    # the same steps through the library
    sf = yh.SceneFile(scene_path(*SCENE[:1], **SCENE[1]))
    new = Moved(yh, sf.desc)
    loaded, turning = new.frames(), new.index(emissive=False)
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    for k in range(STEPS):
        if k > 0:
            for o in turning:
                new.objects[o].frame[:] = [float(x) for x in _turned(loaded[o], k)]
            ctx.update_objects(0, new.rows(yh))
        ctx.init_state(yh.TraceParams.default(resolution=RES))
        ctx.trace_samples(SPP)
        want, want_var = ctx.temporal_accumulate_variance(ctx.temporal_default_params(), ctx.variance_default_params())
    bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)  # noqa: E731
    assert np.array_equal(bits(_read_pfm(acc, RES)), bits(want[..., :3]))
    assert np.array_equal(bits(_read_pfm(var, RES)), bits(np.repeat(want_var[..., None], 3, -1))), "the variance plane as a grey image"
    filtered = ctx.denoise_variance_image(ctx.variance_default_params(), want)[0]
    assert np.array_equal(bits(_read_pfm(dn, RES)), bits(filtered[..., :3]))
    assert not np.array_equal(filtered[..., :3], ctx.denoise(ctx.denoise_default_params(), want)[..., :3]), "and not the fixed-sigma filter's"
    assert ctx.temporal_steps().max() > 1 and want_var.max() > 0
    # --variance alone keeps yh_denoise's filter; the flags without --temporal are refused
    dn2 = str(tmp_path / "acc_dn2.pfm")
    _turntable(tmp_path, "var-only", "--temporal", acc, "--denoise", dn2, "--variance", var)
    assert np.array_equal(bits(_read_pfm(dn2, RES)), bits(ctx.denoise(ctx.denoise_default_params(), want)[..., :3]))
    for flags in (["--variance-guided"], ["--variance", var], ["--temporal", acc, "--variance-guided"]):
        r = subprocess.run([os.path.join(PKG, "ysceneitraces"), scene_path(*SCENE[:1], **SCENE[1]), "--turntable", "2", *flags], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "needs" in r.stdout + r.stderr, flags
    sf.close()
