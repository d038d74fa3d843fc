"""The denoiser above the C ABI: the C++ mirror's denoise_image (tests/cpp/test_mirror_denoise.cpp) and `--denoise FILE` of both command
lines, whose file holds the pixels yh_denoise returns (.pfm: rgb floats, top row first) next to an output that is the one written
without the option."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path

PKG = os.path.join(ROOT, "yocto-hair_amd")
SCENE = ("textured", dict(scale=0.05))


def _read_pfm(path, res):
    raw = open(path, "rb").read()
    head = f"PF\n{res} {res}\n-1\n".encode()
    assert raw.startswith(head), raw[:24]
    return np.frombuffer(raw[len(head):], np.float32).reshape(res, res, 3)


@pytest.mark.gpu
def test_mirror_returns_the_image_of_the_c_abi(built, tmp_path):
    exe = str(tmp_path / "mirror_denoise")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host"), "-Wno-class-memaccess", os.path.join(ROOT, "tests", "cpp", "test_mirror_denoise.cpp"),
                           "-o", exe, "-L" + PKG, "-lyhair", "-Wl,-rpath," + PKG, "-lpthread"])
    r = subprocess.run([exe, scene_path(*SCENE[:1], **SCENE[1])], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)


@pytest.mark.gpu
def test_yscenetrace_writes_the_denoised_image(ctx, yh, tmp_path):
    scene = scene_path(*SCENE[:1], **SCENE[1])
    out, dn, plain = (str(tmp_path / n) for n in ("img.pfm", "dn.pfm", "plain.pfm"))
    common = [os.path.join(PKG, "yscenetrace"), scene, "-r", "64", "-s", "4"]
    r = subprocess.run(common + ["-o", out, "--denoise", dn], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "save denoised: " + dn in r.stdout, (r.stdout, r.stderr)
    assert subprocess.run(common + ["-o", plain], capture_output=True, text=True, timeout=300).returncode == 0
    assert open(out, "rb").read() == open(plain, "rb").read(), "the output itself is untouched"
    sf = yh.SceneFile(scene)
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    ctx.init_state(yh.TraceParams.default(resolution=64))
    ctx.trace_samples(4)
    want = ctx.denoise()
    assert np.array_equal(_read_pfm(out, 64), ctx.download()[..., :3])
    assert np.array_equal(_read_pfm(dn, 64).view(np.uint32), np.ascontiguousarray(want[..., :3]).view(np.uint32))
    assert not np.array_equal(_read_pfm(dn, 64), _read_pfm(out, 64))
    sf.close()


@pytest.mark.gpu
def test_ysceneitraces_writes_the_denoised_preview(ctx, yh, tmp_path):
    """After its preview pass (resolution / pratio at 1 spp) --denoise FILE holds that pass denoised, at the preview's resolution."""
    scene = scene_path(*SCENE[:1], **SCENE[1])
    out, dn = str(tmp_path / "img.pfm"), str(tmp_path / "dn.pfm")
    r = subprocess.run([os.path.join(PKG, "ysceneitraces"), scene, "-r", "64", "--pratio", "2", "-s", "2", "-o", out, "--denoise", dn],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "save denoised: " + dn in r.stdout, (r.stdout, r.stderr)
    sf = yh.SceneFile(scene)
    ctx.upload_scene(sf.desc, sf.maps)
    ctx.set_shard(0, 1)
    ctx.init_state(yh.TraceParams.default(resolution=32))
    ctx.trace_samples(1)
    assert np.array_equal(_read_pfm(dn, 32).view(np.uint32), np.ascontiguousarray(ctx.denoise()[..., :3]).view(np.uint32))
    ctx.init_state(yh.TraceParams.default(resolution=64))
    ctx.trace_samples(2)
    assert np.array_equal(_read_pfm(out, 64), ctx.download()[..., :3])
    sf.close()
