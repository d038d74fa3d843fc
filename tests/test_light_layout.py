"""The light list's layout rule (yocto-hair_amd/host/light_layout.h) without a GPU: the upload and the light edits both lay their
lists out with this one function, so its rows are what both agree on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_light_layout_rule(tmp_path):
    """tests/cpp/test_light_layout.cpp, compiled with g++ alone (the header needs nothing of HIP): objects before environments, each in
    order, with cdf_base running through both; line shapes and empty shapes are no lights; the LDS record of an emitter of at most four
    triangles; 16 lights pass and a 17th is refused with the index of the object or the environment; no light at all; the coarse
    index of the first textured environment of at least 4096 texels; a constant environment has no cdf. Every expectation is written out
    by hand in the program."""
    exe = str(tmp_path / "test_light_layout")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "yocto-hair_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "test_light_layout.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
