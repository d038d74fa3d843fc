"""The planes of yh_gbuffer by name (yocto-hair_amd/host/image_planes.h) without a GPU: the feature pass, the a-trous filter and the
temporal stage address the planes, size them and decide which of them a parameter set reads through this one header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_image_planes_rule(tmp_path):
    """tests/cpp/test_image_planes.cpp, compiled with g++ alone (the header needs nothing of HIP): the order, names and bytes per pixel
    of the eleven planes against the members of yh_gbuffer; the filter's mask for the eight on/off combinations of sigma_normal,
    sigma_position and demodulate, for iterations == 0 and for NULL parameters; the temporal step's mask and the union that
    yh_temporal_display traces; the name of the first missing plane for each single NULL and, with several missing, in the order the
    refusals name them. Every expectation is written out by hand in the program."""
    exe = str(tmp_path / "test_image_planes")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "yocto-hair_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "test_image_planes.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
