"""The parts of yh_upload_scene that need no GPU (yocto-hair_amd/host/blob_layout.h, upload_stages.h), each by a g++-only program: the
upload and the edits lay the traversal array out with one header, and the upload's pure stages are functions over the description."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, name, *args):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "yocto-hair_amd", "host"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe])
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr


def test_blob_layout_rule(tmp_path):
    """tests/cpp/test_blob_layout.cpp over the shape sets of tests/cpp/blob_layout_cases.h: the regions follow each other without overlap,
    every node region is on a 128-byte line, four units of slack follow the last test record, the last 4-wide node and the array's last
    node, lane_units is the end of the 4-wide regions plus 4, the 2^27 and 2^30 refusals trip exactly at the limit; the growth step of
    yh_update_shape keeps a width that fits and moves one that does not to the aligned end with room count + count / 8. The numbers are
    those of tests/golden/blob_layout.txt, written by the code the header replaced."""
    _run(tmp_path, "test_blob_layout", os.path.join(ROOT, "tests", "golden", "blob_layout.txt"))


def test_upload_pure_stages(tmp_path):
    """tests/cpp/test_upload_stages.cpp on a hand-made description: one object row, the environments' rows, the area cdf as one float chain
    in element order, a small light's record, the coarse index of a cdf of 4096 and of 4097 entries, the texture conversion (what is
    uploaded, which textures get a linear copy, the two refusal codes) and the bytes the fingerprint mixes."""
    _run(tmp_path, "test_upload_stages")
