#!/usr/bin/env python3
"""tests/golden/instances.npz: the `fur-field` scene (tools/make_scenes.py: two instanced objects) rendered by the REFERENCE'S
COMMAND LINE, which is where the reference expands instances (apps/yscenetrace/yscenetrace.cpp:150-181) — the scene shim of
oracle/_ref/libyh_ref.so does not. Needs oracle/_ref/yscenetrace_ref (make -C oracle ref, where the reference's sources
exist). Images only: `path` at 1 and 4 samples per pixel, `normal` at 1, 64 x 64, default seed and parameters.

    python tools/make_instance_goldens.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_scenes  # noqa: E402

REF_CLI = os.path.join(ROOT, "oracle", "_ref", "yscenetrace_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden", "instances.npz")
# what the goldens were rendered on; tests/test_instances.py builds the same scene
SCENE, SCENE_KW, RESOLUTION = "fur-field", dict(scale=0.25, count=300), 64
RENDERS = {"path_1": ("path", 1), "path_4": ("path", 4), "normal_1": ("normal", 1)}


def read_pfm(path):
    """The reference's .pfm (yocto_image.cpp:1527-1556): "PF", "w h", "-1", float32 RGB rows, top row first."""
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0
        return np.frombuffer(f.read(), "<f4").reshape(h, w, 3).copy()


def reference_render(scene_json, shader, spp, out_dir, resolution=RESOLUTION):
    out = os.path.join(out_dir, f"{shader}_{spp}.pfm")
    r = subprocess.run([REF_CLI, scene_json, "-r", str(resolution), "-s", str(spp), "-t", shader, "-o", out],
                       capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(out):
        raise RuntimeError(f"yscenetrace_ref exited {r.returncode}: {(r.stdout + r.stderr)[-300:]}")
    return read_pfm(out)


if __name__ == "__main__":
    if not os.path.exists(REF_CLI):
        sys.exit("oracle/_ref/yscenetrace_ref is missing: make -C oracle ref")
    with tempfile.TemporaryDirectory(prefix="yhair_instances_") as tmp:
        scene = make_scenes.ensure_scene(SCENE, tmp, **SCENE_KW)
        images = {k: reference_render(scene, shader, spp, tmp) for k, (shader, spp) in RENDERS.items()}
    np.savez_compressed(GOLDEN, **images)
    print(GOLDEN, {k: (v.shape, float(v.mean())) for k, v in images.items()}, os.path.getsize(GOLDEN), "bytes")
