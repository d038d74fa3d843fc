#!/usr/bin/env python3
"""Writes tests/golden/maps.npz: the REFERENCE's own images of the `maps` scene (tools/make_scenes.py: make_maps), rendered
with oracle/_ref/libyh_ref.so (built by `make -C oracle ref`) through tests/oracle_capi.Ref. They are what holds the
CPU oracle's restatement of the maps to the reference (tests/test_oracle_golden.py renders every entry bit for bit) and what the
parity of the maps on the device (tests/test_material_maps.py) is checked against.

Entries (float32 (H, W, 4) images unless noted):
  <shader>_<spp>             the whole scene, shader in path / naive / eyelight / normal, spp 1 and 8, seed 961748941, RES^2
  <shader>_8_s777            path / naive / eyelight at 8 spp and seed 777: the seed-to-seed noise floor
  rng_8                      uint64 (H*W, 2): the pixels' PCG32 state and increment after path_8
  only-<map>/<shader>_<spp>  the scene with that one map (tools/make_scenes.py MAP_KINDS), path / naive / eyelight, spp 1, 8
                             and 8 at seed 777, at VRES^2
  res, vres, seeds           what the images were made with
usage: tools/make_map_goldens.py [--out tests/golden/maps.npz]"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "yocto-hair_amd", "python")]
import make_scenes  # noqa: E402
import oracle_capi as oc  # noqa: E402
import yhair_capi as yh  # noqa: E402

RES, VRES = 48, 32
SEED, SEED2 = 961748941, 777
SHADERS = ("path", "naive", "eyelight")


def render(ref, path, res, shader, spp, seed=SEED, want_rng=False):
    sc = ref.scene(path)
    try:
        return sc.render(yh.TraceParams.default(resolution=res, seed=seed, shader=shader), spp, want_rng=want_rng)
    finally:
        sc.close()


def entries(scenes):
    ref = oc.Ref()
    out = {"res": np.int32(RES), "vres": np.int32(VRES), "seeds": np.array([SEED, SEED2], np.uint64)}
    p = make_scenes.ensure_scene("maps", scenes)
    for shader in SHADERS + ("normal",):
        out[f"{shader}_1"] = render(ref, p, RES, shader, 1)
        if shader == "path":
            out["path_8"], out["rng_8"] = render(ref, p, RES, shader, 8, want_rng=True)
        else:
            out[f"{shader}_8"] = render(ref, p, RES, shader, 8)
        if shader != "normal":
            out[f"{shader}_8_s777"] = render(ref, p, RES, shader, 8, seed=SEED2)
    for kind in make_scenes.MAP_KINDS:
        q = make_scenes.ensure_scene("maps", scenes, only=kind)
        for shader in SHADERS:
            out[f"only-{kind}/{shader}_1"] = render(ref, q, VRES, shader, 1)
            out[f"only-{kind}/{shader}_8"] = render(ref, q, VRES, shader, 8)
            out[f"only-{kind}/{shader}_8_s777"] = render(ref, q, VRES, shader, 8, seed=SEED2)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "maps.npz"))
    a = ap.parse_args()
    if not oc.have_ref():
        raise SystemExit(f"{oc.REF_SO} is missing: build it with `make -C oracle ref`")
    with tempfile.TemporaryDirectory(prefix="yhair_maps_") as d:
        e = entries(d)
    np.savez_compressed(a.out, **e)
    print(a.out, os.path.getsize(a.out), "bytes,", len(e), "entries")
