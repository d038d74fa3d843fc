#!/usr/bin/env python3
"""Generates tests/golden/ref_digests.json from the REAL reference (oracle/_ref/libyh_ref.so, built by
`make -C oracle ref`): the digests of the reference's outputs on every case of tests/ref_cases.py, so that
tests/test_oracle_vs_ref.py holds the oracle to the reference where the reference is not built.

Test infrastructure: digests of expected outputs only — no reference source is stored.
"""
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_scenes  # noqa: E402
import oracle_capi as oc  # noqa: E402
import ref_cases as rc  # noqa: E402


def main():
    if not oc.have_ref():
        raise SystemExit(f"{oc.REF_SO} is missing: build it with `make -C oracle ref`")
    ref = oc.Ref()
    scenes = tempfile.mkdtemp(prefix="yhair_ref_digests_")
    try:
        scene_path = lambda name, **kw: make_scenes.ensure_scene(name, scenes, **kw)  # noqa: E731
        runs = {"bsdf_random_inputs": rc.bsdf_random_inputs, "surface_lobes_random_inputs": rc.surface_lobes_random_inputs,
                "curve_conversion_random_inputs": rc.curve_conversion_random_inputs}
        for name, kw, res, spp in rc.IMAGE_CASES:
            runs[rc.image_key(name, kw, res, spp)] = lambda api, c=(name, kw, res, spp): rc.render(api, scene_path, *c)
        for name, kw, res, spp in rc.SHADER_CASES:
            for shader in rc.SHADERS:
                runs[rc.image_key(name, kw, res, spp, shader)] = lambda api, c=(name, kw, res, spp, shader): rc.render(api, scene_path, *c)
        out = {}
        for key, run in runs.items():
            out[key] = {k: rc.digest(v) for k, v in run(ref).items()}
            print(key, flush=True)
    finally:
        shutil.rmtree(scenes, ignore_errors=True)
    with open(rc.DIGESTS, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
