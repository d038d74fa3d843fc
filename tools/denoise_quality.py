"""The quality condition of tests/test_denoise.py as numbers: on the three test scenes at resolution 64, the mean squared error over the
hit pixels of the 4-spp image and of its denoised form (default parameters, default clamp) against the 1 024-spp render of the same
context. Writes profiles/denoise/quality.txt (or --out) and prints it.

    python tools/denoise_quality.py [--out FILE]
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch  # noqa: F401  (first: torch's bundled HIP runtime must be the one libyhair.so binds to)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yocto-hair_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_scenes  # noqa: E402
import yhair_capi as yh  # noqa: E402

SCENES = (("sphere-hairblock", dict(scale=0.05, zoom=True)), ("textured", dict(scale=0.05)), ("lobes", dict(scale=0.05)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise", "quality.txt"))
    a = ap.parse_args()
    ctx = yh.Context(0)
    lines = ["# tools/denoise_quality.py: MSE over hit pixels against the 1 024-spp render of the same context, resolution 64, 4 spp, default parameters",
             f"# {'scene':18s} {'hit':>6s} {'sigma_position':>15s} {'MSE 4 spp':>12s} {'MSE denoised':>13s} {'ratio':>7s}"]
    with tempfile.TemporaryDirectory(prefix="yhair_denoise_") as scenes:
        for name, kw in SCENES:
            sf = yh.SceneFile(make_scenes.ensure_scene(name, scenes, **kw))
            ctx.upload_scene(sf.desc, sf.maps)
            ctx.set_shard(0, 1)
            ctx.init_state(yh.TraceParams.default(resolution=64))
            ctx.trace_samples(4)
            p = ctx.denoise_default_params()
            noisy, clean = ctx.download(), ctx.denoise(p)
            hit = ctx.trace_gbuffer("centre", ("object",))["object"] >= 0
            ctx.trace_samples(1020)
            ref = ctx.download().astype(np.float64)
            err = lambda img: float(((img[..., :3] - ref[..., :3]) ** 2)[hit].mean())
            lines.append(f"  {name:18s} {hit.mean():6.3f} {p.sigma_position:15.4f} {err(noisy):12.4e} {err(clean):13.4e} {err(clean) / err(noisy):7.3f}")
            sf.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
