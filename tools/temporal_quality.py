"""The quality condition of tests/test_temporal.py as numbers, and the sweep its defaults were settled with: on the three test scenes at
resolution 64 an orbit of eight 1-degree steps at 4 spp; over the hit pixels of the last view, against its 1 024-spp render, the mean squared
error of the last 4-spp render, of the accumulated image, and of both denoised (default denoise parameters). The renders and planes of the
steps are downloaded once per scene; every parameter pair is then accumulated with the host's form yh_reproject, so the sweep needs the
device only for the renders. Writes profiles/temporal/quality.txt (or --out) and prints it.

    python tools/temporal_quality.py [--out FILE]
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
from temporal_latency import turned  # noqa: E402

SCENES = (("sphere-hairblock", dict(scale=0.05, zoom=True)), ("textured", dict(scale=0.05)), ("lobes", dict(scale=0.05)))
STEPS, SPP, RES = 8, 4, 64
SIGMAS = (0.0, 0.01, 0.02, 0.05, 0.1, 0.2)  # x the scene's diagonal (0: no position test)
HISTORIES = (2, 4, 8, 16, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal", "quality.txt"))
    a = ap.parse_args()
    ctx = yh.Context(0)
    lines = [f"# tools/temporal_quality.py: an orbit of {STEPS} steps of 1 degree at {SPP} spp, resolution {RES}; MSE over the hit pixels of the last view against its",
             "# 1 024-spp render. acc = accumulated, dn = denoised with the default parameters; ratios: acc / last render, acc + dn / last render + dn.",
             "# The defaults (max_history 4, sigma_position 0.2 x the scene's diagonal) are marked *; both ratios must be below 1 (tests/test_temporal.py)."]
    with tempfile.TemporaryDirectory(prefix="yhair_temporal_") as scenes:
        for name, kw in SCENES:
            sf = yh.SceneFile(make_scenes.ensure_scene(name, scenes, **kw))
            ctx.upload_scene(sf.desc, sf.maps)
            ctx.set_shard(0, 1)
            default, dp = ctx.temporal_default_params(), ctx.denoise_default_params()
            diagonal = default.sigma_position / 0.2
            camera, steps = yh.Camera.from_buffer_copy(sf.desc.contents.camera), []
            for k in range(STEPS + 1):
                if k:
                    camera = turned(camera, 1.0)
                    ctx.update_camera(camera)
                ctx.init_state(yh.TraceParams.default(resolution=RES, seed=100 + k))
                ctx.trace_samples(SPP)
                g = ctx.trace_gbuffer("centre", ("object", "normal", "position", "albedo"))
                steps.append((ctx.download(), g, np.frombuffer(bytes(camera), np.float32).copy()))
            ctx.trace_samples(1024 - SPP)
            ref = ctx.download().astype(np.float64)
            render, g, _ = steps[-1]
            hit = g["object"] >= 0
            err = lambda img: float(((img[..., :3] - ref[..., :3]) ** 2)[hit].mean())  # noqa: E731
            dn = lambda img: yh.atrous_filter(dp, img, g["object"], g["normal"], g["position"], g["albedo"])  # noqa: E731
            base, base_dn = err(render), err(dn(render))
            lines.append(f"{name}: {hit.mean():.3f} of the pixels hit, diagonal {diagonal:.4g}; MSE of the last render {base:.4e}, denoised {base_dn:.4e} (x {base_dn / base:.3f})")
            lines.append(f"  {'max_history':>11s} {'sigma / diag':>12s} {'reused':>7s} {'longest':>8s} {'acc / render':>13s} {'acc+dn / render+dn':>19s}")
            for mh in HISTORIES:
                for sg in SIGMAS:
                    p = yh.TemporalParams(mh, float(np.float32(sg) * np.float32(diagonal)), 1)
                    hist = prev = None
                    for img, gk, cam in steps:
                        out, length = yh.reproject(p, img, SPP, gk["object"], gk["position"], hist, cam, prev)
                        hist, prev = (out, length, gk["object"], gk["position"]), cam
                    mark = "*" if mh == default.max_history and abs(sg - 0.2) < 1e-9 else " "
                    lines.append(f" {mark}{mh:11d} {sg:12.3f} {(length > SPP).sum() / max(1, (length > 0).sum()):7.3f} {length.max():8d} {err(out) / base:13.3f} {err(dn(out)) / base_dn:19.3f}")
            sf.close()
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
