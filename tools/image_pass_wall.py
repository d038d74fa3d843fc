"""Wall-clock time of one call of each context entry of the image passes (first-hit features, denoiser, temporal stage, display download) on
the metric's scene at 720 x 720: the median and range of --rounds calls after one warm-up call, the entries taken in turn so that drift hits
them alike. tools/denoise_latency.py and tools/temporal_latency.py report kernel event times; this is the whole call — checks,
allocations, copies, kernels and waits — which is what a change of the host code can move. One process measures one library (YHAIR_LIB
names another build), so an A/B is several processes of each, alternating (profiles/image_passes/refactor_ab.txt).

    python tools/image_pass_wall.py [--scale 1.0] [--resolution 720] [--rounds 10] [--label NAME]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch  # noqa: F401  (first: torch's bundled HIP runtime must be the one libyhair.so binds to)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yocto-hair_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_scenes  # noqa: E402
import yhair_capi as yh  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--resolution", type=int, default=720)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--label", default=os.environ.get("YHAIR_LIB", "the library in place"))
    a = ap.parse_args()
    ctx = yh.Context(0)
    with tempfile.TemporaryDirectory(prefix="yhair_wall_") as scenes:
        sf = yh.SceneFile(make_scenes.ensure_scene("sphere-hairblock", scenes, scale=a.scale))
        ctx.upload_scene(sf.desc, sf.maps)
        w, h = ctx.init_state(yh.TraceParams.default(resolution=a.resolution))
        ctx.trace_samples(4)
        dp, tp = ctx.denoise_default_params(), ctx.temporal_default_params()
        names = ("object", "normal", "position", "albedo")
        out = torch.zeros((h, w, 4), device="cuda")
        planes = {"object": torch.zeros((h, w), dtype=torch.int32, device="cuda")}
        planes.update({n: torch.zeros((h, w, 3), device="cuda") for n in names[1:]})
        entries = {
            "yh_trace_gbuffer (four guides)": lambda: ctx.trace_gbuffer("centre", names),
            "yh_trace_gbuffer_device (four guides)": lambda: ctx.trace_gbuffer_device("centre", **planes),
            "yh_denoise": lambda: ctx.denoise(dp),
            "yh_denoise_image_device": lambda: ctx.denoise_image_device(dp, out),
            "yh_denoise_display": lambda: ctx.denoise_display(dp, 0.5, True, True),
            "yh_temporal_accumulate": lambda: ctx.temporal_accumulate(tp),
            "yh_temporal_accumulate_device": lambda: ctx.temporal_accumulate_device(tp, out),
            "yh_temporal_display": lambda: ctx.temporal_display(tp, dp, 0.5, True, True),
            "yh_temporal_lengths": lambda: ctx.temporal_lengths(),
            "yh_download_display": lambda: ctx.download_display(0.5, True, True),
        }
        ms = {k: [] for k in entries}
        for r in range(a.rounds + 1):  # (round 0 warms every entry up)
            for k, fn in entries.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if r:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
        sf.close()
    ctx.close()
    print(f"{a.label}: sphere-hairblock at scale {a.scale}, {w} x {h} pixels, wall ms per call, median (range) of {a.rounds}")
    for k, v in ms.items():
        print(f"  {k:40s} {float(np.median(v)):9.3f}   ({min(v):.3f} .. {max(v):.3f})")


if __name__ == "__main__":
    main()
