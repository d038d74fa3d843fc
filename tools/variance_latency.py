"""Event times of the variance stage (unit/variance.hip) next to their counterparts, on the metric's scene at 720 x 720 in the metric's view
and zoomed in until every pixel is hit. tools/temporal_latency.py's rounds: every round turns the camera by one degree (there and back),
renders 1 spp and takes in turn, each against its counterpart in the same round:
    k_reproject_m + k_var_spatial (yh_temporal_accumulate_variance_device on given planes)   against   k_reproject (yh_temporal_accumulate_device)
    every level of stage F in both forms (yh_atrous_variance_filter_gpu)                     against   k_dn_level in the same form (yh_atrous_filter_gpu)
    yh_svgf_display                                                                          against   yh_temporal_display with the default filter
Medians of 10 in one process; every figure is a HIP-event time of kernels alone (yh_last_trace_ms, yh_atrous_level_ms), without allocations
or copies. Writes profiles/variance/latency.txt (or --out) and prints it.

    python tools/variance_latency.py [--scale 1.0] [--resolution 720] [--rounds 10] [--out FILE]
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

LEVELS = 5  # both filters at five levels, whatever their defaults, so that level l stands next to level l


def measure(ctx, a, view, kw, lines):
    with tempfile.TemporaryDirectory(prefix="yhair_variance_") as scenes:
        sf = yh.SceneFile(make_scenes.ensure_scene("sphere-hairblock", scenes, scale=a.scale, **kw))
        ctx.upload_scene(sf.desc, sf.maps)
        cameras = [yh.Camera.from_buffer_copy(sf.desc.contents.camera), turned(sf.desc.contents.camera, 1.0)]
        tp, dp, vp = ctx.temporal_default_params(), ctx.denoise_default_params(), ctx.variance_default_params()
        dp5, vp5 = dp.copy(iterations=LEVELS), vp.copy(iterations=LEVELS)
        ms = {}
        for r in range(a.rounds + 1):  # (round 0 warms every kind up)
            ctx.update_camera(cameras[0])  # (the round before ended in the other view: a turn)
            w, h = ctx.init_state(yh.TraceParams.default(resolution=a.resolution, seed=5 + r))
            if r == 0:
                out, var = torch.zeros((h, w, 4), device="cuda"), torch.zeros((h, w), device="cuda")
                planes = {"object": torch.zeros((h, w), dtype=torch.int32, device="cuda"), "position": torch.zeros((h, w, 3), device="cuda"),
                          "albedo": torch.zeros((h, w, 3), device="cuda")}
            t = {}
            ctx.trace_samples(1)
            ctx.trace_gbuffer_device("centre", **planes)
            # each kernel once after a turn of one degree (four taps), then once in the still view (the one-tap rule)
            ctx.temporal_accumulate_variance_device(tp, vp, out, var, **planes)
            t["k_reproject_m + k_var_spatial after a 1-degree turn"] = ctx.last_trace_ms()[0]
            ctx.update_camera(cameras[1])  # (an edit takes the image state with it)
            ctx.init_state(yh.TraceParams.default(resolution=a.resolution, seed=105 + r))
            ctx.trace_samples(1)
            ctx.trace_gbuffer_device("centre", **planes)
            ctx.temporal_accumulate_device(tp, out, object=planes["object"], position=planes["position"])
            t["k_reproject after a 1-degree turn"] = ctx.last_trace_ms()[0]
            ctx.temporal_accumulate_device(tp, out, object=planes["object"], position=planes["position"])
            t["k_reproject in the still view"] = ctx.last_trace_ms()[0]
            ctx.temporal_accumulate_variance_device(tp, vp, out, var, **planes)
            t["k_reproject_m + k_var_spatial in the still view, the moments starting again (every tile reads its windows)"] = ctx.last_trace_ms()[0]
            for _ in range(vp.min_steps):
                ctx.temporal_accumulate_variance_device(tp, vp, out, var, **planes)
            t["k_reproject_m + k_var_spatial in the still view, settled (no tile reads a window)"] = ctx.last_trace_ms()[0]
            g = ctx.trace_gbuffer("centre", ("object", "normal", "position", "albedo"))
            image, variance = out.cpu().numpy(), var.cpu().numpy()
            for form in (0, 1):
                ctx.atrous_filter_gpu(form, dp5, image, g["object"], g["normal"], g["position"], g["albedo"])
                for k, x in enumerate(ctx.atrous_level_ms()):
                    t[f"form {form} {'pack' if k == 0 else 'level %d' % (k - 1)}: k_dn"] = x
                ctx.atrous_variance_filter_gpu(form, vp5, image, variance, g["object"], g["normal"], g["position"], g["albedo"])
                for k, x in enumerate(ctx.atrous_level_ms()):
                    t[f"form {form} {'pack' if k == 0 else 'level %d' % (k - 1)}: k_vdn"] = x
            ctx.temporal_display(tp, dp)
            t["yh_temporal_display (default filter)"] = ctx.last_trace_ms()[0]
            ctx.svgf_display(tp, vp)
            t["yh_svgf_display (defaults)"] = ctx.last_trace_ms()[0]
            if r:
                for k, x in t.items():
                    ms.setdefault(k, []).append(x)
        lines.append(f"sphere-hairblock{view} at scale {a.scale}: {w} x {h} pixels, {(g['object'] >= 0).mean():.3f} of them hit; filter defaults: fixed-sigma {dp.iterations} "
                     f"levels, variance-guided {vp.iterations} levels; the levels below are timed at {LEVELS} each")
        med = {k: float(np.median(v)) for k, v in ms.items()}
        for k, v in ms.items():
            lines.append(f"  {k:72s} median {med[k]:8.4f} ms   range {min(v):8.4f} .. {max(v):8.4f} ms   ({len(v)} calls)")
        for form in (0, 1):
            for k in ["pack"] + [f"level {l}" for l in range(LEVELS)]:
                lines.append(f"  form {form} {k}: k_vdn / k_dn x {med[f'form {form} {k}: k_vdn'] / med[f'form {form} {k}: k_dn']:.3f}")
        for l in range(LEVELS):
            lines.append(f"  k_vdn level {l}: form 1 / form 0 x {med[f'form 1 level {l}: k_vdn'] / med[f'form 0 level {l}: k_vdn']:.3f}")
        lines.append(f"  yh_svgf_display / yh_temporal_display x {med['yh_svgf_display (defaults)'] / med['yh_temporal_display (default filter)']:.3f}")
        sf.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--resolution", type=int, default=720)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variance", "latency.txt"))
    a = ap.parse_args()
    ctx = yh.Context(0)
    lines = ["# tools/variance_latency.py: HIP-event times of kernels alone, medians of the rounds of one process (the kernels' registers and LDS: unit/variance.hip's header)"]
    for view, kw in (("", {}), (" zoomed", dict(zoom=True))):
        measure(ctx, a, view, kw, lines)
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
