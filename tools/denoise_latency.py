"""Event times of the denoiser (yh_denoise_image_device, unit/denoise.hip) next to the render it cleans, on the metric's scene at
720 x 720, in the metric's view and zoomed in until every pixel is hit: the whole default denoise with its own guides and with given ones,
every level of the filter in form 0 (taps from memory)
and form 1 (an LDS tile), one 1-spp launch of the path shader and yh_trace_gbuffer_device. Medians of 10 in one process, the kinds
of call taken in turn so that drift hits them alike; every figure is a HIP-event time of kernels alone (yh_last_trace_ms,
yh_atrous_level_ms), without allocations or copies. Writes profiles/denoise/latency.txt (or --out) and prints it.

    python tools/denoise_latency.py [--scale 1.0] [--resolution 720] [--rounds 10] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--resolution", type=int, default=720)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise", "latency.txt"))
    a = ap.parse_args()
    ctx = yh.Context(0)
    lines = []
    # the metric's view (most pixels miss: they pass a level unchanged), then the zoomed view, where every pixel is filtered
    for view, kw in (("", {}), (" zoomed", dict(zoom=True))):
        measure(ctx, a, view, kw, lines)
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text, end="")


def measure(ctx, a, view, kw, lines):
    with tempfile.TemporaryDirectory(prefix="yhair_denoise_") as scenes:
        sf = yh.SceneFile(make_scenes.ensure_scene("sphere-hairblock", scenes, scale=a.scale, **kw))
        ctx.upload_scene(sf.desc, sf.maps)
        w, h = ctx.init_state(yh.TraceParams.default(resolution=a.resolution))
        ctx.trace_samples(4)
        p = ctx.denoise_default_params()
        render = ctx.download()
        g = ctx.trace_gbuffer("centre", ("object", "normal", "position", "albedo"))
        out = torch.zeros((h, w, 4), device="cuda")
        planes = {"object": torch.zeros((h, w), dtype=torch.int32, device="cuda")}
        planes.update({n: torch.zeros((h, w, 3), device="cuda") for n in ("normal", "position", "albedo")})
        levels = {0: [], 1: []}

        def unit(form):
            ctx.atrous_filter_gpu(form, p, render, g["object"], g["normal"], g["position"], g["albedo"])
            levels[form].append(ctx.atrous_level_ms())
        kinds = {
            "yh_denoise_image_device, own guides": lambda: ctx.denoise_image_device(p, out),
            "yh_denoise_image_device, given guides": lambda: ctx.denoise_image_device(p, out, **planes),
            "yh_trace_gbuffer_device, the four guides": lambda: ctx.trace_gbuffer_device("centre", **planes),
            "yh_trace_samples(1), path shader": lambda: ctx.trace_samples(1),
            "yh_atrous_filter_gpu, form 0": lambda: unit(0),
            "yh_atrous_filter_gpu, form 1": lambda: unit(1),
        }
        ms = {k: [] for k in kinds}
        for r in range(a.rounds + 1):  # (round 0 warms every kind up)
            for k, fn in kinds.items():
                fn()
                if r:
                    ms[k].append(ctx.last_trace_ms()[0])
        d = sf.desc.contents
        segs = sum(d.shapes[i].num_lines for i in range(d.num_shapes))
        lines.append(f"sphere-hairblock{view} at scale {a.scale}: {segs} hair segments, {w} x {h} pixels, {(g['object'] >= 0).mean():.3f} of them hit; "
                     f"{p.iterations} iterations, sigma colour {p.sigma_color:g} normal {p.sigma_normal:g} position {p.sigma_position:.4g}")
        med = {}
        for k, v in ms.items():
            med[k] = float(np.median(v))
            lines.append(f"  {k:44s} median {med[k]:8.3f} ms   range {min(v):8.3f} .. {max(v):8.3f} ms   ({len(v)} calls)")
        names = list(kinds)
        lines.append(f"  denoise with own guides / one sample of the path shader: x {med[names[0]] / med[names[3]]:.3f};  the filter alone (given guides): x {med[names[1]] / med[names[3]]:.3f}")
        lines.append(f"  per kernel, medians of {a.rounds} (ms); traffic floor of a level: 64 B per pixel = {64 * w * h / 1e6:.1f} MB")
        lines.append(f"  {'kernel':10s} {'spacing':>8s} {'form 0':>9s} {'form 1':>9s} {'form 1 / form 0':>16s}")
        for k in range(1 + p.iterations):
            t = [float(np.median([row[k] for row in levels[f][1:]])) for f in (0, 1)]
            staged = 1 <= k <= ctx.lib.yhk_dn_tiled_levels()
            lines.append(f"  {'pack' if k == 0 else f'level {k - 1}':10s} {'' if k == 0 else 1 << (k - 1):>8} {t[0]:9.4f} {t[1]:9.4f} {t[1] / t[0]:16.3f}"
                         + ("" if k == 0 or staged else "   (form 1 runs form 0's kernel here)"))
        sf.close()


if __name__ == "__main__":
    main()
