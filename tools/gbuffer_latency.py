"""Event times of the first-hit feature pass (yh_trace_gbuffer) next to the work it resembles, on the metric's scene at 720 x 720:
one 1-spp launch of the `normal` shader (the same first-hit work inside the sample loop) and yh_intersect_batch of the pass's own rays.
Medians of 10 in one process, the four kinds of call taken in turn so that drift hits them alike; every figure is yh_last_trace_ms, the
kernel's HIP-event time without allocations or copies. Writes what profiles/gbuffer/latency.txt holds to stdout.

    python tools/gbuffer_latency.py [--scale 1.0] [--resolution 720] [--rounds 10]
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
    a = ap.parse_args()
    ctx = yh.Context(0)
    with tempfile.TemporaryDirectory(prefix="yhair_gbuffer_") as scenes:
        sf = yh.SceneFile(make_scenes.ensure_scene("sphere-hairblock", scenes, scale=a.scale))
        ctx.upload_scene(sf.desc, sf.maps)
        w, h = ctx.init_state(yh.TraceParams.default(resolution=a.resolution, shader="normal"))
        g = ctx.trace_gbuffer("centre")
        n = w * h
        rays = np.concatenate([g["ray"].reshape(n, 6), np.full((n, 1), 1e-4, np.float32), np.full((n, 1), np.finfo(np.float32).max, np.float32)], axis=1).astype(np.float32)
        kinds = {
            "yh_trace_gbuffer, centre, all planes": lambda: ctx.trace_gbuffer("centre"),
            "yh_trace_gbuffer, centre, object + distance": lambda: ctx.trace_gbuffer("centre", planes=["object", "distance"]),
            "yh_trace_gbuffer, next sample, all planes": lambda: ctx.trace_gbuffer("next"),
            "yh_trace_samples(1), normal shader": lambda: ctx.trace_samples(1),
            "yh_intersect_batch of the pass's rays": lambda: ctx.intersect(rays),
        }
        ms = {k: [] for k in kinds}
        for r in range(a.rounds + 1):  # (round 0 warms every kind up)
            for k, fn in kinds.items():
                fn()
                if r:
                    ms[k].append(ctx.last_trace_ms()[0])
        d = sf.desc.contents
        segs = sum(d.shapes[i].num_lines for i in range(d.num_shapes))
        print(f"sphere-hairblock at scale {a.scale}: {segs} hair segments, {w} x {h} pixels, {(g['object'] >= 0).mean():.3f} of them hit")
        med = {}
        for k, v in ms.items():
            med[k] = float(np.median(v))
            print(f"  {k:46s} median {med[k]:8.3f} ms   range {min(v):8.3f} .. {max(v):8.3f} ms   ({len(v)} calls)")
        names = list(kinds)
        print(f"  all planes / normal shader 1 spp: x {med[names[0]] / med[names[3]]:.2f};  all planes / yh_intersect_batch: x {med[names[0]] / med[names[4]]:.2f};"
              f"  object + distance / all planes: x {med[names[1]] / med[names[0]]:.2f}")
        sf.close()
    ctx.close()


if __name__ == "__main__":
    main()
