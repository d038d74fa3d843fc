"""Event times of the temporal stage (yh_temporal_accumulate_device, unit/reproject.hip) next to the filter it feeds and the render it
accumulates, on the metric's scene at 720 x 720 in the metric's view and zoomed in until every pixel is hit. Every round turns the camera
by one degree (there and back), renders 1 spp and takes in turn: the kernel alone on given planes after the turn (four taps per pixel) and
once more in the still view (the one-tap rule), the call with its own feature pass, the five a-trous levels (yh_atrous_filter_gpu, form 1)
and the 1-spp launch of the path shader. Medians of 10 in one process; every figure is a HIP-event time of kernels alone
(yh_last_trace_ms, yh_atrous_level_ms), without allocations or copies. Writes profiles/temporal/latency.txt (or --out) and prints it.

    python tools/temporal_latency.py [--scale 1.0] [--resolution 720] [--rounds 10] [--out FILE]
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

RESOURCES = "k_reproject: 44 VGPRs, no scratch, no spill, no LDS, occupancy 8 waves per SIMD (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)"


def turned(camera, degrees):
    """A copy of `camera` turned about the vertical through the point it focuses on."""
    c = yh.Camera.from_buffer_copy(camera)
    f = np.array(c.frame[:], np.float64).reshape(4, 3)
    centre = f[3] - c.focus * f[2]
    a = np.radians(degrees)
    K = np.array([[0.0, 0, 1], [0, 0, 0], [-1, 0, 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K  # (Rodrigues about y, as the tests write it)
    # (the rotation as a float32 frame first, then composed in double: bit for bit the cameras of tests/test_temporal.py's orbit)
    r = np.concatenate([R.T, (centre - R @ centre)[None]]).astype(np.float32).astype(np.float64)
    m = r[:3].T
    g = np.concatenate([(m @ f[:3].T).T, (m @ f[3] + r[3])[None]])
    c.frame[:] = [float(np.float32(x)) for x in g.reshape(-1)]
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--resolution", type=int, default=720)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal", "latency.txt"))
    a = ap.parse_args()
    ctx = yh.Context(0)
    lines = [RESOURCES]
    for view, kw in (("", {}), (" zoomed", dict(zoom=True))):
        measure(ctx, a, view, kw, lines)
    ctx.close()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text, end="")


def measure(ctx, a, view, kw, lines):
    with tempfile.TemporaryDirectory(prefix="yhair_temporal_") as scenes:
        sf = yh.SceneFile(make_scenes.ensure_scene("sphere-hairblock", scenes, scale=a.scale, **kw))
        ctx.upload_scene(sf.desc, sf.maps)
        cameras = [yh.Camera.from_buffer_copy(sf.desc.contents.camera), turned(sf.desc.contents.camera, 1.0)]
        tp, dp = ctx.temporal_default_params(), ctx.denoise_default_params()
        names = ("yh_trace_samples(1), path shader", "yh_trace_gbuffer_device, object and position", "k_reproject after a 1-degree turn (four taps)",
                 "k_reproject in the still view (one tap)", "yh_temporal_accumulate_device, own guides", "a-trous levels 0 .. 4 (form 1)", "a-trous pack step")
        ms = {k: [] for k in names}
        reused = []
        for r in range(a.rounds + 1):  # (round 0 warms every kind up)
            ctx.update_camera(cameras[r & 1])
            w, h = ctx.init_state(yh.TraceParams.default(resolution=a.resolution, seed=5 + r))
            if r == 0:
                out = torch.zeros((h, w, 4), device="cuda")
                planes = {"object": torch.zeros((h, w), dtype=torch.int32, device="cuda"), "position": torch.zeros((h, w, 3), device="cuda")}
            t = {}
            ctx.trace_samples(1)
            t[names[0]] = ctx.last_trace_ms()[0]
            ctx.trace_gbuffer_device("centre", **planes)
            t[names[1]] = ctx.last_trace_ms()[0]
            ctx.temporal_accumulate_device(tp, out, **planes)
            t[names[2]] = ctx.last_trace_ms()[0]
            lengths = ctx.temporal_lengths()
            ctx.temporal_accumulate_device(tp, out, **planes)
            t[names[3]] = ctx.last_trace_ms()[0]
            ctx.temporal_accumulate_device(tp, out)
            t[names[4]] = ctx.last_trace_ms()[0]
            g = ctx.trace_gbuffer("centre", ("object", "normal", "position", "albedo"))
            ctx.atrous_filter_gpu(1, dp, out.cpu().numpy(), g["object"], g["normal"], g["position"], g["albedo"])
            level = ctx.atrous_level_ms()
            t[names[5]], t[names[6]] = sum(level[1:]), level[0]
            if r:
                for k in names:
                    ms[k].append(t[k])
                reused.append(float((lengths > 1).sum() / max(1, (lengths > 0).sum())))
        d = sf.desc.contents
        segs = sum(d.shapes[i].num_lines for i in range(d.num_shapes))
        lines.append(f"sphere-hairblock{view} at scale {a.scale}: {segs} hair segments, {w} x {h} pixels, {(g['object'] >= 0).mean():.3f} of them hit; "
                     f"max_history {tp.max_history}, sigma position {tp.sigma_position:.4g}; after a turn {np.median(reused):.3f} of the hit pixels reuse the history")
        med = {}
        for k, v in ms.items():
            med[k] = float(np.median(v))
            lines.append(f"  {k:48s} median {med[k]:8.4f} ms   range {min(v):8.4f} .. {max(v):8.4f} ms   ({len(v)} calls)")
        lines.append(f"  k_reproject after a turn / the five a-trous levels: x {med[names[2]] / med[names[5]]:.3f};  / one sample of the path shader: x {med[names[2]] / med[names[0]]:.3f}")
        lines.append(f"  traffic of k_reproject: 32 B in (colour, id, position) + 32 B out (history) + 16 B out (image) per pixel, 32 B per tap read = "
                     f"{(80 + 4 * 32) * w * h / 1e6:.1f} MB with four taps and no cache, {(80 + 32) * w * h / 1e6:.1f} MB with each history pixel read once")
        sf.close()


if __name__ == "__main__":
    main()
