"""The quality condition of tests/test_variance.py as numbers, and the sweep the defaults of yh_variance_default_params were settled with.
tools/temporal_quality.py's setup: the three test scenes at resolution 64, an orbit of eight 1-degree steps at 4 spp, MSE over the hit
pixels of the last view against its 1 024-spp render. The renders and planes of the steps are downloaded once per scene; every setting is
then run with the host's forms (yh_reproject_moments, yh_variance_spatial, yh_atrous_variance_filter), so the sweep needs the device only
for the renders. Two ratios per scene and setting, for the new chain (accumulate with moments + the variance-guided filter):
    vs render+dn   against the last render through the fixed-sigma filter (yh_atrous_filter, default parameters): the denominator of
                   tests/test_temporal.py
    vs acc+dn      against the accumulated image through the fixed-sigma filter: the parent's chain on the same accumulated image
The sweep runs on the test's orbit; the defaults and their neighbours in it are then held against the other five orbits and seeds of
profiles/temporal/quality.txt at max_history 4, 8 and 16. Writes profiles/variance/quality.txt (or --out) and prints it.

    python tools/variance_quality.py [--out FILE]
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
from temporal_quality import RES, SCENES, SPP, STEPS  # noqa: E402

HISTORIES = (4, 8, 16)
SIGMAS = (1.0, 2.0, 4.0, 8.0, 16.0)
EPSILONS = (1e-6, 1e-4, 1e-2)
MIN_STEPS = (2, 4)
ITERATIONS = (4, 5)


def chain(tp, vp, steps):
    """The orbit through stages M and S, then F on the last view; returns (accumulated, variance, filtered)."""
    hist = mom = prev = None
    for img, g, cam in steps:
        out, length, m, s = yh.reproject_moments(tp, img, SPP, g["object"], g["position"], g["albedo"] if vp.demodulate else None, hist, mom, cam, prev)
        hist, mom, prev = (out, length, g["object"], g["position"]), (m, s), cam
    var = yh.variance_spatial(tp, vp.min_steps, m, s, g["object"], g["position"])
    return out, var, yh.atrous_variance_filter(vp, out, var, g["object"], g["normal"], g["position"], g["albedo"])[0]


ORBITS = ((1.0, 100), (-1.0, 100), (1.0, 300), (-1.0, 500), (0.5, 700), (2.0, 900))  # degrees per step, seed: those of profiles/temporal/quality.txt; the first is the test's
# (iterations, sigma_luminance, epsilon) held against every orbit: the defaults and their neighbours in the sweep
CANDIDATES = ((4, 2.0, 1e-2), (4, 2.0, 1e-4), (4, 1.0, 1e-2), (4, 4.0, 1e-2), (5, 2.0, 1e-2))


def orbit(ctx, sf, degrees, seed):
    """The renders, planes and cameras of the orbit's nine views, and the 1 024-spp render of the last."""
    camera, steps = yh.Camera.from_buffer_copy(sf.desc.contents.camera), []
    ctx.update_camera(camera)
    for k in range(STEPS + 1):
        if k:
            camera = turned(camera, degrees)
            ctx.update_camera(camera)
        ctx.init_state(yh.TraceParams.default(resolution=RES, seed=seed + k))
        ctx.trace_samples(SPP)
        g = ctx.trace_gbuffer("centre", ("object", "normal", "position", "albedo"))
        steps.append((ctx.download(), g, np.frombuffer(bytes(camera), np.float32).copy()))
    ctx.trace_samples(1024 - SPP)
    return steps, ctx.download().astype(np.float64)


def is_default(vp0, it, sl, eps):
    return it == vp0.iterations and abs(sl - vp0.sigma_luminance) < 1e-6 and abs(eps / vp0.epsilon - 1) < 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variance", "quality.txt"))
    a = ap.parse_args()
    ctx = yh.Context(0)
    lines = [f"# tools/variance_quality.py: an orbit of {STEPS} steps of 1 degree at {SPP} spp, resolution {RES}; MSE over the hit pixels of the last view against its",
             "# 1 024-spp render. The new chain = accumulate with moments (M, S) + the variance-guided filter (F). Ratios of its MSE:",
             "#   vs render+dn = / (last render through the fixed-sigma filter);  vs acc+dn = / (the same accumulated image through the fixed-sigma filter).",
             "# The defaults of yh_variance_default_params are marked *; with them the first ratio must be below 1 (tests/test_variance.py)."]
    others = ["# Other orbits and seeds (those of profiles/temporal/quality.txt; the same measure, min_steps the default's): per max_history the two ratios,",
              "# vs render+dn then vs acc+dn. * = the defaults; the first row of a scene is the orbit above and of tests/test_variance.py.",
              f"#   {'scene':16s} {'degrees':>7s} {'seed':>5s} {'iterations':>10s} {'sigma_lum':>9s} {'epsilon':>8s}   max_history 4   max_history 8   max_history 16"]
    worst = {}
    with tempfile.TemporaryDirectory(prefix="yhair_variance_") as scenes:
        for name, kw in SCENES:
            sf = yh.SceneFile(make_scenes.ensure_scene(name, scenes, **kw))
            ctx.upload_scene(sf.desc, sf.maps)
            ctx.set_shard(0, 1)
            tp0, dp, vp0 = ctx.temporal_default_params(), ctx.denoise_default_params(), ctx.variance_default_params()
            for degrees, seed in ORBITS:
                steps, ref = orbit(ctx, sf, degrees, seed)
                render, g, _ = steps[-1]
                hit = g["object"] >= 0
                err = lambda img: float(((img[..., :3] - ref[..., :3]) ** 2)[hit].mean())  # noqa: E731
                dn = lambda img: yh.atrous_filter(dp, img, g["object"], g["normal"], g["position"], g["albedo"])  # noqa: E731
                base_dn = err(dn(render))
                if (degrees, seed) == ORBITS[0]:  # the sweep, on the test's orbit
                    lines.append(f"{name}: {hit.mean():.3f} of the pixels hit; MSE of the last render {err(render):.4e}, through the fixed-sigma filter {base_dn:.4e}")
                    lines.append(f"  {'max_history':>11s} {'iterations':>10s} {'sigma_lum':>9s} {'epsilon':>8s} {'min_steps':>9s} {'mean var':>10s} {'vs render+dn':>13s} {'vs acc+dn':>10s}")
                    for mh in HISTORIES:
                        tp = tp0.copy(max_history=mh)
                        acc_dn = None
                        for it in ITERATIONS:
                            for sl in SIGMAS:
                                for eps in EPSILONS:
                                    for ms in MIN_STEPS:
                                        vp = vp0.copy(iterations=it, sigma_luminance=sl, epsilon=eps, min_steps=ms)
                                        acc, var, out = chain(tp, vp, steps)
                                        acc_dn = err(dn(acc)) if acc_dn is None else acc_dn
                                        same = mh == tp0.max_history and ms == vp0.min_steps and is_default(vp0, it, sl, eps)
                                        lines.append(f" {'*' if same else ' '}{mh:11d} {it:10d} {sl:9.1f} {eps:8.0e} {ms:9d} {float(var[hit].mean()):10.3e} {err(out) / base_dn:13.3f} {err(out) / acc_dn:10.3f}")
                for it, sl, eps in CANDIDATES:
                    vp, cells = vp0.copy(iterations=it, sigma_luminance=sl, epsilon=eps), []
                    for mh in HISTORIES:
                        acc, var, out = chain(tp0.copy(max_history=mh), vp, steps)
                        r1, r2 = err(out) / base_dn, err(out) / err(dn(acc))
                        cells.append(f"{r1:.3f} {r2:.3f}")
                        if mh == tp0.max_history:
                            w = worst.setdefault((it, sl, eps), [0.0, 0.0])
                            w[0], w[1] = max(w[0], r1), max(w[1], r2)
                    others.append(f"# {'*' if is_default(vp0, it, sl, eps) else ' '} {name:16s} {degrees:7.1f} {seed:5d} {it:10d} {sl:9.1f} {eps:8.0e}   " + "     ".join(cells))
            sf.close()
    ctx.close()
    others.append(f"# The largest of the eighteen rows at max_history {tp0.max_history}, vs render+dn and vs acc+dn: "
                  + "; ".join(f"({it}, {sl:g}, {eps:g}) {w[0]:.3f} {w[1]:.3f}" for (it, sl, eps), w in worst.items()))
    text = "\n".join(lines + others) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
