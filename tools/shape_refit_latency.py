"""Latency of a refit of the hair against the vertex edit that builds its tree again, and what a refitted tree costs to render
(profiles/edits/shape_refit_latency.txt).

    python tools/shape_refit_latency.py [--scene sphere-hairblock] [--scale 1.0] [--calls 10] [--render]

One process, the HIP runtime warm (one untimed call of each kind first), wall-clock around the blocking calls, medians and ranges
of --calls calls. The edit is the tests' `sway` (x += a * y^2, tangents recomputed) of the scene's hair shape, alternating between
a = 0.05 and a = 0.1 so that every call changes the arrays; all four forms run in the same process on the same context:
    yh_update_shape / yh_update_shape_device    the yardstick: the reference's tree of the shape again
    yh_refit_shape / yh_refit_shape_device      records and boxes again in the tree of the upload
--render adds the render cost: ms per 64 spp (yh_last_trace_ms, the launches' own time, median of --calls launches once no kernel
trial is pending) on the loaded scene, after an identity refit, and after each of the two sways as a refit and as an update, with
yh_shape_refit_growth beside each.
"""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np
import torch  # noqa: F401  (first: torch's bundled HIP runtime must be the one libyhair.so binds to)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "yocto-hair_amd", "python"))
import make_scenes  # noqa: E402
import yhair_capi as yh  # noqa: E402
from shape_edit_latency import report, tangents, timed  # noqa: E402

F = np.float32
SWAYS = (0.05, 0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sphere-hairblock")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--render", action="store_true")
    ap.add_argument("--resolution", type=int, default=720)
    args = ap.parse_args()
    scenes = tempfile.TemporaryDirectory(prefix="yhair_latency_")
    sf = yh.SceneFile(make_scenes.ensure_scene(args.scene, scenes.name, scale=args.scale))
    src = sf.desc.contents
    hair = next(i for i in range(src.num_shapes) if src.shapes[i].num_lines > 0)
    sh = src.shapes[hair]
    nv, nl = sh.num_vertices, sh.num_lines
    pos0 = np.ctypeslib.as_array(sh.positions, (nv, 3)).copy()
    lines = np.ctypeslib.as_array(sh.lines, (nl, 2)).copy()
    keep, shapes = [], {}
    for a in SWAYS:
        p = pos0.copy()
        p[:, 0] += F(a) * p[:, 1] * p[:, 1]
        n = tangents(p, lines)
        shape = yh.Shape.from_buffer_copy(sh)
        shape.positions, shape.normals = yh.fptr(p), yh.fptr(n)
        keep.append((p, n))
        shapes[a] = shape
    loaded = yh.Shape.from_buffer_copy(sh)
    print(f"{args.scene} at scale {args.scale}: {nl} segments in the edited shape, {src.num_shapes} shapes, {src.num_objects} objects", flush=True)
    ctx = yh.Context(0)
    ctx.upload_scene(sf.desc)
    turn = lambda k: shapes[SWAYS[k % 2]]  # noqa: E731
    T = [{"pos": torch.from_numpy(p).cuda(), "nrm": torch.from_numpy(n).cuda()} for p, n in keep]
    t_lines = torch.from_numpy(lines).cuda()
    radius = torch.from_numpy(np.ctypeslib.as_array(sh.radius, (nv,)).copy()).cuda() if sh.radius else None
    report("yh_update_shape", timed(lambda k: ctx.update_shape(hair, turn(k)), args.calls))
    report("yh_update_shape_device", timed(lambda k: ctx.update_shape_device(hair, T[k % 2]["pos"], normals=T[k % 2]["nrm"], radius=radius, lines=t_lines), args.calls))
    ctx.upload_scene(sf.desc)  # the refits keep the tree of THIS build
    report("yh_refit_shape", timed(lambda k: ctx.refit_shape(hair, turn(k)), args.calls))
    report("yh_refit_shape_device", timed(lambda k: ctx.refit_shape_device(hair, T[k % 2]["pos"], normals=T[k % 2]["nrm"], radius=radius, lines=t_lines), args.calls))
    print(f"  growth after the last refit (a = {SWAYS[args.calls % 2]}): {ctx.shape_refit_growth(hair)}", flush=True)
    if not args.render:
        return

    def ms_per_64(what):
        ctx.set_shard(0, 1)
        ctx.init_state(yh.TraceParams.default(resolution=args.resolution))
        for _ in range(8):  # until the launch shape is settled: a pending trial starts a launch with another kernel
            ctx.trace_samples(64)
            if not ctx.trials_pending():
                break
        ms = []
        for _ in range(args.calls):
            ctx.trace_samples(64)
            ms.append(ctx.last_trace_ms()[0])
        print(f"  {what:<40s} median {np.median(ms):8.2f} ms per 64 spp   range {min(ms):8.2f} .. {max(ms):8.2f}   launch shape {ctx.launch_shape()}   "
              f"growth {['%.4f' % g for g in ctx.shape_refit_growth(hair)]}", flush=True)

    ctx.upload_scene(sf.desc)
    ms_per_64("loaded scene")
    ctx.refit_shape(hair, loaded)
    ms_per_64("identity refit")
    for a in SWAYS:
        ctx.upload_scene(sf.desc)
        ctx.refit_shape(hair, shapes[a])
        ms_per_64(f"sway a = {a}, yh_refit_shape")
        ctx.update_shape(hair, shapes[a])
        ms_per_64(f"sway a = {a}, yh_update_shape")
    ctx.close()


if __name__ == "__main__":
    main()
