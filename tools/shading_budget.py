#!/usr/bin/env python3
"""Developer tool (GPU box): the budget of a wave iteration's SHADING PASS, region by region (include/yhair.h: yh_shade_regions) — the
waves' cycles per wave iteration, the share of iterations in which the region ran and the lanes it ran with — from one instrumented
launch (yh_trace_samples_counted; launch shape 0: side by side has no instrumented build, its quad half is this kernel). The regions
from `miss` on are what cyc_shade spans; `regen` (the loop head) lies outside it. The static instruction counts of the same regions:
tools/isa_blocks.py --marks on a -DYH_ISA_MARKS assembly (profiles/shading_pass/).
usage: tools/shading_budget.py SCENE RES [WORLD [SPP [heavy]]]   e.g. sphere-hairblock 180 8   (WORLD: shard 0 of WORLD only; SPP per launch, default 64;
heavy: the instrumented launch counts the expensive items alone — top_items.expensive_count of the launch before it, Context.set_count_bound)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yocto-hair_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa
import make_scenes, top_items, yhair_capi as yh
name, res = sys.argv[1], int(sys.argv[2])
world = int(sys.argv[3]) if len(sys.argv) > 3 else 1
SPP = int(sys.argv[4]) if len(sys.argv) > 4 else 64
ctx = yh.Context(0)
sf = yh.SceneFile(make_scenes.ensure_scene(name, os.environ.get("YHAIR_SCENES", "/tmp/yhair_scenes"), scale=1.0))
ctx.upload_scene(sf.desc)
ctx.set_shard(0, world)
os.environ["YHAIR_SHAPE"] = "0"
ctx.init_state(yh.TraceParams.default(resolution=res))
ms = []
for _ in range(3):
    ctx.trace_samples(SPP)
    ms.append(ctx.last_trace_ms()[0])
HEAVY = len(sys.argv) > 5 and sys.argv[5] == "heavy"
heavy = top_items.expensive_count(ctx.item_costs()) if HEAVY else 0
ctx.set_count_bound(heavy)
wc = ctx.trace_samples_counted(SPP).as_dict()
reg = ctx.shade_regions()
wi = max(1, wc["wave_iters"])
const_env = ctx.lights_const_env() if hasattr(ctx.lib, "yh_lights_const_env") else 0
print(f"{name} {res}^2" + (f" (shard 0 of {world})" if world > 1 else "") + f", shape 0" + (f", the {heavy} expensive items alone" if HEAVY else "") + f", {SPP} spp: {min(ms):.2f} ms (instrumented {ctx.last_trace_ms()[0]:.2f}); "
      f"lights_const_env {const_env}; wave iterations {wi}; per wave iteration: trace {wc['cyc_trace'] / wi:.0f} cyc, shade {wc['cyc_shade'] / wi:.0f} cyc")
print(f"{'region':12s} {'cyc / iteration':>16s} {'runs in share of iterations':>28s} {'lanes when it runs':>19s} {'cyc when it runs':>17s}")
named = 0
for nm, (cyc, trips, lanes) in reg.items():
    named += cyc if nm != "regen" else 0
    print(f"{nm:12s} {cyc / wi:16.0f} {trips / wi:28.3f} {lanes / max(1, trips):19.1f} {cyc / max(1, trips):17.0f}")
print(f"regions from miss on: {named / wi:.0f} cyc per iteration = {100.0 * named / max(1, wc['cyc_shade']):.1f} % of cyc_shade "
      f"(the rest: the stamps themselves and the exec bookkeeping between the regions)")
ws = max(1, wc["wave_steps"])
print(f"traversal per wave iteration: wave trips {ws / wi:.2f}, cycles per trip {wc['cyc_trace'] / ws:.0f}, quad trips per ray {wc['lane_steps'] / max(1, wc['lane_iters']):.2f}, live quads {wc['lane_iters'] / wi:.2f}; steps ran in share of trips: "
      + ", ".join(f"{nm} {wc['trips_' + nm] / ws:.3f} ({wc['lanes_' + nm] / max(1, wc['trips_' + nm]):.1f} lanes)" for nm in ("node", "line", "tri", "enter", "scene")))
print(f"per camera sample of the counted items: rays {wc['rays'] / max(1, wc['samples']):.3f}, hair shades {wc['hair_shades'] / max(1, wc['samples']):.3f}, surface shades {wc['surf_shades'] / max(1, wc['samples']):.3f}")
print(f"lane-0 stamps per iteration (path_step of lane 0's quad only): geometry {wc['cyc_geom'] / wi:.0f}, sample {wc['cyc_sample'] / wi:.0f}, eval {wc['cyc_eval'] / wi:.0f}, rest {wc['cyc_rest'] / wi:.0f}")
