#!/usr/bin/env python3
"""Developer tool (GPU box): the most expensive work items of consecutive launches — are they the same items, and how
far above the rest? usage: tools/top_items.py [SCENE RES SPP SHAPE]
expensive_count(costs): how many items are expensive by the host's rule (launch_plan.cpp: expensive_items) — what
tools/chain_profile.py and tools/shading_budget.py hand to Context.set_count_bound for a budget of the heavy items alone."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yocto-hair_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tools"))


def expensive_count(costs):
    """Items within 5 x of the most expensive one (costs: Context.item_costs() of the launch before)."""
    c = np.asarray(costs, np.uint64)
    top = int(c.max()) if c.size else 0
    return int(np.count_nonzero(c * np.uint64(5) >= np.uint64(top))) if top > 0 else 0


def main(argv):
    import torch  # noqa
    import make_scenes, yhair_capi as yh
    name = argv[1] if len(argv) > 1 else "sphere-hairblock"
    res = int(argv[2]) if len(argv) > 2 else 720
    spp = int(argv[3]) if len(argv) > 3 else 64
    os.environ["YHAIR_SHAPE"] = argv[4] if len(argv) > 4 else "0"
    ctx = yh.Context(0)
    sf = yh.SceneFile(make_scenes.ensure_scene(name, os.environ.get("YHAIR_SCENES", "/tmp/yhair_scenes"), scale=1.0))
    ctx.upload_scene(sf.desc)
    ctx.init_state(yh.TraceParams.default(resolution=res))
    tx = (res + 7) // 8
    for k in range(5):
        ctx.trace_samples(spp)
        ms = ctx.last_trace_ms()[0]
        c = ctx.item_costs().astype(np.float64) / 100e3
        top = np.argsort(c)[::-1][:12]
        print(f"launch {k}: {ms:.2f} ms; {expensive_count(ctx.item_costs())} expensive items of {c.size}; top items (tile x, tile y, quadrant: ms): "
              + "  ".join(f"({(t >> 2) % tx},{(t >> 2) // tx},{t & 3}: {c[t]:.2f})" for t in top), flush=True)


if __name__ == "__main__":
    main(sys.argv)
