"""The temporal stage of yh_reproject in float64: the formula of tests/reproject_f32.py with every operation in double, and how far the
float32 form strays from it on the strata of tests/temporal_cases.py. This pins the restatement, not the device.

Two figures per stratum, the worst over the sizes: the projection's error max |fx - fx64|, |fy - fy64| in pixels over the pixels both forms
project into the image, and the blend's error max |out - out64| / max |out64| over the pixels where both forms take the history path from
the same taps (a point that rounds across a pixel border or across sigma takes other taps: a decision, not an error).

    python tests/reproject_f64.py        writes profiles/temporal/errors.txt (the test's bar is 4 x the worst projection error there)
"""
import os

import numpy as np

import reproject_f32
from temporal_cases import SIZES, STRATA, arguments, make_case, restated

RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "temporal", "errors.txt")


def reproject64(P, *args):
    return reproject_f32.reproject(P, *args, dtype=np.float64)


def case_errors(stratum, w, h):
    """(projection error in pixels, relative blend error) of the float32 form on one case"""
    case = make_case(stratum, w, h)
    out, length, info = restated(stratum, w, h)
    out64, length64, info64 = reproject64(case["P"], *arguments(case))
    both = info["candidates"] & info64["candidates"]
    proj = 0.0
    if both.any():
        proj = float(max(np.abs(info["fx"].astype(np.float64) - info64["fx"])[both].max(), np.abs(info["fy"].astype(np.float64) - info64["fy"])[both].max()))
    same = info["history"] & info64["history"] & (length == length64)
    same &= (np.floor(info["fx"]) == np.floor(info64["fx"])) & (np.floor(info["fy"]) == np.floor(info64["fy"]))
    blend = 0.0
    if same.any():  # (a pass-through NaN is never in `same`)
        with np.errstate(invalid="ignore"):
            blend = float(np.abs(out[..., :3].astype(np.float64) - out64[..., :3])[same].max() / np.abs(out64[..., :3][same]).max())
    return proj, blend


def stratum_errors():
    """{stratum: (worst projection error, worst blend error) over the sizes}"""
    worst = {}
    for stratum in STRATA:
        errs = [case_errors(stratum, w, h) for (w, h) in SIZES]
        worst[stratum] = (max(e[0] for e in errs), max(e[1] for e in errs))
    return worst


def recorded_worst():
    for line in open(RECORD):
        if line.startswith("worst "):
            return float(line.split()[1])
    raise RuntimeError(RECORD + " has no `worst` line")


if __name__ == "__main__":
    errs = stratum_errors()
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as f:
        f.write("# tests/reproject_f64.py: the float32 restatement of the temporal stage against the same formula in float64, the worst over the\n"
                "# sizes " + ", ".join(f"{w}x{h}" for w, h in SIZES) + ": the projection max |fx - fx64| in pixels, the blend max |out - out64| / max |out64|\n"
                "# stratum          projection  blend\n")
        for k, (p, b) in errs.items():
            f.write(f"{k:16s} {p:.3e}   {b:.3e}\n")
        worst = max(p for p, _ in errs.values())
        f.write(f"worst {worst:.3e}\n")
        f.write(f"bar   {4 * worst:.3e}   (4 x the worst projection error: tests/test_temporal_cpu.py)\n")
    print(open(RECORD).read())
