"""The a-trous filter of yh_denoise in float64: the formula of tests/denoise_f32.py with every operation in double, and how far the
float32 form strays from it on the strata of tests/denoise_cases.py. This pins the restatement, not the device.

The error of one case is relative to the image: max |f32 - f64| over the colour entries that are finite in float64, over the largest
finite |f64| of the image. (Per entry it would be unbounded: a weighted mean of values of both signs cancels.) Where float64 is not finite
float32 must not be either — with one allowance: a finite value beyond float32's range is +-inf there.

    python tests/denoise_f64.py        writes profiles/denoise/errors.txt (the test's bar is 4 x the worst recorded there)
"""
import os

import numpy as np

import denoise_f32
from denoise_cases import ITERATIONS, SIZES, STRATA, make_case, restated

RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "denoise", "errors.txt")


def atrous_filter64(P, rgba, ids, normal=None, position=None, albedo=None):
    return denoise_f32.atrous_filter(P, rgba, ids, normal, position, albedo, dtype=np.float64)


def case_error(P, arrays, f32=None):
    """(relative error of the float32 form on one case, whether the non-finite entries agree); f32: its image where the caller has it."""
    a = (f32 if f32 is not None else denoise_f32.atrous_filter(P, *arrays))[..., :3].astype(np.float64)
    b = atrous_filter64(P, *arrays)[..., :3]
    fin = np.isfinite(b) & (np.abs(b) < np.finfo(np.float32).max)
    agree = bool(np.all(~np.isfinite(a[~fin])))
    both = fin & np.isfinite(a)
    agree = agree and bool(np.array_equal(both, fin))
    if not fin.any():
        return 0.0, agree
    with np.errstate(invalid="ignore"):
        return float(np.abs(a - b)[both].max() / np.abs(b[fin]).max()), agree


def stratum_errors():
    """{stratum: worst relative error over the sizes and iterations}; raises where the non-finite entries disagree."""
    worst = {}
    for stratum in STRATA:
        w_ = 0.0
        for (w, h) in SIZES:
            P, *arrays = make_case(stratum, w, h)
            for it in ITERATIONS:
                err, agree = case_error(dict(P, iterations=it), arrays, restated(stratum, w, h, it))
                assert agree, f"{stratum} {w}x{h} x{it}: float32 and float64 disagree on which entries are finite"
                w_ = max(w_, err)
        worst[stratum] = w_
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
        f.write("# tests/denoise_f64.py: the float32 restatement of the a-trous filter against the same formula in float64,\n"
                "# max |f32 - f64| / max |f64| per image, the worst over the sizes " + ", ".join(f"{w}x{h}" for w, h in SIZES) + " and 0 .. 6 iterations\n")
        for k, v in errs.items():
            f.write(f"{k:16s} {v:.3e}\n")
        f.write(f"worst {max(errs.values()):.3e}\n")
    print(open(RECORD).read())
