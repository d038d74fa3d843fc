"""The strata of tests/temporal_cases.py hold what they are named for, by the float32 restatement's own account (reproject_f32's info):
so that the bit-for-bit comparisons of test_temporal_cpu.py and test_temporal.py cover every rule of include/yhair.h's TEMPORAL."""
import numpy as np
import pytest

from temporal_cases import SIGMA, SIZES, STRATA, make_case, restated

BIG = [s for s in SIZES if s != (1, 1)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("stratum", STRATA)
def test_a_quarter_of_the_hit_pixels_take_the_history_path(stratum, size):
    case = make_case(stratum, *size)
    out, length, info = restated(stratum, *size)
    hit = case["ids"] != -1
    assert hit.any() and (size == (1, 1) or stratum == "edges" or (~hit).any()), "hits and misses (edges: hits along every border)"
    took = info["history"]
    assert not (took & ~hit).any()
    if stratum == "behind":
        assert not took.any() and info["behind"][info["live"]].all(), "every hit pixel lies behind the previous camera"
        assert (length[info["live"]] == case["samples"]).all()
    else:
        assert took.sum() >= 0.25 * hit.sum(), f"{took.sum()} of {hit.sum()} hit pixels"
        assert (length[took] > case["samples"]).all()
    assert (length[~hit] == 0).all()


@pytest.mark.parametrize("size", BIG, ids=lambda s: f"{s[0]}x{s[1]}")
def test_each_rejection_rule_rejects_in_its_stratum(size):
    info = {s: restated(s, *size)[2] for s in STRATA}
    case = {s: make_case(s, *size) for s in STRATA}
    w, h = size
    assert info["still"]["shortcut"][info["still"]["history"]].all() and info["still"]["history"].any(), "still: the one-tap rule"
    for s in ("pan", "orbit"):
        assert not info[s]["shortcut"].any() and info[s]["history"].any()
    # edges: the outer columns and rows project into (-1, 0) and (w - 1, w), (h - 1, h): taps fall off the image and the rest still counts
    e = info["edges"]
    fx, fy, cand = e["fx"], e["fy"], e["candidates"]
    for lo in (((fx > -1) & (fx < 0)), ((fx > w - 1) & (fx < w)), ((fy > -1) & (fy < 0)), ((fy > h - 1) & (fy < h))):
        assert (lo & cand & e["tap_off_image"] & e["history"]).any()
    assert info["ids"]["tap_other_id"].any() and not info["pan"]["tap_other_id"][info["pan"]["history"]].all()
    L = info["lengths"]
    hlen = case["lengths"]["history"][1]
    assert L["tap_empty"].any() and (hlen == 0).any() and (hlen < 0).any() and (hlen > case["lengths"]["P"]["max_history"]).any()
    length = restated("lengths", *size)[1]
    assert length.max() == case["lengths"]["P"]["max_history"] + case["lengths"]["samples"], "the cap"
    assert ((length > case["lengths"]["samples"]) & (length < length.max())).any(), "and lengths below it"
    nf, c = info["non-finite"], case["non-finite"]
    assert nf["tap_non_finite"].any(), "a history colour"
    assert (~np.isfinite(c["rgba"][..., :3]).all(-1) & (c["ids"] != -1)).any() and not (nf["history"] & ~nf["live"]).any(), "a current colour"
    assert (np.isnan(c["position"]).any(-1) & nf["live"] & ~nf["history"]).any(), "a current position"
    assert nf["tap_far"].any(), "a history position"
    m, cm = info["moving"], case["moving"]
    ids = cm["ids"]
    assert (m["shortcut"] & (ids == 0)).any() and not (m["shortcut"] & np.isin(ids, (1, 2, 3))).any(), "bit-equal frames: the one tap"
    for k in (1, 2):
        assert (m["history"] & (ids == k)).any(), f"object {k} moved and is found again"
    assert (ids == 3).any() and m["unusable"][ids == 3].all() and not m["history"][ids == 3].any(), "the unusable object"


@pytest.mark.parametrize("size", BIG, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sigma_has_pixels_on_both_sides(size):
    case = make_case("sigma", *size)
    out, length, info = restated("sigma", *size)
    x, xq = case["position"].astype(np.float64), case["history"][3].astype(np.float64)
    d2 = ((x - xq) ** 2).sum(-1)  # exact: the operands sit on the 2^-10 grid, or x.x is 0
    hit = case["ids"] != -1
    on, grid_above, float_above = d2 == SIGMA ** 2, d2 == (SIGMA + 2.0 ** -10) ** 2, xq[..., 0] == float(np.nextafter(np.float32(SIGMA), np.float32(1)))
    assert (hit & on).any() and (hit & grid_above).any() and (hit & float_above).any()
    assert (hit & (on | grid_above | float_above)).sum() == hit.sum()
    assert info["history"][hit & on].all(), "|y - x_q|^2 == sigma^2 counts"
    assert not info["history"][hit & ~on].any(), "one grid step or one float above does not"
    assert (info["tap_far"] | info["outside"])[hit & ~on].all(), "(a point moved to x = 0 may leave the image at its border instead)"
    assert info["tap_far"][hit & grid_above].any() and info["tap_far"][hit & float_above].any()
