"""Closest hits with the traversal stacks past their windows: variant `deep` of the scene hits-unit (tools/make_scenes.py), a chain of
44 collinear segments whose tree is 15 four-wide nodes deep, in front of the objects of `four`. tests/test_hit_cases.py proves on the
CPU, before anything runs here, that the upload's rule accepts the scene with more than 16 entries to spare, that the rays through
the chain's small end stand 30 entries high at their first leaf — the one-lane kernels keep 16 in LDS (dev_lane.h: lane_push,
lane_pop spill the rest into the overflow array), the quads' LDS stack (YH_QSTACK) is filled as far — and never above what the rule
reserves, and that hundreds of them end on an object whose ENTER entry lay beneath all that.

The rays (hit_cases.deep_rays): 8 192 along and near +-x through the chain and 8 192 of stratum a, repeated to the 65 536 of the
one-lane kernel, as they are through the quad form and the eleven forms of yh_intersect_plain_batch (test_hits_unit.FORMS: the wide
stacks stand as high here — 30 entries over 8- and 16-wide nodes too, within the 7 * depth8 + 2 and 15 * depth16 + 2 the upload reserves,
tests/test_hit_cases.py — and a leaf group can sit on top of ENTER entries that went through a long walk). The bars are tests/test_hits_unit.py's 1 and 3: every row the
oracle's as bits, in order and shuffled, and float64's hit on every row above its margin (tests/hit_f64.py)."""
import numpy as np
import pytest

import hit_cases as hc
import hit_f64
from conftest import scene_path
from test_hits_unit import FORMS, _run, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def deep(yh, oracle, ctx):
    sf = yh.SceneFile(scene_path("hits-unit", variant="deep"))
    rays, ref = hc.deep_rays(), hc.oracle_hits("deep", yh, oracle, scene_path)[0]
    yield dict(sf=sf, rays=rays, ref=ref, perm=np.random.default_rng(10).permutation(len(rays)))
    sf.close()


@pytest.mark.parametrize("form", FORMS)
def test_every_row_is_the_oracles_and_float64s(ctx, deep, form, monkeypatch):
    ctx.upload_scene(deep["sf"].desc)
    assert ctx.scene_once() == 0
    n = len(deep["rays"])
    rep = 4 if form == "lanes" else 1  # (65 536 rows: where yh_intersect_batch takes the one-lane kernel)
    where = lambda r: hc.where(r % n, hc.DEEP_NAMES)  # noqa: E731
    got = _run(ctx, form, np.tile(deep["rays"], (rep, 1)), monkeypatch)
    _same([np.concatenate([a] * rep) for a in deep["ref"]], got, where, f"deep, {form}")
    hit_f64.compare("deep", [a[:n] for a in got], f"the device ({form})")
    perm = deep["perm"] if rep == 1 else np.random.default_rng(11).permutation(rep * n)
    shuffled = _run(ctx, form, np.tile(deep["rays"], (rep, 1))[perm], monkeypatch)
    _same([np.concatenate([a] * rep)[perm] for a in deep["ref"]], shuffled, lambda r: where(perm[r]) + " (shuffled)", f"deep, {form}")
