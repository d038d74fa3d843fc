"""The strata of tests/path_cases.py are what they claim, before a GPU sees them: the numpy pcg32 is yo_rng_stream's, the constructed
streams give the draws they were made for, every edge a stratum names is on its rows, the float64 restatement (tests/path_f64.py) makes
the oracle's decisions on every row, and the scene of the predicted render has hits on every emitter class, hits on non-emitters and
misses. No GPU."""
import numpy as np
import pytest

import path_cases as pc
import path_f64 as p64
from conftest import scene_path

F = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


@pytest.fixture(scope="module")
def cameras(yh):
    return pc.scene_cameras(yh, scene_path)


def test_numpy_pcg32_is_the_oracles(oracle):
    for seed, seq in ((961748941, 1), (0, 0), (1301081, 12345), (2 ** 63 + 5, 2 ** 31 - 1), (199382389514, 77)):
        (state, inc), want = oracle.rng_stream(seed, seq, 257)
        got, after = pc.draws(np.array([[state, inc]], np.uint64), 257)
        assert np.array_equal(_bits(got[0]), _bits(want)), (seed, seq)
        # ... and the states: a second call from the state after 100 draws continues the sequence
        mid = pc.draws(np.array([[state, inc]], np.uint64), 100)[1]
        assert np.array_equal(_bits(pc.draws(np.array([[mid[0], inc]], np.uint64), 157)[0][0]), _bits(want[100:]))
    assert (pc.as_float(np.array([0, 0xFFFFFFFF], np.uint32)) == np.array([0, 1 - 2.0 ** -23], F)).all()  # the draws lie on the 2^-23 grid in [0, 1)


def test_a_state_is_made_for_an_output_and_the_step_is_undone():
    gen = np.random.default_rng(5)
    n = 4096
    out32, rot, low = gen.integers(0, 1 << 32, n, dtype=np.uint64), gen.integers(0, 32, n, dtype=np.uint64), gen.integers(0, 1 << 27, n, dtype=np.uint64)
    rot[:32] = np.arange(32)
    state = pc.state_with_output(out32, rot, low)
    assert np.array_equal(pc.output(state), out32.astype(np.uint32)) and np.array_equal(state >> np.uint64(59), rot)
    inc = gen.integers(0, 1 << 63, n, dtype=np.uint64) << np.uint64(1) | np.uint64(1)
    assert np.array_equal(pc.advance(pc.step_back(state, inc), inc), state)
    for k in range(4):
        mant = gen.integers(0, 1 << 23, n)
        d = pc.draws(pc.streams_with_draw(gen, k, mant), 4)[0]
        assert np.array_equal(d[:, k], (mant * 2.0 ** -23).astype(F))


# ---- begin ------------------------------------------------------------------------------------------------------
def test_cameras_are_todays(cameras):
    assert len(cameras) == len(pc.GENERATED) + len(pc.REF_SCENES) and np.isfinite(cameras).all()
    assert (cameras[:, 12] > 0).all() and (cameras[:, 13:15] > 0).all()
    assert (cameras[:, 16] != 0).any() and (cameras[:, 16] == 0).any()  # the DOF scene and sloth's lens among them
    assert (cameras[:, 13] != cameras[:, 14]).any()


def test_begin_strata(cameras, oracle):
    for name in pc.BEGIN_STRATA:
        s = pc.begin_stratum(name, cameras)
        n = pc.ROWS
        assert s.cams.shape == (n, 17) and s.ijwh.shape == (n, 4) and s.rng.shape == (n, 2) and (s.rng[:, 1] & np.uint64(1) == 1).all()
        i, j, w, h = s.ijwh.T
        assert (w >= 1).all() and (h >= 1).all() and (i >= 0).all() and (i < w).all() and (j >= 0).all() and (j < h).all()
        d4, after = pc.draws(s.rng, 4)
        lu, lv, pu, pv = d4.T
        again = pc.begin_stratum(name, cameras)
        assert np.array_equal(_bits(again.cams), _bits(s.cams)) and np.array_equal(again.rng, s.rng) and np.array_equal(again.ijwh, s.ijwh)
        if name == "a":
            assert (s.cams[:, 16] == 0).all() and np.isfinite(s.cams).all()
            assert {(a, b) for a, b in zip(w, h)} == set(pc.IMAGE_SIZES)
            assert np.allclose(s.cams[:, 13] * h, s.cams[:, 14] * w, rtol=1e-6)  # the film has the image's shape
            assert len(np.unique(s.cams[:, :12], axis=0)) >= 8
        if name == "b":
            assert (s.cams[:, 16] == 0).all()
            for ci, cj in ((0, 0), (1, 0), (0, 1), (1, 1)):
                assert ((i == np.where(ci, w - 1, 0)) & (j == np.where(cj, h - 1, 0))).sum() >= n // 4
            assert ((i == 0) | (i == w - 1)).all() and ((j == 0) | (j == h - 1)).all()
            assert (w[s.one_w] == 1).all() and (h[s.one_h] == 1).all() and s.one_w.sum() >= 256 and s.one_h.sum() >= 256
            for k, col in ((pc.PU, pu), (pc.PV, pv)):
                lo, hi = s.edge & (s.which == k) & s.low, s.edge & (s.which == k) & ~s.low
                assert lo.sum() >= 512 and hi.sum() >= 512
                assert (col[lo] < 2.0 ** -10).all() and (col[hi] > 1 - 2.0 ** -10).all() and (col[hi] < 1).all()
                assert (col[lo] == 0).any() and (col[hi] == F(1 - 2.0 ** -23)).any()
            assert (s.cams[:, 13] != s.cams[:, 14]).mean() > 0.5
            fr = s.cams[:, :12].astype(np.float64).reshape(n, 4, 3)
            det = np.linalg.det(fr[:, :3])
            assert (det < 0).sum() >= n // 8 and (np.abs(np.abs(det) - 1) > 0.1).sum() >= n // 8  # mirrored; not of unit scale
            assert (np.abs(fr[:, :3] - np.eye(3)).max(axis=(1, 2)) > 0.1).sum() >= n // 2        # rotated
        if name == "c":
            ap, fo = s.cams[:, 16], s.cams[:, 15]
            assert (ap > 0).all() and ap[~s.tiny].min() >= 1e-6 and ap.max() <= 10 and fo.min() >= 1e-3 and fo.max() <= 1e4
            assert ap[~s.tiny].min() < 1e-5 and ap.max() > 5 and fo.min() < 1e-2 and fo.max() > 1e3
            assert (lv[s.kind == 0] < 2.0 ** -20).all() and (lv[s.kind == 0] == 0).any()
            for q in range(5):
                x = lu[s.kind == 1 + q].astype(np.float64)
                assert (np.abs(x - q / 4) <= 2.0 ** -10).all() and len(x) >= 512
                assert (x == min(q / 4, 1 - 2.0 ** -23)).any()  # the point itself (1: the largest draw)
            # an aperture so small that p - e rounds to p: the direction is the pinhole's, bit for bit, while the origin moves
            tiny = np.flatnonzero(s.tiny)
            assert (s.cams[tiny, 16] == F(1e-30)).all()
            pin = s.cams[tiny].copy()
            pin[:, 16] = 0
            a = oracle.path_ends("begin", s.cams[tiny], s.ijwh[tiny], s.rng[tiny])[0]
            b = oracle.path_ends("begin", pin, s.ijwh[tiny], s.rng[tiny])[0]
            assert np.array_equal(_bits(a[:, 3:6]), _bits(b[:, 3:6]))
        if name == "d":
            assert (s.cams[s.kind == 0, 12] == 0).all() and (s.cams[s.kind == 1, 15] == 0).all() and (s.cams[s.kind == 2, 16] < 0).all()
            assert (s.cams[s.kind == 3, 13:15] == 0).all() and (s.cams[s.kind == 4, 13] == 0).all() and (s.cams[s.kind == 5, 12:15] == 0).all()
            assert all((s.kind == k).sum() >= 1024 for k in range(6))
            out = oracle.path_ends("begin", s.cams, s.ijwh, s.rng)[0][:, :6]
            assert (~np.isfinite(out)).any(axis=1).sum() >= 1024 and np.isfinite(out).all(axis=1).sum() >= 1024  # both kinds of result
        # the oracle's four draws are these four, on every row
        assert np.array_equal(oracle.path_ends("begin", s.cams, s.ijwh, s.rng)[2], after), name


def test_begin_f64_is_the_oracles_camera(cameras, oracle):
    """Strata a-c: direction and origin (over its length) agree to a median below 3e-7 and a 99th percentile below 1e-5 (a dozen float
    roundings), and on every row within 1e-3: stratum c's frames stretch one axis up to 1e4 times another, which multiplies a rounding of
    the direction before the last normalisation by as much."""
    for name in "abc":
        s = pc.begin_stratum(name, cameras)
        out = oracle.path_ends("begin", s.cams, s.ijwh, s.rng)[0]
        o64, d64 = p64.begin64(s.cams, s.ijwh, pc.draws(s.rng, 4)[0])
        assert np.isfinite(out[:, :6]).all() and np.isfinite(o64).all() and np.isfinite(d64).all(), name
        ed = np.abs(out[:, 3:6] - d64).max(axis=1)
        eo = np.abs(out[:, 0:3] - o64).max(axis=1) / np.maximum(np.linalg.norm(o64, axis=1), 1e-30)
        for e in (ed, eo):
            assert np.median(e) < 3e-7 and np.percentile(e, 99) < 1e-5 and e.max() < 1e-3, (name, np.median(e), np.percentile(e, 99), e.max())
        assert np.array_equal(out[:, 6:9], np.zeros((pc.ROWS, 3), F)) and np.array_equal(out[:, 9:12], np.ones((pc.ROWS, 3), F))


# ---- continue ---------------------------------------------------------------------------------------------------
def test_continue_strata(oracle):
    seen = {}
    for name in pc.CONTINUE_STRATA:
        s = pc.continue_stratum(name)
        n = pc.ROWS
        assert s.weight.shape == (n, 3) and s.bb.shape == (n, 2) and s.rng.shape == (n, 2)
        bounce, bounces = s.bb.T
        draw = pc.draws(s.rng, 1)[0][:, 0]
        with np.errstate(invalid="ignore"):
            top = np.fmax(np.fmax(s.weight[:, 0], s.weight[:, 1]), s.weight[:, 2])
        if name == "a":
            for b in (2, 3, 4, 5):
                assert (bounce == b).sum() >= n // 8
            for rel in range(3):
                assert (bounce[s.rel == rel] + 1 == bounces[s.rel == rel] - 1 + rel).all() and (s.rel == rel).sum() >= n // 8
            assert (bounces[s.rel == 3] == 1).all()
            for b in (3, 4):  # both sides of the roulette's start on both sides of the limit
                for rel in range(4):
                    assert ((bounce == b) & (s.rel == rel)).sum() >= 64
        if name == "b":
            z = s.weight[s.kind <= 2]
            assert (z == 0).all()
            sign = np.signbit(z)
            assert (~sign).all(axis=1).any() and sign.all(axis=1).any() and (sign.any(axis=1) & ~sign.all(axis=1)).any()
            for k, test in ((3, np.isnan), (4, lambda x: x == np.inf), (5, lambda x: x == -np.inf)):
                m = test(s.weight[s.kind == k])
                assert (m.sum(axis=1) == 1).all() and m.any(axis=0).all()  # one component, in each position
            assert (s.weight[s.kind == 6] < 0).all() and (top[s.kind == 7] > 0).all() and (s.weight[s.kind == 7, 0] < 0).all()
            den = top[s.kind == 8]
            assert (den > 0).all() and (den < np.finfo(F).tiny).all()
            with np.errstate(over="ignore", divide="ignore"):
                assert np.isinf(F(1) / den).all()  # 1 / rr_prob overflows
            assert (np.argmax(s.weight[s.kind == 8], axis=1)[:, None] == np.arange(3)).any(axis=0).all()
            assert (bounce[s.kind == 8] > 3).any() and (bounce <= 3).any()
        if name == "c":
            for k, v in ((0, pc.down(pc.P99)), (1, pc.P99), (2, pc.up(pc.P99))):
                assert (top[s.kind == k] == v).all()
            assert pc.down(pc.P99) < pc.P99 < pc.up(pc.P99) and (top[s.kind == 3] > 1.4).all() and (bounce > 3).all()
            for k in range(4):
                assert (np.argmax(s.weight[s.kind == k], axis=1)[:, None] == np.arange(3)).any(axis=0).all()
        if name == "d":
            assert np.array_equal(_bits(s.draw), _bits(draw)) and (draw < pc.P99).all() and (draw > 0).all()
            assert np.array_equal(_bits(top), _bits(s.top))
            assert (top[s.kind == 1] == draw[s.kind == 1]).all()  # this row's draw equals rr_prob exactly
            assert (top[s.kind == 0] == pc.down(draw[s.kind == 0])).all() and (top[s.kind == 2] == pc.up(draw[s.kind == 2])).all()
            for k in range(3):
                assert (np.argmax(s.weight[s.kind == k], axis=1)[:, None] == np.arange(3)).any(axis=0).all()
                assert ((s.kind == k) & (bounce > 3)).sum() >= 2048
            assert (bounce <= 3).sum() >= 512
        # float64 makes the oracle's decisions on every row
        fout, iout, state = oracle.path_ends("continue", s.weight, s.bb, s.rng)
        r = p64.continue64(s.weight, s.bb, draw)
        assert np.array_equal(iout[:, 0], r.flag.astype(np.int32)) and np.array_equal(iout[:, 1], r.bounce.astype(np.int32)), name
        assert np.array_equal(state, np.where(r.roulette, pc.advance(s.rng[:, 0], s.rng[:, 1]), s.rng[:, 0])), name  # one draw, exactly when roulette is played
        same = ~(r.roulette & ~r.killed)
        assert np.array_equal(_bits(fout[same]), _bits(s.weight[same])), name  # the weight changes only where the path survives roulette
        scaled = ~same & np.isfinite(fout).all(axis=1)
        assert np.allclose(fout[scaled], r.weight[scaled], rtol=3e-7, atol=0), name
        seen[name] = r
        if name == "b":
            assert r.dead[s.kind <= 5].all() and not r.dead[s.kind >= 6].any()
            assert r.killed[(s.kind == 6) & r.roulette].all()  # a negative rr_prob: every draw is at least that
            den = (s.kind == 8) & r.roulette
            assert r.killed[den & (draw > 0)].all() and den.sum() >= 128
        if name == "c":
            assert (r.killed[s.kind == 3] == (draw[s.kind == 3] >= pc.P99)).all() and r.killed.any() and (~r.killed).any()
        if name == "d":
            played = r.roulette
            assert r.killed[played & (s.kind <= 1)].all() and not r.killed[played & (s.kind == 2)].any()  # >=: the draw on rr_prob ends the path
    assert all(seen[k].flag.any() and (~seen[k].flag).any() for k in "acd")


# ---- end --------------------------------------------------------------------------------------------------------
def test_end_strata(oracle):
    for name in pc.END_STRATA:
        s = pc.end_stratum(name)
        n = pc.ROWS
        assert s.rad.shape == (n, 8) and s.hit.shape == (n, 1) and set(s.hit.ravel()) == {0, 1}
        rgb, clamp, acc = s.rad[:, :3], s.rad[:, 3], s.rad[:, 4:8]
        with np.errstate(invalid="ignore"):
            top = np.fmax(np.fmax(rgb[:, 0], rgb[:, 1]), rgb[:, 2])
        r = p64.end64(s.rad, s.hit)
        if name == "a":
            assert (clamp == 100).all() and np.isfinite(rgb).all() and not r.clamped.any() and not r.sanitized.any()
        if name == "b":
            for k, test in ((0, np.isnan), (1, lambda x: x == np.inf), (2, lambda x: x == -np.inf)):
                m = test(rgb[s.kind == k])
                assert (m.sum(axis=1) == 1).all() and m.any(axis=0).all()
            assert r.sanitized[np.isin(s.kind, (0, 1, 2, 6))].all() and not r.sanitized[~np.isin(s.kind, (0, 1, 2, 6))].any()
            assert (rgb[s.kind == 3] == 0).all() and (rgb[s.kind == 4] < 0).all() and (rgb[s.kind == 5, 1] < 0).all() and np.signbit(rgb[s.kind == 7]).all()
            assert not r.clamped[np.isin(s.kind, (3, 4, 7))].any() and r.clamped[s.kind == 5].any()
        if name == "c":
            assert set(clamp) == set(pc.CLAMPS)
            fin = np.isfinite(clamp)
            assert (top[s.kind == 1] == clamp[s.kind == 1]).all()
            assert (top[(s.kind == 0) & fin] == pc.down(clamp[(s.kind == 0) & fin])).all() and (top[(s.kind == 2) & fin] == pc.up(clamp[(s.kind == 2) & fin])).all()
            for c in pc.CLAMPS[:3]:  # finite clamps with finite neighbours: scaled exactly above the clamp, in each position
                for k in range(3):
                    sel = (clamp == c) & (s.kind == k)
                    assert (r.clamped[sel] == (k == 2)).all() and (np.argmax(rgb[sel], axis=1)[:, None] == np.arange(3)).any(axis=0).all() and sel.sum() >= 128
            assert not r.clamped[clamp == np.inf].any() and r.sanitized[(clamp == np.inf) & (s.kind >= 1)].all()
            assert r.sanitized[(clamp == pc.FLT_MAX) & (s.kind == 2)].all() and not r.sanitized[(clamp == pc.FLT_MAX) & (s.kind <= 1)].any()
        if name == "d":
            assert (top[s.kind == 0] == F(3e38)).all() and (clamp[s.kind == 0] == 1).all() and r.clamped[s.kind == 0].all()
            den = s.kind == 1
            assert (top[den] < np.finfo(F).tiny).all() and (clamp[den] < top[den]).all() and r.clamped[den].all() and (clamp[den] == 0).any()
            assert (acc[s.kind == 2] == 0).all() and (acc[s.kind == 3, :3] == F(1e7)).all() and (F(1e7) + F(0.3) != np.float64(1e7) + np.float64(F(0.3)))
            assert (acc[s.kind == 4, 3] == 0).all() and (acc[s.kind == 5, 3] == 16777215).all()
            assert (np.argmax(rgb[s.kind == 0], axis=1)[:, None] == np.arange(3)).any(axis=0).all()
        # float64 makes the oracle's decisions: unchanged, zeroed and scaled rows are told apart by what is added
        out = oracle.path_ends("end", s.rad, s.hit)[0]
        added = out[:, :3].astype(np.float64) - acc[:, :3]
        assert np.array_equal(out[:, 3], acc[:, 3] + s.hit[:, 0].astype(F)), name
        with np.errstate(invalid="ignore"):
            assert np.array_equal(_bits(out[r.sanitized, :3]), _bits(acc[r.sanitized, :3])), name  # + 0
        plain = ~r.sanitized & ~r.clamped
        assert np.array_equal(_bits(out[plain, :3]), _bits((acc[plain, :3] + rgb[plain]).astype(F))), name
        ok = np.isfinite(r.acc).all(axis=1) & np.isfinite(out).all(axis=1)
        scale = np.maximum(np.abs(r.acc[:, :3]), np.abs(acc[:, :3].astype(np.float64)))
        assert (np.abs(out[ok, :3] - r.acc[ok, :3]) <= 4e-7 * scale[ok] + 1e-44).all(), name
        if name in "cd":
            cl = r.clamped & ok
            # a scaled row's largest component lands on the clamp (to a rounding): a per-channel clamp would not scale the others
            pos = np.argmax(np.where(np.isfinite(rgb), rgb, -np.inf), axis=1)
            lead = added[np.arange(n), pos]
            sel = cl & (acc[:, :3] == 0).all(axis=1)
            assert sel.sum() >= 64 and np.allclose(lead[sel], clamp[sel], rtol=3e-7, atol=1e-44), name


# ---- the scene of the predicted render ---------------------------------------------------------------------------
@pytest.mark.parametrize("film,w,h", [((0.036, 0.036), 64, 64), ((0.036 * 37 / 41, 0.036), 37, 41)])
def test_render_scene_has_every_kind_of_first_hit(yh, oracle, film, w, h):
    sc = pc.RenderScene(film)
    em = sc.emissions
    assert em.shape == (15, 3) and len({tuple(e) for e in em}) == 15
    top = em.max(axis=1)
    for k, cls in enumerate(pc.CLASSES):
        t = top[3 * k:3 * k + 3]
        assert {"below": (t < pc.CLAMP).all(), "on": (t == pc.CLAMP).all(), "above": (t == pc.up(pc.CLAMP)).all(), "twice": (t == 2 * pc.CLAMP).all(),
                "huge": (t == F(1e30) * pc.CLAMP).all()}[cls]
        assert sorted(np.argmax(em[3 * k:3 * k + 3], axis=1)) == [0, 1, 2]  # in different channels
    osc = oracle.scene(sc.desc(yh))
    obj = osc.intersect(sc.centre_rays(w, h))[0]
    osc.close()
    for e in range(15):
        assert (obj == e).sum() >= 8, f"emitter {e} is hit by {(obj == e).sum()} centre rays"
    assert (obj == 15).sum() >= 32 and (obj == 16).sum() >= 32 and (obj < 0).sum() >= 32  # the mesh, the strands, the environment
    assert osc is not None and yh.TraceParams.default(resolution=max(w, h), bounces=1, clamp=float(pc.CLAMP)).bounces == 1
    # what path_end makes of every class, in float32: below and on the clamp unchanged, above it scaled by clamp / hmax
    acc = np.zeros((15, 4), F)
    pc.path_end_f32(em, np.ones(15, bool), pc.CLAMP, acc)
    assert np.array_equal(acc[:6, :3], em[:6]) and (acc[6:, :3].max(axis=1) <= pc.CLAMP).all() and (acc[9:, :3].max(axis=1) == pc.CLAMP).all()
    assert not np.array_equal(acc[6:9, :3], np.minimum(em[6:9], pc.CLAMP))  # ... which a per-channel clamp would not give
    want = oracle.path_ends("end", np.concatenate([em, np.full((15, 1), pc.CLAMP), np.zeros((15, 4), F)], axis=1), np.ones((15, 1), np.int32))[0]
    assert np.array_equal(_bits(want), _bits(acc))
