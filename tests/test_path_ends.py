"""The code that starts and ends a path on the device (csrc/dev_path.h: path_begin with sample_camera / sample_camera_lane, path_continue,
path_end), row by row through yh_path_ends_batch (unit/path_ends.h: a quad per row and a lane per row) against the oracle's
yo_path_ends_batch, which runs the functions the oracle's renders run; and tied to the sample loops by the feature pass and by a render
whose every pixel can be predicted. Strata: tests/path_cases.py, proved on the CPU by tests/test_path_cases.py.

Bars (none taken from what the device gives):
  1  forms: the quad and the lane form agree on every row of every stratum and operation as BITS, NaNs and the degenerate rows included
     (begin: the ray and the stream's state; the lane form runs no path_begin, so it returns no radiance, weight, bounce or flags);
  2  continue, end: every output is the oracle's on every row — the flag, the bounce count, the stream's state and acc as bits; the weight
     as bits wherever it is no NaN, and a NaN where the oracle's is one (a NaN arises only as 0 x inf from a denormal rr_prob, and its sign
     and payload are the platform's);
  3  begin: the stream's state after the four draws is the oracle's on every row of every stratum; form 0 leaves radiance 0, weight 1,
     bounce 0 and both flags clear. Aperture 0 (strata a, b): the direction is the oracle's as bits, the origin as values (the sign of a
     zero component depends on a lens draw the device rightly skips). Aperture != 0 (stratum c: the device's sinf / cosf are not
     libm's): median and 99th percentile over the stratum of the direction's error (absolute, the largest component) and of the origin's
     (the same over the float64 origin's length) against tests/path_f64.py at most 2 x the oracle's own on the same rows. Stratum a:
     every direction component within 1e-6 of float64 (tests/test_gbuffer.py's bar for the camera). Stratum d: the non-finite mask is
     the oracle's;
  4  the feature pass: fed with the context's camera, every pixel's (i, j) and the streams of yh_download_rng, begin returns the `ray`
     plane of yh_trace_gbuffer in next-sample mode bit for bit, in both forms, on the DOF scene at 64 x 64 and on a 100 x 75 image;
  5  the predicted render (path_cases.RenderScene: fifteen emitters of five classes about the clamp of 1, a diffuse mesh and strands
     in front, a constant environment, a lens; bounces = 1, so a sample's radiance is its first hit's emission): for four samples in
     turn, the ids of the feature pass in next-sample mode, path_end in float32 numpy, one sample rendered — the download equals the
     numpy accumulator over the sample count bit for bit on every pixel, alpha included, under every forced launch shape (k_stream
     among them) at 64 x 64 and at 37 x 41;
  6  n in {1, 3, 4097}: a row does not depend on the batch; the refusals.
What one-token errors in csrc/dev_path.h do to these bars: profiles/path_ends/mutations.txt (ten were tried; each of the nine that change
a bit fails a test here, `>` for `>=` against rr_prob on the 2 389 rows of stratum d whose weight is their own draw and nowhere else).

MEASURED (2026-10-21, AMD Instinct MI355X, gfx950; profiles/path_ends/errors.txt): no assertion fails. Bar 3 on stratum c, device against
the oracle on the same rows: direction median 3.613e-08 against 3.614e-08, p99 1.982e-07 against 1.982e-07; origin median 2.001e-08 against
1.998e-08, p99 2.207e-07 against 2.206e-07 (ratios of 1.00: the bar of 2 x has room). Stratum a: the largest direction error 1.23e-07 against
the bar of 1e-6. Bar 1 holds as bits. The module's GPU tests: 59 passed in 23 s, 22 s of which the first context and the scenes."""
import ctypes as C

import numpy as np
import pytest

import path_cases as pc
import path_f64 as p64
from conftest import scene_path

pytestmark = pytest.mark.gpu
F = np.float32
FORMS = [("quad", 0), ("lane", 1)]
K_BAR = 2.0
TODAY_DIR = 1e-6
SHAPES = ("0", "1", "3", "4", "5", "6", "7", "8")  # as tests/test_gpu_parity.py forces them: 3 is k_stream


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _rows_differing(a, b):
    return np.flatnonzero((_bits(a) != _bits(b)).reshape(len(a), -1).any(axis=1))


def _same_bits(a, b, what):
    bad = _rows_differing(a, b)
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first row {bad[0]}: {a[bad[0]]} against {b[bad[0]]}"


def _same_but_nan_sign(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: {np.count_nonzero(np.isnan(got) != nan)} entries are NaN on one side only"
    _same_bits(np.where(nan, F(0), got), np.where(nan, F(0), want), what)


@pytest.fixture(scope="module")
def cases(yh, oracle):
    """Per operation and stratum: the inputs, the oracle's rows (computed once) and the device's rows per form as they are first asked for."""
    cams = pc.scene_cameras(yh, scene_path)
    out = {}
    for name in pc.BEGIN_STRATA:
        s = pc.begin_stratum(name, cams)
        out["begin", name] = dict(s=s, args=(s.cams, s.ijwh, s.rng))
    for name in pc.CONTINUE_STRATA:
        s = pc.continue_stratum(name)
        out["continue", name] = dict(s=s, args=(s.weight, s.bb, s.rng))
    for name in pc.END_STRATA:
        s = pc.end_stratum(name)
        out["end", name] = dict(s=s, args=(s.rad, s.hit))
    for (op, _), c in out.items():
        c["ref"], c["dev"] = oracle.path_ends(op, *c["args"]), {}
    return out


def _device(ctx, c, op, form):
    if form not in c["dev"]:
        c["dev"][form] = ctx.path_ends(op, form, *c["args"])
    return c["dev"][form]


ALL = [("begin", n) for n in pc.BEGIN_STRATA] + [("continue", n) for n in pc.CONTINUE_STRATA] + [("end", n) for n in pc.END_STRATA]


# ---- 1. forms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,name", ALL, ids=[f"{o}-{n}" for o, n in ALL])
def test_quad_and_lane_forms_agree_as_bits(ctx, cases, op, name):
    c = cases[op, name]
    q, l = _device(ctx, c, op, 0), _device(ctx, c, op, 1)
    if op == "begin":
        _same_bits(q[0][:, :6], l[0][:, :6], f"begin {name}: the ray")
        assert np.array_equal(q[2], l[2]), f"begin {name}: the stream's state"
        assert not l[0][:, 6:].any() and not l[1].any()  # the lane form runs no path_begin
        return
    _same_bits(q[0], l[0], f"{op} {name}: floats")
    if op == "continue":
        assert np.array_equal(q[1], l[1]) and np.array_equal(q[2], l[2]), f"continue {name}: flag, bounce or state"


# ---- 2. continue, end ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [f[0] for f in FORMS])
@pytest.mark.parametrize("name", pc.CONTINUE_STRATA)
def test_continue_is_the_oracles(ctx, cases, name, form):
    c = cases["continue", name]
    fout, iout, state = _device(ctx, c, "continue", dict(FORMS)[form])
    rf, ri, rs = c["ref"]
    for what, got, want in (("the flag", iout[:, 0], ri[:, 0]), ("bounce", iout[:, 1], ri[:, 1]), ("the stream's state", state, rs)):
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"continue {name} {form}: {what} differs on {bad.size} rows, first row {bad[0]}: weight {c['s'].weight[bad[0]]} bounce, bounces {c['s'].bb[bad[0]]}"
    _same_but_nan_sign(fout, rf, f"continue {name} {form}: the weight")
    assert name == "b" or not np.isnan(rf).any()


@pytest.mark.parametrize("form", [f[0] for f in FORMS])
@pytest.mark.parametrize("name", pc.END_STRATA)
def test_end_is_the_oracles(ctx, cases, name, form):
    c = cases["end", name]
    acc = _device(ctx, c, "end", dict(FORMS)[form])[0]
    assert not np.isnan(c["ref"][0]).any()
    bad = _rows_differing(acc, c["ref"][0])
    assert bad.size == 0, f"end {name} {form}: acc differs on {bad.size} rows, first row {bad[0]}: in {c['s'].rad[bad[0]]} device {acc[bad[0]]} oracle {c['ref'][0][bad[0]]}"


# ---- 3. begin ------------------------------------------------------------------------------------------------------
def _begin_errors(c, rows6):
    """Per row: the direction's error (absolute, the largest component) and the origin's (the same over the float64 origin's length)."""
    s = c["s"]
    if "f64" not in c:
        c["f64"] = p64.begin64(s.cams, s.ijwh, pc.draws(s.rng, 4)[0])
    o64, d64 = c["f64"]
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.abs(rows6[:, 3:6].astype(np.float64) - d64).max(axis=1),
                np.abs(rows6[:, 0:3].astype(np.float64) - o64).max(axis=1) / np.maximum(np.linalg.norm(o64, axis=1), 1e-30))


def _stat(e):
    return float(np.median(e)), float(np.percentile(e, 99))


@pytest.mark.parametrize("form", [f[0] for f in FORMS])
@pytest.mark.parametrize("name", pc.BEGIN_STRATA)
def test_begin_draws_and_ray(ctx, cases, name, form):
    c = cases["begin", name]
    s = c["s"]
    fout, iout, state = _device(ctx, c, "begin", dict(FORMS)[form])
    rf, ri, rs = c["ref"]
    bad = np.flatnonzero(state != rs)
    assert bad.size == 0, f"begin {name} {form}: the stream's state after the call differs on {bad.size} rows"
    assert np.array_equal(rs, pc.draws(s.rng, 4)[1])  # four draws
    if form == "quad":  # as path_begin leaves them
        assert np.array_equal(_bits(fout[:, 6:]), _bits(rf[:, 6:])) and np.array_equal(iout, ri) and not iout.any()
    if name in "ab":  # aperture 0
        bad = _rows_differing(fout[:, 3:6], rf[:, 3:6])
        assert bad.size == 0, f"begin {name} {form}: the direction differs on {bad.size} rows, first row {bad[0]}: {fout[bad[0], 3:6]} against {rf[bad[0], 3:6]}"
        assert np.array_equal(fout[:, :3], rf[:, :3]), f"begin {name} {form}: the origin"
        assert np.array_equal(_bits(fout[:, :3]), _bits(s.cams[:, 9:12]))  # the frame's origin itself: e = +0
    if name == "d":
        assert np.array_equal(np.isfinite(fout[:, :6]), np.isfinite(rf[:, :6])), f"begin d {form}: the non-finite mask"
        assert np.array_equal(np.isnan(fout[:, :6]), np.isnan(rf[:, :6]))
        print(f"begin d {form}: rows with a non-finite component in the oracle {np.count_nonzero(~np.isfinite(rf[:, :6]).all(axis=1))}, mask differs on 0")
        return
    dev, ref = _begin_errors(c, fout), _begin_errors(c, rf)
    assert np.isfinite(fout[:, :6]).all()
    for what, e_dev, e_ref in (("direction", dev[0], ref[0]), ("origin", dev[1], ref[1])):
        (md, pd), (mr, pr) = _stat(e_dev), _stat(e_ref)
        print(f"errors begin {name} {form:4s} {what:9s} median device {md:.3e} oracle {mr:.3e}   p99 device {pd:.3e} oracle {pr:.3e}   max device {e_dev.max():.3e} oracle {e_ref.max():.3e}")
    if name == "a":
        err = np.abs(fout[:, 3:6].astype(np.float64) - c["f64"][1])
        assert err.max() <= TODAY_DIR, f"begin a {form}: a direction component {err.max():.3g} from float64"
    if name == "c":
        for what, e_dev, e_ref in (("direction", dev[0], ref[0]), ("origin", dev[1], ref[1])):
            (md, pd), (mr, pr) = _stat(e_dev), _stat(e_ref)
            assert md <= K_BAR * mr and pd <= K_BAR * pr, f"begin c {form}: {what}: median {md:.3e} against the oracle's {mr:.3e}, p99 {pd:.3e} against {pr:.3e}"


# ---- 4. tied to the loops: the feature pass --------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dof-64", "lens-100x75"])
def test_begin_is_the_feature_passes_next_sample_ray(ctx, yh, case):
    from test_gbuffer import _with_camera
    sf = yh.SceneFile(scene_path("sphere-hairblock", scale=0.05, dof=True))
    if case == "dof-64":
        desc, res, size = sf.desc, 64, None
    else:
        edited = _with_camera(yh, sf, film=(0.036, 0.027), aperture=0.25, focus=3.0)
        desc, res, size = edited.ptr, 100, (100, 75)
    ctx.upload_scene(desc, sf.maps)
    ctx.set_shard(0, 1)
    w, h = ctx.init_state(yh.TraceParams.default(resolution=res))
    assert size is None or (w, h) == size
    cam = desc.contents.camera
    assert cam.aperture != 0
    ctx.trace_samples(1)  # (streams that have drawn before, as in any later sample)
    rng = ctx.download_rng()
    g = ctx.trace_gbuffer("next", planes=["ray"])
    assert np.array_equal(ctx.download_rng(), rng)
    j, i = np.divmod(np.arange(w * h), w)
    ijwh = np.stack([i, j, np.full(w * h, w), np.full(w * h, h)], axis=1)
    cams = np.tile(pc.camera_row(cam), (w * h, 1))
    for form, k in FORMS:
        fout, _, state = ctx.path_ends("begin", k, cams, ijwh, rng)
        _same_bits(fout[:, :6], g["ray"].reshape(-1, 6), f"{case} {form}: begin against the feature pass's ray plane")
        assert np.array_equal(state, pc.draws(rng, 4)[1])
    assert not np.array_equal(g["ray"][..., :3], np.broadcast_to(np.array(cam.frame[9:12], F), (h, w, 3)))  # the lens moves the origin
    sf.close()


# ---- 5. tied to the loops: a render that can be predicted ---------------------------------------------------------------
SIZES = {"64x64": ((0.036, 0.036), 64, (64, 64)), "37x41": ((0.036 * 37 / 41, 0.036), 41, (37, 41))}
_RENDER = {}


def _render_scene(ctx, yh, size):
    """The scene of `size` in the context: uploaded unless the test before left that very scene there."""
    film, res, wh = SIZES[size]
    if size not in _RENDER:
        _RENDER[size] = pc.RenderScene(film)
    sc = _RENDER[size]
    ctx.upload_scene(sc.desc(yh))
    ctx.set_shard(0, 1)
    return sc, res, wh


@pytest.mark.parametrize("shape", SHAPES + ("auto",))
@pytest.mark.parametrize("size", list(SIZES))
def test_every_pixel_of_a_one_bounce_render_is_predicted(ctx, yh, size, shape, monkeypatch):
    sc, res, wh = _render_scene(ctx, yh, size)
    if shape != "auto":
        monkeypatch.setenv("YHAIR_SHAPE", shape)
    p = yh.TraceParams.default(resolution=res, bounces=1, clamp=float(pc.CLAMP))
    assert ctx.init_state(p) == wh
    acc = np.zeros((wh[1], wh[0], 4), F)
    seen = set()
    for sample in range(1, 5):
        ids = ctx.trace_gbuffer("next", planes=["object"])["object"]
        pc.path_end_f32(sc.radiance_of(ids), ids >= 0, pc.CLAMP, acc)
        ctx.trace_samples(1)
        if shape != "auto":
            assert ctx.launch_shape() == int(shape)
        img = ctx.download()
        want = pc.resolve_f32(acc, sample)
        bad = np.argwhere((_bits(img) != _bits(want)).any(axis=2))
        assert bad.size == 0, (f"{size}, shape {shape}, sample {sample}: {len(bad)} pixels differ, first (j, i) = {tuple(bad[0])}: first hit {ids[tuple(bad[0])]}, "
                               f"rendered {img[tuple(bad[0])]}, predicted {want[tuple(bad[0])]}")
        seen |= set(np.unique(ids))
    assert seen == set(range(-1, 17))  # every emitter, the mesh, the strands and the environment were somebody's first hit
    assert acc[..., :3].max() == 4 * pc.CLAMP and (acc[..., 3] == 0).any() and (acc[..., 3] == 4).any()


# ---- 6. the batch's shape, the refusals -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [f[0] for f in FORMS])
def test_batch_shape_does_not_change_a_row(ctx, cases, form):
    k = dict(FORMS)[form]
    for op, name in (("begin", "c"), ("continue", "d"), ("end", "c")):
        c = cases[op, name]
        full = _device(ctx, c, op, k)
        rows = np.random.default_rng(3).permutation(pc.ROWS)[:4097]
        for n in (1, 3, 4097):
            got = ctx.path_ends(op, k, *[a[rows[:n]] for a in c["args"]])
            for a, b in zip(got, full):
                if a is not None:
                    assert np.array_equal(_bits(a), _bits(b[rows[:n]])), (op, n)


def test_empty_and_invalid_batches(ctx, yh, cases):
    u64p = C.POINTER(C.c_uint64)
    call = ctx.lib.yh_path_ends_batch
    n = 8
    for op, name in (("begin", "a"), ("continue", "a"), ("end", "a")):
        k = yh.PATH_OPS[op]
        nfi, nii, nfo, nio = yh.PATH_ROWS[k]
        args = [np.ascontiguousarray(a[:n]) for a in cases[op, name]["args"]]
        fout, iout, state = np.full((n, nfo), 7, F), np.full((n, max(nio, 1)), 7, np.int32), np.full(n, 7, np.uint64)
        draws = op != "end"
        ptrs = [yh.fptr(args[0]), yh.iptr(args[1]), args[2].ctypes.data_as(u64p) if draws else None, yh.fptr(fout), yh.iptr(iout) if draws else None,
                state.ctypes.data_as(u64p) if draws else None]
        for form in (0, 1):
            fout[:], state[:] = 7, 7
            assert call(ctx.h, k, form, n, *ptrs) == yh.YH_OK
            assert not (state == 7).any() or not draws
            assert _rows_differing(fout, np.full_like(fout, 7)).size == n
        for form in (2, -1):
            assert call(ctx.h, k, form, n, *ptrs) == yh.YH_E_INVALID
        for bad_n in (0, -1):
            assert call(ctx.h, k, 0, bad_n, *ptrs) == yh.YH_E_INVALID
        assert call(None, k, 0, n, *ptrs) == yh.YH_E_INVALID
        for i, ptr in enumerate(ptrs):
            if ptr is not None:
                assert call(ctx.h, k, 0, n, *[None if j == i else q for j, q in enumerate(ptrs)]) == yh.YH_E_INVALID, (op, i)
    for bad_op in (-1, 3, 17):
        assert call(ctx.h, bad_op, 0, n, *ptrs) == yh.YH_E_INVALID
    # ... and each refusal leaves a usable context
    c = cases["end", "a"]
    _same_bits(ctx.path_ends("end", 0, *[a[:n] for a in c["args"]])[0], c["ref"][0][:n], "after the refusals")
