"""The input strata of the unit-level tests of the code that starts and ends a path (tests/test_path_ends.py: yh_path_ends_batch against
yo_path_ends_batch), and the scene of the render whose every pixel can be predicted. numpy only, fixed seeds, ROWS rows per stratum;
tests/test_path_cases.py proves on the CPU that every stratum is what it claims.

pcg32 (math.h:1396-1442) stands here once, vectorised: `advance`, `rand1f`, `draws`; tests/test_path_cases.py holds it to yo_rng_stream.
A stream whose k-th draw is a given value is CONSTRUCTED, not searched for: the generator's output is a function of the state before
the step — rotr(((s >> 18) ^ s) >> 27, s >> 59) — and that function is inverted in closed form (`state_with_output`), then the
multiplicative step is undone k times (`step_back`). The draws are (m >> 9) * 2^-23 for the 32-bit output m, so a draw is named by its
23-bit mantissa.

begin (cams (n, 17) = frame[12], lens, film x, film y, focus, aperture; ijwh (n, 4); rng (n, 2); draws in order lu, lv, pu, pv):
  a  today's domain: the cameras of the generated scenes and of tests/golden/ref_scenes, images 720 x 720, 100 x 75 and 37 x 64 with the
     film's height made to fit, random pixels and streams, aperture 0
  b  pixel edges, aperture 0: i, j in the four corners; w = 1, h = 1; pu or pv below 2^-10 or above 1 - 2^-10; non-square films; frames
     that are rotated, mirrored and not of unit scale
  c  the lens: aperture 1e-6 ... 10, focus 1e-3 ... 1e4; lv below 2^-20 (r ~ 0); lu within 2^-10 of 0, 1/4, 1/2, 3/4 and 1 (the zeros of
     sinf / cosf and the largest argument); an aperture of 1e-30 (p - e rounds to p)
  d  degenerate: lens = 0 (dc.z = 0), focus = 0, a negative aperture, film = 0: non-finite or arbitrary results, the oracle's behaviour counts
continue (weight (n, 3), bb (n, 2) = bounce, bounces; rng (n, 2)):
  a  the counts: bounce on 2, 3, 4, 5 (roulette begins at bounce > 3) and elsewhere in 0 ... 9; bounce + 1 on bounces - 1, bounces,
     bounces + 1; bounces = 1; weights in (0, 2)
  b  the weight check: all +0, all -0, mixed signed zeros; one component NaN, +inf, -inf in each position; negative weights; a denormal hmax
     (1 / rr_prob overflows)
  c  hmax(weight) on 0.99f and its float neighbour on either side, and well above 1; the largest component in each position
  d  hmax(weight) EQUAL to the row's own next draw, and its float neighbour on either side (the >= of the roulette); the largest in each position
end (rad (n, 8) = radiance[3], clamp, acc[4]; hit (n, 1)):
  a  today's domain: radiance in (0, 3), clamp 100 (the default), acc a few samples' sums, hit both ways
  b  sanitize: one component NaN, +inf, -inf in each position; all zero; negative components
  c  hmax(radiance) on clamp and its float neighbour on either side, the largest in each position; clamp 0.25, 1, 100, FLT_MAX, +inf
  d  extremes: hmax 3e38 against clamp 1; a denormal hmax with clamp below it; acc at 0, at 1e7 (+ 0.3 rounds), alpha 0 and 16 777 215
"""
import ctypes as C
import types

import numpy as np

ROWS = 8192
F = np.float32
U64 = np.uint64
FLT_MAX = np.finfo(F).max
P99 = F(0.99)  # the roulette's cap, as a float
BEGIN_STRATA, CONTINUE_STRATA, END_STRATA = "abcd", "abcd", "abcd"
SEED = 7300
INF = F(np.inf)


def up(x):
    with np.errstate(over="ignore"):  # (above FLT_MAX: inf)
        return np.nextafter(np.asarray(x, F), INF)


def down(x):
    return np.nextafter(np.asarray(x, F), -INF)


# ---------------------------------------------------------------------------------------------------------------
# pcg32
# ---------------------------------------------------------------------------------------------------------------
MULT = U64(6364136223846793005)
MULT_INV = U64(pow(6364136223846793005, -1, 1 << 64))


def output(state):
    """The 32-bit output the generator gives when it steps from `state`."""
    state = np.asarray(state, U64)
    xs = ((((state >> U64(18)) ^ state) >> U64(27)) & U64(0xFFFFFFFF)).astype(np.uint32)
    rot = (state >> U64(59)).astype(np.uint32)
    return (xs >> rot) | (xs << ((np.uint32(32) - rot) & np.uint32(31)))


def advance(state, inc):
    return np.asarray(state, U64) * MULT + np.asarray(inc, U64)


def step_back(state, inc):
    return (np.asarray(state, U64) - np.asarray(inc, U64)) * MULT_INV


def as_float(out32):
    """rand1f of a 32-bit output (math.h:1434-1442): the top 23 bits as the mantissa of a float in [1, 2), minus 1."""
    return ((np.asarray(out32, np.uint32) >> np.uint32(9)) | np.uint32(0x3F800000)).view(F) - F(1)


def draws(rng, k):
    """The next k draws of every stream of rng (n, 2) = state, inc: ((n, k) float32, the states afterwards)."""
    rng = np.asarray(rng, U64).reshape(-1, 2)
    state, inc = rng[:, 0].copy(), rng[:, 1]
    out = np.zeros((len(rng), k), F)
    for d in range(k):
        out[:, d] = as_float(output(state))
        state = advance(state, inc)
    return out, state


def state_with_output(out32, rot, low27):
    """A state whose step gives out32: its top five bits are `rot`, its low 27 bits `low27` (they do not reach the output)."""
    o, r = np.asarray(out32, U64), np.asarray(rot, U64)
    xs = ((o << r) | (o >> ((U64(32) - r) & U64(31)))) & U64(0xFFFFFFFF)  # rotl: the output is rotr(xs, rot)
    z = (r << U64(32)) | xs            # = t ^ (t >> 18) for t = state >> 27 (37 bits), whose top 18 bits are z's
    t = z ^ (z >> U64(18)) ^ (z >> U64(36))
    return (t << U64(27)) | np.asarray(low27, U64)


def random_streams(gen, n):
    return np.stack([gen.integers(0, 1 << 64, n, dtype=U64), gen.integers(0, 1 << 63, n, dtype=U64) << U64(1) | U64(1)], axis=1)


def streams_with_draw(gen, k, mantissa):
    """(n, 2) streams whose draw number k (from 0) is mantissa * 2^-23; everything else random."""
    mantissa = np.asarray(mantissa, U64)
    n = len(mantissa)
    assert (mantissa < U64(1 << 23)).all()
    inc = gen.integers(0, 1 << 63, n, dtype=U64) << U64(1) | U64(1)
    out32 = (mantissa << U64(9)) | gen.integers(0, 512, n, dtype=U64)
    state = state_with_output(out32, gen.integers(0, 32, n, dtype=U64), gen.integers(0, 1 << 27, n, dtype=U64))
    for _ in range(k):
        state = step_back(state, inc)
    return np.stack([state, inc], axis=1)


# ---------------------------------------------------------------------------------------------------------------
# begin
# ---------------------------------------------------------------------------------------------------------------
LU, LV, PU, PV = 0, 1, 2, 3  # the order of the draws
IMAGE_SIZES = ((720, 720), (100, 75), (37, 64))
GENERATED = [("sphere-hairblock", dict(scale=0.02)), ("sphere-hairblock", dict(scale=0.05, zoom=True)), ("sphere-hairblock", dict(scale=0.05, dof=True)),
             ("straight-hair", dict(scale=0.05)), ("curly-hair", dict(scale=0.05)), ("hair-curls", dict(scale=0.05)), ("lobes", dict(scale=0.05)),
             ("volumes", dict(scale=0.05)), ("textured", dict(scale=0.05)), ("crowd", dict(scale=0.05))]
REF_SCENES = ("sloth", "bold-man", "straight-hair", "curly-hair", "hair-curls", "sphere-hairblock")


def camera_row(cam):
    """The 17 floats of a yh_camera (ctypes) in the kernels' order."""
    return np.array(list(cam.frame) + [cam.lens, cam.film[0], cam.film[1], cam.focus, cam.aperture], F)


_CAMERAS = {}


def scene_cameras(yh, scene_path):
    """(m, 17): the cameras of the generated scenes and of the reference's own scene descriptions, as the loader makes them."""
    if "rows" not in _CAMERAS:
        rows = []
        for name, kw in GENERATED + [("ref-" + w, dict(scale=0.01)) for w in REF_SCENES]:
            sf = yh.SceneFile(scene_path(name, **kw))
            rows.append(camera_row(sf.desc.contents.camera))
            sf.close()
        _CAMERAS["rows"] = np.array(rows, F)
    return _CAMERAS["rows"]


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _frames(gen, n, kinds):
    """(n, 12) frames x, y, z, o cycling through `kinds`: identity, rotated, mirrored (negative determinant), scaled (0.01 ... 100, not uniform)."""
    out = np.zeros((n, 12), F)
    for r in range(n):
        kind = kinds[r % len(kinds)]
        M = np.eye(3) if kind == "identity" else _rot(gen.normal(size=3), gen.uniform(0, 2 * np.pi))
        if kind == "mirrored":
            M = M @ np.diag([1.0, -1.0, 1.0])
        if kind == "scaled":
            M = M @ np.diag(10 ** gen.uniform(-2, 2, 3))
        out[r] = np.concatenate([M.T.reshape(-1), gen.uniform(-30, 30, 3) if kind != "identity" else np.zeros(3)])
    return out


def _begin(cams, ijwh, rng, **claims):
    return types.SimpleNamespace(cams=np.ascontiguousarray(cams, F), ijwh=np.ascontiguousarray(ijwh, np.int32), rng=np.ascontiguousarray(rng, U64),
                                 args=None, **claims)


def begin_stratum(name, cameras):
    """cameras: scene_cameras(...). Returns cams, ijwh, rng and, per stratum, the index sets its claims are made on."""
    gen = np.random.default_rng(SEED + ord(name))
    n = ROWS
    rows = np.arange(n)
    if name == "a":
        cams = cameras[gen.integers(0, len(cameras), n)].copy()
        size = np.array(IMAGE_SIZES)[gen.integers(0, 3, n)]
        w, h = size[:, 0], size[:, 1]
        wide = w >= h  # the film the image was sized from (pt.cpp:1933-1939): the larger side keeps the camera's film
        film = np.maximum(cams[:, 13], cams[:, 14])
        cams[:, 13] = np.where(wide, film, film * (w / h).astype(F))
        cams[:, 14] = np.where(wide, film * (h / w).astype(F), film)
        cams[:, 16] = 0
        ijwh = np.stack([gen.integers(0, w), gen.integers(0, h), w, h], axis=1)
        return _begin(cams, ijwh, random_streams(gen, n))
    if name == "b":
        cams = cameras[gen.integers(0, len(cameras), n)].copy()
        cams[:, :12] = _frames(gen, n, ("rotated", "mirrored", "scaled", "identity"))
        cams[:, 13] = gen.choice([0.036, 0.024, 0.01, 0.07], n)
        cams[:, 14] = gen.choice([0.036, 0.0135, 0.02025, 0.09], n)
        cams[:, 16] = 0
        w, h = gen.choice([1, 2, 37, 64, 100, 720], n), gen.choice([1, 3, 41, 64, 75, 720], n)
        one_w, one_h = rows % 16 == 0, rows % 16 == 1
        w[one_w], h[one_h] = 1, 1
        corner = (rows // 8) % 4  # the four corners
        i, j = np.where(corner & 1, w - 1, 0), np.where(corner & 2, h - 1, 0)
        edge = rows % 8 < 4  # half the rows: a pixel draw on an edge of [0, 1)
        which = np.where(rows % 2 == 0, PU, PV)
        low = (rows // 2) % 2 == 0
        mant = np.where(low, gen.integers(0, 1 << 13, n), (1 << 23) - 1 - gen.integers(0, 1 << 13, n))
        mant = np.where(rows % 64 < 8, np.where(low, 0, (1 << 23) - 1), mant)  # ... and on the ends of [0, 1 - 2^-23] themselves
        rng = random_streams(gen, n)
        for k in (PU, PV):
            sel = edge & (which == k)
            rng[sel] = streams_with_draw(gen, k, mant[sel])
        return _begin(cams, np.stack([i, j, w, h], axis=1), rng, edge=edge, which=which, low=low, one_w=one_w, one_h=one_h)
    if name == "c":
        cams = cameras[gen.integers(0, len(cameras), n)].copy()
        cams[:, :12] = _frames(gen, n, ("identity", "rotated", "scaled", "mirrored"))
        cams[:, 15] = 10 ** gen.uniform(-3, 4, n)
        cams[:, 16] = 10 ** gen.uniform(-6, 1, n)
        tiny = rows % 8 == 7
        cams[tiny, 16] = 1e-30
        size = np.array(IMAGE_SIZES)[gen.integers(0, 3, n)]
        w, h = size[:, 0], size[:, 1]
        ijwh = np.stack([gen.integers(0, w), gen.integers(0, h), w, h], axis=1)
        kind = rows % 8  # 0: lv ~ 0; 1-5: lu about 0, 1/4, 1/2, 3/4, 1; 6, 7: random draws
        rng = random_streams(gen, n)
        sel = kind == 0
        rng[sel] = streams_with_draw(gen, LV, gen.integers(0, 8, int(sel.sum())))  # below 2^-20
        near = 1 << 13  # 2^-10 in mantissa units
        for q in range(5):
            sel = kind == 1 + q
            m = int(sel.sum())
            centre = q << 21
            lo, hi = max(centre - near, 0), min(centre + near, (1 << 23) - 1)
            mant = gen.integers(lo, hi + 1, m)
            mant[:4] = [lo, hi, min(max(centre, 0), (1 << 23) - 1), min(centre + 1, (1 << 23) - 1)]
            rng[sel] = streams_with_draw(gen, LU, mant)
        return _begin(cams, ijwh, rng, kind=kind, tiny=tiny)
    if name == "d":
        cams = cameras[gen.integers(0, len(cameras), n)].copy()
        cams[:, 15] = 10 ** gen.uniform(-1, 2, n)
        cams[:, 16] = np.where(rows % 2 == 0, 0, 10 ** gen.uniform(-3, 0, n))
        kind = (rows // 2) % 6  # 0 lens = 0; 1 focus = 0; 2 a negative aperture; 3 film = 0 (both); 4 film x = 0; 5 lens = 0 and film = 0 (q = 0)
        cams[kind == 0, 12] = 0
        cams[kind == 1, 15] = 0
        cams[kind == 2, 16] = -(10 ** gen.uniform(-3, 0, int((kind == 2).sum())))
        cams[kind == 3, 13:15] = 0
        cams[kind == 4, 13] = 0
        cams[kind == 5, 12:15] = 0
        size = np.array(IMAGE_SIZES)[gen.integers(0, 3, n)]
        w, h = size[:, 0], size[:, 1]
        ijwh = np.stack([gen.integers(0, w), gen.integers(0, h), w, h], axis=1)
        return _begin(cams, ijwh, random_streams(gen, n), kind=kind)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------
# continue
# ---------------------------------------------------------------------------------------------------------------
def _place(largest, others, pos):
    """(n, 3) with `largest` at column pos and `others` (n, 2) in the two other columns."""
    n = len(largest)
    out = np.zeros((n, 3), F)
    rows = np.arange(n)
    out[rows, pos] = largest
    out[rows, (pos + 1) % 3], out[rows, (pos + 2) % 3] = others[:, 0], others[:, 1]
    return out


def _continue(weight, bounce, bounces, rng, **claims):
    return types.SimpleNamespace(weight=np.ascontiguousarray(weight, F), bb=np.ascontiguousarray(np.stack([bounce, bounces], axis=1), np.int32),
                                 rng=np.ascontiguousarray(rng, U64), **claims)


def continue_stratum(name):
    gen = np.random.default_rng(SEED + 100 + ord(name))
    n = ROWS
    rows = np.arange(n)
    rng = random_streams(gen, n)
    if name == "a":
        bounce = np.where(rows % 2 == 0, 2 + (rows // 2) % 4, gen.integers(0, 10, n))
        rel = (rows // 8) % 4  # bounce + 1 on bounces - 1, bounces, bounces + 1; bounces = 1
        bounces = np.where(rel == 3, 1, bounce + 1 - (rel - 1))
        return _continue(gen.uniform(0.01, 2, (n, 3)), bounce, bounces, rng, rel=rel)
    if name == "b":
        kind = rows % 16
        w = gen.uniform(0.05, 1.5, (n, 3)).astype(F)
        w[kind == 0] = 0.0
        w[kind == 1] = -0.0
        mixed = np.array([[0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [-0.0, -0.0, 0.0]], F)
        w[kind == 2] = mixed[(rows[kind == 2] // 16) % 3]
        for k, v in ((3, np.nan), (4, np.inf), (5, -np.inf)):  # in each position
            sel = np.flatnonzero(kind == k)
            w[sel, (sel // 16) % 3] = v
        sel = kind == 6  # all negative: a negative rr_prob
        w[sel] = -w[sel]
        sel = kind == 7  # one negative component: hmax stays positive
        w[sel, 0] = -w[sel, 0]
        sel = np.flatnonzero(kind == 8)  # a denormal hmax: 1 / rr_prob overflows
        w[sel] = _place(F(2.0 ** -149) * gen.integers(1, 1 << 20, len(sel)).astype(F), np.zeros((len(sel), 2), F), (sel // 16) % 3)
        sel = np.flatnonzero(kind == 9)  # hmax tiny but normal, the others negative
        w[sel] = _place(F(1e-37) * gen.uniform(1, 9, len(sel)).astype(F), -gen.uniform(0, 1, (len(sel), 2)).astype(F), (sel // 16) % 3)
        bounce = np.where(rows % 32 < 16, gen.integers(4, 8, n), gen.integers(0, 4, n))
        return _continue(w, bounce, np.full(n, 64), rng, kind=kind)
    if name == "c":
        kind, pos = rows % 4, (rows // 4) % 3
        top = np.select([kind == 0, kind == 1, kind == 2], [np.full(n, down(P99)), np.full(n, P99), np.full(n, up(P99))], gen.uniform(1.5, 40, n)).astype(F)
        w = _place(top, (top[:, None] * gen.uniform(0, 1, (n, 2))).astype(F), pos)
        return _continue(w, gen.integers(4, 9, n), np.full(n, 64), rng, kind=kind, pos=pos, top=top)
    if name == "d":
        # streams whose next draw lies in (2^-10, 0.98): the cap plays no part and the neighbours exist
        draw = np.zeros(n, F)
        todo = np.ones(n, bool)
        while todo.any():
            rng[todo] = random_streams(gen, int(todo.sum()))
            draw[todo] = draws(rng[todo], 1)[0][:, 0]
            todo = ~((draw > 2.0 ** -10) & (draw < 0.98))
        kind, pos = rows % 3, (rows // 3) % 3  # 0: hmax one float below the draw, 1: on it, 2: one float above
        top = np.select([kind == 0, kind == 1], [down(draw), draw], up(draw)).astype(F)
        w = _place(top, (top[:, None] * gen.uniform(0, 1, (n, 2))).astype(F), pos)
        bounce = np.where(rows % 8 == 7, gen.integers(0, 4, n), gen.integers(4, 9, n))
        return _continue(w, bounce, np.full(n, 64), rng, kind=kind, pos=pos, draw=draw, top=top)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------
# end
# ---------------------------------------------------------------------------------------------------------------
CLAMPS = np.array([0.25, 1.0, 100.0, FLT_MAX, np.inf], F)


def _end(radiance, clamp, acc, hit, **claims):
    rad = np.concatenate([np.asarray(radiance, F), np.asarray(clamp, F).reshape(-1, 1), np.asarray(acc, F)], axis=1)
    return types.SimpleNamespace(rad=np.ascontiguousarray(rad, F), hit=np.ascontiguousarray(np.asarray(hit, np.int32).reshape(-1, 1)), **claims)


def end_stratum(name):
    gen = np.random.default_rng(SEED + 200 + ord(name))
    n = ROWS
    rows = np.arange(n)
    hit = rows % 2
    acc = np.concatenate([gen.uniform(0, 3, (n, 3)) * gen.integers(0, 9, (n, 1)), gen.integers(0, 9, (n, 1))], axis=1).astype(F)
    if name == "a":
        return _end(gen.uniform(0, 3, (n, 3)), np.full(n, 100), acc, hit)
    if name == "b":
        kind = (rows // 2) % 8
        r = gen.uniform(0, 3, (n, 3)).astype(F)
        for k, v in ((0, np.nan), (1, np.inf), (2, -np.inf)):
            sel = np.flatnonzero(kind == k)
            r[sel, (sel // 16) % 3] = v
        r[kind == 3] = 0.0
        sel = kind == 4  # all negative
        r[sel] = -r[sel]
        sel = kind == 5  # one negative component
        r[sel, 1] = -r[sel, 1]
        sel = np.flatnonzero(kind == 6)  # two components non-finite
        r[sel, (sel // 16) % 3], r[sel, (sel // 16 + 1) % 3] = np.nan, np.inf
        r[kind == 7] = -0.0
        return _end(r, CLAMPS[(rows // 16) % 3], acc, hit, kind=kind)
    if name == "c":
        kind, pos = (rows // 2) % 3, (rows // 6) % 3  # hmax one float below clamp, on it, one float above
        clamp = CLAMPS[(rows // 18) % 5]
        top = np.select([kind == 0, kind == 1], [down(clamp), clamp], up(clamp)).astype(F)  # (above FLT_MAX: inf, which sanitize takes; above inf: inf)
        with np.errstate(invalid="ignore", over="ignore"):
            others = (np.where(np.isfinite(top), top, FLT_MAX)[:, None] * gen.uniform(0, 1, (n, 2))).astype(F)
        return _end(_place(top, others, pos), clamp, acc, hit, kind=kind, pos=pos, top=top)
    if name == "d":
        kind, pos = (rows // 2) % 6, (rows // 12) % 3
        r, clamp = gen.uniform(0, 3, (n, 3)).astype(F), np.full(n, 100, F)
        sel = kind == 0  # far above the clamp
        m = int(sel.sum())
        r[sel], clamp[sel] = _place(np.full(m, 3e38, F), gen.uniform(0, 3e38, (m, 2)).astype(F), pos[sel]), 1
        sel = kind == 1  # a denormal hmax with the clamp below it
        m = int(sel.sum())
        top = F(2.0 ** -149) * gen.integers(2, 1 << 22, m).astype(F)
        r[sel] = _place(top, np.zeros((m, 2), F), pos[sel])
        clamp[sel] = np.where(np.arange(m) % 8 == 0, 0, top * gen.uniform(0, 1, m)).astype(F)  # (a clamp of 0 among them: the scale is 0)
        acc[kind == 2] = 0.0
        sel = kind == 3  # the addition rounds
        acc[sel, :3], r[sel], clamp[sel] = 1e7, 0.3, 100
        sel = kind == 4
        acc[sel, 3] = 0
        sel = kind == 5
        acc[sel, 3] = 16777215
        return _end(r, clamp, acc, hit, kind=kind, pos=pos)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------
# the scene of the render that can be predicted
# ---------------------------------------------------------------------------------------------------------------
CLAMP = F(1.0)
ENVIRONMENT = (0.25, 0.5, 0.125)
# emission classes against the trace parameter clamp = 1: hmax below it, exactly on it, a float above it, 2 x and 1e30 x it
CLASSES = ("below", "on", "above", "twice", "huge")
_TOP = {"below": F(0.75), "on": F(1.0), "above": up(F(1.0)), "twice": F(2.0), "huge": F(1e30)}


def emitter_emissions():
    """(15, 3): class k // 3 with its largest component in channel k % 3; the other channels 1/2 and 1/4 of it."""
    out = np.zeros((15, 3), F)
    for k in range(15):
        top = _TOP[CLASSES[k // 3]]
        out[k, k % 3], out[k, (k + 1) % 3], out[k, (k + 2) % 3] = top, top * F(0.5), top * F(0.25)
    return out


class RenderScene:
    """Fifteen emitting two-triangle quads on a 4 x 4 grid in the plane z = 0 (the sixteenth cell is empty), seen from z = 10 through a lens;
    in front of them a bent diffuse mesh over the lower left cells and plain strands across the upper rows, neither emitting; a constant
    environment. Objects 0-14: the emitters, 15: the mesh, 16: the strands. Materials: 0-14 the emitters', 15 diffuse, 16 hair."""

    def __init__(self, film=(0.036, 0.036)):
        gen = np.random.default_rng(SEED + 900)
        self.film = film
        q = np.array([(-0.5, -0.5, 0), (0.5, -0.5, 0), (0.5, 0.5, 0), (-0.5, 0.5, 0)], F)
        self.shapes = [dict(pos=q, tris=np.array([(0, 1, 2), (0, 2, 3)], np.int32), lines=None, rad=None)]
        k = 6
        g = np.linspace(-0.6, 0.6, k + 1)
        x, y = np.meshgrid(g, g, indexing="ij")
        pos = np.stack([x.ravel(), y.ravel(), 0.2 * np.sin(2 * x.ravel()) * np.cos(1.5 * y.ravel())], axis=1).astype(F)
        idx = lambda i, j: i * (k + 1) + j  # noqa: E731
        tris = [t for i in range(k) for j in range(k) for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))]
        self.shapes.append(dict(pos=pos, tris=np.array(tris, np.int32), lines=None, rad=None))
        spos, lines = [], []
        for s in range(10):
            p = np.cumsum(np.concatenate([[[-3.4, gen.uniform(-0.2, 3.2), gen.uniform(-0.2, 0.2)]], gen.normal(0, 0.08, (12, 3)) + [0.56, 0, 0]]), axis=0)
            base = len(spos)
            spos += list(p)
            lines += [(base + i, base + i + 1) for i in range(12)]
        self.shapes.append(dict(pos=np.array(spos, F), tris=None, lines=np.array(lines, np.int32), rad=np.full(len(spos), 0.04, F)))
        self.emissions = emitter_emissions()
        self.material_emission = np.concatenate([self.emissions, np.zeros((2, 3), F)])
        self.objects = []
        for e in range(15):
            frame = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, -2.4 + 1.6 * (e % 4), -2.4 + 1.6 * (e // 4), 0], F)
            self.objects.append((frame, 0, e))
        self.objects.append((np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, -1.6, -1.6, 1.0], F), 1, 15))
        self.objects.append((np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 2.0], F), 2, 16))
        self._keep = None

    def desc(self, yh):
        if self._keep is None:
            fp, ip = yh.c_float_p, yh.c_int_p
            shapes = (yh.Shape * len(self.shapes))()
            for d, s in zip(shapes, self.shapes):
                d.num_vertices, d.positions = len(s["pos"]), s["pos"].ctypes.data_as(fp)
                if s["lines"] is not None:
                    d.num_lines, d.lines, d.radius = len(s["lines"]), s["lines"].ctypes.data_as(ip), s["rad"].ctypes.data_as(fp)
                else:
                    d.num_triangles, d.triangles = len(s["tris"]), s["tris"].ctypes.data_as(ip)
            mats = (yh.Material * 17)()
            for k, d in enumerate(mats):
                d.color[:] = [0.5, 0.5, 0.5] if k < 15 else [0.7, 0.4, 0.2] if k == 15 else [0.6, 0.4, 0.2]
                d.emission[:] = [float(v) for v in self.material_emission[k]]
                d.roughness, d.opacity, d.ior, d.trdepth = 1.0, 1.0, 1.5, 0.01
                d.beta_m, d.beta_n, d.alpha, d.eta = 0.3, 0.3, 2.0, 1.55
                d.thin = 1 if k == 16 else 0
            objs = (yh.Object * len(self.objects))()
            for d, (frame, shape, material) in zip(objs, self.objects):
                d.frame[:] = frame.tolist()
                d.shape, d.material = shape, material
            envs = (yh.Environment * 1)()
            envs[0].frame[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
            envs[0].emission[:] = list(ENVIRONMENT)
            sd = yh.SceneDesc()
            sd.num_shapes, sd.shapes = len(shapes), C.cast(shapes, C.POINTER(yh.Shape))
            sd.num_materials, sd.materials = len(mats), C.cast(mats, C.POINTER(yh.Material))
            sd.num_objects, sd.objects = len(objs), C.cast(objs, C.POINTER(yh.Object))
            sd.num_environments, sd.environments = 1, C.cast(envs, C.POINTER(yh.Environment))
            sd.camera.frame[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 10]
            sd.camera.lens, sd.camera.film[0], sd.camera.film[1], sd.camera.focus, sd.camera.aperture = 0.05, self.film[0], self.film[1], 9.0, 0.05
            self._keep = (sd, shapes, mats, objs, envs)
        return C.pointer(self._keep[0])

    def centre_rays(self, w, h):
        """The pinhole rays through the pixel centres (pt.cpp:211-229 with the lens point at zero), (h * w, 8) float32 with tmin 1e-4, tmax FLT_MAX."""
        i, j = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        u, v = (i + 0.5) / w, (j + 0.5) / h
        q = np.stack([self.film[0] * (0.5 - u), self.film[1] * (v - 0.5), np.full_like(u, 0.05)], -1)
        d = -q / np.linalg.norm(q, axis=-1, keepdims=True)  # (the frame is the identity)
        n = w * h
        return np.concatenate([np.tile([[0, 0, 10.0]], (n, 1)), d.reshape(n, 3), np.full((n, 1), 1e-4), np.full((n, 1), FLT_MAX)], axis=1).astype(F)

    def radiance_of(self, object_ids):
        """What one sample of the path shader with bounces = 1 carries for these first hits: the material's emission, the environment's on a miss."""
        ids = np.asarray(object_ids)
        material = np.array([o[2] for o in self.objects])[np.maximum(ids, 0)]
        return np.where((ids >= 0)[..., None], self.material_emission[material], np.array(ENVIRONMENT, F)).astype(F)


def path_end_f32(radiance, hit, clamp, acc):
    """path_end (csrc/dev_path.h) in float32 numpy on finite radiance: the clamp's scale, the addition, alpha. acc (..., 4) is changed in place."""
    rgb = np.asarray(radiance, F)
    top = rgb.max(axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        scaled = rgb * (F(clamp) / top)
    rgb = np.where(top > F(clamp), scaled, rgb).astype(F)
    acc[..., :3] += rgb
    acc[..., 3] += np.where(hit, F(1), F(0))
    return acc


def resolve_f32(acc, samples):
    """k_resolve (unit/framebuffer.hip): the accumulator over the sample count, in float32."""
    return (acc / F(samples)).astype(F)
