"""The closest hit, restated in float64 numpy without a tree, a box or a cull: every primitive of every object of hits-unit
(make_scenes.hits_unit_geometry), the reference's formulas (math.h:3426-3505: intersect_line, intersect_triangle) in object space, the
frame's inverse taken in float64. What a tree, a box test or a cull loses, this finds.

Float32 decides differently from float64 where a deciding quantity sits on its threshold, so every row carries a MARGIN: how far, in
relative terms, the row is from another outcome. Every test of a primitive is a set of quantities that pass when positive, each
divided by its own scale:
    segment:   |det| / (a c);  (t - tmin) / max(|t|, tmin);  (tmax - t) / |t|;  (r^2 - d2) / max(r^2, d2, 2^-40 size^2), size^2 the squares of
               the points d2 is the difference of (below that, d2 is float32's rounding: an r = 0 tip met exactly)
    triangle:  |det| / (|edge1| |pvec|);  u;  1 - u;  v;  1 - u - v;  the two of t
A primitive's own margin is |the smallest of them|: a hit is lost when one fails, a miss becomes a hit when all its failing ones pass.
The row's margin is the smallest of: the winner's own; of every other hit, its relative gap in t behind the winner; of every miss,
the larger of its own margin and of its gap behind the winner (it has to become a hit AND be nearer; one in front has only to become
a hit). The clamp of s is continuous and decides nothing. Rows whose margin exceeds M (profiles/hits_unit/margins.txt) must be found
by every float32 form: the same object and element, the distance within T."""
import functools

import numpy as np

CHUNK = 4096
# profiles/hits_unit/margins.txt (measured on the CPU against the oracle by `python tests/hit_f64.py`): per variant, M = the smallest
# power of two above which the oracle names float64's object and element on every row of every stratum, T = twice the oracle's largest
# relative distance error on stratum a. In `far` the reference itself moves every ray into object space in float32, at coordinates
# whose float is 2^-11 ... 2^-7 wide: it differs from float64 at every margin below 1, and the bar there holds next to nothing.
# `ties` (its one stratum stands where stratum a does): a primitive that is there many times is ONE primitive to float64 — the copies' t is
# one number, so who wins among them is the float32 forms' to say (the visiting order; bar 1 holds it to the oracle) — and an element is
# compared by the first primitive of its geometry (make_scenes._hits_ties: canon).
M = {"four": 2.0 ** -11, "six": 2.0 ** -12, "far": 2.0 ** 0, "deep": 2.0 ** -3, "ties": 2.0 ** -22}
T = {"four": 1.88e-4, "six": 9.85e-5, "far": 7.87e-2, "deep": 3.2e-4, "ties": 3.58e-7}
_TINY = 1e-300


def _tests(o, d, tmin, tmax, g):
    """(t, hit, smallest quantity) per (ray, primitive) of one object: rays (n, 3) in object space. Every product of a ray with a
    primitive is one matrix product (the squares and triple products expanded), so nothing of size rays x primitives x 3 is made;
    in float64 the cancellation this costs is some 1e-15 of the coordinates' squares, far below any margin in use."""
    p = g["positions"].astype(np.float64)
    tmin, tmax = tmin[:, None], tmax[:, None]
    dot = lambda a, b: (a * b).sum(-1)  # noqa: E731
    with np.errstate(all="ignore"):
        if "lines" in g:
            p0, p1 = p[g["lines"][:, 0]], p[g["lines"][:, 1]]
            r0, r1 = (g["radius"].astype(np.float64)[g["lines"][:, k]][None] for k in (0, 1))
            v = p1 - p0
            a, b, c = dot(d, d)[:, None], d @ v.T, dot(v, v)[None]
            dd, e = dot(d, o)[:, None] - d @ p0.T, o @ v.T - dot(v, p0)[None]   # dot(u, w), dot(v, w) with w = o - p0
            ww = dot(o, o)[:, None] - 2 * (o @ p0.T) + dot(p0, p0)[None]
            det = a * c - b * b
            t, s = (b * e - c * dd) / det, np.clip((a * e - b * dd) / det, 0, 1)
            d2 = np.maximum(ww + t * t * a + s * s * c + 2 * t * dd - 2 * s * e - 2 * t * s * b, 0)  # |w + d t - v s|^2
            r = r0 * (1 - s) + r1 * s
            # (d2 is a difference of points: below the square of 2^-20 of their size it is rounding in float32, whatever r is — an r = 0 tip met exactly)
            size2 = dot(o, o)[:, None] + t * t * a + (dot(p0, p0) + dot(p1, p1))[None]
            q = [np.abs(det) / np.maximum(a * c, _TINY), (r * r - d2) / np.maximum(np.maximum(np.maximum(r * r, d2), 2.0 ** -40 * size2), _TINY)]
            # d2 == r * r is a hit (the test is d2 > r * r): a quantity of exactly 0 passes
            never = np.broadcast_to(c == 0, det.shape)  # a segment of zero length: det is 0 in every arithmetic
        else:
            tri = g["triangles"]
            p0, p1, p2 = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
            e1, e2 = p1 - p0, p2 - p0
            nrm, od = np.cross(e1, e2), np.cross(o, d)
            det = -(d @ nrm.T)                                       # dot(e1, cross(d, e2))
            u = (od @ e2.T - d @ np.cross(e2, p0).T) / det           # dot(o - p0, cross(d, e2))
            v = (-(od @ e1.T) - d @ np.cross(p0, e1).T) / det        # dot(d, cross(o - p0, e1))
            t = (o @ nrm.T - dot(p0, nrm)[None]) / det               # dot(e2, cross(o - p0, e1))
            pv = np.sqrt(np.maximum(dot(d, d)[:, None] * dot(e2, e2)[None] - (d @ e2.T) ** 2, 0))  # |cross(d, e2)|
            q = [np.abs(det) / np.maximum(np.linalg.norm(e1, axis=-1)[None] * pv, _TINY), u, 1 - u, v, 1 - u - v]
            never = np.broadcast_to((np.linalg.norm(nrm, axis=-1) == 0)[None], det.shape)  # no area: det is 0 for every ray
        q += [(t - tmin) / np.maximum(np.maximum(np.abs(t), tmin), _TINY), (tmax - t) / np.maximum(np.abs(t), _TINY)]
        worst = np.min(np.stack(q), axis=0)
        flat = (det == 0) | ~np.isfinite(t)
        hit = ~flat & (q[0] > 0) & (worst >= 0)
        worst = np.where(flat, 0.0, worst)
        t = np.where(flat, np.inf, t)
        worst = np.where(never, -np.inf, worst)
    return t, hit, worst


def closest(geo, rays):
    """object, element (int, -1: no hit), distance (float64, inf) and margin (float64) of every row of `rays` (n, 8) float32."""
    rays, back = np.unique(np.ascontiguousarray(rays, np.float32).view(np.uint32), axis=0, return_inverse=True)  # (the strata repeat rows)
    back = back.ravel()
    rays = rays.view(np.float32).astype(np.float64)
    n = len(rays)
    obj, elem = np.full(n, -1), np.full(n, -1)
    dist, margin = np.full(n, np.inf), np.full(n, np.inf)
    inv = []
    for g in geo:
        f = g["frame"].astype(np.float64).reshape(4, 3)
        inv.append((np.linalg.inv(f[:3]), f[3]))
    for lo in range(0, n, CHUNK):
        r = rays[lo:lo + CHUNK]
        ts, hits, worsts, owner = [], [], [], []
        for k, g in enumerate(geo):
            m, org = inv[k]
            t, hit, worst = _tests((r[:, 0:3] - org) @ m, r[:, 3:6] @ m, r[:, 6], r[:, 7], g)
            ts.append(t), hits.append(hit), worsts.append(worst), owner.append(np.full(t.shape[1], k))
        t, hit, worst, owner = np.concatenate(ts, 1), np.concatenate(hits, 1), np.concatenate(worsts, 1), np.concatenate(owner)
        first = np.concatenate([[0], np.cumsum([x.shape[1] for x in ts])])
        th = np.where(hit, t, np.inf)
        # the later primitive wins a tie (math.h: t > tmax rejects, t == tmax accepts)
        win = th.shape[1] - 1 - np.argmin(th[:, ::-1], axis=1)
        rows = np.arange(len(r))
        any_hit = hit.any(1)
        tw = np.where(any_hit, th[rows, win], np.inf)
        with np.errstate(all="ignore"):
            gap = np.where(np.isfinite(tw)[:, None], (t - tw[:, None]) / np.maximum(np.abs(tw[:, None]), _TINY), -np.inf)  # a miss has no winner to beat
            other = np.where(hit, np.abs(gap), np.maximum(np.abs(worst), np.where(np.isfinite(gap), gap, -np.inf)))
        other[rows[any_hit], win[any_hit]] = np.abs(worst[rows[any_hit], win[any_hit]])
        other = np.where(np.isnan(other), 0.0, other)
        margin[lo:lo + CHUNK] = other.min(1)
        sel = rows[any_hit]
        obj[lo + sel] = owner[win[sel]]
        elem[lo + sel] = win[sel] - first[owner[win[sel]]]
        dist[lo + sel] = tw[sel]
    return obj[back], elem[back], dist[back], margin[back]


@functools.lru_cache(maxsize=None)
def main_batch(variant):
    """closest() on hit_cases.main_batch(variant) — on `deep`, hit_cases.deep_rays() — computed once."""
    import hit_cases as hc
    import make_scenes
    geo = make_scenes.hits_unit_geometry(variant)
    if variant != "ties":
        return closest(geo, hc.deep_rays() if variant == "deep" else hc.main_batch(variant))
    once, keep = [], []
    for g in geo:  # every geometry once
        kind = "lines" if "lines" in g else "triangles"
        keep.append(np.unique(g["canon"]) if "canon" in g else np.arange(len(g[kind])))
        once.append({**g, kind: g[kind][keep[-1]]})
    obj, elem, dist, margin = closest(once, hc.ties_rays())
    for k, rows in enumerate(keep):
        elem = np.where(obj == k, rows[np.clip(elem, 0, len(rows) - 1)], elem)
    return obj, elem, dist, margin


def _canon(variant, obj, elem):
    """`elem` with every copy of a primitive named by the first of its geometry (variant `ties`; elsewhere as given)."""
    if variant != "ties":
        return elem
    import make_scenes
    elem = elem.copy()
    for k, g in enumerate(make_scenes.hits_unit_geometry(variant)):
        if "canon" in g:
            elem = np.where(obj == k, g["canon"][np.clip(elem, 0, len(g["canon"]) - 1)], elem)
    return elem


def _names(variant):
    import hit_cases as hc
    return hc.DEEP_NAMES if variant == "deep" else hc.TIES_NAMES if variant == "ties" else hc.NAMES


def compare(variant, got, what="the oracle"):
    """Holds (object, element, uv, distance) of main_batch(variant) to float64 on the rows above M[variant]; returns the share of rows
    at or below it per stratum."""
    import hit_cases as hc
    names = _names(variant)
    fo, fe, ft, fm = main_batch(variant)
    above = fm > M[variant]
    wrong = np.flatnonzero(above & ((got[0] != fo) | (_canon(variant, got[0], got[1]) != fe)))
    assert wrong.size == 0, (f"{variant}: {what} differs from float64 on {wrong.size} rows above the margin, first {hc.where(wrong[0], names)}: "
                             f"{got[0][wrong[0]]}/{got[1][wrong[0]]} against {fo[wrong[0]]}/{fe[wrong[0]]}, margin {fm[wrong[0]]:.3g}")
    hit = above & (fo >= 0)
    rel = np.abs(got[3][hit].astype(np.float64) - ft[hit]) / ft[hit]
    assert rel.size or M[variant] >= 1, f"{variant}: no hit above the margin"
    assert not rel.size or rel.max() <= T[variant], f"{variant}: {what}'s distance is {rel.max():.3g} off float64's, row {hc.where(np.flatnonzero(hit)[rel.argmax()], names)}"
    return {name: float((~above)[k * hc.N:(k + 1) * hc.N].mean()) for k, name in enumerate(names)}


def measure(variant, got):
    """(M, T, share of rows at or below M per stratum) as measured against `got`, the oracle's hits on main_batch(variant)."""
    import hit_cases as hc
    names = _names(variant)
    fo, fe, ft, fm = main_batch(variant)
    agree = (got[0] == fo) & (_canon(variant, got[0], got[1]) == fe)
    worst = fm[~agree].max() if (~agree).any() else 0.0
    m = 2.0 ** np.ceil(np.log2(worst)) if worst > 0 else 0.0
    a_at = names.index("a") if "a" in names else 0  # (`ties`: its one stratum)
    sa = slice(a_at * hc.N, (a_at + 1) * hc.N)
    a = agree[sa] & (fo[sa] >= 0)
    t = 2 * (np.abs(got[3][sa][a].astype(np.float64) - ft[sa][a]) / ft[sa][a]).max()
    return m, t, {name: float((fm <= m)[k * hc.N:(k + 1) * hc.N].mean()) for k, name in enumerate(names)}


if __name__ == "__main__":  # the table of profiles/hits_unit/margins.txt
    import os
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(root, "tools"), os.path.join(root, "yocto-hair_amd", "python")]
    import hit_cases as hc
    import make_scenes
    import oracle_capi as oc
    oc.yh.load()
    with tempfile.TemporaryDirectory() as tmp:
        for v in M:
            m, t, share = measure(v, hc.oracle_hits(v, oc.yh, oc.Oracle(), lambda n, **kw: make_scenes.ensure_scene(n, tmp, **kw))[0])
            print(f"{v:5s} M = 2^{int(np.log2(m)):d}  T = {t:.4g}  rows at or below M per stratum: " + "  ".join(f"{k} {100 * x:.2f}%" for k, x in share.items()))
