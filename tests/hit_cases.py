"""The rays of the closest-hit tests (test_hits_unit.py, test_oracle_vs_ref.py, oracle/make_golden.py): eight strata of N = 8192 rays
on the scene hits-unit (tools/make_scenes.py), numpy only, fixed seeds. All eight together are the 65 536 rays at which
yh_intersect_batch takes the one-lane kernel; every one of them has tmin = 1e-4f, is finite and has a direction. The rows with another
tmin are a batch of their own (quad_only) for the quad forms.

    a  today's domain: random rays aimed at the objects from outside and from inside their boxes
    b  segment edges: at p0, p1 and joints (the clamp of s); at perpendicular distance r and r +- 1 ulp; r = 0 tips, the segment of
       zero length, the strand that is there twice; parallel, anti-parallel and nearly parallel to the x strand (det == 0)
    c  triangle edges: through vertices, through points of shared edges at dyadic parameters (u = 0, v = 0, u + v = 1: ties between
       neighbours), in the plane of the grid (det == 0), at the sliver, the triangle without area and the coincident pair
    d  range edges: t == tmax and its float neighbours at the first and at the second hit; t == tmin = 1e-4f
       (quad_only: t == tmin for tmin = 0, 2^-10, 1)
    e  box edges: axis-parallel rays inside and on the faces of the flat box of `tris` and of leaf boxes (0 * inf); direction
       components of +-2^-126, 2^-127, 2^-128, 2^-149 and 1e-30 beside components of order 1; rays through a box corner (t0 == t1)
    f  frames: b and c on the sheared, the rotated and (six, far) the mirrored and scaled objects, and rays along the faces of the
       objects' world boxes from just outside to just inside (the padded-box cull of ENTER)
    g  crowding: 128 hit rows of b, each 64 times in a row, the last 16 of each 64 moved an ulp
    h  through: rays that hit one object and would hit another just behind it, both ways

Variant `ties` has one batch of its own (ties: N rows on primitives that are there many times over, whose copies fill several leaves),
variant `deep` another (deep_rays); wide_walk and wide_walk_any walk yh_bvh_build_wide's nodes as the device does, for the CPU proofs of
tests/test_hit_cases.py.

An edge row is built ON the edge, exactly (the scene's numbers are multiples of 2^-10), with the same ray one float of the deciding
input to either side next to it: rows 3 k, 3 k + 1, 3 k + 2 of a block are (below, on, above), Stratum.triple holds k or -1.
Strata b - e are aimed at the two objects under the identity frame (a-strands, c-tris), whose object space is world space: their
primitive-level form (Stratum.object / .prim: what the row was aimed at) needs no transform."""
import functools

import numpy as np

import make_scenes

N = 8192
NAMES = "abcdefgh"
TMIN = np.float32(1e-4)
FMAX = np.float32(3.4e38)
F = np.float32


class Stratum:
    def __init__(self, rays, triple, obj, prim):
        self.rays, self.triple, self.object, self.prim = rays, triple, obj, prim


class _Rows:
    """Collects blocks of rays: origin, direction (object space of `obj`, float64 on the grid), tmin, tmax, the primitive aimed at."""

    def __init__(self, geo):
        self.geo, self.rays, self.triple, self.obj, self.prim, self.ntriples = geo, [], [], [], [], 0

    def add(self, obj, o, d, prim=-1, tmin=TMIN, tmax=FMAX, triples=False):
        o, d = np.atleast_2d(np.asarray(o, np.float64)), np.atleast_2d(np.asarray(d, np.float64))
        n = max(len(o), len(d))
        o, d = np.broadcast_to(o, (n, 3)), np.broadcast_to(d, (n, 3))
        f = self.geo[obj]["frame"].astype(np.float64).reshape(4, 3)
        r = np.empty((n, 8), np.float32)
        r[:, 0:3], r[:, 3:6] = o @ f[:3] + f[3], d @ f[:3]
        r[:, 6], r[:, 7] = tmin, tmax
        self.rays.append(r)
        if triples:
            assert n % 3 == 0
            self.triple.append(self.ntriples + np.arange(n) // 3)
            self.ntriples += n // 3
        else:
            self.triple.append(np.full(n, -1))
        self.obj.append(np.full(n, obj)), self.prim.append(np.broadcast_to(np.asarray(prim), (n,)).copy())

    def add_triples(self, obj, o, d, prim, axis, tmin=TMIN, tmax=FMAX, ulps=1):
        """Each row three times: the world origin's component `axis` (per row) `ulps` float32 below, on, and above. Under the identity
        frame that is the object-space origin, and `on` is exact."""
        o, d = np.atleast_2d(np.asarray(o, np.float64)), np.atleast_2d(np.asarray(d, np.float64))
        n = max(len(o), len(d))
        rep = lambda x: np.repeat(np.broadcast_to(np.asarray(x), (n,)), 3)  # noqa: E731
        self.add(obj, np.repeat(np.broadcast_to(o, (n, 3)), 3, axis=0), np.repeat(np.broadcast_to(d, (n, 3)), 3, axis=0), rep(prim), rep(tmin), rep(tmax), triples=True)
        rays, axis, rows = self.rays[-1], rep(axis), np.arange(3 * n)
        for side, to in ((0, -np.inf), (2, np.inf)):
            sel = rows[rows % 3 == side]
            v = rays[sel, axis[sel]]
            for _ in range(ulps):
                v = np.nextafter(v, F(to))
            rays[sel, axis[sel]] = v

    def add_tmax_triples(self, obj, o, d, prim, t, tmin=TMIN):
        """Each row three times with tmax one float32 below t, t, and one above."""
        o, d = np.atleast_2d(np.asarray(o, np.float64)), np.atleast_2d(np.asarray(d, np.float64))
        n = max(len(o), len(d))
        t = np.repeat(np.broadcast_to(np.asarray(t, np.float32), (n,)), 3)
        side = np.arange(3 * n) % 3
        tmax = np.where(side == 0, np.nextafter(t, F(-np.inf)), np.where(side == 2, np.nextafter(t, F(np.inf)), t))
        rep = lambda x: np.repeat(np.broadcast_to(x, (n, 3)), 3, axis=0)  # noqa: E731
        self.add(obj, rep(o), rep(d), np.repeat(np.broadcast_to(np.asarray(prim), (n,)), 3), np.repeat(np.broadcast_to(np.asarray(tmin, np.float32), (n,)), 3), tmax, triples=True)

    def stratum(self, n=N):
        """Exactly n rows: whole blocks as built, then the built rows again from the start (whole triples) up to n."""
        rays, tr, ob, pr = (np.concatenate(x) for x in (self.rays, self.triple, self.obj, self.prim))
        assert len(rays) > 0
        if len(rays) > n:  # cut at a triple's boundary
            cut = n
            while tr[cut] >= 0 and tr[cut] == tr[cut - 1]:
                cut -= 1
            rays, tr, ob, pr = rays[:cut], tr[:cut], ob[:cut], pr[:cut]
        k = np.arange(n) % len(rays)
        tr = np.where(np.arange(n) < len(rays), tr[k], -1)  # (the filling rows repeat rays, not triples)
        return Stratum(np.ascontiguousarray(rays[k]), tr, ob[k], pr[k])


def _unit(v):
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-30)


def world_boxes(geo):
    """The objects' world boxes in float64 (radii included)."""
    out = []
    for g in geo:
        f = g["frame"].astype(np.float64).reshape(4, 3)
        p, r = g["positions"].astype(np.float64), g["radius"].astype(np.float64)
        lo, hi = (p - r[:, None]).min(0), (p + r[:, None]).max(0)
        c = np.array([[(hi if k & 4 else lo)[0], (hi if k & 2 else lo)[1], (hi if k & 1 else lo)[2]] for k in range(8)]) @ f[:3] + f[3]
        out.append((c.min(0), c.max(0)))
    return out


def _dy(rng, lo, hi, shape, q=1024):
    """Random multiples of 1 / q in [lo, hi]."""
    return rng.integers(int(lo * q), int(hi * q) + 1, shape) / q


def _prim_points(g, rng, n, plain=False):
    """n random points on primitives of an object (object space, float64) and the primitives' indices; plain: not on the strands along
    an axis (collinear neighbours and the twins: every hit near a joint of theirs is a tie) nor on the coincident triangles."""
    p = g["positions"].astype(np.float64)
    if "lines" in g:
        k = rng.integers(24 if plain and g["shape"] == "strands" else 0, len(g["lines"]), n)
        s = rng.uniform(0.25, 0.75, (n, 1)) if plain else rng.random((n, 1))  # (plain: away from the joints, where both neighbours are hit at nearly one t)
        return p[g["lines"][k, 0]] * (1 - s) + p[g["lines"][k, 1]] * s, k
    k = rng.integers(0, 128, n)
    k = np.where(plain & (k == 37), 36, k)
    u, v = rng.random((n, 1)), rng.random((n, 1))
    flip = (u + v) > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    t = g["triangles"][k]
    return p[t[:, 0]] * (1 - u - v) + p[t[:, 1]] * u + p[t[:, 2]] * v, k


# the axis-aligned strands of `strands` (make_scenes._hits_strands): first segment, axis, vertices
_ZERO = 13  # the segment of zero length (the second of strand 3)
_AXIAL = ((0, 0), (4, 1), (8, 2), (16, 2), (20, 2))  # (first segment, axis) of the four-segment strands along an axis


def _segment_edges(R, obj, rng):
    """Stratum b on one `strands` object."""
    g = R.geo[obj]
    p, r, lines = g["positions"].astype(np.float64), g["radius"].astype(np.float64), g["lines"]
    add3 = R.add_triples
    # perpendicular distance exactly r, on the axis-aligned strands at dyadic s: origin = c + r e - 2 w, direction w
    for first, ax in _AXIAL:
        for seg in range(first, first + 4):
            a, b = lines[seg]
            for s in (0.0, 0.25, 0.5, 0.75, 1.0):
                c, rr = p[a] * (1 - s) + p[b] * s, r[a] * (1 - s) + r[b] * s
                for e_ax in range(3):
                    if e_ax == ax:
                        continue
                    w_ax = 3 - ax - e_ax
                    for sign in (1.0, -1.0):
                        e, w = np.zeros(3), np.zeros(3)
                        e[e_ax], w[w_ax] = sign, 1.0
                        add3(obj, c + rr * e - 2 * w, w, seg, e_ax)
                        add3(obj, c + rr * e + 1.5 * w, -w, seg, e_ax)
    # at p0, p1 and joints of every segment: through the vertex, moved along the segment's direction (s crosses 0 or 1)
    seg = rng.integers(0, len(lines), 400)
    end = rng.integers(0, 2, 400)
    v = p[lines[seg, end]]
    d = _dy(rng, -1, 1, (400, 3), 8)
    d[np.abs(d).sum(1) == 0] = (1, 0, 0)
    add3(obj, v - 2 * d, d, seg, np.abs(p[lines[seg, 1]] - p[lines[seg, 0]]).argmax(1))
    # r = 0 tips, beside them: perpendicular rays a few grid steps from the tip along the strand (r small) and beyond it
    tips = np.flatnonzero((r[lines[:, 1]] == 0) & (r[lines[:, 0]] > 0))
    for seg in tips:
        a, b = lines[seg]
        ax = np.abs(p[b] - p[a]).argmax()
        w = np.zeros(3)
        w[(ax + 1) % 3] = 1.0
        for back in (0.0, 1 / 1024, 1 / 64, 1 / 8):
            c = p[b] - back * (p[b] - p[a])
            add3(obj, c - 2 * w, w, seg, (ax + 2) % 3)
    # the segment of zero length: through its point, every which way
    d = _dy(rng, -1, 1, (30, 3), 8)
    d[np.abs(d).sum(1) == 0] = (0, 1, 0)
    add3(obj, p[lines[_ZERO, 0]] - 2 * d, d, _ZERO, 0)
    # parallel, anti-parallel and nearly parallel to the x strand: det == 0, det = a few ulps of a * c
    y0, z0, r0 = p[0, 1], p[0, 2], r[0]
    for sign in (1.0, -1.0):
        for off in (0.0, 1 / 1024, r0 / 2, r0, 2 * r0):
            for tilt in (0.0, 2.0 ** -22, 2.0 ** -20, 2.0 ** -12, -2.0 ** -21):
                add3(obj, (-3 * sign, y0 + off, z0), (sign, tilt, 0.0), 0, 1)
    # the same families on seeded strands, where the edge is only nearly met: perpendicular at distance r (rounded)
    seg = rng.integers(24, len(lines), 500)
    a, b = lines[seg, 0], lines[seg, 1]
    s = _dy(rng, 0, 1, (500, 1), 8)
    c, rr = p[a] * (1 - s) + p[b] * s, r[a] * (1 - s[:, 0]) + r[b] * s[:, 0]
    axis = _unit(p[b] - p[a])
    e = _unit(np.cross(axis, rng.normal(size=(500, 3))))
    w = np.cross(axis, e)
    add3(obj, c + rr[:, None] * e - 2 * w, w, seg, np.abs(e).argmax(1))


def _triangle_edges(R, obj, rng):
    """Stratum c on one `tris` object."""
    add3 = R.add_triples
    n = 420
    cell = lambda x, y: np.clip(((y + 1) * 4).astype(int), 0, 7) * 16 + np.clip(((x + 1) * 4).astype(int), 0, 7) * 2  # noqa: E731
    dirs = np.array([(0, 0, -1), (0, 0, 1), (0.25, 0.5, -1), (-0.5, 0.125, 1), (1, 1, -0.25), (0.5, -0.25, -0.125)], np.float64)
    # vertices of the grid
    x, y = _dy(rng, -1, 1, n, 4), _dy(rng, -1, 1, n, 4)
    # points of horizontal, vertical and diagonal edges at dyadic parameters (1/8 of an edge)
    k = _dy(rng, 0, 0.25, n, 32)
    hx, hy = np.clip(_dy(rng, -1, 0.75, n, 4) + k, -1, 1), _dy(rng, -1, 1, n, 4)
    gx, gy = _dy(rng, -1, 0.75, n, 4), _dy(rng, -1, 0.75, n, 4)
    x = np.concatenate([x, hx, hy, gx + k]); y = np.concatenate([y, hy, hx, gy + 0.25 - k])  # noqa: E702
    axis = np.concatenate([np.zeros(n, int), np.ones(n, int), np.zeros(n, int), np.zeros(n, int)])
    d = dirs[rng.integers(0, len(dirs), len(x))]
    pt = np.stack([x, y, np.zeros_like(x)], 1)
    add3(obj, pt - 2 * d, d, cell(x, y), axis)
    # in the plane of the grid: det == 0 for every triangle, and the same a float of z off the plane
    m = 60
    add3(obj, np.stack([np.full(m, -2.0), _dy(rng, -1, 1, m, 32), np.zeros(m)], 1), (1.0, 0.0, 0.0), 0, 2)
    add3(obj, np.stack([_dy(rng, -1, 1, m, 32), np.full(m, 2.0), np.zeros(m)], 1), (0.25, -1.0, 0.0), 0, 2)
    # the triangle without area (128), the sliver (129: y in [1.25, 1.25 + 2^-10]) and the coincident pair (37 and 130: cell (2, 2), upper half)
    xs = _dy(rng, 0, 1, m, 64)
    add3(obj, np.stack([xs, np.full(m, 1.25), np.full(m, 2.0)], 1), (0, 0, -1.0), 128, 1)
    xs = _dy(rng, -1, 0, m, 64)
    for yy in (1.25, 1.25 + 1 / 2048, 1.25 + 1 / 1024):
        add3(obj, np.stack([xs, np.full(m, yy), np.full(m, 2.0)], 1), (0, 0, -1.0), 129, 1)
    add3(obj, np.stack([xs, np.full(m, 1.25), np.full(m, 2.0)], 1), (0, 0, -1.0), 129, 0)
    u, v = _dy(rng, 0, 0.25, m, 64), _dy(rng, 0, 0.25, m, 64)
    px, py = -0.5 + np.maximum(u, 0.25 - v), -0.5 + np.maximum(v, 0.25 - u)  # inside or on the edges of the upper triangle of cell (2, 2)
    dd = dirs[rng.integers(0, len(dirs), m)]
    add3(obj, np.stack([px, py, np.zeros(m)], 1) - 2 * dd, dd, 130, 0)


def _range_edges(R, rng, quad_only):
    """Stratum d (a-strands = object 0, c-tris = object 2, both under the identity frame)."""
    p, r = R.geo[0]["positions"].astype(np.float64), R.geo[0]["radius"].astype(np.float64)
    m = 150
    # straight down onto the x strand (t = 1.75 at the closest approach, the hit the line test reports) and the grid behind it (t = 2)
    x = _dy(rng, -1, 1, m, 64)
    off = _dy(rng, -16 / 1024, 16 / 1024, m, 1024)
    o = np.stack([x, 0.25 + off, np.full(m, 2.0)], 1)
    seg = np.clip(((x + 1) * 2).astype(int), 0, 3)
    tile = np.clip(((0.25 + off + 1) * 4).astype(int), 0, 7) * 16 + np.clip(((x + 1) * 4).astype(int), 0, 7) * 2
    if not quad_only:
        R.add_tmax_triples(0, o, (0, 0, -1.0), seg, 1.75)
        R.add_tmax_triples(2, o, (0, 0, -1.0), tile, 2.0)
        R.add_tmax_triples(2, o + (0, 0, 0.5), (0, 0, -2.0), tile, 1.25)     # dot(d, d) != 1: the same plane at t = 1.25
        R.add_tmax_triples(0, o + (0, 0, 1.25), (0, 0, -2.0), seg, 1.5)
        # t == tmin = 1e-4f: the origin that far above and below the plane z = 0 of the grid (t = o.z exactly), one and three floats to either side
        t = np.float64(TMIN)
        R.add_triples(2, np.stack([x, 0.25 + off, np.full(m, t)], 1), (0, 0, -1.0), tile, 2)
        R.add_triples(2, np.stack([x, 0.25 + off, np.full(m, -t)], 1), (0, 0, 1.0), tile, 2)
        R.add_triples(2, np.stack([x, 0.25 + off, np.full(m, t)], 1), (0, 0, -1.0), tile, 2, ulps=3)
        # a finite tmax well short of, between and past the two hits
        for tmax in (1.0, 1.875, 4.0):
            R.add(0, o, (0, 0, -1.0), seg, tmax=F(tmax))
    else:
        for tmin in (0.0, 2.0 ** -10, 1.0):
            R.add_triples(2, np.stack([x, 0.25 + off, np.full(m, tmin)], 1), (0, 0, -1.0), tile, 2, tmin=F(tmin))
            R.add_triples(2, np.stack([x, 0.25 + off, np.full(m, -tmin)], 1), (0, 0, 1.0), tile, 2, tmin=F(tmin))
            # the x strand from the side: the closest approach at t == tmin
            R.add_triples(0, np.stack([x, np.full(m, 0.25 - tmin), 0.25 + off], 1), (0, 1.0, 0), seg, 1, tmin=F(tmin))
            R.add_tmax_triples(0, o, (0, 0, -1.0), seg, 1.75, tmin=F(tmin))
            R.add_tmax_triples(2, o, (0, 0, -1.0), tile, 2.0, tmin=F(tmin))
            R.add(0, o, (0, 0, -1.0), seg, tmin=F(tmin), tmax=F(1.875))


def _box_edges(R, rng):
    """Stratum e (a-strands = object 0, c-tris = object 2)."""
    m = 80
    t = _dy(rng, -1, 1, m, 64)
    # along z on and beside the faces x = +-1, y = -1 of the flat box of `tris` (the grid's outer edges), along x and y in its plane z = 0
    for face in (-1.0, 1.0):
        R.add_triples(2, np.stack([np.full(m, face), t, np.full(m, 2.0)], 1), (0, 0, -1.0), 0, 0)
        R.add_triples(2, np.stack([np.full(m, face), t, np.full(m, -2.0)], 1), (0, 0, 2.0), 0, 0)
    R.add_triples(2, np.stack([t, np.full(m, -1.0), np.full(m, 2.0)], 1), (0, 0, -1.0), 0, 1)
    R.add_triples(2, np.stack([np.full(m, -3.0), t, np.zeros(m)], 1), (1.0, 0, 0), 0, 2)
    R.add_triples(2, np.stack([t, np.full(m, 3.0), np.zeros(m)], 1), (0, -1.0, 0), 0, 2)
    R.add_triples(2, np.stack([t, t[::-1], np.zeros(m)], 1), (0, 1.0, 0), 0, 2)   # from inside the flat box
    # along an axis on the faces of the leaf boxes of the axis-aligned strands: x = px +- r (tangent to the segment: d2 == r * r too)
    p, r, lines = R.geo[0]["positions"].astype(np.float64), R.geo[0]["radius"].astype(np.float64), R.geo[0]["lines"]
    for first, ax in _AXIAL:
        for seg in range(first, first + 4):
            a, b = lines[seg]
            rmax = max(r[a], r[b])
            end = a if r[a] >= r[b] else b
            for e_ax in range(3):
                if e_ax == ax:
                    continue
                w_ax = 3 - ax - e_ax
                for sign in (1.0, -1.0):
                    e, w = np.zeros(3), np.zeros(3)
                    e[e_ax], w[w_ax] = sign, 1.0
                    R.add_triples(0, p[end] + rmax * e - 3 * w, w, seg, e_ax)
                    R.add_triples(0, p[end] + rmax * e + 3 * w, -2 * w, seg, e_ax)
    # tiny and denormal direction components beside components of order 1: 1 / d finite on one row, infinite on the next
    k = 120
    tgt, prim = _prim_points(R.geo[0], rng, k)
    big = _unit(rng.normal(size=(k, 3)))
    for comps in ((2.0 ** -126, 2.0 ** -127, 2.0 ** -128), (-2.0 ** -126, -2.0 ** -127, -2.0 ** -128), (1e-30, 2.0 ** -149, 0.0), (-1e-30, -2.0 ** -149, -0.0)):
        for ax in range(3):
            d = np.repeat(big, 3, 0)
            d[:, ax] = np.tile(np.array(comps), k)
            o = np.repeat(tgt, 3, 0) - 3 * np.where(np.abs(d) < 1e-20, 0, d)
            R.add(0, o, d, np.repeat(prim, 3), triples=True)
    tgt, prim = _prim_points(R.geo[2], rng, k)
    for comps in ((2.0 ** -126, 2.0 ** -127, 2.0 ** -128), (-1e-30, -2.0 ** -149, -0.0)):
        for ax in (0, 1):
            d = np.repeat(big, 3, 0)
            d[:, ax] = np.tile(np.array(comps), k)
            o = np.repeat(tgt, 3, 0) - 3 * np.where(np.abs(d) < 1e-20, 0, d)
            R.add(2, o, d, np.repeat(prim, 3), triples=True)
    # through a corner of the flat box so that the slabs meet in one point (t0 == t1 == 2), and a float beside it
    for cx, cy in ((1.0, -1.0), (-1.0, 1.0), (1.0, 1.25 + 1 / 1024), (-1.0, -1.0)):
        for dz in (0.25, -0.125, 0.5):
            d = np.array([cx, -cy if abs(cy) == 1 else -1.0, -dz])
            c = np.array([cx, cy, 0.0])
            R.add_triples(2, np.tile(c - 2 * d, (8, 1)), d, 0, 0)
            R.add_triples(2, np.tile(c - 2 * d, (8, 1)), d, 0, 1)


def _box_grazing(R, rng, m=120):
    """Rays along the faces of every object's world box, from two paddings outside to two inside (world space: object -1)."""
    boxes = world_boxes(R.geo)
    ident = dict(frame=np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32))
    R.geo = list(R.geo) + [ident]
    w = len(R.geo) - 1
    for k, (lo, hi) in enumerate(boxes):
        pad = 1e-3 * (hi - lo).max() + 1e-5
        for ax in range(3):
            for face, sgn in ((lo[ax], -1.0), (hi[ax], 1.0)):
                run = (ax + 1 + int(rng.integers(0, 2))) % 3
                o = rng.uniform(lo, hi, (m, 3))
                o[:, ax] = face + sgn * pad * np.linspace(2.0, -2.0, m)
                o[:, run] = lo[run] - 1.0
                d = np.zeros((m, 3))
                d[:, run] = 1.0
                d[:, 3 - ax - run] = rng.uniform(-0.2, 0.2, m) * (np.arange(m) % 2)
                R.add(w, o, d, -1)
    R.geo = R.geo[:-1]


def _todays_domain(geo):
    """Stratum a: random rays aimed at the objects from outside and from inside their boxes."""
    boxes = world_boxes(geo)
    rng = np.random.default_rng(101)
    R = _Rows(geo)
    per = N // len(geo) + 1
    for k, g in enumerate(geo):
        tgt, prim = _prim_points(g, rng, per, plain=True)
        f = g["frame"].astype(np.float64).reshape(4, 3)
        lo, hi = boxes[k]
        lo, hi = lo - 0.25 * (hi - lo < 0.1), hi + 0.25 * (hi - lo < 0.1)  # (a flat box: origins off its plane, the rays in it are stratum c's)
        wt = tgt @ f[:3] + f[3]
        outside = (lo + hi) / 2 + _unit(rng.normal(size=(per, 3))) * (hi - lo).max() * rng.uniform(1.0, 3.0, (per, 1))
        inside = rng.uniform(lo, hi, (per, 3))
        o = np.where(np.arange(per)[:, None] % 4 == 0, inside, outside)
        aim = wt + rng.normal(0, 0.3, (per, 3)) * (np.arange(per)[:, None] % 5 == 0)  # (one in five aimed loosely: misses and grazing hits)
        finv = np.linalg.inv(f[:3])
        R.add(k, (o - f[3]) @ finv, _unit(aim - o) @ finv, prim)
    return R.stratum()


@functools.lru_cache(maxsize=None)
def strata(variant):
    """name -> Stratum of N rays on hits-unit's `variant` (four, six, far)."""
    geo = make_scenes.hits_unit_geometry(variant)
    out = {"a": _todays_domain(geo)}
    # b - e
    for name, build in (("b", lambda R, rng: _segment_edges(R, 0, rng)), ("c", lambda R, rng: _triangle_edges(R, 2, rng)),
                        ("d", lambda R, rng: _range_edges(R, rng, False)), ("e", _box_edges)):
        R = _Rows(geo)
        build(R, np.random.default_rng(200 + ord(name)))
        out[name] = R.stratum()
    # f
    rng = np.random.default_rng(301)
    R = _Rows(geo)
    _box_grazing(R, rng)
    grazing = sum(len(r) for r in R.rays)
    others = [k for k in range(len(geo)) if k not in (0, 2) or variant == "far"]
    for k in others:
        Q = _Rows(geo)
        (_segment_edges if geo[k]["shape"] == "strands" else _triangle_edges)(Q, k, rng)
        rows = np.concatenate(Q.rays)
        keep = (N - grazing) // len(others) // 3  # an equal share of what the grazing rows leave, in whole triples, so that `on` keeps its neighbours
        t3 = np.sort(rng.choice(len(rows) // 3, min(len(rows) // 3, keep), replace=False))
        pick = (3 * t3[:, None] + np.arange(3)).ravel()
        R.rays.append(rows[pick]), R.triple.append(np.full(len(pick), -1)), R.obj.append(np.full(len(pick), k)), R.prim.append(np.concatenate(Q.prim)[pick])
    out["f"] = R.stratum()
    # g: 128 rows of b that hit by construction (on the edge, on the axis-aligned strands between their segments' ends: the twins' ties among them)
    b = out["b"]
    nax = 5 * 4 * 5 * 2 * 2 * 2 * 3  # the rows of b's first family (perpendicular distance exactly r)
    inner = np.isin((np.arange(N) // 24) % 5, (1, 2, 3))  # at s = 0.25, 0.5, 0.75 (an end of a strand lies on the shape's box: not every row there hits)
    cand = np.flatnonzero((np.arange(N) < nax) & (b.triple >= 0) & (np.arange(N) % 3 == 1) & inner)
    pick = cand[np.linspace(0, len(cand) - 1, 128).astype(int)]
    rays = np.repeat(b.rays[pick], 64, axis=0)
    late = np.arange(len(rays)) % 64 >= 48
    ax = np.abs(rays[:, 3:6]).argmin(1)  # (an axis the ray does not run along)
    moved = rays[np.arange(len(rays)), ax]
    rays[late, ax[late]] = np.nextafter(moved[late], np.where(np.arange(len(rays))[late] % 2 == 0, F(np.inf), F(-np.inf)))
    out["g"] = Stratum(rays, np.full(N, -1), np.repeat(b.object[pick], 64), np.repeat(b.prim[pick], 64))
    # h: from a point of one object to a point of another and on, both ways
    rng = np.random.default_rng(401)
    R = _Rows(geo + [dict(frame=np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32))])
    pairs = [(0, 2), (1, 3)] + ([(4, 5), (1, 5)] if len(geo) >= 6 else [])
    per = N // (2 * len(pairs)) + 1
    for a_, b_ in pairs:
        pa, _ = _prim_points(geo[a_], rng, per)
        pb, _ = _prim_points(geo[b_], rng, per)
        fa, fb = (geo[k]["frame"].astype(np.float64).reshape(4, 3) for k in (a_, b_))
        wa, wb = pa @ fa[:3] + fa[3], pb @ fb[:3] + fb[3]
        near = wa + (wb - wa) * rng.uniform(0.0, 0.05, (per, 1)) + rng.normal(0, 0.05, (per, 3))  # a target just behind the first hit
        aside = rng.normal(0, 0.04, (per, 3)) * (np.arange(per)[:, None] % 3 == 0)  # every third ray beside the first point: some miss it, some miss all
        d = _unit(near - wa + 1e-9)
        R.add(len(geo), wa + aside - 3 * d, d, -1)
        d = _unit(wa - wb + 1e-9)
        R.add(len(geo), wb + aside - 3 * d, d, -1)
    R.geo = geo
    out["h"] = R.stratum()
    for s in out.values():
        assert s.rays.shape == (N, 8) and np.isfinite(s.rays).all() and (s.rays[:, 6] == TMIN).all() and np.abs(s.rays[:, 3:6]).max(1).min() > 0
    return out


@functools.lru_cache(maxsize=None)
def quad_only(variant):
    """The rows with a tmin other than 1e-4f (stratum d's second half): for the quad forms only."""
    R = _Rows(make_scenes.hits_unit_geometry(variant))
    _range_edges(R, np.random.default_rng(501), True)
    s = R.stratum(sum(len(r) for r in R.rays))
    assert np.isfinite(s.rays).all()
    return s


def main_batch(variant):
    """The 65 536 rays of the eight strata, in order."""
    return np.concatenate([strata(variant)[k].rays for k in NAMES])


def where(row, names=NAMES):
    """'stratum x row r' of a row of main_batch (or, with DEEP_NAMES, of deep_rays)."""
    return f"stratum {names[row // N]} row {row % N}"


DEEP_NAMES = ("x", "a")
_CHAIN = 0  # the object `a-chain` of variant `deep`


@functools.lru_cache(maxsize=None)
def deep_rays():
    """The rays of tests/test_hits_deep.py on variant `deep` (the chain of make_scenes._hits_chain, then `four`): stratum x, N rays along
    and near +-x through the chain, then stratum a of the variant. The chain's segments lie on ONE line, its x axis, and the line
    test takes the ray's closest approach to that line: a ray through the chain's small end, the apex of the cone its boxes fill,
    enters every box and hits no segment. Near-first, it walks down to the smallest segment with the siblings of every level on the
    stack, on top of the ENTER entries of the objects that share the chain's leaf of the scene tree — and those objects, behind the
    chain, are where such a ray's hit is: it comes out of an entry that went through the overflow array. Origins and directions are
    dyadic with few bits, so the rays meet the apex exactly, in world space and in the chain's own."""
    geo = make_scenes.hits_unit_geometry("deep")
    rng = np.random.default_rng(601)
    R = _Rows(geo)
    m = N // 8
    nseg = make_scenes.HITS_CHAIN_SEGMENTS
    unit = 2.0 ** 19  # one world unit in the chain's own space
    col = lambda v: np.full((m, 1), v)  # noqa: E731
    slopes = lambda: rng.integers(-26, 27, (m, 2)) / 256  # noqa: E731  (the boxes fill a cone of slope 1 / 8 ... 1 / 10 about the x axis)
    # on the axis exactly, from before the small end along +x: parallel to every segment (det == 0), through every box
    R.add(_CHAIN, np.concatenate([-unit * 2.0 ** -rng.integers(0, 4, (m, 1)), np.zeros((m, 2))], 1), (1.0, 0, 0), 0)
    # through the apex from one world unit before it, inside the cone
    for _ in range(4):
        d = np.concatenate([col(1.0), slopes()], 1)
        R.add(_CHAIN, -unit * d, d, 0)
    # the same line the other way, from 16 world units beyond the apex: the large segments first, a shallow stack
    d = np.concatenate([col(1.0), slopes()], 1)
    R.add(_CHAIN, 16 * unit * d, -d, nseg - 1)
    # from inside the chain, on and beside the axis, both ways: these hit it
    k = rng.integers(0, nseg, m)
    x = 2.0 ** (k - 20.0) * rng.uniform(0.6, 1.4, m)
    for sign in (1.0, -1.0):
        R.add(_CHAIN, np.concatenate([x[:, None], x[:, None] * rng.uniform(-0.2, 0.2, (m, 2))], 1), np.concatenate([col(sign), rng.uniform(-0.15, 0.15, (m, 2))], 1), k)
    x_stratum = R.stratum()
    assert len(np.concatenate(R.rays)) == N
    rays = np.concatenate([x_stratum.rays, _todays_domain(geo).rays])
    assert rays.shape == (2 * N, 8) and np.isfinite(rays).all() and (rays[:, 6] == TMIN).all()
    return rays


TIES_NAMES = ("t",)
TIES_OBJECTS = {"stack": 4, "sheaf": 5, "plates": 6, "rungs": 7}  # variant `ties`: its shapes' objects, behind those of `four`
_SIGNS = np.array([[(-1.0) ** (k >> 2 & 1), (-1.0) ** (k >> 1 & 1), (-1.0) ** (k & 1)] for k in range(8)])
_MAGS = np.array([(1, 0.5, 0.25), (0.25, 1, 0.5), (0.5, 0.25, 1), (1, 1, 1), (1, 0.125, 0.75), (0.375, 1, 0.0625)])
_AXES6 = np.concatenate([np.eye(3), -np.eye(3)])


def _ties_segment(R, obj, p0, p1, r0, r1, prim, rng, n_general):
    """Strata b's families on one segment along an axis that is there many times: distance r exactly at dyadic s, the ends, and rays of
    every sign triple and along every axis through points of it."""
    p0, p1 = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    ax = int(np.abs(p1 - p0).argmax())
    for s in (0.0, 0.25, 0.5, 0.75, 1.0):
        c, rr = p0 * (1 - s) + p1 * s, r0 * (1 - s) + r1 * s
        for e_ax in range(3):
            if e_ax == ax:
                continue
            w_ax = 3 - ax - e_ax
            for sign in (1.0, -1.0):
                e, w = np.zeros(3), np.zeros(3)
                e[e_ax], w[w_ax] = sign, 1.0
                R.add_triples(obj, c + rr * e - 2 * w, w, prim, e_ax)
                R.add_triples(obj, c + rr * e + 1.5 * w, -w, prim, e_ax)
    d = (_SIGNS[:, None] * _MAGS[None]).reshape(-1, 3)
    for v in (p0, p1):  # through an end, moved along the segment: s crosses 0 or 1
        R.add_triples(obj, v - 2 * d, d, prim, ax)
    s = _dy(rng, 0, 1, (n_general, 1), 16)
    c = p0 * (1 - s) + p1 * s
    off = np.zeros((n_general, 3))
    off[:, (ax + 1) % 3] = _dy(rng, -8 / 1024, 8 / 1024, n_general, 1024)
    d = np.concatenate([d, _AXES6[np.abs(_AXES6[:, ax]) == 0]])[rng.integers(0, len(d) + 4, n_general)]
    R.add(obj, c + off - 2 * d, d, prim)


def _ties_rows(geo):
    rng = np.random.default_rng(701)
    R = _Rows(geo)
    ob = TIES_OBJECTS
    # the stack: one segment, 64 times
    _ties_segment(R, ob["stack"], (-0.5, 0, 0), (0.5, 0, 0), 24 / 1024, 16 / 1024, 1, rng, 700)
    # the sheaf: the joints and ends of a strand along z that is there six times
    z = [-1 + 0.5 * k for k in range(5)]
    rad = [20 / 1024, 16 / 1024, 12 / 1024, 8 / 1024, 4 / 1024]
    for k in range(4):
        _ties_segment(R, ob["sheaf"], (0, 0, z[k]), (0, 0, z[k + 1]), rad[k], rad[k + 1], k, rng, 120)
    # the plates: stratum c's families on one triangle that is there 32 times — vertices, points of its edges at dyadic parameters, inside
    v = np.array([(-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.0, 0.5, 0.0)])
    k = _dy(rng, 0, 1, (240, 1), 16)
    e = rng.integers(0, 3, 240)
    pts = np.concatenate([v, v[e] * (1 - k) + v[(e + 1) % 3] * k])
    u, w = _dy(rng, 0, 1, (400, 1), 64), _dy(rng, 0, 1, (400, 1), 64)
    flip = (u + w) > 1
    u, w = np.where(flip, 1 - u, u), np.where(flip, 1 - w, w)
    inside = v[0] * (1 - u - w) + v[1] * u + v[2] * w
    d = np.concatenate([(_SIGNS[:, None] * _MAGS[None]).reshape(-1, 3), [(0, 0, 1.0), (0, 0, -1.0)]])
    dd = d[rng.integers(0, len(d), len(pts))]
    R.add_triples(ob["plates"], pts - 2 * dd, dd, 0, rng.integers(0, 2, len(pts)))
    dd = d[rng.integers(0, len(d), len(inside))]
    R.add(ob["plates"], inside - 2 * dd, dd, 0)
    for vert in v[:2]:  # along z through a lower vertex: on a face of the shape's box in x, of the triangle's own box in x and y (0 * inf twice)
        for sz in (1.0, -1.0):
            for ax in (0, 1):
                R.add_triples(ob["plates"], np.tile(vert - (0, 0, 2 * sz), (4, 1)), (0, 0, sz), 0, ax)
                R.add_triples(ob["plates"], np.tile(vert - (0, 0, 2 * sz), (4, 1)), (0, 0, 2 * sz), 0, ax)
    small = np.array([(-0.25, -1.5, 0.0), (0.25, -1.5, 0.0), (0.0, -1.0, 0.0)])
    dd = d[rng.integers(0, len(d), 24)]
    R.add_triples(ob["plates"], small[rng.integers(0, 3, 24)] - 2 * dd, dd, 32, rng.integers(0, 2, 24))
    for dirn, o in (((1.0, 0, 0), (-2.0, 0, 0)), ((-1.0, 0, 0), (2.0, 0, 0)), ((0, 1.0, 0), (0, -2.0, 0)), ((0.5, -1.0, 0), (0, 2.0, 0))):  # in its plane: det == 0
        m = 20
        o = np.tile(np.array(o, np.float64), (m, 1))
        o[:, 1 if dirn[1] == 0 else 0] = _dy(rng, -0.5, 0.5, m, 32)
        R.add_triples(ob["plates"], o, dirn, 0, 2)
    # the rungs: across one site (+-z: its leaves alone) and along +-y through all four (every leaf of the shape on one line)
    for y, first in ((-3.0, 0), (-1.0, 4), (1.0, 12), (3.0, 21)):
        x = _dy(rng, -0.25, 0.25, (20, 1), 64)
        for sz in (1.0, -1.0):
            for sy in (1.0, -1.0):
                o = np.concatenate([x, np.full((20, 1), y + sy * 16 / 1024), np.full((20, 1), -2.0 * sz)], 1)
                R.add_triples(ob["rungs"], o, (0, 0, sz), first, 1)
        dd = (_SIGNS[:, None] * np.array([(0.5, 0.0625, 1), (1, 0.03125, 0.5), (0.25, 0.0625, 1)])[None]).reshape(-1, 3)
        R.add(ob["rungs"], np.array([0.0, y, 0.0]) - 2 * dd, dd, first)
    x = _dy(rng, -0.25, 0.25, (30, 1), 64)
    for sy in (1.0, -1.0):
        for zz in (0.0, 16 / 1024, -16 / 1024, 8 / 1024):
            R.add_triples(ob["rungs"], np.concatenate([x, np.full((30, 1), -5.0 * sy), np.full((30, 1), zz)], 1), (0, sy, 0), 0 if sy > 0 else 21, 2)
        for tilt in (0.03125, -0.03125):
            R.add(ob["rungs"], np.concatenate([x, np.full((30, 1), -5.0 * sy), np.zeros((30, 1))], 1), (tilt, sy, 0), 0 if sy > 0 else 21)
    # a finite tmax on the tie's t and its float neighbours: t = 2 and t = 1 by construction (the closest approach to the axis; the plane)
    x = _dy(rng, -0.5, 0.5, (40, 1), 64)
    rr = 24 / 1024 * (1 - (x + 0.5)) + 16 / 1024 * (x + 0.5)
    for sgn in (1.0, -1.0):
        o = np.concatenate([x, sgn * rr, np.full((40, 1), -2.0 * sgn)], 1)
        R.add_tmax_triples(ob["stack"], o, (0, 0, sgn), 1, 2.0)
        R.add_tmax_triples(ob["stack"], o, (0, 0, 2 * sgn), 1, 1.0)
        R.add_tmax_triples(ob["plates"], inside[:40] + (0, 0, 2.0 * sgn), (0, 0, -sgn), 0, 2.0)
        R.add_tmax_triples(ob["plates"], inside[40:80] + (0, 0, 2.0 * sgn), (0, 0, -2 * sgn), 0, 1.0)
        R.add_tmax_triples(ob["rungs"], np.concatenate([x[:, :1] / 2, np.full((40, 1), -5.0 * sgn), np.zeros((40, 1))], 1), (0, sgn, 0), 0 if sgn > 0 else 21, 2.0)
        R.add_tmax_triples(ob["rungs"], np.concatenate([x[:, :1] / 2, np.full((40, 1), -5.0 * sgn), np.zeros((40, 1))], 1), (0, sgn, 0), 4 if sgn > 0 else 12, 4.0)
    return R


@functools.lru_cache(maxsize=None)
def ties():
    """The Stratum of variant `ties` (four and the shapes of make_scenes._hits_ties): N rows that follow strata b and c onto primitives that
    are there many times over — at the ends, at distance r exactly, on edges and vertices, with both signs of every direction component
    and along every axis, and a slice with a finite tmax on the tie's t and its float neighbours. Every hit on such a primitive is a hit
    on each of its copies at the same t as bits, and the copies fill several leaves: who wins is the visiting order's to say."""
    R = _ties_rows(make_scenes.hits_unit_geometry("ties"))
    built = sum(len(r) for r in R.rays)
    assert N // 2 <= built <= N, built  # (every block as built; the rest repeats rows from the start)
    s = R.stratum()
    assert s.rays.shape == (N, 8) and np.isfinite(s.rays).all() and (s.rays[:, 6] == TMIN).all() and np.abs(s.rays[:, 3:6]).max(1).min() > 0
    return s


def ties_rays():
    return ties().rays


def wide_walk(slots, o, d):
    """The heights of the traversal stack while rays (o, d: (n, 3), the shape's own space) walk a 4-wide tree, yh_bvh_build_wide's
    `slots` (nodes, 4, 8), in the order of csrc/dev_lane.h: lane_step — of a node's hit slots the first in near-first order is
    walked next, the others are pushed so that they pop in that order; no hit shortens the ray, so every box on its line is entered.
    Returns, per ray, (the largest height, the height when the first leaf is reached: until then no device form has shortened the
    ray either)."""
    w = np.ascontiguousarray(slots).view(np.uint32)
    n = len(o)
    o, d = o.astype(np.float32), d.astype(np.float32)
    with np.errstate(all="ignore"):
        dinv = (np.float32(1) / d).astype(np.float32)
    sign = (dinv < 0).astype(np.int64)
    none, leaf = -1, -2
    cur, sp = np.zeros(n, np.int64), np.zeros(n, np.int64)
    stack = np.full((n, 4 * len(slots) + 4), none, np.int64)
    top, first = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    while ((cur != none) | (sp > 0)).any():
        pop = np.flatnonzero((cur == none) & (sp > 0))
        sp[pop] -= 1
        cur[pop] = stack[pop, sp[pop]]
        at_leaf = cur == leaf
        first = np.where(at_leaf & (first < 0), sp, first)
        cur[at_leaf] = none
        idx = np.flatnonzero(cur >= 0)
        if idx.size == 0:
            continue
        node = slots[cur[idx]].astype(np.float32)                      # (m, 4, 8)
        ref, axes = w[cur[idx], :, 6].astype(np.int64), w[cur[idx], 0, 7].astype(np.int64)
        with np.errstate(all="ignore"):
            ta = (node[:, :, 0:3] - o[idx, None]) * dinv[idx, None]
            tb = (np.stack([node[:, :, 3], node[:, :, 4], node[:, :, 5]], -1) - o[idx, None]) * dinv[idx, None]
            t0 = np.fmax(np.fmin(ta, tb).max(-1), TMIN)
            t1 = np.fmax(ta, tb).min(-1) * np.float32(1.00000024)
        hm = (t0 <= t1) & (ref != 0xFFFFFFFF)
        sg = lambda a: np.take_along_axis(sign[idx], (a & 3)[:, None], 1)[:, 0]  # noqa: E731
        s0, sg0, sg1 = sg(axes), sg(axes >> 2), sg(axes >> 4)
        r = np.arange(4)[None]
        pair = (r >> 1) ^ s0[:, None]
        vq = (pair << 1) | ((r & 1) ^ np.where(pair == 1, sg1[:, None], sg0[:, None]))
        vh, vref = np.take_along_axis(hm, vq, 1), np.take_along_axis(ref, vq, 1)
        vref = np.where(vref & 0x80000000, leaf, vref)
        before = np.cumsum(vh, 1) - vh                                  # hits visited before slot r
        nxt = np.full(len(idx), none, np.int64)
        for k in (3, 2, 1, 0):
            nxt = np.where(vh[:, k] & (before[:, k] == 0), vref[:, k], nxt)
        for k in (3, 2, 1):                                             # the last visited lies deepest
            put = idx[vh[:, k] & (before[:, k] >= 1)]
            stack[put, sp[put]] = vref[vh[:, k] & (before[:, k] >= 1), k]
            sp[put] += 1
        cur[idx] = nxt
        top = np.maximum(top, sp)
    return top, first


_AXES_AT = (0, 2, 6, 14)  # host/bvh_build.cpp: bit offset of the axes of the binary nodes at each level below a wide node's root


def wide_walk_any(slots, o, d):
    """wide_walk for yh_bvh_build_wide's `slots` (nodes, width, 8) at width 4, 8 or 16, with the rank rules of csrc/dev_trace.h: slot o is
    the path of sides s1 s2 .. from the wide node's root, and its place in the visiting order is those bits, each flipped when the ray
    runs against the axis of the binary node it was taken at (two, three or four near / far decisions from the axes word). Returns per
    ray (the largest height, the height at the first leaf, the leaf entries on top of the stack at the first leaf, whether a node entry
    ends that run: else the bottom of the stack does)."""
    width = slots.shape[1]
    levels = {4: 2, 8: 3, 16: 4}[width]
    w = np.ascontiguousarray(slots).view(np.uint32)
    n = len(o)
    o, d = o.astype(np.float32), d.astype(np.float32)
    with np.errstate(all="ignore"):
        dinv = (np.float32(1) / d).astype(np.float32)
    sign = (dinv < 0).astype(np.int64)
    none, leaf = -1, -2
    cur, sp = np.zeros(n, np.int64), np.zeros(n, np.int64)
    stack = np.full((n, width * len(slots) + width), none, np.int64)
    top, first = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    run, under = np.zeros(n, np.int64), np.zeros(n, bool)
    slot = np.arange(width)
    while ((cur != none) | (sp > 0)).any():
        pop = np.flatnonzero((cur == none) & (sp > 0))
        sp[pop] -= 1
        cur[pop] = stack[pop, sp[pop]]
        at_leaf = cur == leaf
        for i in np.flatnonzero(at_leaf & (first < 0)):  # the stack as a leaf group finds it
            k = 0
            while k < sp[i] and stack[i, sp[i] - 1 - k] == leaf:
                k += 1
            run[i], under[i] = k, k < sp[i]
        first = np.where(at_leaf & (first < 0), sp, first)
        cur[at_leaf] = none
        idx = np.flatnonzero(cur >= 0)
        if idx.size == 0:
            continue
        node = slots[cur[idx]].astype(np.float32)                      # (m, width, 8)
        ref, axes = w[cur[idx], :, 6].astype(np.int64), w[cur[idx], 0, 7].astype(np.int64)
        with np.errstate(all="ignore"):
            ta = (node[:, :, 0:3] - o[idx, None]) * dinv[idx, None]
            tb = (np.stack([node[:, :, 3], node[:, :, 4], node[:, :, 5]], -1) - o[idx, None]) * dinv[idx, None]
            t0 = np.fmax(np.fmin(ta, tb).max(-1), TMIN)
            t1 = np.fmax(ta, tb).min(-1) * np.float32(1.00000024)
        hm = (t0 <= t1) & (ref != 0xFFFFFFFF)
        rank = np.zeros((len(idx), width), np.int64)
        for j in range(levels):  # level j: the node reached by the first j sides of the slot's path
            path = slot >> (levels - j) if j else np.zeros(width, np.int64)
            ax = (axes[:, None] >> (_AXES_AT[j] + 2 * path[None])) & 3
            near = np.take_along_axis(sign[idx], ax, 1)
            rank |= (((slot >> (levels - 1 - j)) & 1)[None] ^ near) << (levels - 1 - j)
        order = np.argsort(rank, 1)                                     # order[:, k]: the slot visited k-th
        vh, vref = np.take_along_axis(hm, order, 1), np.take_along_axis(ref, order, 1)
        vref = np.where(vref & 0x80000000, leaf, vref)
        before = np.cumsum(vh, 1) - vh
        nxt = np.full(len(idx), none, np.int64)
        for k in range(width - 1, -1, -1):
            nxt = np.where(vh[:, k] & (before[:, k] == 0), vref[:, k], nxt)
        for k in range(width - 1, 0, -1):                               # the last visited lies deepest
            m = vh[:, k] & (before[:, k] >= 1)
            put = idx[m]
            stack[put, sp[put]] = vref[m, k]
            sp[put] += 1
        cur[idx] = nxt
        top = np.maximum(top, sp)
    return top, first, run, under


def primitive_form(variant, name):
    """Strata b - e at primitive level: the rows aimed at a primitive of an identity-frame object as (rays, p0, p1, r0, r1) for the
    segments, (rays, p0, p1, p2) for the triangles, and (rays, boxes) for both: the primitive's box and the shape's."""
    geo = make_scenes.hits_unit_geometry(variant)
    s = strata(variant)[name]
    seg = np.flatnonzero((s.object == 0) & (s.prim >= 0))
    tri = np.flatnonzero((s.object == 2) & (s.prim >= 0))
    g0, g2 = geo[0], geo[2]
    l, t = g0["lines"][s.prim[seg]], g2["triangles"][s.prim[tri]]
    lines = (s.rays[seg], g0["positions"][l[:, 0]], g0["positions"][l[:, 1]], g0["radius"][l[:, 0]], g0["radius"][l[:, 1]])
    tris = (s.rays[tri], g2["positions"][t[:, 0]], g2["positions"][t[:, 1]], g2["positions"][t[:, 2]])
    rmax = np.maximum(lines[3], lines[4])[:, None]
    bl = np.concatenate([np.minimum(lines[1], lines[2]) - rmax, np.maximum(lines[1], lines[2]) + rmax], 1)
    bt = np.concatenate([np.minimum(np.minimum(tris[1], tris[2]), tris[3]), np.maximum(np.maximum(tris[1], tris[2]), tris[3])], 1)
    whole = lambda g, n: np.tile(np.concatenate([(g["positions"] - g["radius"][:, None]).min(0), (g["positions"] + g["radius"][:, None]).max(0)]), (n, 1))  # noqa: E731
    boxes = (np.concatenate([lines[0], tris[0], lines[0], tris[0]]), np.concatenate([bl, bt, whole(g0, len(seg)), whole(g2, len(tri))]).astype(np.float32))
    return lines, tris, boxes


_ORACLE = {}


def oracle_hits(variant, yh, oracle, scene_path):
    """The oracle's (object, element, uv, distance) on main_batch and on quad_only of a variant: computed once per session, read by
    every test that needs them."""
    if variant not in _ORACLE:
        sf = yh.SceneFile(scene_path("hits-unit", variant=variant))
        osc = oracle.scene(sf.desc)
        if variant == "deep":  # (one batch: deep_rays)
            _ORACLE[variant] = (osc.intersect(deep_rays()),)
        elif variant == "ties":  # (one batch: ties_rays)
            _ORACLE[variant] = (osc.intersect(ties_rays()),)
        else:
            _ORACLE[variant] = (osc.intersect(main_batch(variant)), osc.intersect(quad_only(variant).rays))
        osc.close(), sf.close()
    return _ORACLE[variant]
