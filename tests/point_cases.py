"""The scenes and the input strata of the unit-level shading-point tests (tests/test_point_unit.py) and of their golden vectors
(oracle/make_golden.py: points_unit.npz): two scenes built in memory over the same geometry — PLAIN (every material diffuse or hair,
no texture, no map: launch shape 0 runs the LDS and fetch-first path) and GENERAL (textures, maps, volumes) — and per stratum ROWS
rows (object, element, uv, outgoing) with fixed seeds. numpy only; `Scene.desc(yh)` makes the yh_scene_desc and the map table.

Shapes: grid_nt (triangles; unnormalised vertex normals; texcoords over [-1.5, 2.5]), grid_n (normals only), grid_t (texcoords only, a
zero-area triangle among them), grid_0 (neither; a zero-area triangle), strands (lines with tangents, radius and texcoords), strands_0
(lines with nothing), special (hand-made triangles under an identity frame: vertex normals that cancel, degenerate, zero, mirrored
and unit uv mappings, an axis-aligned flat triangle), tctable (triangles whose VERTEX texcoords are the special values: a row at a
vertex, uv in {(0, 0), (1, 0), (0, 1)}, gets that texcoord exactly), light (two triangles), strand_axis (segments along x with
tangent (1, 0, 0) exactly). Frames: identity, rigid, scaled and sheared, mirrored (negative determinant).

Textures (1-based, Scene.tex): float 1x1, 1x7, 5x3, 32x32 (texels above 1); byte 1x1, 1x7, 5x3, 32x32 (bytes 0, 10, 11, 255 among them:
10 and 11 straddle the sRGB knee at 0.04045); `nmb` a byte normal map; `nmf` a float one; `nm0` the float 1x1 texel (0.5, 0.5, 0.5)
(nm = 0); `fop` float values around 0.999; `brz` bytes with a block of zeros (roughness 0: a delta mixture); `ftiny` float colours
down to 1e-6 (the density's 1e-4 clamp).

Strata:
  a  today's domain: the hits the oracle finds for random rays aimed at the objects, outgoing = -d (the nm0 object is left out: its
     shading normal is the normalisation of rounding noise away from its exact rows)
  b  uv edges: u, v in {0, 1, 1 - 2^-24, 2^-149, 1e-40}, u + v = 1, lines at u in {0, 1} and v in {0, 1}
  c  texcoords: tctable under every texture size and both lookups at its vertices (texel boundaries k/w, integers, +-1, -0,
     negative values, -1e-9 ... -6e-8 (s + sx rounds to sx), +-1e6) and inside; shapes without texcoords under textures
  d  normals: vertex normals that cancel at the hit (exactly, and nearly), unnormalised normals, the zero-area triangles, the
     sheared and the mirrored frame
  e  the rule: thin and closed, facing and facing away, dot(n, outgoing) exactly 0 (and -0), a strand with outgoing parallel to its
     tangent, outgoing of length 0.5 and 3
  f  normal maps: with and without texcoords (zero tangents), div == 0, both signs of flip_v, the zero texel, a line shape
  g  scalar maps and textures: opacity x mean around 0.999, on hair, roughness maps with 0, transmission x the emission texture's
     linear x, specular and metallic maps, colour x texture, emission x texture, the scattering texture, the density at its clamp
"""
import ctypes as C
import types

import numpy as np

ROWS = 2048
GOLDEN_ROWS = 512
F = np.float32
BELOW1 = np.nextafter(F(1), F(0))
STRATA = "abcdefg"
SEEDS = {s: 4100 + k for k, s in enumerate(STRATA)}
UV_EDGES = np.array([0, 1, BELOW1, 2.0 ** -149, 1e-40], F)


def unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


# ---------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------
def _grid(rng, k, normals, texcoords, zero_area=False):
    """A k x k patch of 2 k^2 triangles over [-1, 1]^2, bent a little."""
    g = np.linspace(-1, 1, k + 1)
    x, y = np.meshgrid(g, g, indexing="ij")
    pos = np.stack([x.ravel(), y.ravel(), 0.25 * np.sin(2 * x.ravel()) * np.cos(1.5 * y.ravel())], axis=1)
    idx = lambda i, j: i * (k + 1) + j  # noqa: E731
    tris = [t for i in range(k) for j in range(k) for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))]
    s = dict(pos=pos.astype(F), tris=np.array(tris, np.int32), lines=None, rad=None, nrm=None, tc=None)
    if zero_area:  # the last triangle names one vertex twice
        s["tris"][-1, 2] = s["tris"][-1, 1]
    if normals:  # the surface's normal, tilted, of length 0.5 to 3
        n = unit(np.stack([-0.5 * np.cos(2 * pos[:, 0]) * np.cos(1.5 * pos[:, 1]), 0.375 * np.sin(2 * pos[:, 0]) * np.sin(1.5 * pos[:, 1]), np.ones(len(pos))], axis=1))
        s["nrm"] = (unit(n + rng.normal(0, 0.1, n.shape)) * rng.uniform(0.5, 3, (len(n), 1))).astype(F)
    if texcoords:
        s["tc"] = (np.stack([x.ravel(), y.ravel()], axis=1) * 2 + 0.5 + rng.normal(0, 0.02, (len(pos), 2))).astype(F)
    return s


def _strands(rng, count, per, full):
    pos, lines, nrm = [], [], []
    for c in range(count):
        p = np.cumsum(np.concatenate([rng.uniform(-1, 1, (1, 3)) * [1, 1, 0.3], rng.normal(0, 0.12, (per, 3)) + [0, 0.15, 0]]), axis=0)
        base = len(pos)
        pos += list(p)
        t = np.gradient(p, axis=0)
        nrm += list(unit(t) * rng.uniform(0.5, 2, (len(p), 1)))
        lines += [(base + i, base + i + 1) for i in range(per)]
    pos = np.array(pos, F)
    s = dict(pos=pos, tris=None, lines=np.array(lines, np.int32), rad=None, nrm=None, tc=None)
    if full:
        s["nrm"], s["rad"] = np.array(nrm, F), rng.uniform(0.01, 0.03, len(pos)).astype(F)
        s["tc"] = rng.uniform(-1, 2, (len(pos), 2)).astype(F)
    return s


# the triangles of `special` (identity frame): name -> element
SPECIAL = dict(cancel=0, uv_same=1, uv_zero=2, uv_unit=3, uv_mirror=4, flat=5, tilted=6, uv_corner=7)


def _special():
    pos, nrm, tc, tris = [], [], [], []

    def tri(p, n, t):
        b = len(pos)
        pos.extend(p), nrm.extend(n), tc.extend(t), tris.append((b, b + 1, b + 2))

    z = (0, 0, 1)
    tri([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 0, 1), (0, 0, -1), (0, 1, 0)], [(0, 0), (1, 0), (0, 1)])       # cancel: 0.5 n0 + 0.5 n1 = 0
    tri([(2, 0, 0), (3, 0, 0), (2, 1, 0)], [z, z, z], [(0.25, 0.75)] * 3)                                        # uv_same: div == 0
    tri([(4, 0, 0), (5, 0, 0), (4, 1, 0)], [z, z, z], [(0, 0)] * 3)                                              # uv_zero: texcoord 0 exactly
    tri([(0, 2, 0), (1, 2, 0), (0, 3, 0)], [z, z, z], [(0, 0), (1, 0), (0, 1)])                                  # uv_unit
    tri([(2, 2, 0), (3, 2, 0), (2, 3, 0)], [z, z, z], [(0, 0), (0, 1), (1, 0)])                                  # uv_mirror: the other flip_v
    tri([(4, 2, 0), (5, 2, 0), (4, 3, 0)], [z, z, z], [(0.1, 0.2), (0.9, 0.3), (0.2, 0.8)])                      # flat: n = +z exactly
    tri([(0, 4, 0.2), (1, 4, 0), (0, 5, 0.4)], [(0.3, 0.1, 1), (-0.2, 0.2, 2), (0.1, -0.3, 0.7)], [(-0.4, 0.3), (1.3, 0.1), (0.2, 1.6)])  # tilted
    tri([(2, 4, 0), (3, 4, 0), (2, 5, 0)], [z, z, z], [(3, -2), (4, -2), (3, -1)])                               # uv_corner: integers at the vertices
    return dict(pos=np.array(pos, F), nrm=np.array(nrm, F), tc=np.array(tc, F), tris=np.array(tris, np.int32), lines=None, rad=None)


# what the vertices of tctable carry (each value as u and as v of some vertex)
TC_VALUES = np.array(
    [k / 32 for k in (0, 1, 16, 31, 32, 33)] + [k / 5 for k in range(1, 5)] + [k / 3 for k in (1, 2)] + [k / 7 for k in range(1, 7)]
    + [0, 1, -1, 2, -0.0, -0.3, -2.75, -0.999999, -1e-9, -1e-8, -3e-8, -6e-8, -1e-38, 1e6, -1e6, 1000000.375, -1000000.375, 0.5, 0.999999], F)


def _tctable():
    m = len(TC_VALUES)
    pos, tc, tris = [], [], []
    for k in range(m):  # triangle k: texcoords (a, b), (b, c), (c, a) of three consecutive values
        a, b, c = TC_VALUES[k], TC_VALUES[(k + 7) % m], TC_VALUES[(k + 19) % m]
        x, y = 1.2 * (k % 7), 1.2 * (k // 7)
        base = len(pos)
        pos += [(x, y, 0), (x + 1, y, 0.1), (x, y + 1, 0.2)]
        tc += [(a, b), (b, c), (c, a)]
        tris.append((base, base + 1, base + 2))
    return dict(pos=np.array(pos, F) * F(0.3), tc=np.array(tc, F), tris=np.array(tris, np.int32), nrm=None, lines=None, rad=None)


def _light():
    return dict(pos=np.array([(-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1)], F), tris=np.array([(0, 1, 2), (0, 2, 3)], np.int32), nrm=None, tc=None, lines=None, rad=None)


def _strand_axis():
    pos = np.array([(k, 0, 0) for k in range(5)], F)
    return dict(pos=pos, lines=np.array([(k, k + 1) for k in range(4)], np.int32), nrm=np.tile(np.array([[1, 0, 0]], F), (5, 1)), rad=np.full(5, 0.05, F),
                tc=None, tris=None)


SHAPES = ["grid_nt", "grid_n", "grid_t", "grid_0", "strands", "strands_0", "special", "tctable", "light", "strand_axis"]


def _shapes():
    rng = np.random.default_rng(4000)
    return [_grid(rng, 6, True, True), _grid(rng, 4, True, False), _grid(rng, 4, False, True, zero_area=True), _grid(rng, 3, False, False, zero_area=True),
            _strands(rng, 8, 5, True), _strands(rng, 5, 4, False), _special(), _tctable(), _light(), _strand_axis()]


def _rot(axis, angle):
    a = unit(np.asarray(axis, np.float64))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _frame(kind, origin):
    """12 floats x, y, z, o (the columns of the matrix, then the origin)."""
    if kind == "identity":
        M = np.eye(3)
    elif kind == "rigid":
        M = _rot((1, 2, 3), 0.7)
    elif kind == "sheared":
        M = _rot((3, 1, 2), -0.4) @ np.array([[1.5, 0.4, 0], [0, 0.6, 0.3], [0, 0, 1.2]])
    else:  # mirrored: negative determinant
        M = _rot((2, 3, 1), 1.1) @ np.diag([1.0, -0.8, 1.3])
    return np.concatenate([M.T.reshape(-1), np.asarray(origin, np.float64)]).astype(F)


# ---------------------------------------------------------------------------------------------------------------
# textures
# ---------------------------------------------------------------------------------------------------------------
def _textures():
    """(the textures, name -> 1-based index)."""
    rng = np.random.default_rng(4001)
    out, index = [], {}

    def add(name, px, is_byte):
        out.append(dict(name=name, w=px.shape[1], h=px.shape[0], is_byte=is_byte, px=np.ascontiguousarray(px, np.uint8 if is_byte else F)))
        index[name] = len(out)

    for w, h in ((1, 1), (1, 7), (5, 3), (32, 32)):
        add(f"f{w}x{h}", rng.uniform(0, 1, (h, w, 3)) ** 2 * 2.5, False)  # up to 2.5
    key = np.array([0, 10, 11, 255], np.uint8)
    for w, h in ((1, 1), (1, 7), (5, 3), (32, 32)):
        px = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        flat = px.reshape(-1)
        flat[:: 5] = key[np.arange(len(flat[:: 5])) % 4]
        if w == 1 and h == 1:
            flat[:] = [11, 10, 255]
        add(f"b{w}x{h}", px, True)
    n = unit(np.stack([rng.normal(0, 0.35, (32, 32)), rng.normal(0, 0.35, (32, 32)), np.ones((32, 32))], axis=2))
    add("nmb", np.clip(np.round((n * 0.5 + 0.5) * 255), 0, 255), True)
    n = unit(np.stack([rng.normal(0, 0.5, (3, 5)), rng.normal(0, 0.5, (3, 5)), np.ones((3, 5))], axis=2))
    add("nmf", n * 0.5 + 0.5, False)
    add("nm0", np.full((1, 1, 3), 0.5), False)
    add("fop", np.repeat(0.999 + rng.choice([-1, 1], (3, 5, 1)) * rng.uniform(2e-5, 6e-4, (3, 5, 1)), 3, axis=2), False)
    px = rng.integers(1, 256, (3, 5, 1)).astype(np.uint8)
    px[:, :3] = 0
    add("brz", np.repeat(px, 3, axis=2), True)
    add("ftiny", 10 ** rng.uniform(-6, 0, (3, 5, 3)), False)
    return out, index


# ---------------------------------------------------------------------------------------------------------------
# materials, objects, scenes
# ---------------------------------------------------------------------------------------------------------------
MAT_DEFAULT = dict(emission=(0, 0, 0), color=(0.5, 0.5, 0.5), specular=0.0, metallic=0.0, roughness=1.0, transmission=0.0, opacity=1.0, ior=1.5, thin=0,
                   sigma_a=(0, 0, 0), beta_m=0.3, beta_n=0.3, alpha=2.0, eta=1.55, eumelanin=0.0, pheomelanin=0.0, scattering=(0, 0, 0), scanisotropy=0.0,
                   trdepth=0.01, emission_tex=0, color_tex=0, scattering_tex=0)
MAP_KEYS = ("specular_tex", "metallic_tex", "roughness_tex", "transmission_tex", "opacity_tex", "normal_tex")

# (object name, shape, frame, material in the general scene, material in the plain scene)
OBJECTS = [
    ("main", "grid_nt", "rigid", "spec_ctex", "closed"), ("metal", "grid_nt", "sheared", "metal_maps", "thin"),
    ("trans", "grid_nt", "mirrored", "thin_trans", "closed"), ("plain_n", "grid_n", "rigid", "closed", "closed"),
    ("plain_t", "grid_t", "sheared", "thin", "thin"), ("bare", "grid_0", "mirrored", "thin_spec", "thin"),
    ("hair", "strands", "rigid", "hair_op", "hair"), ("hair_0", "strands_0", "sheared", "hair", "hair2"),
    ("special", "special", "identity", "nmapped", "closed"), ("special_thin", "special", "identity", "thin", "thin"),
    ("special_nmf", "special", "identity", "thin_nmf", "black"), ("special_nm0", "special", "identity", "nm_zero", "closed"),
    ("no_tc_nm", "grid_n", "sheared", "nm_notc", "thin"), ("hair_nm", "strands", "mirrored", "hair_nm", "hair2"),
    ("volume", "grid_nt", "rigid", "volume", "closed"), ("opacity", "grid_nt", "rigid", "op_straddle", "thin"),
    ("rough0", "grid_nt", "sheared", "rough_zero", "closed"), ("light", "light", "rigid", "emit", "emit"),
    ("axis", "strand_axis", "identity", "hair", "hair"), ("bare_tex", "grid_0", "rigid", "ctex_notc", "closed"),
] + [(f"tc{k}", "tctable", "identity", f"tc{k}", "closed") for k in range(8)]
FRAGILE = ("special_nm0",)  # left out of stratum a
OBJ = {o[0]: i for i, o in enumerate(OBJECTS)}


def _materials(T):
    """name -> (yh_material fields, yh_material_maps fields); T: texture name -> 1-based index."""
    m = {
        "closed": (dict(color=(0.7, 0.4, 0.2)), {}),
        "thin": (dict(color=(0.2, 0.6, 0.3), thin=1), {}),
        "black": (dict(color=(0, 0, 0), thin=1), {}),
        "emit": (dict(color=(0.3, 0.3, 0.3), emission=(4, 3, 2.5)), {}),
        "hair": (dict(color=(0.6, 0.4, 0.2), thin=1), {}),
        "hair2": (dict(color=(0, 0, 0), sigma_a=(0.3, 0.5, 1.1), beta_m=0.6, thin=1), {}),
        "spec_ctex": (dict(color=(0.8, 0.7, 0.6), specular=0.5, roughness=0.3, color_tex=T["f32x32"]), dict(specular_tex=T["b5x3"])),
        "metal_maps": (dict(color=(0.9, 0.6, 0.3), metallic=0.7, roughness=0.6, color_tex=T["b32x32"]), dict(metallic_tex=T["b32x32"], roughness_tex=T["b5x3"])),
        "thin_trans": (dict(color=(0.5, 0.8, 0.9), thin=1, transmission=0.6, roughness=0.2, specular=0.3, emission=(1, 2, 3), emission_tex=T["b32x32"]), {}),
        "thin_spec": (dict(color=(0.4, 0.4, 0.7), thin=1, specular=0.3, roughness=0.4), {}),
        "hair_op": (dict(color=(0.5, 0.3, 0.1), thin=1, opacity=0.9), dict(opacity_tex=T["b32x32"])),
        "hair_nm": (dict(color=(0.3, 0.3, 0.5), thin=1, opacity=1.0), dict(opacity_tex=T["fop"], normal_tex=T["nmb"])),
        "nmapped": (dict(color=(0.6, 0.6, 0.6), specular=0.2, roughness=0.5), dict(normal_tex=T["nmb"])),
        "thin_nmf": (dict(color=(0.6, 0.5, 0.4), thin=1, specular=0.1, roughness=0.5), dict(normal_tex=T["nmf"])),
        "nm_zero": (dict(color=(0.5, 0.5, 0.5)), dict(normal_tex=T["nm0"])),
        "nm_notc": (dict(color=(0.5, 0.6, 0.7), thin=1, color_tex=T["f5x3"]), dict(normal_tex=T["nmb"])),
        "volume": (dict(color=(0.9, 0.8, 0.7), transmission=0.8, roughness=0.1, specular=0.4, scattering=(0.7, 0.5, 0.3), scanisotropy=0.3, trdepth=0.1,
                        color_tex=T["ftiny"], scattering_tex=T["b5x3"], emission_tex=T["f1x7"], emission=(0.2, 0.1, 0.3)), {}),
        "op_straddle": (dict(color=(0.7, 0.7, 0.2), opacity=1.0), dict(opacity_tex=T["fop"])),
        "rough_zero": (dict(color=(0.9, 0.5, 0.5), metallic=1.0, roughness=0.8), dict(roughness_tex=T["brz"])),
        "ctex_notc": (dict(color=(0.9, 0.9, 0.9), color_tex=T["b1x7"], emission=(1, 1, 1), emission_tex=T["f5x3"]), dict(specular_tex=T["f1x1"])),
    }
    sizes = ["f1x1", "f1x7", "f5x3", "f32x32", "b1x1", "b1x7", "b5x3", "b32x32"]
    for k, name in enumerate(sizes):  # both lookups of every size: colour and emission decoded, the emission's x and the specular map linear
        m[f"tc{k}"] = (dict(color=(0.8, 0.9, 0.7), specular=0.6, roughness=0.5, thin=1, transmission=0.3, emission=(0.5, 1.0, 1.5), color_tex=T[name],
                            emission_tex=T[name]), dict(specular_tex=T[name]))
    return m


class Scene:
    def __init__(self, general):
        self.general = general
        self.shapes = _shapes()
        self.textures, self.tex = _textures()
        mats = _materials(self.tex)
        names = []
        self.objects = []
        for i, (oname, shape, frame, gmat, pmat) in enumerate(OBJECTS):
            mat = gmat if general else pmat
            if mat not in names:
                names.append(mat)
            origin = (6.0 * (i % 6), 6.0 * (i // 6), 0.5 * (i % 3))
            self.objects.append(dict(name=oname, frame=_frame(frame, origin), shape=SHAPES.index(shape), material=names.index(mat), frame_kind=frame))
        self.material_names = names
        self.materials = [{**MAT_DEFAULT, **mats[n][0]} for n in names]
        self.maps = [{**{k: 0 for k in MAP_KEYS}, **mats[n][1]} for n in names]
        lo, hi = self.bbox()
        self.diagonal = float(np.linalg.norm(hi - lo))
        self._keep = None

    def bbox(self):
        pts = np.concatenate([self.world(o, self.shapes[o["shape"]]["pos"].astype(np.float64)) for o in self.objects])
        return pts.min(axis=0), pts.max(axis=0)

    @staticmethod
    def world(o, p):
        f = o["frame"].astype(np.float64)
        return p[:, 0:1] * f[0:3] + p[:, 1:2] * f[3:6] + p[:, 2:3] * f[6:9] + f[9:12]

    def num_elements(self, obj):
        s = self.shapes[self.objects[obj]["shape"]]
        return len(s["lines"] if s["lines"] is not None else s["tris"])

    def is_lines(self, obj):
        return self.shapes[self.objects[obj]["shape"]]["lines"] is not None

    def desc(self, yh):
        """(pointer to yh_scene_desc, the yh_material_maps table or None); the arrays live as long as this Scene."""
        if self._keep is None:
            fp, ip = yh.c_float_p, yh.c_int_p
            shapes = (yh.Shape * len(self.shapes))()
            for d, s in zip(shapes, self.shapes):
                d.num_vertices, d.positions = len(s["pos"]), s["pos"].ctypes.data_as(fp)
                d.normals = s["nrm"].ctypes.data_as(fp) if s["nrm"] is not None else None
                d.radius = s["rad"].ctypes.data_as(fp) if s["rad"] is not None else None
                d.texcoords = s["tc"].ctypes.data_as(fp) if s["tc"] is not None else None
                if s["lines"] is not None:
                    d.num_lines, d.lines = len(s["lines"]), s["lines"].ctypes.data_as(ip)
                else:
                    d.num_triangles, d.triangles = len(s["tris"]), s["tris"].ctypes.data_as(ip)
            mats = (yh.Material * len(self.materials))()
            for d, m in zip(mats, self.materials):
                for k, v in m.items():
                    if isinstance(v, tuple):
                        getattr(d, k)[:] = [float(x) for x in v]
                    else:
                        setattr(d, k, v)
            maps = (yh.MaterialMaps * len(self.maps))()
            for d, m in zip(maps, self.maps):
                for k, v in m.items():
                    setattr(d, k, v)
            objs = (yh.Object * len(self.objects))()
            for d, o in zip(objs, self.objects):
                d.frame[:] = o["frame"].tolist()
                d.shape, d.material = o["shape"], o["material"]
            texs = (yh.Texture * len(self.textures))()
            for d, t in zip(texs, self.textures):
                d.width, d.height, d.is_byte, d.pixels = t["w"], t["h"], int(t["is_byte"]), t["px"].ctypes.data
            envs = (yh.Environment * 1)()
            envs[0].frame[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
            envs[0].emission[:] = [0.5, 0.5, 0.5]
            sd = yh.SceneDesc()
            sd.num_shapes, sd.shapes = len(shapes), C.cast(shapes, C.POINTER(yh.Shape))
            sd.num_materials, sd.materials = len(mats), C.cast(mats, C.POINTER(yh.Material))
            sd.num_objects, sd.objects = len(objs), C.cast(objs, C.POINTER(yh.Object))
            sd.num_environments, sd.environments = 1, C.cast(envs, C.POINTER(yh.Environment))
            sd.num_textures, sd.textures = len(texs), C.cast(texs, C.POINTER(yh.Texture))
            sd.camera.frame[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1, 15, 10, 60]
            sd.camera.lens, sd.camera.film[0], sd.camera.film[1], sd.camera.focus, sd.camera.aperture = 0.05, 0.036, 0.036, 60.0, 0.0
            self._keep = (sd, shapes, mats, maps, objs, texs, envs)
        sd, maps = self._keep[0], self._keep[3]
        return C.pointer(sd), (maps if self.general else None)


_SCENES = {}


def scene(general):
    if general not in _SCENES:
        _SCENES[general] = Scene(general)
    return _SCENES[general]


# ---------------------------------------------------------------------------------------------------------------
# strata
# ---------------------------------------------------------------------------------------------------------------
def _uv(rng, n, lines):
    """Uniform on the triangle (u + v <= 1), or on [0, 1]^2 for a line."""
    u, v = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    if not lines:
        over = u + v > 1
        u, v = np.where(over, 1 - u, u), np.where(over, 1 - v, v)
    return np.stack([u, v], axis=1).astype(F)


def _rows(rng, sc, picks, n):
    """n rows cycling through `picks`: (object name, elements or None for all); uv uniform, outgoing isotropic."""
    obj, elem, uv = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 2), F)
    for i in range(n):
        name, elems = picks[i % len(picks)]
        o = OBJ[name]
        obj[i] = o
        elem[i] = rng.integers(0, sc.num_elements(o)) if elems is None else elems[(i // len(picks)) % len(elems)]
        uv[i] = _uv(rng, 1, sc.is_lines(o))[0]
    wo = unit(rng.normal(size=(n, 3))).astype(F)
    return types.SimpleNamespace(obj=obj, elem=elem, uv=uv, wo=wo, case=np.arange(n) % len(picks))


def rays(seed, n):
    """Random rays at the objects of the scenes: from a shell around an object's origin towards a point near it."""
    rng = np.random.default_rng(seed)
    sc = scene(True)
    k = rng.integers(0, len(sc.objects), n)
    centre = np.array([o["frame"][9:12] for o in sc.objects], np.float64)[k]
    target = centre + rng.uniform(-1, 1, (n, 3)) * [1.5, 1.5, 0.5]
    origin = target + unit(rng.normal(size=(n, 3))) * rng.uniform(3, 8, (n, 1))
    d = unit(target - origin)
    return np.concatenate([origin, d, np.full((n, 1), 1e-4), np.full((n, 1), 3.4e38)], axis=1).astype(F)


def inputs(name, oracle_scene=None):
    """The rows of stratum `name`: obj, elem (int32), uv (n, 2), wo (n, 3) float32, case. Stratum a needs `oracle_scene`
    (oracle_capi.OracleScene of either scene: the geometry is shared) to find its hits."""
    rng = np.random.default_rng(SEEDS[name])
    sc = scene(True)
    n = ROWS
    row = np.arange(n)
    if name == "a":
        r = rays(SEEDS["a"], 6 * n)
        obj, elem, uv, _ = oracle_scene.intersect(r)
        keep = np.flatnonzero((obj >= 0) & ~np.isin(obj, [OBJ[f] for f in FRAGILE]))[:n]
        assert len(keep) == n, len(keep)
        s = types.SimpleNamespace(obj=obj[keep], elem=elem[keep], uv=uv[keep], wo=(-r[keep, 3:6]).astype(F), case=np.zeros(n, np.int64))
    elif name == "b":
        picks = [(o, None) for o in ("main", "metal", "trans", "plain_n", "plain_t", "bare", "special", "tc3", "hair", "hair_0", "hair_nm", "axis")]
        s = _rows(rng, sc, picks, n)
        e = UV_EDGES
        for i in range(n):
            lines = sc.is_lines(int(s.obj[i]))
            kind = (i // len(picks)) % 4
            a, b = e[(i // 7) % len(e)], e[(i // 3) % len(e)]
            if lines:  # u in {0, 1, ...} with any v; v in {0, 1} with any u
                s.uv[i] = (a, s.uv[i, 1]) if kind < 2 else (s.uv[i, 0], e[i % 2])
            elif kind == 0:
                s.uv[i] = (a, b) if float(a) + float(b) <= 1 else (a, 0)
            elif kind == 1:
                s.uv[i] = (s.uv[i, 0], F(1) - s.uv[i, 0])  # u + v = 1 (as floats: 1 - u is exact or rounds)
            elif kind == 2:
                s.uv[i] = (a, F(1) - a) if a <= 1 else (0, 1)
            else:
                s.uv[i] = (s.uv[i, 0], b) if float(s.uv[i, 0]) + float(b) <= 1 else (0, b)
    elif name == "c":
        picks = [(f"tc{k}", None) for k in range(8)] + [("no_tc_nm", None), ("bare_tex", None)]
        s = _rows(rng, sc, picks, n)
        corner = np.array([(0, 0), (1, 0), (0, 1)], F)
        at_vertex = (row // len(picks)) % 4 != 3  # three rows of four at a vertex: the table's values exactly
        tc = np.isin(s.obj, [OBJ[f"tc{k}"] for k in range(8)])
        s.elem[tc] = ((row // len(picks)) // 4 * 3 + row % 3)[tc] % sc.num_elements(OBJ["tc0"])
        s.uv[tc & at_vertex] = corner[(row // (4 * len(picks))) % 3][tc & at_vertex]
        edge = ~tc & (row % 3 == 0)  # the element uv IS the texcoord there: its edges
        s.uv[edge] = np.stack([UV_EDGES[(row // 3) % 5], np.zeros(n, F)], axis=1)[edge]
    elif name == "d":
        picks = [("special", [SPECIAL["cancel"]]), ("special_thin", [SPECIAL["cancel"]]), ("main", None), ("metal", None), ("trans", None), ("plain_n", None),
                 ("plain_t", [31]), ("bare", [17]), ("no_tc_nm", None), ("special", [SPECIAL["tilted"]]), ("plain_t", None), ("bare", None)]
        s = _rows(rng, sc, picks, n)
        cancel = s.case < 2
        t = rng.uniform(0, 1, n).astype(F)
        # 0.5 n0 + 0.5 n1 = 0 exactly on eight rows, nearly so on eight more (within a percent of the whole: beyond the p99); the rest anywhere on the triangle
        exact, near = cancel & (row < 8 * len(picks)), cancel & (row >= 8 * len(picks)) & (row < 16 * len(picks))
        s.uv[exact] = (0.5, 0)
        s.uv[near] = np.stack([F(0.5) + (t - F(0.5)) * F(1e-3), np.zeros(n, F)], axis=1)[near]
    elif name == "e":
        picks = [("main", None), ("trans", None), ("plain_t", None), ("bare", None), ("special_thin", [SPECIAL["flat"]]), ("special", [SPECIAL["flat"]]),
                 ("axis", None), ("hair", None), ("hair_0", None), ("metal", None), ("special_thin", [SPECIAL["tilted"]]), ("plain_n", None)]
        s = _rows(rng, sc, picks, n)
        kind = (row // len(picks)) % 4
        flat = np.isin(s.case, (4, 5))
        inplane = np.array([(1, 2, 0), (-3, 1, 0), (0.5, -0.25, -0.0), (2, 0, 0), (0, -1, 0), (1, 1, -0.0)], F)
        s.wo[flat & (kind == 0)] = inplane[(row // 5) % 6][flat & (kind == 0)]  # dot(n, outgoing) = 0 exactly, +0 and -0
        s.wo[flat & (kind == 1)] = (inplane[(row // 5) % 6] + np.array([0, 0, 1], F) * np.where(row % 2 == 0, F(1e-6), F(-1e-6))[:, None])[flat & (kind == 1)]
        axis = s.case == 6
        along = np.array([(2, 0, 0), (-1, 0, 0), (0.5, 0, -0.0), (1, 1e-4, 0)], F)
        s.wo[axis & (kind < 2) & (row < 16 * len(picks))] = along[(row // len(picks)) % 4][axis & (kind < 2) & (row < 16 * len(picks))]  # parallel to the tangent
        s.wo[kind == 2] *= F(0.5)
        s.wo[kind == 3] *= F(3)
    elif name == "f":
        sp = SPECIAL
        picks = [("special", [sp["uv_unit"], sp["uv_mirror"]]), ("special", [sp["uv_same"], sp["uv_zero"]]), ("special", [sp["tilted"], sp["flat"], sp["uv_corner"]]),
                 ("special_nmf", [sp["uv_unit"], sp["uv_mirror"], sp["tilted"], sp["uv_same"]]), ("no_tc_nm", None), ("hair_nm", None),
                 ("special_nm0", [sp["uv_zero"]]), ("special_nm0", [sp["uv_unit"], sp["uv_mirror"], sp["uv_corner"]]), ("special_nmf", [sp["cancel"]])]
        s = _rows(rng, sc, picks, n)
        corner = np.array([(0, 0), (1, 0), (0, 1)], F)
        s.uv[s.case == 7] = corner[(row // len(picks)) % 3][s.case == 7]  # the zero texel needs its texcoord exact: vertices with integer texcoords
    elif name == "g":
        picks = [("opacity", None), ("hair", None), ("hair_nm", None), ("rough0", None), ("trans", None), ("main", None), ("metal", None), ("volume", None),
                 ("tc3", None), ("tc7", None), ("bare_tex", None), ("volume", None)]
        s = _rows(rng, sc, picks, n)
        vol = s.case == 11  # straight through the surface from outside and from inside: both cross
        s.wo[vol] = (s.wo * np.where(row % 2 == 0, F(1), F(-1))[:, None])[vol]
    else:
        raise KeyError(name)
    s.name, s.n = name, n
    s.obj, s.elem = np.ascontiguousarray(s.obj, np.int32), np.ascontiguousarray(s.elem, np.int32)
    s.uv, s.wo = np.ascontiguousarray(s.uv, F), np.ascontiguousarray(s.wo, F)
    return s
