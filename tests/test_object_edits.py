"""yh_update_objects: the frames and materials of an uploaded scene's objects change without a new upload — the C ABI, the per-object
kernel (unit/objects.hip), the scene-level tree built again, the room the upload leaves for wide scene nodes, the Python binding, the
C++ mirror's opt-in (set_object_edits) and `ysceneitraces --turntable STEPS --turntable-objects`.

The yardstick of every edit is a FRESH context that got yh_upload_scene of the edited description (tests/test_scene_edits.py): images
as uint32 and RNG states, 256 rays of yh_intersect_batch and 256 rows of yh_lights_batch in both forms must be the same bits. A fresh
upload's results are computed once per edited description and shared (under the host's own choice of launch shape: every shape renders
the same bits, tests/test_instances.py and tests/test_gpu_parity.py).

sphere-hairblock has no area light (the sky lights it), so the case that moves an area light runs on scene-once `full`, whose two
quads are small lights in the kernels' LDS light table, and on crowd's quad.

The CPU half checks, with float32 numpy world boxes and yh_bvh_build, that the edits exercise what they claim before a GPU sees them.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_scene_edits import Edited, _fresh, _render, _same

sys.path.insert(0, os.path.join(ROOT, "tools"))
from scene_level_visits import object_boxes as _object_boxes  # noqa: E402  (world boxes of a description's objects, float32)

RES, SPP, F = 48, 2, np.float32
PKG = os.path.join(ROOT, "yocto-hair_amd")
HAIRBLOCK = ("sphere-hairblock", dict(scale=0.02))
CROWD = ("crowd", dict(scale=0.05))                 # 70 balls + hair block + light: the scene level is walked as 4-wide nodes
FLIP = ("crowd", dict(scale=0.05, count=44))        # 46 objects: the LDS table or wide nodes, depending on the tree's node count
FIELD = ("fur-field", dict(scale=0.25, count=256))  # 256 tufts + 32 pebbles + floor + light
INSTANCE_SHAPES = ("0", "1", "3", "4", "5", "6", "7", "8")  # what tests/test_instances.py forces through YHAIR_SHAPE


# ---------------------------------------------------------------------------------------------
# frames (12 floats: x, y, z, o as columns) and descriptions with their own object rows
# ---------------------------------------------------------------------------------------------
def _f32(v):
    return [float(F(x)) for x in np.asarray(v, np.float64).reshape(-1)]


def _compose(a, b):
    """a * b: the frame that applies b, then a."""
    a, b = np.array(a, np.float64).reshape(4, 3), np.array(b, np.float64).reshape(4, 3)
    m = a[:3].T
    return _f32(np.concatenate([(m @ b[:3].T).T, (m @ b[3] + a[3])[None]]))


def _rotation(axis, degrees, origin=(0, 0, 0)):
    """A rotation about `axis` through `origin` (Rodrigues)."""
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.radians(degrees)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    o = np.asarray(origin, np.float64)
    return _f32(np.concatenate([R.T, (o - R @ o)[None]]))


def _scaling(sx, sy, sz):
    return [sx, 0, 0, 0, sy, 0, 0, 0, sz, 0, 0, 0]


def _translation(x, y, z):
    return [1, 0, 0, 0, 1, 0, 0, 0, 1, x, y, z]


class Moved(Edited):
    """A copy of a description with its own object rows (and, with `extra`, more materials behind the loaded ones)."""

    def __init__(self, yh, desc, extra=()):
        super().__init__(yh, desc)
        src = desc.contents if hasattr(desc, "contents") else desc
        self.n = src.num_objects
        self.objects = (yh.Object * self.n)(*[yh.Object.from_buffer_copy(src.objects[i]) for i in range(self.n)])
        self.d.objects = C.cast(self.objects, C.POINTER(yh.Object))
        if extra:
            rows = [self.materials[i] for i in range(src.num_materials)] + list(extra)
            self.materials = (yh.Material * len(rows))(*rows)
            self.d.materials, self.d.num_materials = C.cast(self.materials, C.POINTER(yh.Material)), len(rows)

    def rows(self, yh, first=0, count=None):
        count = self.n - first if count is None else count
        return (yh.Object * count)(*[yh.Object.from_buffer_copy(self.objects[first + i]) for i in range(count)])

    def frames(self):
        return [list(self.objects[i].frame) for i in range(self.n)]

    def set_frames(self, frames, first=0):
        for i, f in enumerate(frames):
            self.objects[first + i].frame[:] = _f32(f)
        return self

    def index(self, lines=None, emissive=None, material=None):
        """Objects by what they are: made of lines or not, emissive or not, with material row `material`."""
        out = []
        for i in range(self.n):
            o = self.objects[i]
            if lines is not None and (self.d.shapes[o.shape].num_lines > 0) != lines:
                continue
            if emissive is not None and any(self.materials[o.material].emission[:]) != emissive:
                continue
            if material is not None and o.material != material:
                continue
            out.append(i)
        return out


def _chains(n, chains, reach=3.0, size=0.25, ratio=0.45):
    """n ball frames in `chains` rows from the origin along +x, -x, +z, -z, each ball `ratio` times as far out and as large as the one
    before: the middle split (pt.cpp:564-595) takes one ball off such a row at a time, so the scene tree has nearly a node per ball
    and a level per ball of a row — many more nodes and levels than a grid of the same balls."""
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1)][:chains]
    out = []
    for k in range(n):
        d, i = dirs[k % chains], k // chains
        s = ratio ** i
        out.append([size * s, 0, 0, 0, size * s, 0, 0, 0, size * s, reach * s * d[0], 0.3 * size * s, reach * s * d[2]])
    return out


def _levels(yh, boxes):
    """(node count, levels) of the tree yh_bvh_build makes over (n, 6) float32 boxes."""
    lib = yh.load()
    boxes = np.ascontiguousarray(boxes, F)
    n = len(boxes)
    nb = lib.yh_bvh_build(n, yh.fptr(boxes), None, None)
    nodes = np.zeros((nb, 8), F)
    assert lib.yh_bvh_build(n, yh.fptr(boxes), yh.fptr(nodes), None) == nb
    start, meta = nodes[:, 6].view(np.int32), nodes[:, 7].view(np.int32)
    level = np.zeros(nb, np.int64)
    for i in range(nb):  # (breadth-first numbering: a node's children lie behind it)
        if (meta[i] >> 16) & 1:
            level[start[i]] = level[start[i] + 1] = level[i] + 1
    return nb, int(level.max()) + 1


def _tree(yh, desc):
    """(node count, levels) of the scene tree over the description's world boxes."""
    return _levels(yh, _object_boxes(desc))


def _shape_levels(yh, sh):
    """Levels of a shape's tree: over its primitives' boxes (line_bounds / triangle_bounds, math.h:3037-3044)."""
    pos = np.ctypeslib.as_array(sh.positions, (sh.num_vertices, 3))
    if sh.num_lines > 0:
        idx, rad = np.ctypeslib.as_array(sh.lines, (sh.num_lines, 2)), np.ctypeslib.as_array(sh.radius, (sh.num_vertices,))
        p, r = pos[idx], rad[idx][..., None]
        return _levels(yh, np.concatenate([(p - r).min(1), (p + r).max(1)], 1))[1]
    p = pos[np.ctypeslib.as_array(sh.triangles, (sh.num_triangles, 3))]
    return _levels(yh, np.concatenate([p.min(1), p.max(1)], 1))[1]


def _stack_need(yh, desc, scene_levels, wide):
    """What the upload asks of the traversal stack (host/scene_upload.cpp: stack_needs): the scene level's share — three entries per
    level of 4-wide nodes and a leaf's three objects, or one per binary level — and three per 4-wide level of the deepest shape."""
    depth4 = max(1 + max(0, _shape_levels(yh, desc.shapes[i]) - 2) // 2 for i in range(desc.num_shapes))
    scene = 3 * (1 + max(0, scene_levels - 2) // 2) + 4 if wide else scene_levels + 4
    return scene + 3 * depth4 + 2


def _lds_f4(n, nodes):
    """The scene-level table's float4 count (host/scene_upload.cpp); the scene level is walked as wide nodes beyond 10 KB."""
    return 11 * n + 2 * nodes + (n + 3) // 4


# ---------------------------------------------------------------------------------------------
# the edits of the GPU tests
# ---------------------------------------------------------------------------------------------
def _crowd_edits(yh, sf):
    """base, grown (every ball into four rows), part (balls 10-29 moved a little), and the rows each edit passes."""
    base = Moved(yh, sf.desc)
    balls = base.index(lines=False, emissive=False)
    assert balls == list(range(balls[0], balls[0] + len(balls)))  # (alphabetical: ball000 ... in a row)
    grown = Moved(yh, sf.desc)
    for i, f in zip(balls, _chains(len(balls), 4)):
        grown.objects[i].frame[:] = _f32(f)
    part = Moved(yh, sf.desc)
    some = balls[10:30]
    for k, i in enumerate(some):
        part.objects[i].frame[:] = _compose(_translation(0.15 * (k % 3), 0.2 + 0.05 * k, -0.1 * (k % 4)), _compose(part.objects[i].frame[:], _rotation((1, 2, 0), 40 + 7 * k)))
    return base, grown, part, balls, some


def _flip_descriptions(yh, sf):
    """The 46-object crowd as loaded (a grid: few nodes, the LDS table) and with its balls in two rows (many nodes: wide)."""
    grid, rows = Moved(yh, sf.desc), Moved(yh, sf.desc)
    balls = rows.index(lines=False, emissive=False)
    for i, f in zip(balls, _chains(len(balls), 2)):
        rows.objects[i].frame[:] = _f32(f)
    return grid, rows, balls


def _too_deep(yh, sf):
    """crowd with all 70 balls in ONE row: a scene tree of nearly 70 levels."""
    deep = Moved(yh, sf.desc)
    balls = deep.index(lines=False, emissive=False)
    for i, f in zip(balls, _chains(len(balls), 1, reach=1000.0, size=80.0, ratio=1 / 3)):
        deep.objects[i].frame[:] = _f32(f)
    return deep, balls


# ---------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------
def test_library_exports_and_header_declares_yh_update_objects(yh):
    lib = yh.load()
    header = open(os.path.join(ROOT, "include", "yhair.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libyhair.so")], capture_output=True, text=True, check=True).stdout
    assert hasattr(lib, "yh_update_objects") and " T yh_update_objects\n" in exported
    assert "int yh_update_objects(yh_context* ctx, int first, int count, const yh_object* objects);" in header
    assert "yh_update_objects" in yh.EXPORTS and callable(yh.Context.update_objects)
    row = (yh.Object * 1)()
    assert lib.yh_update_objects(None, 0, 1, row) == yh.YH_E_INVALID
    assert lib.yh_update_objects(None, 0, 0, None) == yh.YH_E_INVALID


def _compile_mirror_test(tmp_path):
    exe = str(tmp_path / "mirror_object_edits")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host"), "-Wno-class-memaccess", os.path.join(ROOT, "tests", "cpp", "test_mirror_object_edits.cpp"),
                           "-o", exe, "-L" + PKG, "-lyhair", "-Wl,-rpath," + PKG, "-lpthread"])
    return exe


def test_mirror_classifies_object_edits_without_a_device(built, tmp_path):
    """With the opt-in a frame or material change is edit_objects; a shape change, an added object, an object change next to a
    texture change, emission on or off by reassignment are edit_upload; without the opt-in everything is as before — checked by the
    C++ program itself (tests/cpp/test_mirror_object_edits.cpp)."""
    exe = _compile_mirror_test(tmp_path)
    r = subprocess.run([exe, "--classify"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def test_the_edits_exercise_what_they_claim(yh):
    """The inputs of the GPU tests, before a GPU sees them: crowd's edit changes the scene tree's node count and depth (and stays a
    wide scene level within the stack); the two frame sets of the form flip lie at least 8 nodes on either side of the 10 KB line of
    the scene-level table, and both upload; the too-deep case needs more stack than the library reports."""
    lib = yh.load()
    lib.yhk_stack_entries.restype = C.c_int
    limit = lib.yhk_stack_entries()
    sf = yh.SceneFile(scene_path(*CROWD[:1], **CROWD[1]))
    base, grown, part, balls, some = _crowd_edits(yh, sf)
    n = base.n
    (nb, lb), (ng, lg), (npart, lpart) = _tree(yh, base.d), _tree(yh, grown.d), _tree(yh, part.d)
    print(f"crowd: {n} objects; base {nb} nodes / {lb} levels, grown {ng} / {lg}, part {npart} / {lpart}; stack limit {limit}")
    assert len(balls) == 70 and n == 72 and 0 < some[0] and some[-1] < n - 1
    assert ng >= nb + 16 and lg >= lb + 4, "the edit of all balls must grow the tree"
    assert _object_boxes(part.d)[some].tobytes() != _object_boxes(base.d)[some].tobytes()
    for nodes in (nb, ng, npart):
        assert _lds_f4(n, nodes) * 16 > 10240  # wide, all three
    assert max(_stack_need(yh, base.d, lv, True) for lv in (lb, lg, lpart)) <= limit
    deep, _ = _too_deep(yh, sf)
    nd, ld = _tree(yh, deep.d)
    need = _stack_need(yh, deep.d, ld, True)
    print(f"too deep: {nd} nodes / {ld} levels, {need} stack entries")
    assert _lds_f4(n, nd) * 16 > 10240 and need > limit
    sf.close()
    sf = yh.SceneFile(scene_path(*FLIP[:1], **FLIP[1]))
    grid, rows, _ = _flip_descriptions(yh, sf)
    n = grid.n
    (ngrid, lgrid), (nrows, lrows) = _tree(yh, grid.d), _tree(yh, rows.d)
    at = next(k for k in range(4 * n) if _lds_f4(n, k) * 16 > 10240)  # the first node count that is walked wide
    print(f"flip: {n} objects; grid {ngrid} nodes / {lgrid} levels, rows {nrows} / {lrows}; wide from {at} nodes")
    assert n == 46 and ngrid <= at - 1 - 8 and nrows >= at + 8
    assert _stack_need(yh, grid.d, lgrid, False) <= limit and _stack_need(yh, rows.d, lrows, True) <= limit  # both upload
    sf.close()


# ---------------------------------------------------------------------------------------------
# on the GPU: the yardstick
# ---------------------------------------------------------------------------------------------
def _rays_at(desc, n=256, seed=5):
    """n rays from around the camera into the box of all objects nearer than 20 units."""
    boxes = _object_boxes(desc).astype(np.float64)
    boxes = boxes[np.abs(boxes).max(axis=1) < 20]
    lo, hi = boxes[:, :3].min(0), boxes[:, 3:].max(0)
    rng = np.random.default_rng(seed)
    eye = np.array(desc.camera.frame[9:12], np.float64)
    o = eye + rng.normal(0, 0.3, (n, 3))
    d = rng.uniform(lo, hi, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d, np.full((n, 1), 1e-4), np.full((n, 1), 3.4e38)], axis=1).astype(F)


def _light_rows(desc, n=256, seed=29):
    boxes = _object_boxes(desc).astype(np.float64)
    boxes = boxes[np.abs(boxes).max(axis=1) < 20]
    lo, hi = boxes[:, :3].min(0), boxes[:, 3:].max(0)
    rng = np.random.default_rng(seed)
    P = rng.uniform(lo - 0.5, hi + 0.5, (n, 3)).astype(F)
    D = rng.normal(size=(n, 3))
    D = (D / np.linalg.norm(D, axis=1, keepdims=True)).astype(F)
    RN = np.minimum(rng.uniform(0, 1, (n, 4)).astype(F), np.nextafter(F(1), F(0)))
    return P, D, RN


def _results(c, yh, desc, plain):
    """Everything the contract names, of context `c` holding `desc`: image and RNG states, closest hits, light rows in both forms,
    yh_scene_once and (plain scenes) the plain traversal's closest hits in both forms."""
    img, rng = _render(c, yh, spp=SPP, res=RES)
    rays = _rays_at(desc)
    out = dict(image=(img, rng), hits=c.intersect(rays), lights=[c.lights(form, *_light_rows(desc)) for form in (0, 1)], once=c.scene_once())
    if plain:
        out["plain"] = [c.intersect_plain(form, rays) for form in (0, 1)]
    return out


_FRESH = {}


def _fresh_results(yh, key, desc, plain=False):
    """The yardstick, once per edited description: a new context, yh_upload_scene, the same calls (under the host's own choice of
    launch shape, whatever the calling test forces)."""
    if key not in _FRESH:
        forced = os.environ.pop("YHAIR_SHAPE", None)
        c = yh.Context(0)
        try:
            c.upload_scene(C.pointer(desc))
            _FRESH[key] = _results(c, yh, desc, plain)
        finally:
            c.close()
            if forced is not None:
                os.environ["YHAIR_SHAPE"] = forced
    return _FRESH[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check(got, want, what):
    _same(got["image"], want["image"], what)
    for name, a, b in zip(("object", "element", "uv", "distance"), got["hits"], want["hits"]):
        assert np.array_equal(_bits(a), _bits(b)), f"{what}: yh_intersect_batch {name} differs from a fresh upload's"
    for form in (0, 1):
        assert np.array_equal(_bits(got["lights"][form]), _bits(want["lights"][form])), f"{what}: yh_lights_batch form {form} differs from a fresh upload's"
    assert got["once"] == want["once"], what
    if "plain" in want:
        for form in (0, 1):
            for a, b in zip(got["plain"][form], want["plain"][form]):
                assert np.array_equal(_bits(a), _bits(b)), f"{what}: yh_intersect_plain_batch form {form} differs from a fresh upload's"


def _differs(a, b):
    return not np.array_equal(a["image"][0], b["image"][0])


# ---------------------------------------------------------------------------------------------
# 1. the LDS-table form: sphere-hairblock
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hairblock(yh):
    sf = yh.SceneFile(scene_path(*HAIRBLOCK[:1], **HAIRBLOCK[1]))
    yield sf
    sf.close()


@pytest.mark.gpu
def test_moved_hair_object_renders_as_a_fresh_upload(ctx, yh, hairblock):
    """A rotation, a non-uniform scale and a translation of the hair object (its inverse frame is not the transpose), then a second
    edit on top of it and the way back to the loaded frame."""
    base, new = Moved(yh, hairblock.desc), Moved(yh, hairblock.desc)
    hair = new.index(lines=True)[0]
    f = new.objects[hair].frame[:]
    new.objects[hair].frame[:] = _compose(_translation(-0.4, 0.25, 0.3), _compose(f, _compose(_rotation((1, 1, 0.3), 35), _scaling(1.2, 0.7, 0.9))))
    ctx.upload_scene(base.ptr)
    before = _results(ctx, yh, base.d, True)
    _check(before, _fresh_results(yh, "hairblock", base.d, True), "the upload itself")
    ctx.update_objects(hair, new.rows(yh, hair, 1))
    got = _results(ctx, yh, new.d, True)
    _check(got, _fresh_results(yh, "hairblock-moved", new.d, True), "hair object moved")
    assert _differs(got, before), "the edit changed nothing"
    ctx.update_objects(0, base.rows(yh))  # every row, back
    _check(_results(ctx, yh, base.d, True), _fresh_results(yh, "hairblock", base.d, True), "moved back")


# ---------------------------------------------------------------------------------------------
# 2. scene-once: one to four objects, the scene level resolved once per ray
# ---------------------------------------------------------------------------------------------
def _once_edit(yh, sf, variant):
    new = Moved(yh, sf.desc)
    hair, others = new.index(lines=True)[0], new.index(lines=False, emissive=False)
    if variant == "one":
        new.objects[hair].frame[:] = _compose(_rotation((0, 1, 0), 50, (0.5, 1, -0.5)), new.objects[hair].frame[:])
    elif variant == "disjoint":  # the block pushed into the sphere: the boxes overlap
        new.objects[hair].frame[:] = _compose(_translation(-0.8, -0.2, 0.0), new.objects[hair].frame[:])
    elif variant == "overlap":   # ... and pulled out of it: they separate
        new.objects[hair].frame[:] = _compose(_translation(1.1, 0.4, 0.0), new.objects[hair].frame[:])
    elif variant == "tie":       # one of the two coincident quads tilted: the ties are gone
        q = others[0]
        new.objects[q].frame[:] = _compose(_rotation((1, 0, 0), 20, (0.4, 0.4, -0.5)), new.objects[q].frame[:])
    elif variant == "full":      # an area light moves (a small light of the LDS light table), and the sphere
        light = new.index(emissive=True)[0]
        new.objects[light].frame[:] = _compose(_translation(-1.0, -1.2, 0.5), _compose(_rotation((0, 0, 1), 25), new.objects[light].frame[:]))
        new.objects[others[0]].frame[:] = _compose(_translation(0.3, 0.1, 0.2), new.objects[others[0]].frame[:])
    return new


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["one", "disjoint", "overlap", "tie", "full"])
def test_scene_once_scenes_render_and_intersect_as_a_fresh_upload(ctx, yh, variant):
    sf = yh.SceneFile(scene_path("scene-once", variant=variant))
    base, new = Moved(yh, sf.desc), _once_edit(yh, sf, variant)
    ctx.upload_scene(base.ptr)
    once = ctx.scene_once()
    assert once == base.n and 1 <= once <= 4
    before = _results(ctx, yh, base.d, True)
    ctx.update_objects(0, new.rows(yh))
    got = _results(ctx, yh, new.d, True)
    assert got["once"] == once, "yh_scene_once changed"
    _check(got, _fresh_results(yh, "once-" + variant, new.d, True), variant)
    assert _differs(got, before), "the edit changed nothing"
    if variant == "full":  # the light directions are the moved light's
        assert not np.array_equal(got["lights"][0], before["lights"][0])
    sf.close()


# ---------------------------------------------------------------------------------------------
# 3. crowd: the wide scene level
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crowd(yh):
    sf = yh.SceneFile(scene_path(*CROWD[:1], **CROWD[1]))
    yield sf
    sf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", INSTANCE_SHAPES)
def test_crowd_grows_moves_a_part_and_shrinks_back(ctx, yh, crowd, shape, monkeypatch):
    """Every ball edited so that the scene tree's node count grows; a sub-range only (first > 0, count < n), which also moves the
    light's neighbours; then every row back to the loaded frames, which must equal the base upload: the count of wide scene nodes
    shrinks and the slots of the reservation that it no longer uses are cleared."""
    base, grown, part, balls, some = _crowd_edits(yh, crowd)
    monkeypatch.setenv("YHAIR_SHAPE", shape)
    ctx.upload_scene(base.ptr)
    r0 = _results(ctx, yh, base.d, False)
    _check(r0, _fresh_results(yh, "crowd", base.d), f"the upload itself, shape {shape}")
    ctx.update_objects(balls[0], grown.rows(yh, balls[0], len(balls)))
    r1 = _results(ctx, yh, grown.d, False)
    assert ctx.launch_shape() == int(shape)
    _check(r1, _fresh_results(yh, "crowd-grown", grown.d), f"grown, shape {shape}")
    ctx.update_objects(0, base.rows(yh))
    _check(_results(ctx, yh, base.d, False), _fresh_results(yh, "crowd", base.d), f"back to the base frames, shape {shape}")
    ctx.update_objects(some[0], part.rows(yh, some[0], len(some)))
    r2 = _results(ctx, yh, part.d, False)
    _check(r2, _fresh_results(yh, "crowd-part", part.d), f"a sub-range, shape {shape}")
    assert _differs(r1, r0) and _differs(r2, r0)


@pytest.mark.gpu
def test_crowd_light_moves(ctx, yh, crowd):
    base, new = Moved(yh, crowd.desc), Moved(yh, crowd.desc)
    light = new.index(emissive=True)[0]
    new.objects[light].frame[:] = _compose(_translation(-1.5, -2.0, 0.5), _compose(_rotation((1, 0, 1), 30), new.objects[light].frame[:]))
    ctx.upload_scene(base.ptr)
    before = [ctx.lights(form, *_light_rows(new.d)) for form in (0, 1)]
    ctx.update_objects(light, new.rows(yh, light, 1))
    got = _results(ctx, yh, new.d, False)
    _check(got, _fresh_results(yh, "crowd-light", new.d), "the area light moved")
    assert not np.array_equal(got["lights"][0], before[0]) and not np.array_equal(got["lights"][1], before[1])


# ---------------------------------------------------------------------------------------------
# 4. fur-field: instances
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["0", "3"], ids=["quad", "k_stream"])
def test_every_tuft_turns_about_its_own_root(ctx, yh, shape, monkeypatch):
    sf = yh.SceneFile(scene_path(*FIELD[:1], **FIELD[1]))
    base, new = Moved(yh, sf.desc), Moved(yh, sf.desc)
    tufts = new.index(lines=True)
    assert len(tufts) == 256 and tufts == list(range(tufts[0], tufts[0] + 256)) and tufts[0] > 0
    for k, i in enumerate(tufts):
        f = new.objects[i].frame[:]
        new.objects[i].frame[:] = _compose(_rotation((0.2, 1, 0.1), 25 + 1.3 * k, f[9:12]), f)  # about its root: the frame's origin stays
        assert np.allclose(new.objects[i].frame[9:12], f[9:12], atol=1e-5)
    monkeypatch.setenv("YHAIR_SHAPE", shape)
    ctx.upload_scene(base.ptr)
    before = _results(ctx, yh, base.d, False)
    ctx.update_objects(tufts[0], new.rows(yh, tufts[0], 256))
    got = _results(ctx, yh, new.d, False)
    assert ctx.launch_shape() == int(shape)
    _check(got, _fresh_results(yh, "field-turned", new.d), f"tufts turned, shape {shape}")
    assert _differs(got, before), "the edit changed nothing"
    sf.close()


# ---------------------------------------------------------------------------------------------
# 5. an object's material reassigned
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hair_object_takes_another_hair_material(ctx, yh, hairblock):
    d = hairblock.desc.contents
    hair_row = next(d.objects[i].material for i in range(d.num_objects) if d.shapes[d.objects[i].shape].num_lines > 0)
    blond = yh.Material.from_buffer_copy(d.materials[hair_row])
    blond.eumelanin, blond.pheomelanin, blond.beta_m = 0.3, 0.2, 0.45
    base, new = Moved(yh, hairblock.desc, extra=[blond]), Moved(yh, hairblock.desc, extra=[blond])
    hair = new.index(lines=True)[0]
    new.objects[hair].material = d.num_materials  # the added row
    ctx.upload_scene(base.ptr)
    before = _results(ctx, yh, base.d, True)
    ctx.update_objects(hair, new.rows(yh, hair, 1))
    got = _results(ctx, yh, new.d, True)
    _check(got, _fresh_results(yh, "hairblock-blond", new.d, True), "another hair material")
    assert _differs(got, before), "the edit changed nothing"
    for a, b in zip(got["hits"], before["hits"]):  # (the geometry stays)
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.gpu
def test_crowd_ball_goes_from_red_to_veil(ctx, yh, crowd):
    base, new = Moved(yh, crowd.desc), Moved(yh, crowd.desc)
    d = crowd.desc.contents
    red = next(i for i in range(d.num_materials) if np.allclose(d.materials[i].color[:], [0.8, 0.2, 0.2]))
    veil = next(i for i in range(d.num_materials) if abs(d.materials[i].opacity - 0.6) < 1e-6)
    # (a red ball in front: ball 0 of the grid's last row is nearest to the camera)
    ball = max(new.index(material=red), key=lambda i: new.objects[i].frame[11])
    new.objects[ball].material = veil
    ctx.upload_scene(base.ptr)
    before = _results(ctx, yh, base.d, False)
    ctx.update_objects(ball, new.rows(yh, ball, 1))
    got = _results(ctx, yh, new.d, False)
    _check(got, _fresh_results(yh, "crowd-veil", new.d), "red to veil")
    assert _differs(got, before), "the edit changed nothing"


# ---------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------
def _argument_refusals(yh, sf):
    m = Moved(yh, sf.desc)
    d, n = sf.desc.contents, m.n
    hair = m.index(lines=True)[0]
    emitter = next(i for i in range(d.num_materials) if any(d.materials[i].emission[:]))
    rows = m.rows(yh)

    def row(i, **fields):
        o = yh.Object.from_buffer_copy(m.objects[i])
        for k, v in fields.items():
            setattr(o, k, v)
        return (yh.Object * 1)(o)

    other_shape = next(s for s in range(d.num_shapes) if s != m.objects[hair].shape)
    return {
        "null": lambda lib, h: lib.yh_update_objects(h, 0, 1, None),
        "first-negative": lambda lib, h: lib.yh_update_objects(h, -1, 1, rows),
        "first-behind-the-list": lambda lib, h: lib.yh_update_objects(h, n + 1, 0, rows),
        "count-negative": lambda lib, h: lib.yh_update_objects(h, 0, -1, rows),
        "count-past-the-end": lambda lib, h: lib.yh_update_objects(h, n - 1, 2, rows),
        "count-huge": lambda lib, h: lib.yh_update_objects(h, 1, 2**31 - 1, rows),
        "another-shape": lambda lib, h: lib.yh_update_objects(h, hair, 1, row(hair, shape=other_shape)),
        "shape-out-of-range": lambda lib, h: lib.yh_update_objects(h, hair, 1, row(hair, shape=d.num_shapes)),
        "material-out-of-range": lambda lib, h: lib.yh_update_objects(h, hair, 1, row(hair, material=d.num_materials)),
        "material-negative": lambda lib, h: lib.yh_update_objects(h, hair, 1, row(hair, material=-1)),
        "hair-takes-the-lights-material": lambda lib, h: lib.yh_update_objects(h, hair, 1, row(hair, material=emitter)),
        "second-row-of-two": lambda lib, h: lib.yh_update_objects(h, 0, n, (yh.Object * n)(*[rows[i] if i != n - 1 else row(i, material=emitter)[0] for i in range(n)])),
    }, rows


ARGUMENT_REFUSALS = ["null", "first-negative", "first-behind-the-list", "count-negative", "count-past-the-end", "count-huge", "another-shape",
                     "shape-out-of-range", "material-out-of-range", "material-negative", "hair-takes-the-lights-material", "second-row-of-two"]


@pytest.fixture(scope="module")
def refusal_baseline(yh, hairblock):
    """2 + 2 samples on the untouched scene, from a context of its own: what every refused context must go on rendering."""
    return _fresh(yh, hairblock.desc, spp=2, first=2, res=RES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ARGUMENT_REFUSALS)
def test_refused_arguments_leave_the_context_rendering(ctx, yh, hairblock, refusal_baseline, name):
    calls, _keep = _argument_refusals(yh, hairblock)
    ctx.upload_scene(hairblock.desc)
    ctx.set_shard(0, 1)
    ctx.init_state(yh.TraceParams.default(resolution=RES))
    ctx.trace_samples(2)
    assert calls[name](ctx.lib, ctx.h) == yh.YH_E_INVALID, name
    assert ctx.lib.yh_last_error(ctx.h).decode().startswith("yh_update_objects:"), ctx.lib.yh_last_error(ctx.h)
    ctx.trace_samples(2)  # the image state is still there, and the scene is the earlier one
    _same((ctx.download(), ctx.download_rng()), refusal_baseline, name)
    assert ctx.scene_once() == refusal_baseline[2]


def _refused_by_its_result(ctx, yh, base, new, first, count, words):
    """Upload `base`, render 2 samples, try the edit, render 2 more: refused with `words`, and the 2 + 2 samples are a fresh upload's."""
    want = _fresh(yh, base.ptr, spp=2, first=2, res=RES)
    ctx.upload_scene(base.ptr)
    ctx.set_shard(0, 1)
    ctx.init_state(yh.TraceParams.default(resolution=RES))
    ctx.trace_samples(2)
    assert ctx.lib.yh_update_objects(ctx.h, first, count, new.rows(yh, first, count)) == yh.YH_E_INVALID
    message = ctx.lib.yh_last_error(ctx.h).decode()
    assert message.startswith("yh_update_objects:") and all(w in message for w in words), message
    ctx.trace_samples(2)
    _same((ctx.download(), ctx.download_rng()), want, message)
    rays = _rays_at(base.d)
    fresh = yh.Context(0)
    fresh.upload_scene(base.ptr)
    for a, b in zip(ctx.intersect(rays), fresh.intersect(rays)):
        assert np.array_equal(_bits(a), _bits(b))
    fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("way", ["table-to-wide", "wide-to-table"])
def test_a_scene_level_that_changes_its_form_is_refused(ctx, yh, way):
    sf = yh.SceneFile(scene_path(*FLIP[:1], **FLIP[1]))
    grid, rows, balls = _flip_descriptions(yh, sf)
    base, new = (grid, rows) if way == "table-to-wide" else (rows, grid)
    _refused_by_its_result(ctx, yh, base, new, balls[0], len(balls), ["upload the scene"])
    sf.close()


@pytest.mark.gpu
def test_a_tree_too_deep_is_refused(ctx, yh, crowd):
    deep, balls = _too_deep(yh, crowd)
    _refused_by_its_result(ctx, yh, Moved(yh, crowd.desc), deep, balls[0], len(balls), ["BVH too deep for the traversal stack"])


# ---------------------------------------------------------------------------------------------
# 7. call order
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_call_order(yh, hairblock):
    rows = Moved(yh, hairblock.desc).rows(yh)
    c = yh.Context(0)
    assert c.lib.yh_update_objects(c.h, 0, len(rows), rows) == yh.YH_E_STATE  # before an upload
    c.upload_scene(hairblock.desc)
    c.init_state(yh.TraceParams.default(resolution=RES))
    c.trace_samples(1)
    c.update_objects(0, rows)  # (an edit that changes no value is an edit all the same)
    assert c.lib.yh_trace_samples(c.h, 1) == yh.YH_E_STATE
    c.init_state(yh.TraceParams.default(resolution=RES))
    c.trace_samples(1)
    c.update_objects(1, [])  # (... and so is one of no rows)
    assert c.lib.yh_trace_samples(c.h, 1) == yh.YH_E_STATE
    c.close()


# ---------------------------------------------------------------------------------------------
# 8., 9. the mirror and the command line
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mirror_passes_object_edits_on_with_the_opt_in(built, tmp_path):
    """set_frame on the hair object after an init_state, with set_object_edits: one upload and one edit, pixels those of a scene
    built that way from the start."""
    exe = _compile_mirror_test(tmp_path)
    r = subprocess.run([exe, scene_path(*HAIRBLOCK[:1], **HAIRBLOCK[1])], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)


@pytest.mark.gpu
def test_turntable_of_the_objects_command_line(built, tmp_path):
    cli, scene = os.path.join(PKG, "ysceneitraces"), scene_path(*HAIRBLOCK[:1], **HAIRBLOCK[1])
    common = [cli, scene, "-r", "32", "-s", "2"]
    r = subprocess.run(common + ["--turntable", "3", "--turntable-objects", "-o", str(tmp_path / "x.pfm")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    plain = subprocess.run(common + ["-o", str(tmp_path / "y.pfm")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, (plain.stdout, plain.stderr)
    steps = [open(tmp_path / f"x-{k:03d}.pfm", "rb").read() for k in range(3)]
    assert sorted(os.listdir(tmp_path)) == ["x-000.pfm", "x-001.pfm", "x-002.pfm", "y.pfm"]
    assert steps[0] == open(tmp_path / "y.pfm", "rb").read()
    assert len(set(steps)) == 3
    assert r.stdout.count("edit to preview:") == 2 and r.stdout.count("the objects alone were passed on") == 2, r.stdout
    assert "the scene was uploaded again" not in r.stdout and "the camera alone" not in r.stdout
