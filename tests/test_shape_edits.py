"""yh_update_shape / yh_update_shape_device: the positions, tangents, radii, texcoords and indices of ONE shape of an uploaded scene
change without a new upload — the C ABI, the per-element kernels (unit/shapes.hip), the shape's tree, records and wide nodes made
again by the upload's own code, the room every shape has for its wide nodes and the append behind the traversal array when a width
outgrows it (yh_shape_nodes), the scene level made again, the Python binding and the C++ mirror's opt-in (set_shape_edits).

The yardstick of every edit is a FRESH context that got yh_upload_scene of the edited description (tests/test_scene_edits.py,
tests/test_object_edits.py): images as uint32 and RNG states at 48 x 48, 2 spp, 256 rays of yh_intersect_batch, 256 rows of
yh_lights_batch in both forms and yh_scene_once must be the same bits. A fresh upload's results are computed once per edited
description and shared.

The CPU half checks with yh_bvh_build and yh_bvh_build_wide on float32 numpy boxes that the edits exercise what they claim.

Two things the scenes force on these tests. In `textured` the quad is the shape of the floor AND of an area light, and a shape
named by an emitter is refused: the texcoord edit runs on a description whose floor has its own copy of the quad. No test scene
has a line shape without radius: the `double` case that passes a radius where the upload had none runs on a description whose
hair was uploaded with radius NULL. Two refusals have no test: the 30-bit limit (a traversal array of 32 GB) and more wide scene
nodes than the reserved room (the upload reserves a node per object, the most a tree over them can have).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_scene_edits import Edited, _fresh, _render, _same  # noqa: F401
from test_object_edits import (CROWD, FIELD, FLIP, HAIRBLOCK, INSTANCE_SHAPES, Moved, _bits, _check, _compose, _differs, _f32, _fresh_results, _lds_f4, _levels,
                               _rays_at, _results, _rotation, _stack_need, _translation, _tree)

RES, F, I32 = 48, np.float32, np.int32
PKG = os.path.join(ROOT, "yocto-hair_amd")
HAIRBLOCK_BIG = ("sphere-hairblock", dict(scale=0.05))  # 80 000 segments: the hair is built on the device (>= 32 768)
TEXTURED = ("textured", dict(scale=0.05))
SIZES = {"host-built": HAIRBLOCK, "device-built": HAIRBLOCK_BIG}
SWAY_A = (0.05, 0.1, 0.2, 0.4, 0.8)  # x += a * y^2: the first that grows one of the three wide-node counts is used
ARRAYS = (("positions", F, 3), ("normals", F, 3), ("radius", F, 0), ("texcoords", F, 2), ("lines", I32, 2), ("triangles", I32, 3))


# ---------------------------------------------------------------------------------------------
# descriptions with their own shapes
# ---------------------------------------------------------------------------------------------
class Reshaped(Moved):
    """A copy of a description with its own shape list (and object rows); set() points a shape at numpy arrays it keeps alive."""

    def __init__(self, yh, desc, extra_shapes=0):
        super().__init__(yh, desc)
        src = desc.contents if hasattr(desc, "contents") else desc
        self.num_shapes = src.num_shapes + extra_shapes
        self.shapes = (yh.Shape * self.num_shapes)(*[yh.Shape.from_buffer_copy(src.shapes[min(i, src.num_shapes - 1)]) for i in range(self.num_shapes)])
        self.d.shapes, self.d.num_shapes = C.cast(self.shapes, C.POINTER(yh.Shape)), self.num_shapes
        self.keep = []

    def arrays(self, i):
        """The shape's arrays as numpy copies (None where the shape has none)."""
        s, out = self.shapes[i], {}
        for name, dtype, cols in ARRAYS:
            n = s.num_vertices if dtype is F else (s.num_lines if name == "lines" else s.num_triangles)
            p = getattr(s, name)
            out[name] = np.ctypeslib.as_array(p, (n, cols) if cols else (n,)).copy() if p and n > 0 else None
        return out

    def set(self, yh, i, **arrays):
        s = self.shapes[i]
        for name, a in arrays.items():
            dtype = dict((n, t) for n, t, _ in ARRAYS)[name]
            if a is None:
                setattr(s, name, C.cast(None, yh.c_float_p if dtype is F else yh.c_int_p))
                continue
            a = np.ascontiguousarray(a, dtype)
            self.keep.append(a)
            setattr(s, name, yh.fptr(a) if dtype is F else yh.iptr(a))
        return self

    def shape_of(self, lines):
        """The first shape made of lines (True) / the first non-emissive triangle shape (False)."""
        for i in range(self.num_shapes):
            users = [o for o in range(self.n) if self.objects[o].shape == i]
            if (self.shapes[i].num_lines > 0) == lines and users and not any(any(self.materials[self.objects[o].material].emission[:]) for o in users):
                return i
        raise AssertionError("no such shape")


def _edited(yh, desc, shape, arrays):
    return Reshaped(yh, desc).set(yh, shape, **{k: v for k, v in arrays.items() if v is not None})


# ---------------------------------------------------------------------------------------------
# the deformations: float32 numpy on a shape's own arrays
# ---------------------------------------------------------------------------------------------
def _tangents(positions, lines):
    """Per-vertex tangents of a line shape: the normalised sum of the directions of the segments at the vertex."""
    d = positions[lines[:, 1]] - positions[lines[:, 0]]
    t = np.zeros_like(positions)
    np.add.at(t, lines[:, 0], d), np.add.at(t, lines[:, 1], d)
    return (t / np.maximum(np.linalg.norm(t, axis=1, keepdims=True), F(1e-20))).astype(F)


def _double(A):
    """Positions x 2 and radius x 2: exact in float, so the tree and the three wide counts are those of the uploaded shape."""
    radius = A["radius"] * F(2) if A["radius"] is not None else np.full(len(A["positions"]), 0.002, F)
    return dict(A, positions=A["positions"] * F(2), radius=radius)


def _sway(A, a):
    p = A["positions"].copy()
    p[:, 0] += F(a) * p[:, 1] * p[:, 1]
    return dict(A, positions=p, normals=_tangents(p, A["lines"]))


def _prim_boxes(A):
    """line_bounds / triangle_bounds (math.h:3037-3044) in float32."""
    if A["lines"] is not None:
        r = A["radius"] if A["radius"] is not None else np.full(len(A["positions"]), 0.001, F)
        p, r = A["positions"][A["lines"]], r[A["lines"]][..., None]
        return np.ascontiguousarray(np.concatenate([(p - r).min(1), (p + r).max(1)], 1), F)
    p = A["positions"][A["triangles"]]
    return np.ascontiguousarray(np.concatenate([p.min(1), p.max(1)], 1), F)


def _wide_counts(yh, A):
    """The shape's 4-, 8- and 16-wide node counts, from the host's collapse."""
    boxes = _prim_boxes(A)
    return [yh.load().yh_bvh_build_wide(len(boxes), yh.fptr(boxes), w, None) for w in (4, 8, 16)]


_SWAY = {}


def _chosen_sway(yh, key, A):
    """(a, counts of the uploaded shape, counts after the sway) for the first a of SWAY_A that grows a count."""
    if key not in _SWAY:
        base = _wide_counts(yh, A)
        for a in SWAY_A:
            now = _wide_counts(yh, _sway(A, a))
            if any(n > b for n, b in zip(now, base)):
                _SWAY[key] = (a, base, now)
                break
        else:
            raise AssertionError(f"{key}: no sway of {SWAY_A} grows a wide-node count over {base}")
    return _SWAY[key]


def _deep_lines(n=72, reach=1000.0, ratio=1 / 3):
    """n disjoint segments along +x, each `ratio` times as far out, as long and as thick as the one before: the middle split
    (pt.cpp:564-595) peels one off per level."""
    s = (F(ratio) ** np.arange(n)).astype(F)
    a = np.stack([F(reach) * s, np.zeros(n, F), np.zeros(n, F)], 1)
    b = a * F(1.05)
    positions = np.stack([a, b], 1).reshape(-1, 3).astype(F)
    lines = np.arange(2 * n, dtype=I32).reshape(n, 2)
    return dict(positions=positions, normals=_tangents(positions, lines), radius=np.repeat(F(0.01 * reach) * s, 2).astype(F), lines=lines, triangles=None, texcoords=None)


def _flat_lines(n=72):
    """The same counts, evenly spaced: a shallow tree."""
    a = np.stack([np.arange(n, dtype=F) * F(0.02), np.full(n, 1.0, F), np.zeros(n, F)], 1)
    b = a + np.array([0.015, 0, 0], F)
    positions = np.stack([a, b], 1).reshape(-1, 3).astype(F)
    lines = np.arange(2 * n, dtype=I32).reshape(n, 2)
    return dict(positions=positions, normals=_tangents(positions, lines), radius=np.full(2 * n, 0.004, F), lines=lines, triangles=None, texcoords=None)


def _small_lines_descriptions(yh, sf):
    """sphere-hairblock with its hair replaced by 72 flat segments (uploads), and by the 72 deep ones (too deep)."""
    flat, deep = Reshaped(yh, sf.desc), Reshaped(yh, sf.desc)
    s = flat.shape_of(True)
    for d, A in ((flat, _flat_lines()), (deep, _deep_lines())):
        d.shapes[s].num_vertices, d.shapes[s].num_lines = len(A["positions"]), len(A["lines"])
        d.set(yh, s, **{k: v for k, v in A.items() if v is not None})
    return flat, deep, s


def _flip_descriptions(yh, sf):
    """The 46-object crowd with its balls where they are, on their grid, but ball k of either half 0.45 times the size of ball
    k - 1, the second half turned by 180 degrees about y: an object's centroid is its grid place plus its scale times the ball
    shape's centre. Centred (as loaded) the centroids are the grid's and the scene tree is balanced — few nodes, the kernels' LDS
    table. With the shape moved out to x = 1e10 (where float32 collapses it to a point) the centroids lie on two geometric rows
    that dwarf the grid — nearly a node per ball, 4-wide nodes."""
    centred = Reshaped(yh, sf.desc)
    ball = centred.shape_of(False)
    balls = [o for o in range(centred.n) if centred.objects[o].shape == ball]
    for k, o in enumerate(balls):
        s, turn = 0.45 ** (k // 2), -1 if k % 2 else 1
        centred.objects[o].frame[:] = _f32([turn * s, 0, 0, 0, s, 0, 0, 0, turn * s] + list(centred.objects[o].frame[9:12]))
    A = centred.arrays(ball)
    moved = Reshaped(yh, centred.d).set(yh, ball, positions=A["positions"] + np.array([1e10, 0, 0], F))
    return centred, moved, ball


# ---------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------
NEW_ENTRIES = ("yh_update_shape", "yh_update_shape_device", "yh_shape_nodes")


def test_library_exports_header_declares_and_binding_lists_the_entry_points(yh):
    lib = yh.load()
    header = open(os.path.join(ROOT, "include", "yhair.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libyhair.so")], capture_output=True, text=True, check=True).stdout
    for name in NEW_ENTRIES:
        assert hasattr(lib, name) and f" T {name}\n" in exported, name
        assert name in yh.EXPORTS
    assert "int yh_update_shape(yh_context* ctx, int shape, const yh_shape* now);" in header
    assert "int yh_update_shape_device(yh_context* ctx, int shape, const yh_shape* now);" in header
    assert "int yh_shape_nodes(const yh_context* ctx, int shape, int64_t offset[3], int count[3], int room[3]);" in header
    for method in ("update_shape", "update_shape_device", "shape_nodes"):
        assert callable(getattr(yh.Context, method))
    shape = yh.Shape()
    assert lib.yh_update_shape(None, 0, C.byref(shape)) == yh.YH_E_INVALID and lib.yh_update_shape_device(None, 0, None) == yh.YH_E_INVALID
    assert lib.yh_shape_nodes(None, 0, None, None, None) == yh.YH_E_INVALID


def test_the_edits_exercise_what_they_claim(yh):
    """`double` keeps the three wide counts, the chosen `sway` grows at least one, on every shape the GPU tests sway; `deep` needs
    more stack than the library has and stays under 128 levels, the flat segments and ordinary hair stay far below; the two
    descriptions of the form flip lie at least 8 nodes on either side of the 10 KB line of the scene-level table."""
    lib = yh.load()
    lib.yhk_stack_entries.restype = C.c_int
    limit = lib.yhk_stack_entries()
    for key, (name, kw) in dict(SIZES, crowd=CROWD, field=FIELD).items():
        sf = yh.SceneFile(scene_path(name, **kw))
        d = Reshaped(yh, sf.desc)
        s = d.shape_of(True)
        A = d.arrays(s)
        a, base, now = _chosen_sway(yh, key, A)
        levels = _levels(yh, _prim_boxes(A))[1]
        print(f"{key}: {len(A['lines'])} segments, {levels} levels, wide counts {base}; double {_wide_counts(yh, _double(A))}; sway a = {a}: {now}")
        assert _wide_counts(yh, _double(A)) == base
        assert any(n > b for n, b in zip(now, base))
        assert 3 * (1 + (levels - 2) // 2) + 8 <= limit // 2, "ordinary hair stays far below the stack limit"
        assert (len(A["lines"]) >= 32768) == (key in ("device-built", "crowd"))
        sf.close()
    sf = yh.SceneFile(scene_path(*HAIRBLOCK[:1], **HAIRBLOCK[1]))
    flat, deep, s = _small_lines_descriptions(yh, sf)
    lf, ld = _levels(yh, _prim_boxes(flat.arrays(s)))[1], _levels(yh, _prim_boxes(deep.arrays(s)))[1]
    need_flat, need_deep = _stack_need(yh, flat.d, _tree(yh, flat.d)[1], False), _stack_need(yh, deep.d, _tree(yh, deep.d)[1], False)
    print(f"deep: {ld} levels, {need_deep} stack entries (limit {limit}); flat: {lf} levels, {need_flat} entries")
    assert 60 < ld < 128 and need_deep > limit == 96 and need_flat < limit // 2
    sf.close()
    sf = yh.SceneFile(scene_path(*FLIP[:1], **FLIP[1]))
    centred, moved, _ = _flip_descriptions(yh, sf)
    n = centred.n
    (nc, lc), (nm, lm) = _tree(yh, centred.d), _tree(yh, moved.d)
    at = next(k for k in range(4 * n) if _lds_f4(n, k) * 16 > 10240)
    print(f"flip: {n} objects; centred {nc} nodes / {lc} levels, moved {nm} / {lm}; wide from {at} nodes")
    assert n == 46 and nc <= at - 1 - 8 and nm >= at + 8
    assert _stack_need(yh, centred.d, lc, False) <= limit and _stack_need(yh, moved.d, lm, True) <= limit  # both upload
    sf.close()


def _compile_mirror_test(tmp_path):
    exe = str(tmp_path / "mirror_shape_edits")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host"), "-Wno-class-memaccess", os.path.join(ROOT, "tests", "cpp", "test_mirror_shape_edits.cpp"),
                           "-o", exe, "-L" + PKG, "-lyhair", "-Wl,-rpath," + PKG, "-lpthread"])
    return exe


def test_mirror_classifies_shape_edits_without_a_device(built, tmp_path):
    """Without the opt-in a position edit is classified as before; with it, edit_shapes; edit_upload again as soon as a count or an
    index differs — checked by the C++ program itself (tests/cpp/test_mirror_shape_edits.cpp)."""
    exe = _compile_mirror_test(tmp_path)
    r = subprocess.run([exe, "--classify"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


# ---------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes(yh):
    """Scene files by (name, options), loaded once."""
    held = {}

    def get(name, kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in held:
            held[key] = yh.SceneFile(scene_path(name, **kw))
        return held[key]
    yield get
    for sf in held.values():
        sf.close()


def _cases(yh, key, sf):
    """base, its line shape, and the descriptions of `double` and `sway` with what the CPU says of their wide counts."""
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    A = base.arrays(s)
    a, cnt0, cnt1 = _chosen_sway(yh, key, A)
    return base, s, _edited(yh, sf.desc, s, _double(A)), _edited(yh, sf.desc, s, _sway(A, a)), cnt0, cnt1


# ---- 1. both hairblock sizes: in place, growing, and back into the appended room ----
@pytest.mark.gpu
@pytest.mark.parametrize("edit", ["double", "sway", "back"])
@pytest.mark.parametrize("size", list(SIZES))
def test_hair_edit_renders_as_a_fresh_upload(ctx, yh, scenes, size, edit):
    base, s, dbl, swy, cnt0, cnt1 = _cases(yh, size, scenes(*SIZES[size]))
    ctx.upload_scene(base.ptr)
    off0, got0, room0 = ctx.shape_nodes(s)
    assert got0 == cnt0 == room0, "an upload gives every width exactly the room its nodes take"
    if edit == "double":
        ctx.update_shape(s, dbl.shapes[s])
        assert ctx.shape_nodes(s) == (off0, cnt0, room0), "the same tree: written in place"
        _check(_results(ctx, yh, dbl.d, True), _fresh_results(yh, f"shape-{size}-double", dbl.d, True), f"{size} double")
        return
    ctx.update_shape(s, swy.shapes[s])
    off1, got1, room1 = ctx.shape_nodes(s)
    grew = [b > a for a, b in zip(cnt0, cnt1)]
    print(f"{size}: counts {cnt0} -> {cnt1}, offsets {off0} -> {off1}, room {room1}")
    assert got1 == cnt1 and any(grew)
    assert [a != b for a, b in zip(off0, off1)] == grew, "exactly the widths that grew move"
    assert room1 == [c + c // 8 if g else r for c, g, r in zip(cnt1, grew, room0)]
    assert all(o % 4 == 0 for o in off1)
    if edit == "sway":
        got = _results(ctx, yh, swy.d, True)
        _check(got, _fresh_results(yh, f"shape-{size}-sway", swy.d, True), f"{size} sway")
        assert _differs(got, _fresh_results(yh, f"shape-{size}-base", base.d, True)), "the edit changed nothing"
        return
    ctx.update_shape(s, base.shapes[s])
    assert ctx.shape_nodes(s) == (off1, cnt0, room1), "the uploaded arrays again fit the appended room"
    _check(_results(ctx, yh, base.d, True), _fresh_results(yh, f"shape-{size}-base", base.d, True), f"{size} back")


@pytest.mark.gpu
def test_double_passes_a_radius_where_the_upload_had_none(ctx, yh, scenes):
    sf = scenes(*HAIRBLOCK)
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    base.set(yh, s, radius=None)
    A = base.arrays(s)
    assert A["radius"] is None
    new = Reshaped(yh, sf.desc).set(yh, s, **{k: v for k, v in _double(A).items() if v is not None})
    assert np.all(new.arrays(s)["radius"] == F(0.002))
    ctx.upload_scene(base.ptr)
    nodes = ctx.shape_nodes(s)
    ctx.update_shape(s, new.shapes[s])
    assert ctx.shape_nodes(s) == nodes
    _check(_results(ctx, yh, new.d, True), _fresh_results(yh, "shape-noradius-double", new.d, True), "radius 0.001 -> 0.002")


# ---- 2. crowd: every launch shape, the wide scene level ----
@pytest.mark.gpu
@pytest.mark.parametrize("shape", INSTANCE_SHAPES)
def test_crowd_hair_sways_under_every_launch_shape(ctx, yh, scenes, shape, monkeypatch):
    base, s, _, swy, cnt0, cnt1 = _cases(yh, "crowd", scenes(*CROWD))
    monkeypatch.setenv("YHAIR_SHAPE", shape)
    ctx.upload_scene(base.ptr)
    ctx.update_shape(s, swy.shapes[s])
    assert ctx.shape_nodes(s)[1] == cnt1
    got = _results(ctx, yh, swy.d, False)
    assert ctx.launch_shape() == int(shape)
    _check(got, _fresh_results(yh, "shape-crowd-sway", swy.d), f"crowd sway, shape {shape}")


# ---- 3. topology and triangle shapes ----
@pytest.mark.gpu
@pytest.mark.parametrize("how", ["ends-swapped", "order-reversed"])
def test_another_topology_with_the_same_counts(ctx, yh, scenes, how):
    sf = scenes(*HAIRBLOCK)
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    lines = base.arrays(s)["lines"]
    new = Reshaped(yh, sf.desc).set(yh, s, lines=lines[:, ::-1] if how == "ends-swapped" else lines[::-1])
    ctx.upload_scene(base.ptr)
    ctx.update_shape(s, new.shapes[s])
    got = _results(ctx, yh, new.d, True)
    _check(got, _fresh_results(yh, "shape-" + how, new.d, True), how)
    want = _fresh_results(yh, "shape-host-built-base", base.d, True)
    assert not all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got["hits"], want["hits"])), "elements and uv follow the indices"


@pytest.mark.gpu
def test_squashed_sphere(ctx, yh, scenes):
    sf = scenes(*HAIRBLOCK)
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(False)
    assert base.shapes[s].num_triangles > 0 and base.shapes[s].texcoords
    new = Reshaped(yh, sf.desc).set(yh, s, positions=base.arrays(s)["positions"] * np.array([1, 0.5, 1], F))
    ctx.upload_scene(base.ptr)
    ctx.update_shape(s, new.shapes[s])
    got = _results(ctx, yh, new.d, True)
    _check(got, _fresh_results(yh, "shape-squash", new.d, True), "squash")
    assert _differs(got, _fresh_results(yh, "shape-host-built-base", base.d, True)), "the edit changed nothing"


def _textured_with_the_floors_own_quad(yh, sf):
    """textured with one more shape, a copy of the quad, for the non-emissive object that names the quad."""
    base = Reshaped(yh, sf.desc, extra_shapes=1)
    own = base.num_shapes - 1
    quad = next(i for i in range(own) if base.shapes[i].num_triangles == 2)
    base.shapes[own] = type(base.shapes[0]).from_buffer_copy(base.shapes[quad])
    floor = next(o for o in range(base.n) if base.objects[o].shape == quad and not any(base.materials[base.objects[o].material].emission[:]))
    assert base.materials[base.objects[floor].material].color_tex > 0
    base.objects[floor].shape = own
    return base, own


@pytest.mark.gpu
def test_texcoord_edit_on_textureds_quad(ctx, yh, scenes):
    sf = scenes(*TEXTURED)
    base, own = _textured_with_the_floors_own_quad(yh, sf)
    new, _ = _textured_with_the_floors_own_quad(yh, sf)
    uv = base.arrays(own)["texcoords"]
    new.set(yh, own, texcoords=(uv * F(0.5) + F(0.25))[:, ::-1])
    ctx.upload_scene(base.ptr)
    before = _results(ctx, yh, base.d, False)
    ctx.update_shape(own, new.shapes[own])
    got = _results(ctx, yh, new.d, False)
    _check(got, _fresh_results(yh, "shape-textured-uv", new.d), "texcoords")
    assert _differs(got, before), "the edit changed nothing"
    for a, b in zip(got["hits"], before["hits"]):  # (the geometry stays)
        assert np.array_equal(_bits(a), _bits(b))


# ---- 4. fur-field: one tuft shape under 256 objects ----
@pytest.mark.gpu
def test_every_tuft_of_the_field_sways(ctx, yh, scenes):
    base, s, _, swy, cnt0, cnt1 = _cases(yh, "field", scenes(*FIELD))
    assert sum(base.objects[o].shape == s for o in range(base.n)) == 256
    ctx.upload_scene(base.ptr)
    before = _results(ctx, yh, base.d, False)
    ctx.update_shape(s, swy.shapes[s])
    assert ctx.shape_nodes(s)[1] == cnt1
    got = _results(ctx, yh, swy.d, False)
    _check(got, _fresh_results(yh, "shape-field-sway", swy.d), "tufts sway")
    assert _differs(got, before), "the edit changed nothing"


# ---- 5. the device form ----
def _on_device(A):
    import torch
    return {k: torch.from_numpy(v).cuda() if v is not None else None for k, v in A.items()}


def _torch_tangents(p, lines):
    import torch
    a, b = lines[:, 0].long(), lines[:, 1].long()
    d = p[b] - p[a]
    t = torch.zeros_like(p).index_add_(0, a, d).index_add_(0, b, d)
    return (t / torch.clamp(torch.linalg.norm(t, dim=1, keepdim=True), min=1e-20)).contiguous()


def _description_of(yh, desc, s, T):
    return _edited(yh, desc, s, {k: v.cpu().numpy() if v is not None else None for k, v in T.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("edit", ["double", "sway", "back"])
@pytest.mark.parametrize("size", list(SIZES))
def test_device_form_renders_as_a_fresh_upload_of_the_tensors(ctx, yh, scenes, size, edit):
    """The deformations in torch on the GPU, passed by pointer (the small hair is thereby built on the device); the yardstick
    uploads the tensors' .cpu() copies."""
    import torch
    sf = scenes(*SIZES[size])
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    A = base.arrays(s)
    a = _chosen_sway(yh, size, A)[0]
    T = _on_device(A)
    ctx.upload_scene(base.ptr)
    off0 = ctx.shape_nodes(s)[0]
    if edit == "double":
        T = dict(T, positions=T["positions"] * 2, radius=T["radius"] * 2)
    else:
        p = T["positions"].clone()
        p[:, 0] += a * p[:, 1] * p[:, 1]
        T = dict(T, positions=p, normals=_torch_tangents(p, T["lines"]))
    ctx.update_shape_device(s, T["positions"], normals=T["normals"], radius=T["radius"], lines=T["lines"])
    new = _description_of(yh, sf.desc, s, T)
    assert ctx.shape_nodes(s)[1] == _wide_counts(yh, new.arrays(s))
    if edit == "double":
        assert ctx.shape_nodes(s)[0] == off0
    if edit == "back":
        off1 = ctx.shape_nodes(s)[0]
        T = _on_device(A)
        ctx.update_shape_device(s, T["positions"], normals=T["normals"], radius=T["radius"], lines=T["lines"])
        new = base
        assert ctx.shape_nodes(s)[0] == off1
    torch.cuda.synchronize()
    key = f"shape-{size}-base" if edit == "back" else f"shape-{size}-{edit}-torch"
    _check(_results(ctx, yh, new.d, True), _fresh_results(yh, key, new.d, True), f"device form, {size} {edit}")


@pytest.mark.gpu
def test_device_form_squashes_the_sphere(ctx, yh, scenes):
    """A triangle shape with texcoords and no radius through the device form: the per-vertex rows (vpos, vtex, elems) are written
    from the caller's device arrays."""
    import torch
    sf = scenes(*HAIRBLOCK)
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(False)
    T = _on_device(base.arrays(s))
    assert T["radius"] is None and T["texcoords"] is not None and T["lines"] is None
    T = dict(T, positions=(T["positions"] * torch.tensor([1, 0.5, 1], device="cuda")).contiguous(), texcoords=T["texcoords"].flip(1).contiguous())
    ctx.upload_scene(base.ptr)
    ctx.update_shape_device(s, T["positions"], normals=T["normals"], triangles=T["triangles"], texcoords=T["texcoords"])
    new = _description_of(yh, sf.desc, s, T)
    assert ctx.shape_nodes(s)[1] == _wide_counts(yh, new.arrays(s))
    got = _results(ctx, yh, new.d, True)
    _check(got, _fresh_results(yh, "shape-squash-torch", new.d, True), "device form, squash")
    assert _differs(got, _fresh_results(yh, "shape-host-built-base", base.d, True)), "the edit changed nothing"
    with pytest.raises(yh.YhError, match="positions"):
        ctx.update_shape_device(s, None, triangles=T["triangles"])
    with pytest.raises(yh.YhError, match="torch tensor"):
        ctx.update_shape_device(s, base.arrays(s)["positions"], triangles=T["triangles"])


# ---- 6. interplay with the other edits ----
@pytest.mark.gpu
@pytest.mark.parametrize("order", ["shape-then-objects", "objects-then-shape"])
def test_shape_edit_with_object_material_and_camera_edits(ctx, yh, scenes, order):
    sf = scenes(*HAIRBLOCK)
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    A = base.arrays(s)
    final = _edited(yh, sf.desc, s, _sway(A, _chosen_sway(yh, "host-built", A)[0]))
    hair = final.index(lines=True)[0]
    final.objects[hair].frame[:] = _compose(_translation(-0.3, 0.2, 0.25), _compose(final.objects[hair].frame[:], _rotation((1, 1, 0.3), 30)))
    ctx.upload_scene(base.ptr)
    if order == "shape-then-objects":
        ctx.update_shape(s, final.shapes[s])
        ctx.update_objects(hair, final.rows(yh, hair, 1))
    else:
        ctx.update_objects(hair, final.rows(yh, hair, 1))
        ctx.update_shape(s, final.shapes[s])
    _check(_results(ctx, yh, final.d, True), _fresh_results(yh, "shape-interplay", final.d, True), order)
    m = final.materials[final.objects[hair].material]
    m.beta_m, m.eumelanin, m.pheomelanin = 0.6, 0.4, 0.3
    m.sigma_a[:] = [0.0, 0.0, 0.0]
    final.camera.aperture, final.camera.focus = 0.1, 4.0
    ctx.update_materials(0, final.materials)
    ctx.update_camera(final.camera)
    _check(_results(ctx, yh, final.d, True), _fresh_results(yh, "shape-interplay-material-camera", final.d, True), order + ", then material and camera")


# ---- 7. refusals ----
def _argument_refusals(yh, sf):
    """name -> (which entry, shape index, the yh_shape to pass or None)."""
    d = Reshaped(yh, sf.desc)
    hair, sphere = d.shape_of(True), d.shape_of(False)

    def changed(i, **fields):
        s = type(d.shapes[0]).from_buffer_copy(d.shapes[i])
        for k, v in fields.items():
            setattr(s, k, v)
        return s

    H, S = d.shapes[hair], d.shapes[sphere]
    bad_lines = d.arrays(hair)["lines"]
    bad_lines[len(bad_lines) // 2, 1] = H.num_vertices
    neg_tris = d.arrays(sphere)["triangles"]
    neg_tris[-1, 0] = -1
    d.keep += [bad_lines, neg_tris]
    return {
        "null": (hair, None),
        "shape-negative": (-1, changed(hair)),
        "shape-behind-the-list": (d.num_shapes, changed(hair)),
        "fewer-vertices": (hair, changed(hair, num_vertices=H.num_vertices - 1)),
        "more-lines": (hair, changed(hair, num_lines=H.num_lines + 1)),
        "fewer-triangles": (sphere, changed(sphere, num_triangles=S.num_triangles - 1)),
        "triangle-count-on-a-line-shape": (hair, changed(hair, num_triangles=2)),
        "lines-against-triangles": (sphere, changed(hair, num_vertices=S.num_vertices)),
        "triangles-against-lines": (hair, changed(sphere, num_vertices=H.num_vertices)),
        "normals-dropped": (hair, changed(hair, normals=None)),
        "texcoords-added": (hair, changed(hair, texcoords=H.positions)),
        "texcoords-dropped": (sphere, changed(sphere, texcoords=None)),
        "positions-null": (hair, changed(hair, positions=None)),
        "lines-null": (hair, changed(hair, lines=None)),
        "index-past-the-vertices": (hair, changed(hair, lines=yh.iptr(bad_lines))),
        "index-negative": (sphere, changed(sphere, triangles=yh.iptr(neg_tris))),
    }, d


ARGUMENT_REFUSALS = ["null", "shape-negative", "shape-behind-the-list", "fewer-vertices", "more-lines", "fewer-triangles", "triangle-count-on-a-line-shape",
                     "lines-against-triangles", "triangles-against-lines", "normals-dropped", "texcoords-added", "texcoords-dropped", "positions-null", "lines-null",
                     "index-past-the-vertices", "index-negative"]


@pytest.fixture(scope="module")
def refusal_baseline(yh, scenes):
    """2 + 2 samples on the untouched scene, from a context of its own: what every refused context must go on rendering."""
    return _fresh(yh, scenes(*HAIRBLOCK).desc, spp=2, first=2, res=RES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ARGUMENT_REFUSALS)
def test_refused_arguments_leave_the_context_rendering(ctx, yh, scenes, refusal_baseline, name):
    calls, _keep = _argument_refusals(yh, scenes(*HAIRBLOCK))
    index, shape = calls[name]
    ctx.upload_scene(scenes(*HAIRBLOCK).desc)
    ctx.set_shard(0, 1)
    ctx.init_state(yh.TraceParams.default(resolution=RES))
    ctx.trace_samples(2)
    assert ctx.lib.yh_update_shape(ctx.h, index, C.byref(shape) if shape is not None else None) == yh.YH_E_INVALID, name
    assert ctx.lib.yh_last_error(ctx.h).decode().startswith("yh_update_shape:"), ctx.lib.yh_last_error(ctx.h)
    ctx.trace_samples(2)  # the image state is still there, and the scene is the earlier one
    _same((ctx.download(), ctx.download_rng()), refusal_baseline, name)
    assert ctx.scene_once() == refusal_baseline[2]


def _refused_by_its_result(ctx, yh, base, call, entry, words):
    """Upload `base`, render 2 samples, try the edit, render 2 more: refused with `words`, the 2 + 2 samples and 256 closest hits
    are a fresh upload's."""
    want = _fresh(yh, base.ptr, spp=2, first=2, res=RES)
    ctx.upload_scene(base.ptr)
    ctx.set_shard(0, 1)
    ctx.init_state(yh.TraceParams.default(resolution=RES))
    ctx.trace_samples(2)
    with pytest.raises(yh.YhError) as refused:
        call()
    message = str(refused.value)
    assert f"yhair error {yh.YH_E_INVALID}: {entry}:" in message and all(w in message for w in words), message
    ctx.trace_samples(2)
    _same((ctx.download(), ctx.download_rng()), want, message)
    rays = _rays_at(base.d)
    fresh = yh.Context(0)
    fresh.upload_scene(base.ptr)
    for a, b in zip(ctx.intersect(rays), fresh.intersect(rays)):
        assert np.array_equal(_bits(a), _bits(b))
    fresh.close()


@pytest.mark.gpu
def test_an_out_of_range_index_is_refused_in_the_device_form(ctx, yh, scenes):
    import torch
    base = Reshaped(yh, scenes(*HAIRBLOCK).desc)
    s = base.shape_of(True)
    T = _on_device(base.arrays(s))
    T["lines"][7, 0] = base.shapes[s].num_vertices
    torch.cuda.synchronize()
    _refused_by_its_result(ctx, yh, base, lambda: ctx.update_shape_device(s, T["positions"], normals=T["normals"], radius=T["radius"], lines=T["lines"]),
                           "yh_update_shape_device", ["vertex index out of range"])


@pytest.mark.gpu
def test_normals_where_the_upload_had_none_are_refused(ctx, yh, scenes):
    sf = scenes(*HAIRBLOCK)
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    base.set(yh, s, normals=None)
    with_normals = Reshaped(yh, sf.desc)
    _refused_by_its_result(ctx, yh, base, lambda: ctx.update_shape(s, with_normals.shapes[s]), "yh_update_shape", ["normals"])


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["crowd", "scene-once-full"])
def test_the_shape_of_an_emitter_is_refused(ctx, yh, scenes, scene):
    sf = scenes(*CROWD) if scene == "crowd" else scenes("scene-once", dict(variant="full"))
    base = Reshaped(yh, sf.desc)
    light = base.index(emissive=True)[0]
    s = base.objects[light].shape
    new = Reshaped(yh, sf.desc).set(yh, s, positions=base.arrays(s)["positions"] * F(1.5))
    _refused_by_its_result(ctx, yh, base, lambda: ctx.update_shape(s, new.shapes[s]), "yh_update_shape", ["emits"])


@pytest.mark.gpu
def test_a_tree_too_deep_is_refused_as_its_upload_is(ctx, yh, scenes):
    flat, deep, s = _small_lines_descriptions(yh, scenes(*HAIRBLOCK))
    fresh = yh.Context(0)
    with pytest.raises(yh.YhError, match="BVH too deep for the traversal stack"):
        fresh.upload_scene(deep.ptr)
    fresh.close()
    _refused_by_its_result(ctx, yh, flat, lambda: ctx.update_shape(s, deep.shapes[s]), "yh_update_shape", ["BVH too deep for the traversal stack"])


@pytest.mark.gpu
@pytest.mark.parametrize("way", ["table-to-wide", "wide-to-table"])
def test_a_scene_level_that_changes_its_form_is_refused(ctx, yh, scenes, way):
    centred, moved, ball = _flip_descriptions(yh, scenes(*FLIP))
    base, new = (centred, moved) if way == "table-to-wide" else (moved, centred)
    _refused_by_its_result(ctx, yh, base, lambda: ctx.update_shape(ball, new.shapes[ball]), "yh_update_shape", ["upload the scene", "scene level"])


# ---- 8. call order ----
@pytest.mark.gpu
def test_call_order(yh, scenes):
    base = Reshaped(yh, scenes(*HAIRBLOCK).desc)
    s = base.shape_of(True)
    c = yh.Context(0)
    off, cnt, room = (C.c_int64 * 3)(), (C.c_int * 3)(), (C.c_int * 3)()
    assert c.lib.yh_update_shape(c.h, s, C.byref(base.shapes[s])) == yh.YH_E_STATE  # before an upload
    assert c.lib.yh_update_shape_device(c.h, s, C.byref(base.shapes[s])) == yh.YH_E_STATE
    assert c.lib.yh_shape_nodes(c.h, s, off, cnt, room) == yh.YH_E_STATE
    c.upload_scene(base.ptr)
    c.init_state(yh.TraceParams.default(resolution=RES))
    c.trace_samples(1)
    c.update_shape(s, base.shapes[s])  # (an edit that changes no value is an edit all the same)
    assert c.lib.yh_trace_samples(c.h, 1) == yh.YH_E_STATE
    c.init_state(yh.TraceParams.default(resolution=RES))
    c.trace_samples(1)
    c.close()


# ---- 9. the mirror ----
@pytest.mark.gpu
def test_mirror_passes_shape_edits_on_with_the_opt_in(built, tmp_path):
    """set_positions on the hair after an init_state, with set_shape_edits: one upload and one edit, pixels those of a scene built
    that way from the start; without the opt-in: a second upload."""
    exe = _compile_mirror_test(tmp_path)
    r = subprocess.run([exe, scene_path(*HAIRBLOCK[:1], **HAIRBLOCK[1])], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)
