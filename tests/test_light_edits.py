"""yh_set_light_edits: with the opt-in, the seven edits that change the LIGHT LIST of an uploaded scene — an emission turned on or off
(yh_update_materials, yh_update_environments), an object that takes or loses an emitter's material (yh_update_objects), the vertices
of an emitter's shape (yh_update_shape / _device, yh_refit_shape / _device) — make the list again by the upload's rule, on the device
(unit/light_list.hip), instead of refusing. yh_light_list, the unit-level pair yh_triangle_cdf / yh_triangle_cdf_gpu, the Python
binding and the C++ mirror's opt-in (set_light_edits).

The yardstick of every edit is a FRESH context that got yh_upload_scene of the edited description (tests/test_object_edits.py): images
as uint32 and RNG states at 48 x 48, 2 spp, 256 rays of yh_intersect_batch, 256 rows of yh_lights_batch in both forms, yh_scene_once,
yh_intersect_plain_batch in both forms where the scene is plain, yh_light_list and whether the GENERAL variant runs must be the same
bits. A fresh upload's results are computed once per edited description and shared.

The session's context is shared with the suites that pin the refusals: every test here that opts in opts out again (`lit`).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_scene_edits import _lookat
from test_object_edits import HAIRBLOCK, INSTANCE_SHAPES, Moved, _check, _differs, _f32, _fresh_results, _results
from test_shape_edits import Reshaped

F, I32 = np.float32, np.int32
PKG = os.path.join(ROOT, "yocto-hair_amd")
CDF_SIZES = (1, 2, 4, 5, 63, 64, 65, 128, 129, 4097)
NEW_ENTRIES = ("yh_set_light_edits", "yh_light_list", "yh_triangle_cdf", "yh_triangle_cdf_gpu")
LIGHTS_UNIT = ("lights-unit", dict(scale=0.05))
LIGHTS_UNIT_BIG = ("lights-unit", dict(scale=0.05, biglight=True))


# ---------------------------------------------------------------------------------------------
# the unit-level pair: triangles whose areas spread over six orders of magnitude
# ---------------------------------------------------------------------------------------------
def _cdf_triangles(n, seed=7):
    """n triangles on 3 n vertices of their own, edge lengths 10^-3 .. 1 (areas over six orders of magnitude), every third of them
    large, and one without area (n >= 2: two of its vertices coincide)."""
    rng = np.random.default_rng(seed + n)
    size = (10.0 ** rng.uniform(-3, 0, n)).astype(F)
    size[::3] = F(1) + size[::3]
    p0 = rng.uniform(-1, 1, (n, 3)).astype(F)
    e1, e2 = (rng.normal(size=(n, 3)) * size[:, None]).astype(F), (rng.normal(size=(n, 3)) * size[:, None]).astype(F)
    positions = np.stack([p0, p0 + e1, p0 + e2], 1).astype(F)
    if n >= 2:
        positions[n // 2, 2] = positions[n // 2, 1]
    positions = positions.reshape(-1, 3)
    return positions, np.arange(3 * n, dtype=I32).reshape(n, 3)


def _areas(positions, triangles):
    """triangle_area (math.h:3306) in float32, the reference's operation order."""
    p0, p1, p2 = (positions[triangles[:, k]] for k in range(3))
    a, b = p1 - p0, p2 - p0
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    return np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]) / F(2)


def _chain(area):
    out, run = np.zeros(len(area), F), None
    for t, a in enumerate(area):
        run = F(a) if run is None else F(a + run)
        out[t] = run
    return out


def _tree_scan(area):
    """What a wave's log-step scan gives: x[i] += x[i - d] for d = 1, 2, 4, ..."""
    x, d = area.copy(), 1
    while d < len(x):
        x[d:] = x[d:] + x[:-d].copy()
        d *= 2
    return x


def test_library_exports_header_declares_and_binding_lists_the_entry_points(yh):
    lib = yh.load()
    header = open(os.path.join(ROOT, "include", "yhair.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libyhair.so")], capture_output=True, text=True, check=True).stdout
    for name in NEW_ENTRIES:
        assert hasattr(lib, name) and f" T {name}\n" in exported, name
        assert name in yh.EXPORTS
    for line in ("int yh_set_light_edits(yh_context* ctx, int on);",
                 "int yh_light_list(const yh_context* ctx, int* object, int* environment, int* cdf_count, int* in_lds, int capacity);",
                 "int yh_triangle_cdf(int num_vertices, const float* positions, int num_triangles, const int* triangles, float* cdf);",
                 "int yh_triangle_cdf_gpu(yh_context* ctx, int num_vertices, const float* positions, int num_triangles, const int* triangles, float* cdf);"):
        assert line in header, line
    for method in ("set_light_edits", "light_list", "triangle_cdf_gpu"):
        assert callable(getattr(yh.Context, method))
    assert callable(yh.triangle_cdf)
    assert lib.yh_set_light_edits(None, 1) == lib.yh_light_list(None, None, None, None, None, 0) == yh.YH_E_INVALID
    assert lib.yh_triangle_cdf_gpu(None, 0, None, 0, None, None) == yh.YH_E_INVALID


@pytest.mark.parametrize("n", CDF_SIZES)
def test_host_cdf_is_the_sequential_float_chain(yh, n):
    """yh_triangle_cdf against area[t] + cdf[t - 1] in float32 numpy, one addition after the other. The inputs must be able to tell a
    reordered sum from the chain: from n = 63 on, a log-step scan and a float64 sum rounded at the end both differ from it somewhere."""
    positions, triangles = _cdf_triangles(n)
    area = _areas(positions, triangles)
    want = _chain(area)
    if n >= 2:
        assert area[n // 2] == 0 and want[n // 2] == want[n // 2 - 1], "the triangle without area: a tie in the cdf"
    if n >= 63:
        assert area.max() / area[area > 0].min() > 1e5
        assert not np.array_equal(_tree_scan(area), want), "a log-step scan gives the chain's bits on these inputs: they test nothing"
        assert not np.array_equal(np.cumsum(area.astype(np.float64)).astype(F), want), "a float64 sum gives the chain's bits on these inputs"
    got = yh.triangle_cdf(positions, triangles)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_host_cdf_refuses_an_index_outside_the_vertices(yh):
    lib = yh.load()
    positions, triangles = _cdf_triangles(5)
    out = np.zeros(5, F)
    for bad in (15, -1, 1 << 30):
        t = triangles.copy()
        t[3, 1] = bad
        assert lib.yh_triangle_cdf(15, yh.fptr(positions), 5, yh.iptr(t), yh.fptr(out)) == yh.YH_E_INVALID
        with pytest.raises(yh.YhError):
            yh.triangle_cdf(positions, t)
    assert lib.yh_triangle_cdf(15, yh.fptr(positions), 5, yh.iptr(triangles), yh.fptr(out)) == yh.YH_OK
    assert lib.yh_triangle_cdf(15, yh.fptr(positions), 0, yh.iptr(triangles), yh.fptr(out)) == yh.YH_E_INVALID
    assert lib.yh_triangle_cdf(15, None, 5, yh.iptr(triangles), yh.fptr(out)) == yh.YH_E_INVALID


def _compile_mirror_test(tmp_path):
    exe = str(tmp_path / "mirror_light_edits")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host"), "-Wno-class-memaccess", os.path.join(ROOT, "tests", "cpp", "test_mirror_light_edits.cpp"),
                           "-o", exe, "-L" + PKG, "-lyhair", "-Wl,-rpath," + PKG, "-lpthread"])
    return exe


def test_mirror_classifies_light_edits_without_a_device(built, tmp_path):
    """Without the opt-in an emission toggle is edit_upload as today; with it, an edit of the kind its entry point takes — checked by
    the C++ program itself (tests/cpp/test_mirror_light_edits.cpp)."""
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


@pytest.fixture
def lit(ctx):
    """The session's context with the opt-in on, and off again afterwards: the other suites pin the refusals on it."""
    ctx.set_light_edits(True)
    yield ctx
    ctx.set_light_edits(False)


def _general(c, yh):
    """Whether the scene runs the GENERAL kernel variants: the plain traversal's entry point refuses those."""
    try:
        c.intersect_plain(0, np.zeros((4, 8), F))
        return False
    except yh.YhError as e:
        assert "GENERAL" in str(e), e
        return True


def _all(c, yh, desc):
    """Everything the contract names (tests/test_object_edits.py: _results), the light list and the kernel variant."""
    general = _general(c, yh)
    out = _results(c, yh, desc, not general)
    out["general"], out["list"] = general, c.light_list()
    return out


_FRESH = {}


def _fresh_all(yh, key, desc):
    if key not in _FRESH:
        forced = os.environ.pop("YHAIR_SHAPE", None)
        c = yh.Context(0)
        try:
            c.upload_scene(C.pointer(desc))
            _FRESH[key] = _all(c, yh, desc)
        finally:
            c.close()
            if forced is not None:
                os.environ["YHAIR_SHAPE"] = forced
    return _FRESH[key]


def _check_all(c, yh, key, desc, what):
    got, want = _all(c, yh, desc), _fresh_all(yh, key, desc)
    assert got["list"] == want["list"], f"{what}: yh_light_list {got['list']} against a fresh upload's {want['list']}"
    assert got["general"] == want["general"], f"{what}: the GENERAL variant {'runs' if got['general'] else 'does not run'}, after a fresh upload it is the reverse"
    assert ("plain" in got) == ("plain" in want)
    _check(got, want, what)
    return got


def _material(d, emission=None, color=None):
    """The material row with that emission / colour."""
    for i in range(d.d.num_materials):
        m = d.materials[i]
        if (emission is None or _f32(m.emission[:]) == _f32(emission)) and (color is None or _f32(m.color[:]) == _f32(color)):
            return i
    raise AssertionError("no such material")


def _object(d, material, nth=0):
    return [o for o in range(d.n) if d.objects[o].material == material][nth]


def _lamp_shape(d):
    """The shape of the first object whose material emits."""
    return d.objects[next(o for o in range(d.n) if any(d.materials[d.objects[o].material].emission[:]))].shape


def _copy(yh, d):
    return Reshaped(yh, d.d)


def _black(m):
    m.emission[:] = [0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("n", CDF_SIZES + (40000,))
def test_device_cdf_is_the_hosts(ctx, yh, n):
    positions, triangles = _cdf_triangles(n)
    host, dev = yh.triangle_cdf(positions, triangles), ctx.triangle_cdf_gpu(positions, triangles)
    assert np.array_equal(host.view(np.uint32), dev.view(np.uint32)), f"first difference at {np.flatnonzero(host.view(np.uint32) != dev.view(np.uint32))[:4]}"
    bad = triangles.copy()
    bad[n // 2, 2] = 3 * n
    with pytest.raises(yh.YhError, match="yh_triangle_cdf_gpu"):
        ctx.triangle_cdf_gpu(positions, bad)


# ---- 1. lights-unit: two small quads and the textured sky ----
@pytest.mark.gpu
def test_lights_unit_lights_go_off_and_on_again(lit, yh, scenes):
    """light1 off and on, light2 off and on (yh_update_materials), the sky off and on (yh_update_environments): its cdf comes back by
    a copy, and the second "on" samples as the first upload does."""
    sf = scenes(*LIGHTS_UNIT)
    base = Moved(yh, sf.desc)
    l1, l2 = _material(base, emission=(10, 10, 10)), _material(base, emission=(30, 25, 20))
    lit.upload_scene(base.ptr)
    assert [x[1] for x in lit.light_list()] == [-1, -1, 0] and [x[3] for x in lit.light_list()] == [True, True, False]
    first = _check_all(lit, yh, "lu-base", base.d, "lights-unit as uploaded")
    for name, row in (("light1", l1), ("light2", l2)):
        off = Moved(yh, base.d)
        _black(off.materials[row])
        lit.update_materials(row, [off.materials[row]])
        assert len(lit.light_list()) == 2
        got = _check_all(lit, yh, f"lu-{name}-off", off.d, f"{name} off")
        assert _differs(got, first)
        lit.update_materials(row, [base.materials[row]])
        _check_all(lit, yh, "lu-base", base.d, f"{name} on again")
    off = Moved(yh, base.d)
    off.envs[0].emission[:] = [0, 0, 0]
    lit.update_environments(off.env_array(yh))
    assert [x[1] for x in lit.light_list()] == [-1, -1]
    _check_all(lit, yh, "lu-sky-off", off.d, "the sky off")
    lit.update_environments(base.env_array(yh))
    again = _check_all(lit, yh, "lu-base", base.d, "the sky on again")
    for form in (0, 1):
        assert np.array_equal(again["lights"][form].view(np.uint32), first["lights"][form].view(np.uint32))


@pytest.mark.gpu
def test_lights_unit_objects_take_and_lose_an_emitters_material(lit, yh, scenes):
    """Through yh_update_objects: the floor becomes a light ahead of the two others (every index shifts); light2 takes the floor's
    material; ball0 emits — a light too big for LDS: plain goes to GENERAL — and back."""
    sf = scenes(*LIGHTS_UNIT)
    base = Moved(yh, sf.desc)
    lamp, grey, red = _material(base, emission=(10, 10, 10)), _material(base, color=(0.7, 0.7, 0.7)), _material(base, color=(0.8, 0.2, 0.2))
    floor, ball0, light2 = _object(base, grey), _object(base, red), _object(base, _material(base, emission=(30, 25, 20)))
    lit.upload_scene(base.ptr)
    was = lit.light_list()
    assert floor < min(x[0] for x in was if x[0] >= 0) and not _general(lit, yh)
    step1 = Moved(yh, base.d)
    step1.objects[floor].material = lamp
    lit.update_objects(floor, step1.rows(yh, floor, 1))
    assert [x[0] for x in lit.light_list()][:3] == [floor] + [x[0] for x in was[:2]], "a light ahead of the others: every index shifts"
    _check_all(lit, yh, "lu-floor-lit", step1.d, "the floor takes the light's material")
    step2 = Moved(yh, step1.d)
    step2.objects[light2].material = grey
    lit.update_objects(0, step2.rows(yh))
    _check_all(lit, yh, "lu-light2-dark", step2.d, "light2 takes the floor's material")
    step3 = Moved(yh, step2.d)
    step3.objects[ball0].material = lamp
    lit.update_objects(ball0, step3.rows(yh, ball0, 1))
    assert _general(lit, yh) and (ball0, -1, step3.d.shapes[step3.objects[ball0].shape].num_triangles, False) in lit.light_list()
    _check_all(lit, yh, "lu-ball-lit", step3.d, "ball0 emits")
    lit.update_objects(ball0, step2.rows(yh, ball0, 1))
    assert not _general(lit, yh)
    _check_all(lit, yh, "lu-light2-dark", step2.d, "ball0 dark again")


def _reshape(A):
    """A non-uniform scale and a shear: x' = 1.5 x + 0.25 y, y' = 0.75 y, z' = 1.25 z + 0.125 x (normals stay: a light's are not read)."""
    p = A["positions"]
    q = np.stack([F(1.5) * p[:, 0] + F(0.25) * p[:, 1], F(0.75) * p[:, 1], F(1.25) * p[:, 2] + F(0.125) * p[:, 0]], 1).astype(F)
    return dict(A, positions=q)


def _shape_edit(c, yh, how, s, new):
    """The vertex edit of shape `s` to description `new`, through one of the four entry points."""
    if how in ("update", "refit"):
        (c.update_shape if how == "update" else c.refit_shape)(s, new.shapes[s])
        return
    import torch
    A = new.arrays(s)
    t = {k: torch.from_numpy(v).cuda().contiguous() for k, v in A.items() if v is not None}
    (c.update_shape_device if how == "update-device" else c.refit_shape_device)(s, t["positions"], normals=t.get("normals"), triangles=t["triangles"], texcoords=t.get("texcoords"))


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["update", "update-device", "refit", "refit-device"])
def test_biglight_grid_is_reshaped(lit, yh, scenes, how):
    """The 18-triangle grid of lights-unit (a light read through memory: the GENERAL variant) scaled and sheared, its cdf made from the new
    arrays as they sit on the device."""
    sf = scenes(*LIGHTS_UNIT_BIG)
    base = Reshaped(yh, sf.desc)
    s = next(i for i in range(base.num_shapes) if base.shapes[i].num_triangles == 18)
    new = _copy(yh, base).set(yh, s, positions=_reshape(base.arrays(s))["positions"])
    lit.upload_scene(base.ptr)
    assert _general(lit, yh) and (False, 18) in [(x[3], x[2]) for x in lit.light_list()]
    before = _fresh_all(yh, "big-base", base.d)
    _shape_edit(lit, yh, how, s, new)
    got = _check_all(lit, yh, "big-reshaped", new.d, f"the grid reshaped by {how}")
    assert _differs(got, before) and not np.array_equal(got["lights"][0], before["lights"][0])


# ---- 2. envs-unit: a fan of N triangles; N = 4 has a triangle without area, N = 5 leaves the LDS table ----
# (degenerate: the fan's fourth triangle collapses, so N >= 4)
FAN_CASES = [(n, how) for n in (1, 2, 3, 4, 5) for how in ("update", "update-device")] + [(4, "degenerate"), (5, "degenerate")]


@pytest.mark.gpu
@pytest.mark.parametrize("n,how", FAN_CASES)
def test_fan_light_is_reshaped(lit, yh, scenes, n, how):
    sf = scenes("envs-unit", dict(scale=0.05, variant=f"lights-{n}"))
    base = Reshaped(yh, sf.desc)
    s = _lamp_shape(base)
    assert base.shapes[s].num_triangles == n and base.shapes[s].num_vertices == n + 2
    A = _reshape(base.arrays(s))
    if how == "degenerate":  # rim vertices 3 and 4 coincide: triangle (0, 4, 5) has no area, a tie in the cdf (N = 4: the second one)
        A["positions"][4] = A["positions"][5]
        assert _areas(A["positions"], A["triangles"])[3] == 0
    new = _copy(yh, base).set(yh, s, positions=A["positions"])
    lit.upload_scene(base.ptr)
    assert lit.light_list()[0][2:] == (n, n <= 4) and _general(lit, yh) == (n > 4)
    _shape_edit(lit, yh, "refit" if how == "degenerate" else how, s, new)
    got = _check_all(lit, yh, f"fan-{n}-{'degenerate' if how == 'degenerate' else 'reshaped'}", new.d, f"the fan of {n} by {how}")
    assert _differs(got, _fresh_all(yh, f"fan-{n}-base", base.d))


# ---- 3. envs-unit multi: constant | textured without emission (67 x 63) | sky.hdr | 67 x 63 ----
@pytest.mark.gpu
def test_environments_turn_on_and_off(lit, yh, scenes):
    """b-black (4221 texels >= 4096) turns on: its cdf is made at the edit, and it takes the coarse index over from c-sky behind it;
    c-sky off; all four on."""
    sf = scenes("envs-unit", dict(scale=0.05, variant="multi"))
    base = Moved(yh, sf.desc)
    assert base.n_envs == 4 and not any(base.envs[1].emission[:]) and base.envs[1].tex_width * base.envs[1].tex_height == 4221
    lit.upload_scene(base.ptr)
    assert [x[1] for x in lit.light_list() if x[1] >= 0] == [0, 2, 3]
    b_on = Moved(yh, base.d)
    b_on.envs[1].emission[:] = [1.0, 0.5, 0.25]
    lit.update_environments(b_on.env_array(yh))
    assert [x[1:3] for x in lit.light_list() if x[1] >= 0][:2] == [(0, 0), (1, 4221)]
    got = _check_all(lit, yh, "multi-b-on", b_on.d, "b-black on")
    assert _differs(got, _fresh_all(yh, "multi-base", base.d))
    c_off = Moved(yh, b_on.d)
    c_off.envs[2].emission[:] = [0, 0, 0]
    lit.update_environments(c_off.env_array(yh))
    assert [x[1] for x in lit.light_list() if x[1] >= 0] == [0, 1, 3]
    _check_all(lit, yh, "multi-c-off", c_off.d, "c-sky off")
    lit.update_environments(b_on.env_array(yh))
    _check_all(lit, yh, "multi-b-on", b_on.d, "all four on")
    lit.update_environments(base.env_array(yh))
    _check_all(lit, yh, "multi-base", base.d, "b-black off again")


# ---- 4. sphere-hairblock at the golden scale: the area light's quad stretched under hair, then an object edit, then a camera edit ----
def _hairblock_with_its_light(yh, sf):
    """sphere-hairblock carries an `arealight` material that no object uses (its light is the constant sky). The description here gives
    it one: a quad of two triangles above the hair, facing down, as one more shape and one more object. Returns (description, the
    light's object, its shape)."""
    d = Reshaped(yh, sf.desc, extra_shapes=1)
    s, lamp = d.num_shapes - 1, _material(d, emission=(20, 20, 20))
    d.shapes[s] = yh.Shape()
    d.shapes[s].num_vertices, d.shapes[s].num_triangles = 4, 2
    d.set(yh, s, positions=np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0.5, 0.5, 0], [-0.5, 0.5, 0]], F), triangles=np.array([[0, 1, 2], [2, 3, 0]], I32))
    rows = [yh.Object.from_buffer_copy(d.objects[o]) for o in range(d.n)] + [yh.Object()]
    rows[-1].frame[:] = _f32([1, 0, 0, 0, 0, 1, 0, -1, 0, 0.3, 2.5, -0.3])
    rows[-1].shape, rows[-1].material = s, lamp
    d.n += 1
    d.objects = (yh.Object * d.n)(*rows)
    d.d.objects, d.d.num_objects = C.cast(d.objects, C.POINTER(yh.Object)), d.n
    return d, d.n - 1, s


def test_hairblock_description_with_its_light(yh):
    sf = yh.SceneFile(scene_path(*HAIRBLOCK[:1], **HAIRBLOCK[1]))
    d, lamp, s = _hairblock_with_its_light(yh, sf)
    again = _copy(yh, d)
    assert again.n == d.n == sf.desc.contents.num_objects + 1 and again.objects[lamp].shape == s == again.num_shapes - 1
    assert _lamp_shape(again) == s and again.shapes[s].num_triangles == 2 and again.arrays(s)["positions"].shape == (4, 3)
    sf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", INSTANCE_SHAPES)
def test_hairblock_light_is_stretched_under_every_launch_shape(lit, yh, scenes, shape, monkeypatch):
    base, lamp, s = _hairblock_with_its_light(yh, scenes(*HAIRBLOCK))
    p = base.arrays(s)["positions"]
    step1 = _copy(yh, base).set(yh, s, positions=(p * np.array([1.75, 1.25, 1.0], F)).astype(F))
    step2 = _copy(yh, step1)
    step2.objects[lamp].frame[9] += 0.5
    step3 = _copy(yh, step2)
    step3.camera.frame[:] = _lookat((0.4, 1.2, 4.5), (0, 0.6, 0))
    monkeypatch.setenv("YHAIR_SHAPE", shape)
    lit.upload_scene(base.ptr)
    lit.update_shape(s, step1.shapes[s])
    got = _check_all(lit, yh, "hb-stretched", step1.d, f"the light's quad stretched, shape {shape}")
    assert _differs(got, _fresh_all(yh, "hb-base", base.d))
    lit.update_objects(lamp, step2.rows(yh, lamp, 1))
    _check_all(lit, yh, "hb-moved", step2.d, f"then the light moved, shape {shape}")
    lit.update_camera(step3.camera)
    _check_all(lit, yh, "hb-camera", step3.d, f"then the camera, shape {shape}")


# ---- 5. what is still refused: the context goes on rendering what it held ----
def _refused(c, yh, call, words, baseline, desc, what):
    with pytest.raises(yh.YhError) as e:
        call()
    for w in words:
        assert w in str(e.value), (what, str(e.value))
    got = _all(c, yh, desc)
    assert got["list"] == baseline["list"] and got["general"] == baseline["general"], what
    _check(got, baseline, what)


def _seventeen(yh, sf):
    """16 emitting quads in a row and one dark one behind them, under a sky without emission: 16 lights."""
    base = Moved(yh, sf.desc)
    lamp, grey = _material(base, emission=(10, 10, 10)), _material(base, color=(0.7, 0.7, 0.7))
    quad = base.objects[_object(base, lamp)].shape
    d = Moved(yh, sf.desc)
    d.n = 17
    d.objects = (yh.Object * 17)()
    for k in range(17):
        d.objects[k].frame[:] = _f32([0.2, 0, 0, 0, 0, -0.2, 0, 0.2, 0, -2.0 + 0.25 * k, 0.0 if k == 16 else 3.0, 0.1 * (k % 3)])
        d.objects[k].shape, d.objects[k].material = quad, grey if k == 16 else lamp
    d.d.objects, d.d.num_objects = C.cast(d.objects, C.POINTER(yh.Object)), 17
    d.envs[0].emission[:] = [0, 0, 0]
    return d, grey


@pytest.mark.gpu
def test_a_seventeenth_light_is_refused(lit, yh, scenes):
    d, grey = _seventeen(yh, scenes(*LIGHTS_UNIT))
    lit.upload_scene(d.ptr)
    assert len(lit.light_list()) == 16
    baseline = _all(lit, yh, d.d)
    lamp_row = yh.Material.from_buffer_copy(d.materials[grey])
    lamp_row.emission[:] = [1, 1, 1]
    _refused(lit, yh, lambda: lit.update_materials(grey, [lamp_row]), ("yh_update_materials", "more than 16 lights", "object 16"), baseline, d.d, "the dark quad lit")
    sky = d.env_array(yh)
    sky[0].emission[:] = [1, 1, 1]
    _refused(lit, yh, lambda: lit.update_environments(sky), ("yh_update_environments", "more than 16 lights"), baseline, d.d, "the sky as a 17th light")


@pytest.mark.gpu
def test_the_only_light_stays_on(lit, yh, scenes):
    sf = scenes("envs-unit", dict(scale=0.05, variant="lights-1"))
    d = Moved(yh, sf.desc)
    d.envs[0].emission[:] = [0, 0, 0]
    lamp = _material(d, emission=(10, 10, 10))
    lit.upload_scene(d.ptr)
    assert len(lit.light_list()) == 1
    baseline = _all(lit, yh, d.d)
    off = yh.Material.from_buffer_copy(d.materials[lamp])
    _black(off)
    _refused(lit, yh, lambda: lit.update_materials(lamp, [off]), ("yh_update_materials", "without a light"), baseline, d.d, "the only light off")
    rows = d.rows(yh)
    rows[_object(d, lamp)].material = _material(d, color=(0.7, 0.7, 0.7))
    _refused(lit, yh, lambda: lit.update_objects(0, rows), ("yh_update_objects", "without a light"), baseline, d.d, "the only light's object dark")
    tex = yh.Material.from_buffer_copy(d.materials[lamp])
    tex.emission_tex = 1
    _refused(lit, yh, lambda: lit.update_materials(lamp, [tex]), ("yh_update_materials", "names another texture"), baseline, d.d, "emission_tex changed")


@pytest.mark.gpu
def test_without_the_opt_in_the_refusals_return(ctx, yh, scenes):
    """yh_set_light_edits(ctx, 0) after 1: the four original refusals, in their words."""
    sf = scenes(*LIGHTS_UNIT)
    base = Reshaped(yh, sf.desc)
    lamp, grey = _material(base, emission=(10, 10, 10)), _material(base, color=(0.7, 0.7, 0.7))
    ctx.set_light_edits(True)
    ctx.upload_scene(base.ptr)
    ctx.set_light_edits(False)
    baseline = _all(ctx, yh, base.d)
    off = yh.Material.from_buffer_copy(base.materials[lamp])
    _black(off)
    said = "the light list changes, upload the scene"
    _refused(ctx, yh, lambda: ctx.update_materials(lamp, [off]), ("yh_update_materials", "turns its emission off", said), baseline, base.d, "a material toggle")
    sky = base.env_array(yh)
    sky[0].emission[:] = [0, 0, 0]
    _refused(ctx, yh, lambda: ctx.update_environments(sky), ("yh_update_environments", "turns its emission off", said), baseline, base.d, "an environment toggle")
    rows = base.rows(yh)
    rows[_object(base, grey)].material = lamp
    _refused(ctx, yh, lambda: ctx.update_objects(0, rows), ("yh_update_objects", "turns its emission on", said), baseline, base.d, "an object toggle")
    s = base.objects[_object(base, lamp)].shape
    for call, name in ((ctx.update_shape, "yh_update_shape"), (ctx.refit_shape, "yh_refit_shape")):
        _refused(ctx, yh, lambda: call(s, base.shapes[s]), (name + ":", "whose material emits: the light tables are made from it"), baseline, base.d, name)


@pytest.mark.gpu
def test_call_order(yh):
    """yh_light_list before an upload is YH_E_STATE; the opt-in may come before one."""
    c = yh.Context(0)
    try:
        a = (C.c_int * 4)()
        assert c.lib.yh_light_list(c.h, a, a, a, a, 4) == yh.YH_E_STATE
        c.set_light_edits(True), c.set_light_edits(False)
        assert c.lib.yh_light_list(c.h, a, a, a, a, 4) == yh.YH_E_STATE
    finally:
        c.close()


@pytest.mark.gpu
def test_mirror_passes_light_edits_on_with_the_opt_in(built, tmp_path):
    """The mirror on lights-unit: a muted light, the sky off, an object darkened and an emitter's quad stretched are four edits and no
    upload with set_light_edits; pixels those of scenes built that way from the start (tests/cpp/test_mirror_light_edits.cpp)."""
    exe = _compile_mirror_test(tmp_path)
    r = subprocess.run([exe, scene_path(*LIGHTS_UNIT[:1], **LIGHTS_UNIT[1])], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)
