"""Instanced scene files (`"instance": "<name>"` -> instances/<name>.ply, yocto_sceneio.cpp:848-867,1198-1217) through every layer:
the reader expands them as the reference's command line does (yscenetrace.cpp:150-181: one object per frame, in the object's
place, frame = instance_frame * object_frame), and the many-object scene level they create is traced on the device like any other.

Yardsticks: tests/golden/instances.npz (tools/make_instance_goldens.py: the reference's COMMAND LINE on `fur-field`), the CPU
oracle (bit-identical to it, test 2 below) and `fur-field-expanded`, the same scene written as one JSON object per frame.
The bars of the GPU half are those of tests/test_gpu_parity.py, as they stand there.
"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden, scene_path

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_instance_goldens as mig  # noqa: E402
import make_scenes  # noqa: E402
from scene_level_visits import object_boxes as _object_boxes  # noqa: E402  (world boxes of a description's objects)

GOLDEN_KW = mig.SCENE_KW                    # the goldens' scene: 300 tufts + 37 pebbles + floor + light = 339 objects (scene table in memory)
SMALL_KW = dict(scale=0.25, count=8)        # 8 + 1 + 2 = 11 objects: the scene table fits LDS (plain kernels, binary walk)
LARGE_KW = dict(scale=0.05, count=2048)     # 2048 + 256 + 2 objects: a scene tree 10-12 levels deep
FRAME_NAMES = ["xx", "xy", "xz", "yx", "yy", "yz", "zx", "zy", "zz", "ox", "oy", "oz"]


def _objects(d):
    return [(tuple(np.array(o.frame[:], np.float32).view(np.uint32)), o.shape, o.material) for o in (d.objects[i] for i in range(d.num_objects))]


def _num_objects(count):
    return count + max(1, count // 8) + 2


# ---------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------
def test_fixture_is_small_and_complete():
    g = golden("instances.npz")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "instances.npz")) < 1 << 20
    assert sorted(g.files) == ["normal_1", "path_1", "path_4"]
    assert all(g[k].shape == (64, 64, 3) and np.isfinite(g[k]).all() for k in g.files)


@pytest.mark.parametrize("kw", [SMALL_KW, GOLDEN_KW, LARGE_KW], ids=["8", "300", "2048"])
def test_instanced_scene_loads_like_its_expansion(yh, kw):
    """yh_scene_load expands an instanced object in place, one yh_object per frame in file order, with the frame the reference
    composes — bitwise the objects of the scene that spells every instance out, sharing the shapes the file names."""
    sf = yh.SceneFile(scene_path("fur-field", **kw))
    ex = yh.SceneFile(scene_path("fur-field-expanded", **kw))
    d, e = sf.desc.contents, ex.desc.contents
    assert d.num_objects == _num_objects(kw["count"]) == e.num_objects
    assert d.num_shapes == 3 == e.num_shapes and d.num_materials == e.num_materials  # arealight (floor and light), sphere, tuft
    assert _objects(d) == _objects(e)
    # floor, light, pebbles, tufts: alphabetical, the copies in their object's place
    shapes = [d.objects[i].shape for i in range(d.num_objects)]
    n_pebbles = max(1, kw["count"] // 8)
    assert shapes[0] == shapes[1] and len(set(shapes[2:2 + n_pebbles])) == 1 and len(set(shapes[2 + n_pebbles:])) == 1
    assert d.shapes[shapes[-1]].num_lines > 0 and d.shapes[shapes[2]].num_triangles > 0
    # instance * object, not object * instance: the tuft's own frame turns +z up, so every copy's z axis has a y component
    assert all(abs(d.objects[i].frame[7]) > 0.1 for i in range(2 + n_pebbles, d.num_objects))
    sf.close(), ex.close()


def test_oracle_renders_the_reference_command_lines_images(yh, oracle, tmp_path):
    """The oracle on the expanded description = the reference's command line on the instanced file, RGB bit for bit (`path` at 1
    and 4 spp, `normal` at 1) — from the committed goldens, and from a live run where oracle/_ref has been built."""
    g = golden("instances.npz")
    path = scene_path(mig.SCENE, **GOLDEN_KW)
    sf = yh.SceneFile(path)
    osc = oracle.scene(sf.desc)
    for key, (shader, spp) in mig.RENDERS.items():
        img = osc.render(yh.TraceParams.default(resolution=mig.RESOLUTION, shader=shader), spp)
        assert np.array_equal(img[..., :3], g[key]), key
        if os.path.exists(mig.REF_CLI):
            assert np.array_equal(mig.reference_render(path, shader, spp, str(tmp_path)), g[key]), key
    assert (img[..., 3] > 0).mean() > 0.4
    osc.close(), sf.close()


def _tiny_scene(tmp_path, objects, name="s"):
    """A scene directory with the sphere and the area-light quad, one camera, one sky; `objects`: the JSON objects."""
    d = tmp_path / name
    (d / "shapes").mkdir(parents=True), (d / "instances").mkdir()
    for s in ("sphere", "arealight"):
        shutil.copy(os.path.join(ROOT, "assets", s + ".ply"), d / "shapes" / (s + ".ply"))
    scene = {"cameras": {"default": {"lens": 0.05, "aspect": 1.0, "lookat": [0, 3, 9, 0, 0.3, 0, 0, 1, 0]}},
             "environments": {"sky": {"emission": [0.5, 0.5, 0.5]}},
             "materials": {"grey": {"color": [0.6, 0.6, 0.6]}, "lamp": {"emission": [8, 8, 8]}},
             "objects": objects}
    (d / (name + ".json")).write_text(json.dumps(scene))
    return d, str(d / (name + ".json"))


def _some_frames(n, seed=3):
    rng = np.random.default_rng(seed)
    f = rng.uniform(-1, 1, (n, 12)).astype(np.float32)
    f[:, [0, 4, 8]] += 2  # (far from singular)
    return f


def test_instance_reader_edges(yh, tmp_path):
    ball = {"shape": "sphere", "material": "grey", "frame": [0.5, 0, 0, 0, 0, 0.5, 0, -0.5, 0, 0.1, 0.2, 0.3]}
    frames = _some_frames(5)
    want = make_scenes.compose_frames(frames, ball["frame"])

    def load(objects, name):
        d, path = _tiny_scene(tmp_path, objects, name)
        return d, path

    def frames_of(path):
        sf = yh.SceneFile(path)
        d = sf.desc.contents
        out = np.array([d.objects[i].frame[:] for i in range(d.num_objects)], np.float32).reshape(-1, 12)
        shapes = {d.objects[i].shape for i in range(d.num_objects)}
        sf.close()
        return out, shapes

    # the twelve properties by name, in any order of the header; ascii as well as binary
    for name, kw in (("binary", {}), ("shuffled", dict(order=[9, 3, 0, 11, 5, 8, 1, 7, 2, 10, 4, 6])), ("ascii", dict(ascii=True)),
                     ("ascii-shuffled", dict(ascii=True, order=list(range(11, -1, -1))))):
        d, path = load({"ball": dict(ball, instance="copies")}, name)
        make_scenes.write_instance_ply(d / "instances" / "copies.ply", frames, **kw)
        got, _ = frames_of(path)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    # double properties are converted; an element in front of `instance` is read past
    d, path = load({"ball": dict(ball, instance="copies")}, "double")
    with open(d / "instances" / "copies.ply", "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement other 2\nproperty uchar a\nproperty list uchar int l\nelement instance 5\n" +
                 "".join(f"property double {n}\n" for n in FRAME_NAMES) + "end_header\n").encode())
        f.write(bytes([7, 2]) + np.array([1, 2], "<i4").tobytes() + bytes([9, 0]))
        f.write(frames.astype("<f8").tobytes())
    got, _ = frames_of(path)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # an empty string is no instance; a file without frames makes its object vanish
    d, path = load({"ball": dict(ball, instance=""), "gone": dict(ball, instance="none"), "lamp": {"shape": "arealight", "material": "lamp"}}, "empty")
    make_scenes.write_instance_ply(d / "instances" / "none.ply", np.zeros((0, 12), np.float32))
    got, _ = frames_of(path)
    assert len(got) == 2 and np.array_equal(got[0], np.array(ball["frame"], np.float32))
    # two objects share one file (and one shape): the second in its own place, with its own frame
    other = dict(ball, frame=[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 2, 0], instance="copies")
    d, path = load({"a": dict(ball, instance="copies"), "b": other}, "shared")
    make_scenes.write_instance_ply(d / "instances" / "copies.ply", frames)
    got, shapes = frames_of(path)
    assert len(got) == 10 and len(shapes) == 1
    assert np.array_equal(got[:5].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[5:].view(np.uint32), make_scenes.compose_frames(frames, other["frame"]).view(np.uint32))
    # what cannot be read is an error that names the file
    d, path = load({"ball": dict(ball, instance="nowhere")}, "missing-file")
    with pytest.raises(yh.YhError, match=r"instances/nowhere\.ply: file not found"):
        yh.SceneFile(path)
    d, path = load({"ball": dict(ball, instance="copies")}, "missing-element")
    shutil.copy(os.path.join(ROOT, "assets", "sphere.ply"), d / "instances" / "copies.ply")
    with pytest.raises(yh.YhError, match=r"instances/copies\.ply: no instance element"):
        yh.SceneFile(path)
    d, path = load({"ball": dict(ball, instance="copies")}, "missing-property")
    with open(d / "instances" / "copies.ply", "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement instance 5\n" + "".join(f"property float {n}\n" for n in FRAME_NAMES if n != "zy") +
                 "end_header\n").encode())
        f.write(frames[:, :11].tobytes())
    with pytest.raises(yh.YhError, match=r"instances/copies\.ply: instance element without property zy"):
        yh.SceneFile(path)
    # subdivision surfaces stay outside, with a message of their own
    d, path = load({"ball": dict(ball, subdiv="cube")}, "subdiv")
    with pytest.raises(yh.YhError, match="subdivision surfaces are outside the hair path") as e:
        yh.SceneFile(path)
    assert "instance" not in str(e.value).replace(path, "")  # (the message proper: the directory of this test has the word in its name)


@pytest.mark.parametrize("name,kw", [("fur-field", GOLDEN_KW), ("fur-field", LARGE_KW), ("crowd", dict(scale=0.05))], ids=["fur-field-300", "fur-field-2048", "crowd"])
def test_wide_scene_nodes_keep_the_reference_visiting_order(yh, name, kw):
    """The check of test_wide_nodes_keep_the_reference_visiting_order on OBJECT boxes: the scene tree of an instanced scene
    collapsed two levels per node visits the leaves (up to four consecutive scene primitives each) in the binary walk's order
    for all eight direction signs, and every object appears once."""
    from test_abi import _binary_leaf_order, _wide_leaf_order
    lib = yh.load()
    sf = yh.SceneFile(scene_path(name, **kw))
    boxes = _object_boxes(sf.desc.contents)
    n = len(boxes)
    nb = lib.yh_bvh_build(n, yh.fptr(boxes), None, None)
    nodes = np.zeros((nb, 8), np.float32)
    lib.yh_bvh_build(n, yh.fptr(boxes), yh.fptr(nodes), None)
    nw = lib.yh_bvh_build_wide(n, yh.fptr(boxes), 4, None)
    slots = np.zeros((nw, 4, 8), np.float32)
    assert lib.yh_bvh_build_wide(n, yh.fptr(boxes), 4, yh.fptr(slots)) == nw
    assert nw < nb / 2
    for sign in range(8):
        want = _binary_leaf_order(nodes, sign, set())
        assert _wide_leaf_order(slots, 4, sign, set()) == want, sign
        assert sorted(want) == sorted(set(want)) and sum(k for _, k in want) == n and max(k for _, k in want) <= 4
    sf.close()


def test_mirror_and_command_lines_load_an_instanced_scene(yh, tmp_path):
    """The C++ mirror's init_scene (host/yscene_cli.h) makes one ptr::object per frame; yscenetrace and ysceneitraces get past
    the scene file (without a GPU they stop at the device, with the library's message; with one they render)."""
    kw = dict(scale=0.05, count=20)
    path = scene_path("fur-field", **kw)
    pkg = os.path.join(ROOT, "yocto-hair_amd")
    exe = str(tmp_path / "mirror_instances")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(pkg, "host"), "-Wno-class-memaccess", os.path.join(ROOT, "tests", "cpp", "test_mirror_instances.cpp"),
                           "-o", exe, "-L" + pkg, "-lyhair", "-Wl,-rpath," + pkg, "-lpthread"])
    r = subprocess.run([exe, path, str(_num_objects(20))], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert r.stdout.strip() == f"{_num_objects(20)} objects, 3 shapes"
    for cli in ("yscenetrace", "ysceneitraces"):
        out = str(tmp_path / (cli + ".pfm"))
        r = subprocess.run([os.path.join(pkg, cli), path, "-r", "32", "-s", "1", "-o", out], capture_output=True, text=True, timeout=300)
        text = r.stdout + r.stderr
        assert "instance" not in text and "outside the hair path" not in text, text
        assert (r.returncode == 0 and os.path.exists(out)) or "no HIP device available" in text, text


# ---------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------
GPU_KW = [SMALL_KW, GOLDEN_KW, LARGE_KW]
GPU_IDS = ["8-in-lds", "300-in-memory", "2048-in-memory"]


def _field_rays(kw, m=4096, seed=20241016):
    """Rays towards the field from around its camera, as oracle/make_golden.py draws a scene's base rays."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(kw["count"])))
    ext = max(1.0, 0.15 * side)
    org = rng.uniform(-1, 1, (m, 3)) * [ext, 0.4 * ext, 0.5 * ext] + [0.4 * ext, 0.9 * ext + 0.6, 2.0 * ext + 1.0]
    tgt = rng.uniform(-1, 1, (m, 3)) * [1.1 * ext, 0.15, 1.1 * ext] + [0, 0.1, 0]
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([org, d, np.full((m, 1), 1e-4), np.full((m, 1), 3.4028235e38)], 1).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", GPU_KW, ids=GPU_IDS)
def test_instanced_closest_hits_bit_exact(ctx, oracle, yh, kw):
    """100 000 rays as test_closest_hits_bit_exact draws them (origins scattered, axis-aligned and zero directions, finite tmax)
    through yh_intersect_batch, every one against the oracle: object, element, uv and distance bit for bit — with the one-lane
    kernel (the default for a batch of this size) and with the quad kernel."""
    sf = yh.SceneFile(scene_path("fur-field", **kw))
    ctx.upload_scene(sf.desc)
    base = _field_rays(kw)
    rng = np.random.default_rng(5)
    m = 100000
    rays = np.repeat(base, m // len(base) + 1, axis=0)[:m].copy()
    rays[:, :3] += rng.normal(0, 0.3, (m, 3)).astype(np.float32)
    rays[:6, 3:6] = [[1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0, 0], [0, 1, 1], [-1, 0, 0]]
    rays[6:1000, 7] = rng.uniform(0.5, 30, 994)  # finite tmax
    osc = oracle.scene(sf.desc)
    ho, hg = osc.intersect(rays), ctx.intersect(rays)
    print(f"count {kw['count']}: {np.mean(ho[0] >= 0):.3f} of the rays hit, {len(np.unique(ho[0]))} distinct objects; "
          f"mismatches {[int(np.sum(a != b)) for a, b in zip(ho, hg)]}")
    for a, b in zip(ho, hg):
        assert np.array_equal(a, b)
    assert 0.2 < np.mean(hg[0] >= 0) < 0.98
    os.environ["YHAIR_INTERSECT"] = "quad"
    try:
        hq = ctx.intersect(rays)
    finally:
        del os.environ["YHAIR_INTERSECT"]
    for a, b in zip(ho, hq):
        assert np.array_equal(a, b)
    osc.close(), sf.close()


def _world_box_face_rays(boxes, rng, m):
    """m axis-parallel rays that lie ON a face of an object's world box (`boxes`: (n, 6) float32), both ways along either axis of the face: a
    slab of the box, and of every scene node whose box ends there, is 0 * inf."""
    k, ax, hi = rng.integers(0, len(boxes), m), rng.integers(0, 3, m), rng.integers(0, 2, m)
    run = (ax + 1 + rng.integers(0, 2, m)) % 3
    sign = np.where(rng.integers(0, 2, m) == 1, 1.0, -1.0).astype(np.float32)
    rows = np.arange(m)
    lo, up = boxes[k, :3], boxes[k, 3:]
    o = (lo + (up - lo) * rng.random((m, 3)).astype(np.float32)).astype(np.float32)
    o[rows, ax] = boxes[k, ax + 3 * hi]                     # on the face, as the float32 the box holds
    o[rows, run] = np.where(sign > 0, lo[rows, run] - 1, up[rows, run] + 1)  # from outside, towards the box
    d = np.zeros((m, 3), np.float32)
    d[rows, run] = sign
    return np.concatenate([o, d, np.full((m, 1), 1e-4, np.float32), np.full((m, 1), 3.4028235e38, np.float32)], 1).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", GPU_KW[1:], ids=GPU_IDS[1:])
def test_wide_forms_walk_the_scene_level_from_memory(ctx, oracle, yh, kw):
    """The scene level as 4-wide nodes read from memory under eight and sixteen lanes per ray — every quad of the octet or the sixteen runs
    the scene node — through the four memory-table forms of yh_intersect_plain_batch (the traversal of the GENERAL variants of launch shapes
    4, 7, 6 and 8): _field_rays and 512 axis-parallel rays on faces of the objects' world boxes, the oracle's hits bit for bit. The plain
    forms refuse this scene, whose table does not fit LDS."""
    sf = yh.SceneFile(scene_path("fur-field", **kw))
    ctx.upload_scene(sf.desc)
    rng = np.random.default_rng(17)
    rays = np.concatenate([_field_rays(kw), _world_box_face_rays(_object_boxes(sf.desc.contents), rng, 512)])
    osc = oracle.scene(sf.desc)
    ho = osc.intersect(rays)
    faces = ho[0][-512:] >= 0
    print(f"count {kw['count']}: {np.mean(ho[0] >= 0):.3f} of the rays hit, {int(faces.sum())} of the 512 on box faces")
    assert 0.2 < np.mean(ho[0][:-512] >= 0) < 1.0 and len(np.unique(ho[0])) > kw["count"] // 8 and 16 <= faces.sum() <= 496  # (the rays: hits on many objects, misses, both on the faces)
    for form in (3, 4, 5, 6):
        with pytest.raises(yh.YhError):
            ctx.intersect_plain(form, rays[:4])
        hg = ctx.intersect_plain(form | yh.INTERSECT_TABLE_IN_MEMORY, rays)
        for name, a, b in zip(("object", "element", "uv", "distance"), ho, hg):
            same = (a.view(np.uint32) == b.view(np.uint32)) if a.dtype == np.float32 else (a == b)
            bad = np.flatnonzero(~same.reshape(len(a), -1).all(1))
            assert bad.size == 0, f"form {form} from memory: {name} differs on {bad.size} rows, first {bad[0]}: oracle {a[bad[0]]} device {b[bad[0]]}"
    osc.close(), sf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["fast-bsdf", "exact-bsdf"])
@pytest.mark.parametrize("kw", GPU_KW, ids=GPU_IDS)
def test_instanced_launch_shapes_and_kernels_render_identical_pixels(ctx, yh, kw, exact, monkeypatch):
    """The form of test_launch_shapes_and_kernels_render_identical_pixels: every launch shape and k_stream, forced in turn, and
    the host's own choice give the same pixels and RNG states."""
    sf = yh.SceneFile(scene_path("fur-field", **kw))
    ctx.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=88, hair_exact=exact)
    images = {}
    for shape in ("0", "1", "3", "4", "5", "6", "7", "8"):
        monkeypatch.setenv("YHAIR_SHAPE", shape)
        ctx.init_state(p)
        ctx.trace_samples(3), ctx.trace_samples(5)
        images[shape] = (ctx.download(), ctx.download_rng())
    monkeypatch.delenv("YHAIR_SHAPE")
    ctx.init_state(p)
    ctx.trace_samples(3), ctx.trace_samples(5)
    images["auto"] = (ctx.download(), ctx.download_rng())
    base = images["0"]
    assert base[0][..., 3].max() > 0
    for k, (img, rng) in images.items():
        assert np.array_equal(img, base[0]), f"shape {k} renders different pixels"
        assert np.array_equal(rng, base[1]), f"shape {k} leaves different RNG states"
    sf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", GPU_KW[:2], ids=GPU_IDS[:2])
def test_instanced_images_match_the_oracle(ctx, oracle, yh, kw):
    """The three bars of tests/test_gpu_parity.py against the oracle: at 1 spp >= 90 % of the pixels within rel 1e-3 and the
    alpha channel identical; at 16 spp relRMSE <= 0.5 x the seed-to-seed floor and >= 99 % of the pixels within 4 sigma; and the
    instanced file renders bitwise what its expansion renders."""
    from test_gpu_parity import BAR_1SPP, K_SIGMA, _k_sigma_share, _rel, _relrmse
    sf = yh.SceneFile(scene_path("fur-field", **kw))
    ctx.upload_scene(sf.desc)
    osc = oracle.scene(sf.desc)
    res = 64
    p = yh.TraceParams.default(resolution=res)
    ctx.init_state(p)
    ctx.trace_samples(1)
    img, rng1 = ctx.download(), ctx.download_rng()
    ref = osc.render(p, 1)
    close = _rel(img[..., :3], ref[..., :3]).max(axis=2) < 1e-3
    print(f"count {kw['count']}: 1 spp {close.mean():.4f} of pixels within rel 1e-3, alpha equal {np.mean(img[..., 3] == ref[..., 3]):.4f}")
    assert np.isfinite(img).all()
    assert close.mean() >= BAR_1SPP, f"only {close.mean():.3f} of pixels within rel 1e-3 at 1 spp"
    assert np.array_equal(img[..., 3], ref[..., 3])  # primary visibility is exact
    ctx.init_state(p)
    ctx.trace_samples(16)
    img16 = ctx.download()
    ref16 = osc.render(p, 16)
    floor = _relrmse(osc.render(yh.TraceParams.default(resolution=res, seed=12345), 16), ref16)
    err = _relrmse(img16, ref16)
    print(f"count {kw['count']}: 16 spp relRMSE {err:.4f}, seed floor {floor:.4f}")
    assert err <= 0.5 * floor, f"relRMSE {err:.4f} vs seed floor {floor:.4f}"
    share, rms = _k_sigma_share(ctx, osc, yh, res, 16, ref16)
    print(f"count {kw['count']}: {share:.4f} of pixels within {K_SIGMA} sigma (relRMSE {rms:.4f})")
    assert share >= 0.99, f"16 spp: {share:.4f} of pixels within {K_SIGMA} sigma"
    # the expansion, spelt out in JSON: the same objects, so the same bits
    ex = yh.SceneFile(scene_path("fur-field-expanded", **kw))
    ctx.upload_scene(ex.desc)
    ctx.init_state(p)
    ctx.trace_samples(1)
    assert np.array_equal(ctx.download(), img) and np.array_equal(ctx.download_rng(), rng1)
    osc.close(), sf.close(), ex.close()


@pytest.mark.gpu
def test_every_instance_of_an_emitter_is_a_light(yh, oracle, tmp_path):
    """init_lights walks objects (pt.cpp:1695-1740): three frames of an emissive quad are three lights — the oracle counts
    them, and the device picks among the same lights (1-spp parity on a scene lit by them). Seventeen are one more than the
    light table holds: YH_E_INVALID naming the limit, and a context without a scene."""
    from test_gpu_parity import BAR_1SPP, _rel
    floor = {"shape": "arealight", "material": "grey", "frame": [3, 0, 0, 0, 0, -3, 0, 3, 0, 0, 0, 0]}
    ball = {"shape": "sphere", "material": "grey", "frame": [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0.3, 0]}
    lamp = {"shape": "arealight", "material": "lamp", "frame": [0.2, 0, 0, 0, 0, 0.2, 0, -0.2, 0, 0, 3, 0], "instance": "lamps"}

    def lamps(n):
        f = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), (n, 1))
        f[:, 9] = np.linspace(-2.5, 2.5, n)
        f[:, 0] = np.linspace(0.8, 1.3, n)
        return f
    c = yh.Context(0)
    d, path = _tiny_scene(tmp_path, {"ball": ball, "floor": floor, "lamp": lamp}, "three")
    make_scenes.write_instance_ply(d / "instances" / "lamps.ply", lamps(3))
    sf = yh.SceneFile(path)
    osc = oracle.scene(sf.desc)
    assert sf.desc.contents.num_objects == 5 and osc.num_lights() == 4  # three lamps and the sky
    c.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=64)
    c.init_state(p)
    c.trace_samples(1)
    img, ref = c.download(), osc.render(p, 1)
    close = _rel(img[..., :3], ref[..., :3]).max(axis=2) < 1e-3
    assert close.mean() >= BAR_1SPP and np.array_equal(img[..., 3], ref[..., 3])
    osc.close(), sf.close()
    d, path = _tiny_scene(tmp_path, {"ball": ball, "floor": floor, "lamp": lamp}, "seventeen")
    make_scenes.write_instance_ply(d / "instances" / "lamps.ply", lamps(17))
    sf = yh.SceneFile(path)
    assert sf.desc.contents.num_objects == 19
    with pytest.raises(yh.YhError, match=f"yhair error {yh.YH_E_INVALID}: more than 16 lights"):
        c.upload_scene(sf.desc)
    with pytest.raises(yh.YhError, match="yh_upload_scene"):  # the failed upload left no scene behind
        c.init_state(p)
    c.close(), sf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [GOLDEN_KW, LARGE_KW], ids=["300", "2048"])
def test_device_collapse_of_the_scene_tree_is_the_hosts(ctx, yh, kw):
    """yh_bvh_build_wide_gpu against yh_bvh_build_wide on the object boxes of fur-field, slot for slot (the comparison of
    test_device_wide_collapses_are_the_host_collapses at width 4)."""
    lib = yh.load()
    sf = yh.SceneFile(scene_path("fur-field", **kw))
    boxes = _object_boxes(sf.desc.contents)
    n = len(boxes)
    nh = lib.yh_bvh_build_wide(n, yh.fptr(boxes), 4, None)
    host = np.zeros((nh, 4, 8), np.float32)
    assert lib.yh_bvh_build_wide(n, yh.fptr(boxes), 4, yh.fptr(host)) == nh
    assert lib.yh_bvh_build_wide_gpu(ctx.h, n, yh.fptr(boxes), 4, None) == nh
    dev = np.zeros((nh, 4, 8), np.float32)
    assert lib.yh_bvh_build_wide_gpu(ctx.h, n, yh.fptr(boxes), 4, yh.fptr(dev)) == nh
    assert np.array_equal(host[..., :6].view(np.uint32), dev[..., :6].view(np.uint32))
    href, dref = host[..., 6].view(np.uint32).astype(np.int64), dev[..., 6].view(np.uint32).astype(np.int64)
    empty, leaf = href == 0xFFFFFFFF, (href >> 30) == 3
    node = ~empty & ~leaf
    assert np.array_equal(dref[empty | leaf], href[empty | leaf])
    assert np.array_equal(dref[node], href[node] * 4)
    haxes, daxes = host[..., 7].view(np.uint32), dev[..., 7].view(np.uint32)
    assert np.array_equal(daxes & 0xFF, haxes & 0xFF)
    occ = ((~empty).astype(np.uint32) << np.arange(4, dtype=np.uint32)).sum(axis=1)
    assert np.array_equal((daxes >> 8) & 0xF, np.broadcast_to(occ[:, None], daxes.shape))
    sf.close()


@pytest.mark.gpu
def test_a_deep_scene_uploads_and_renders_or_is_refused_by_the_stack_check(yh, oracle, tmp_path):
    """4096 instances (a scene tree of a dozen levels) next to the full-size hair block (1.6 M segments: a shape tree of full
    depth): the stack a traversal needs is the sum of both. Either the upload is refused by its check, with its message, or
    every kernel traces the scene like the oracle — never a launch that overruns a stack column."""
    kw = dict(scale=0.05, count=4096)
    src = os.path.dirname(scene_path("fur-field", **kw))
    d = tmp_path / "deep"
    shutil.copytree(src, d)
    make_scenes.write_hair_ply(str(d / "shapes" / "hair-block.ply"), make_scenes.gen_hair_block(100_000), 0.004, 0.001)
    name = os.path.basename(src) + ".json"
    scene = json.loads((d / name).read_text())
    scene["objects"]["hairblock"] = {"frame": [3, 0, 0, 0, 0, 3, 0, -3, 0, 0, 0.2, 0], "shape": "hair-block", "material": "fur"}
    (d / name).write_text(json.dumps(scene))
    sf = yh.SceneFile(str(d / name))
    assert sf.desc.contents.num_objects == _num_objects(4096) + 1
    c = yh.Context(0)
    try:
        c.upload_scene(sf.desc)
    except yh.YhError as e:
        assert "BVH too deep for the traversal stack" in str(e), str(e)
        print("refused:", e)
        c.close(), sf.close()
        return
    rays = _field_rays(kw, m=20000)
    osc = oracle.scene(sf.desc)
    ho = osc.intersect(rays)
    for mode in ("lane5", "quad"):
        os.environ["YHAIR_INTERSECT"] = mode
        try:
            hg = c.intersect(rays)
        finally:
            del os.environ["YHAIR_INTERSECT"]
        for a, b in zip(ho, hg):
            assert np.array_equal(a, b), mode
    assert np.mean(ho[0] == 1) > 0.01  # floor, hairblock, light, ...: some rays end in the hair block
    p = yh.TraceParams.default(resolution=64)
    c.init_state(p)
    c.trace_samples(1)
    img = c.download()
    assert np.isfinite(img).all() and np.array_equal(img[..., 3], osc.render(p, 1)[..., 3])  # primary visibility is exact
    osc.close(), c.close(), sf.close()
