"""GPU parity tests (-m gpu): the HIP path, called through the C ABI of include/yhair.h,
against the CPU oracle and the committed golden vectors of the real reference.

Bars (SURVEY.md 7 "parity definition"):
  * RNG streams, closest hits (object, element, uv, distance): BIT-EXACT (the kernels are built
    with -ffp-contract=off and use correctly-rounded / and sqrt);
  * hair BSDF eval / pdf: relative error <= 1e-4 (device libm vs glibc, last-ulp differences
    amplified by exp()); sampled directions: 5e-5 absolute;
  * images: a one-ulp change can flip a lobe choice and send that path elsewhere, so the per-pixel
    tolerance is statistical — at 1 spp >= 60 % of pixels within rel 1e-3 (a wrong RNG order or
    algorithm drops this to ~0 %, the same reference rebuilt with FMA contraction sits at 66-95 %),
    at 16 spp image relRMSE(gpu, ref) <= 0.5 x relRMSE(ref seed A, ref seed B);
  * the reference's four Monte-Carlo self-tests pass on the device with their own thresholds.
"""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_SCENES, ROOT, SCENES, golden, scene_path, scene_tag

pytestmark = pytest.mark.gpu

REL_BSDF = 1e-4   # stated float tolerance for f and pdf
ABS_DIR = 5e-5    # stated tolerance for sampled directions
# Share of 1-spp pixels within rel 1e-3 of the reference. Measured 0.95-1.00 on every golden scene
# (oracle/divergence_report.py, profiles/); the same reference rebuilt with FMA contraction keeps 0.95
# in dense hair, a wrong RNG order or algorithm gives ~0.
BAR_1SPP = 0.90
K_SIGMA = 4.0     # per-pixel |gpu - ref| <= k sqrt(var_ref / N + var_gpu / N) for >= 99 % of pixels


def _rel(a, b, floor=1e-6):
    return np.abs(a - b) / np.maximum(np.abs(b), floor)


def _relrmse(a, b):
    return float(np.sqrt(np.mean((a[..., :3] - b[..., :3]) ** 2)) / max(1e-12, np.mean(b[..., :3])))


# ---------------------------------------------------------------------------------------------
# unit level
# ---------------------------------------------------------------------------------------------
def test_hair_brdf_matches_reference_vectors(ctx):
    g = golden("hair_bsdf.npz")
    b = ctx.hair_brdf(g["mats"], g["v"], g["normal"], g["tangent"])
    ref = g["brdf"]
    # all fields built from + - * / sqrt are exact; sigma_a-from-colour (log), sin(alpha) and
    # gamma_o (asin) go through device libm
    exact = [3, 4, 5, 6, 7, 8, 9, 10] + list(range(18, 27))
    assert np.array_equal(b[:, exact], ref[:, exact])
    assert np.max(_rel(b, ref, 1e-3)) < 2e-6


def test_hair_eval_pdf_sample_match_reference_vectors(ctx):
    g = golden("hair_bsdf.npz")
    f = ctx.hair_eval(g["brdf"], g["wo"], g["wi"])
    pdf = ctx.hair_pdf(g["brdf"], g["wo"], g["wi"])
    ok = np.isfinite(g["f"]).all(axis=1) & np.isfinite(g["pdf"])
    assert ok.mean() > 0.99
    assert np.max(_rel(f[ok], g["f"][ok], 1e-7)) <= REL_BSDF
    assert np.max(_rel(pdf[ok], g["pdf"][ok], 1e-7)) <= REL_BSDF
    wi = ctx.hair_sample(g["brdf"], g["wo"], g["rn"])
    okd = np.isfinite(g["wi_sampled"]).all(axis=1)
    assert np.max(np.abs(wi[okd] - g["wi_sampled"][okd])) <= ABS_DIR
    # f and pdf at the reference's own sampled directions: the importance weights agree
    fs = ctx.hair_eval(g["brdf"], g["wo"], g["wi_sampled"])
    ps = ctx.hair_pdf(g["brdf"], g["wo"], g["wi_sampled"])
    oks = okd & np.isfinite(g["f_sampled"]).all(axis=1) & (g["pdf_sampled"] > 0)
    assert np.max(_rel(fs[oks], g["f_sampled"][oks], 1e-7)) <= REL_BSDF
    assert np.max(_rel(ps[oks], g["pdf_sampled"][oks], 1e-7)) <= REL_BSDF
    # the README/BASELINE name eval_hair_scattering_pdf is the same entry point
    import ctypes as C
    out = np.zeros(len(pdf), np.float32)
    import yhair_capi as yh
    assert ctx.lib.yh_hair_eval_pdf_batch(ctx.h, len(out), yh.fptr(g["brdf"]), yh.fptr(g["wo"]), yh.fptr(g["wi"]), yh.fptr(out)) == 0
    assert np.array_equal(out, pdf, equal_nan=True)


def test_hair_batches_match_oracle_on_fresh_inputs(ctx, oracle):
    rng = np.random.default_rng(11)
    n = 50000
    mats = np.zeros((n, 12), np.float32)
    mats[:, 3:5] = rng.uniform(0.05, 0.95, (n, 2))
    mats[:, 5] = rng.uniform(0, 4, n)
    mats[:, 6] = 1.55
    mats[:, 10] = rng.uniform(0, 8, n)
    v = rng.uniform(0, 1, n).astype(np.float32)
    d = lambda: (lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))(rng.normal(size=(n, 3)))  # noqa
    tng, wo, wi, nrm = d(), d(), d(), d()
    b = oracle.hair_brdf(mats, v, nrm, tng)
    assert np.max(_rel(ctx.hair_eval(b, wo, wi), oracle.hair_eval(b, wo, wi), 1e-7)) <= REL_BSDF
    assert np.max(_rel(ctx.hair_pdf(b, wo, wi), oracle.hair_pdf(b, wo, wi), 1e-7)) <= REL_BSDF


def _lobe_close(got, want):
    """Rows of (f[3], pdf, sampled[3]) within the stated tolerances; returns the failing fraction.
    Non-finite values (0 * inf in a grazing microfacet term) must be non-finite on both sides."""
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore"):
        ok_f = (same[:, :4] | (_rel(got[:, :4], want[:, :4], 1e-7) <= REL_BSDF)).all(axis=1)
        ok_w = (same[:, 4:] | (np.abs(got[:, 4:] - want[:, 4:]) <= ABS_DIR)).all(axis=1)
    return 1.0 - float(np.mean(ok_f & ok_w)), ok_f, ok_w


def test_surface_lobes_match_reference_vectors(ctx, yh):
    """each lobe of yocto_math.h:4427-4755 on the device vs the reference's
    own outputs. Values and pdfs are + - * / sqrt only: all within 1e-4 (most bit-exact);
    sampled directions go through device atan/sin/cos: 5e-5 absolute. The refraction lobe picks
    reflect-or-refract by `rnl < F(sampled halfway)`, so a last-place change of F flips a row whose rnl sits on it: only rows
    whose rnl lies within 1e-5 of the float64 Fresnel value (decided on the inputs, tests/surface_f64.py; at most 2e-4 of the
    rows) may miss the direction, as in tests/test_surface_unit.py."""
    import surface_f64 as s64
    g = golden("lobes.npz")
    args = (g["params"], g["normal"], g["wo"], g["wi"], g["rn"])
    p64, rn64 = g["params"].astype(np.float64), g["rn"].astype(np.float64)
    fresnel = s64.refraction_fresnel(p64[:, 0], p64[:, 1], g["normal"].astype(np.float64), g["wo"].astype(np.float64), rn64[:, 1], rn64[:, 2])[0]
    aside = np.abs(rn64[:, 0] - fresnel) <= 1e-5
    assert aside.mean() <= 2e-4
    for kind in range(yh.LOBE_COUNT):
        got, want = ctx.surface_lobe(kind, *args), g[f"lobe_{kind}"]
        bad, ok_f, ok_w = _lobe_close(got, want)
        assert ok_f.all(), (kind, np.flatnonzero(~ok_f)[:5])
        if kind == yh.LOBE_REFRACTION:
            assert (ok_w | aside).all(), (kind, np.flatnonzero(~(ok_w | aside))[:5])
        else:
            assert bad <= 0.0, (kind, bad)
        assert np.mean(got[:, :4] == want[:, :4]) > 0.97, kind


def _random_surface_materials(yh, rng, n):
    arr = (yh.Material * n)()
    for i in range(n):
        m = arr[i]
        m.color[:] = rng.choice([0.0, 0.3, 0.9], 3).tolist() if rng.uniform() < 0.3 else rng.uniform(0, 1, 3).tolist()
        m.specular = float(rng.choice([0, 0.5, 1]))
        m.metallic = float(rng.choice([0, 0, 0.4, 1]))
        m.transmission = float(rng.choice([0, 0, 0.6, 1]))
        m.roughness = float(rng.choice([0, 0, 0.05, 0.3, 1]))
        m.opacity = float(rng.choice([1, 1, 0.9995, 0.5]))
        m.ior = float(rng.choice([1.0, 1.33, 1.5]))
        m.thin = int(rng.choice([1, 1, 0]))  # 0 + transmission: the refraction lobe (batch API only)
    return arr


def test_surface_bsdf_mixture_matches_oracle(ctx, oracle, yh):
    """eval_brdf + the rough / delta dispatch (pt.cpp:405-471, 1069-1280): lobe weights, roughness,
    opacity and lobe pdfs bit-exact; value, pdf and sampled direction within tolerance."""
    rng = np.random.default_rng(21)
    n = 20000
    mats = _random_surface_materials(yh, rng, n)
    d = lambda: (lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))(rng.normal(size=(n, 3)))  # noqa
    nn, wo, wi = d(), d(), d()
    k = n // 2  # half of the rows: incoming near the mirror / straight-through direction (delta lobes fire)
    wi[:k:2] = -wo[:k:2] + 2 * np.sum(nn[:k:2] * wo[:k:2], 1, keepdims=True) * nn[:k:2]
    wi[1:k:2] = -wo[1:k:2]
    rn = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    got, want = ctx.surface_bsdf(mats, nn, wo, wi, rn), oracle.surface_bsdf(mats, nn, wo, wi, rn)
    assert np.array_equal(got[:, :22], want[:, :22])
    delta = want[:, 15] == 0
    assert 0.05 < delta.mean() < 0.6
    bad, ok_f, ok_w = _lobe_close(got[:, 22:], want[:, 22:])
    worst = np.flatnonzero(~ok_f)[:3]
    assert ok_f.all() and bad <= 1e-3, (bad, worst, got[worst], want[worst])
    assert (want[:, 22:25] != 0).any(axis=1).mean() > 0.2


def test_curve_conversion_bit_exact_on_device(ctx, yh, tmp_path):
    """pbrt curve -> strand on the GPU (+ - * / sqrt only: bit-exact), through the ABI and through
    the ycurves2ply command line (tokenizer + PLY writer) read back by the scene reader."""
    import os, subprocess
    g = golden("curves.npz")
    pos, nrm, rad, lines = ctx.curves_to_lines(g["P"], g["width0"], g["width1"], int(g["base_vertex"]))
    assert np.array_equal(pos, g["positions"]) and np.array_equal(nrm, g["normals"], equal_nan=True)
    assert np.array_equal(rad, g["radius"]) and np.array_equal(lines, g["lines"])
    assert ctx.curves_to_lines(np.zeros((0, 12)), [], [])[0].shape == (0, 3)
    # command line: a pbrt file with comments, both parameter spellings and a non-curve shape
    n = 64
    pbrt = tmp_path / "hair.pbrt"
    with open(pbrt, "w") as f:
        f.write("# synthetic\nAttributeBegin\nShape \"trianglemesh\" \"integer indices\" [0 1 2] \"point P\" [0 0 0 1 0 0 0 1 0]\n")
        for c in range(n):
            pts = " ".join(repr(float(x)) for x in g["P"][c])
            kind = "point3" if c % 2 else "point"
            f.write(f'Shape "curve" "string type" [ "cylinder" ] "{kind} P" [ {pts} ] '
                    f'"float width0" [ {float(g["width0"][c])!r} ] "float width1" {float(g["width1"][c])!r}\n')
        f.write("AttributeEnd\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "yocto-hair_amd", "ycurves2ply")
    ply = tmp_path / "hair.ply"
    subprocess.check_call([exe, str(pbrt), str(ply)])
    blob = open(ply, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    assert b"element vertex %d" % (5 * n) in head and b"element line %d" % (4 * n) in head
    verts = np.frombuffer(body[: 28 * 5 * n], np.float32).reshape(-1, 7)
    assert np.array_equal(verts[:, 0:3], g["positions"][: 5 * n]) and np.array_equal(verts[:, 6], g["radius"][: 5 * n])
    assert np.array_equal(verts[:, 3:6], g["normals"][: 5 * n], equal_nan=True)
    lrec = np.frombuffer(body[28 * 5 * n:], np.uint8).reshape(-1, 9)
    assert (lrec[:, 0] == 2).all()
    assert np.array_equal(lrec[:, 1:].copy().view(np.int32), g["lines"][: 4 * n] - int(g["base_vertex"]))


@pytest.mark.parametrize("name,kw", [("sphere-hairblock", dict(scale=1.0)), ("hair-curls", dict(scale=0.05)),
                                     ("curly-hair", dict(scale=0.05)), ("crowd", dict(scale=0.05))])
def test_device_bvh_build_is_the_reference_tree(ctx, yh, name, kw):
    """csrc/bvh_gpu.hip builds the reference's tree on the GPU (level-synchronous, std::partition's
    permutation reproduced with a scan): nodes (boxes, children, counts, axes, breadth-first
    numbering) and leaf order are bitwise those of the host builder, which tests/test_abi.py checks
    against the oracle's tree — on small shapes, on the 1.6 M-segment hair block, on degenerate
    inputs (all centres equal; fewer than five primitives)."""
    from test_abi import _shape_boxes
    lib = yh.load()
    sf = yh.SceneFile(scene_path(name, **kw))
    d = sf.desc.contents
    cases = [np.ascontiguousarray(_shape_boxes(d.shapes[si])) for si in range(d.num_shapes)]
    rng = np.random.default_rng(5)
    same = np.tile(np.array([[0, 0, 0, 1, 1, 1]], np.float32), (37, 1))                 # identical centres: median splits
    flat = np.concatenate([rng.uniform(0, 1, (300, 3)) * [1, 0, 0], np.zeros((300, 3))], 1).astype(np.float32)
    flat[:, 3:] = flat[:, :3] + 0.01
    cases += [same, flat, cases[0][:3], cases[0][:1]]
    for boxes in cases:
        n = len(boxes)
        want_n = lib.yh_bvh_build(n, yh.fptr(boxes), None, None)
        want, wp = np.zeros((want_n, 8), np.float32), np.zeros(n, np.int32)
        lib.yh_bvh_build(n, yh.fptr(boxes), yh.fptr(want), yh.iptr(wp))
        got, gp = np.zeros((2 * n + 1, 8), np.float32), np.zeros(n, np.int32)
        got_n = lib.yh_bvh_build_gpu(ctx.h, n, yh.fptr(boxes), yh.fptr(got), yh.iptr(gp))
        assert got_n == want_n, (n, got_n, want_n)
        assert np.array_equal(gp, wp), n
        assert np.array_equal(got[:got_n].view(np.uint32), want.view(np.uint32)), n
    sf.close()


@pytest.mark.parametrize("n", [1, 3, 5, 37, 4099, 200000])
def test_device_wide_collapses_are_the_host_collapses(ctx, yh, n):
    """Round 6: yh_upload_scene makes the 4- / 8- / 16-wide nodes ON THE DEVICE (csrc/bvh_gpu.hip: a flag pass, a scan and one kernel per width write them
    straight into the array the traversal kernels read). Against the host's collapse_wide / _wide8 / _wide16 (host/bvh_build.cpp, themselves checked
    against the binary traversal's visiting order in tests/test_abi.py), slot for slot and bit for bit: the same boxes, the same leaf references, a
    child's reference = width x the host's child index (the device writes the child's first slot), the same split axes; for width 4 the occupied-slot bits."""
    rng = np.random.default_rng(n)
    lo = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    boxes = np.concatenate([lo, lo + rng.uniform(0.001, 0.05, (n, 3)).astype(np.float32)], axis=1)
    boxes[: n // 3, 3:] = boxes[: n // 3, :3] + np.float32(0.01)  # (many equal extents: ties in the split's choice of axis)
    lib = yh.load()
    for width in (4, 8, 16):
        nh = lib.yh_bvh_build_wide(n, yh.fptr(boxes), width, None)
        host = np.zeros((nh, width, 8), np.float32)
        assert lib.yh_bvh_build_wide(n, yh.fptr(boxes), width, yh.fptr(host)) == nh
        nd = lib.yh_bvh_build_wide_gpu(ctx.h, n, yh.fptr(boxes), width, None)
        assert nd == nh, f"width {width}: {nd} wide nodes on the device, {nh} on the host"
        dev = np.zeros((nh, width, 8), np.float32)
        assert lib.yh_bvh_build_wide_gpu(ctx.h, n, yh.fptr(boxes), width, yh.fptr(dev)) == nh
        assert np.array_equal(host[..., :6].view(np.uint32), dev[..., :6].view(np.uint32)), f"width {width}: child boxes differ"
        href, dref = host[..., 6].view(np.uint32).astype(np.int64), dev[..., 6].view(np.uint32).astype(np.int64)
        empty, leaf = href == 0xFFFFFFFF, (href >> 30) == 3
        node = ~empty & ~leaf
        assert np.array_equal(dref[empty | leaf], href[empty | leaf]), f"width {width}: empty / leaf references differ"
        assert np.array_equal(dref[node], href[node] * width), f"width {width}: child references differ"
        haxes, daxes = host[..., 7].view(np.uint32), dev[..., 7].view(np.uint32)
        if width == 4:
            assert np.array_equal(daxes & 0xFF, haxes & 0xFF)
            occ = ((~empty).astype(np.uint32) << np.arange(4, dtype=np.uint32)).sum(axis=1)
            assert np.array_equal((daxes >> 8) & 0xF, np.broadcast_to(occ[:, None], daxes.shape))
        else:
            assert np.array_equal(daxes, haxes)


@pytest.mark.parametrize("name,kw", [("lobes", dict(scale=0.05)), ("textured", dict(scale=0.05)), ("hair-curls", dict(scale=0.05)), ("crowd", dict(scale=0.05))],
                         ids=["lobes", "textured", "hair-curls", "crowd"])
def test_upload_on_the_device_equals_the_upload_on_the_host(ctx, yh, name, kw, monkeypatch):
    """Round 6: yh_upload_scene makes a big shape's bounds, tree and leaf records on the device and every shape's wide nodes there (csrc/bvh_gpu.hip).
    YHAIR_BVH=device sends EVERY shape that way — triangle meshes with and without normals, textured ones, two-triangle lights, instanced hair —
    and YHAIR_BVH=host none: closest hits (object, element, uv, distance) of 60 000 rays and a 4-spp image must be the same bits either way, for the
    quad kernels and for the sixteen-lane form (its 16-wide nodes)."""
    sf = yh.SceneFile(scene_path(name, **kw))
    rng = np.random.default_rng(5)
    n = 60000
    d = rng.normal(size=(n, 3))
    rays = np.concatenate([rng.uniform(-1.5, 1.5, (n, 3)) + [0, 1.0, 3.0], d / np.linalg.norm(d, axis=1, keepdims=True) * [1, 1, -1],
                           np.full((n, 1), 1e-4), np.full((n, 1), 3.4e38)], axis=1).astype(np.float32)
    got = {}
    for mode in ("host", "device"):
        monkeypatch.setenv("YHAIR_BVH", mode)
        ctx.upload_scene(sf.desc)
        hits = ctx.intersect(rays)
        imgs = []
        for shape in ("1", "8"):
            monkeypatch.setenv("YHAIR_SHAPE", shape)
            ctx.init_state(yh.TraceParams.default(resolution=64))
            ctx.trace_samples(4)
            imgs.append(ctx.download())
        monkeypatch.delenv("YHAIR_SHAPE")
        got[mode] = (hits, imgs)
    monkeypatch.delenv("YHAIR_BVH")
    assert (got["host"][0][0] >= 0).mean() > 0.02, "the rays should hit something"
    for a, b in zip(got["host"][0], got["device"][0]):
        assert np.array_equal(a, b), "closest hits differ between the host-side and the device-side upload"
    for a, b in zip(got["host"][1], got["device"][1]):
        assert np.array_equal(a, b), "images differ between the host-side and the device-side upload"
    assert np.array_equal(got["host"][1][0], got["host"][1][1]), "quads and the sixteen-lane form render different pixels"
    sf.close()


def test_empty_and_invalid_batches(ctx, yh):
    z = np.zeros((0, 3), np.float32)
    assert ctx.hair_eval(np.zeros((0, 30), np.float32), z, z).shape == (0, 3)
    assert ctx.lib.yh_hair_eval_batch(ctx.h, -1, None, None, None, None) == yh.YH_E_INVALID
    assert ctx.lib.yh_trace_samples(None, 1) == yh.YH_E_INVALID
    c2 = yh.Context(0)
    assert c2.lib.yh_trace_samples(c2.h, 1) == yh.YH_E_STATE          # no scene / state yet
    assert b"before" in c2.lib.yh_last_error(c2.h)
    p = yh.TraceParams.default()
    assert c2.lib.yh_init_state(c2.h, p) == yh.YH_E_STATE
    c2.close()


def _bad_index(yh, d, keep):
    """a vertex index out of range in the LAST shape, found after the first shapes were built"""
    import ctypes as C
    shapes = (yh.Shape * d.num_shapes)(*[d.shapes[i] for i in range(d.num_shapes)])
    last = shapes[d.num_shapes - 1]
    tri = last.num_triangles > 0
    n = (last.num_triangles * 3) if tri else (last.num_lines * 2)
    idx = np.ctypeslib.as_array(last.triangles if tri else last.lines, shape=(n,)).copy()
    idx[n // 2] = last.num_vertices  # one past the end
    if tri:
        last.triangles = idx.ctypes.data_as(C.POINTER(C.c_int))
    else:
        last.lines = idx.ctypes.data_as(C.POINTER(C.c_int))
    bad = yh.SceneDesc.from_buffer_copy(d)
    bad.shapes = shapes
    keep += [shapes, idx]
    return bad


def _bad_objects(yh, d, keep, edit, count=None):
    """the object list copied (`count` rows: the list repeated from its start), `edit(objects)` applied"""
    n = d.num_objects if count is None else count
    objects = (yh.Object * n)(*[d.objects[i % d.num_objects] for i in range(n)])
    edit(objects)
    bad = yh.SceneDesc.from_buffer_copy(d)
    bad.num_objects, bad.objects = n, objects
    keep.append(objects)
    return bad


def _bad_materials(yh, d, keep, edit):
    materials = (yh.Material * d.num_materials)(*[d.materials[i] for i in range(d.num_materials)])
    edit(materials)
    bad = yh.SceneDesc.from_buffer_copy(d)
    bad.materials = materials
    keep.append(materials)
    return bad


def _bad_shape_named(yh, d, keep):
    def edit(objects):
        objects[d.num_objects - 1].shape = d.num_shapes
    return _bad_objects(yh, d, keep, edit)


def _bad_material_named(yh, d, keep):
    def edit(objects):
        objects[d.num_objects - 1].material = d.num_materials
    return _bad_objects(yh, d, keep, edit)


def _bad_color_tex(yh, d, keep):
    def edit(materials):
        materials[0].color_tex = d.num_textures + 1
    return _bad_materials(yh, d, keep, edit)


def _bad_empty_texture(yh, d, keep):
    """one more texture behind the scene's, of zero width (no material needs to name it: every texture is looked at)"""
    pixels = np.zeros(3, np.uint8)
    textures = (yh.Texture * (d.num_textures + 1))(*[d.textures[i] for i in range(d.num_textures)])
    textures[d.num_textures] = yh.Texture(0, 1, 1, pixels.ctypes.data)
    bad = yh.SceneDesc.from_buffer_copy(d)
    bad.num_textures, bad.textures = d.num_textures + 1, textures
    keep += [textures, pixels]
    return bad


def _bad_no_lights(yh, d, keep):
    def edit(materials):
        for m in materials:
            m.emission[:] = [0, 0, 0]
    bad = _bad_materials(yh, d, keep, edit)
    envs = (yh.Environment * d.num_environments)(*[d.environments[i] for i in range(d.num_environments)])
    for e in envs:
        e.emission[:] = [0, 0, 0]
    bad.environments = envs
    keep.append(envs)
    return bad


def _bad_too_many_lights(yh, d, keep):
    """YH_MAX_LIGHTS + 1 emissive instances of the two-triangle light behind the scene's other objects"""
    emitters = [i for i in range(d.num_objects) if any(d.materials[d.objects[i].material].emission)
                and d.shapes[d.objects[i].shape].num_triangles == 2]
    others = [i for i in range(d.num_objects) if not any(d.materials[d.objects[i].material].emission)]
    assert emitters
    rows = [d.objects[i] for i in others] + [d.objects[emitters[0]]] * 17

    def edit(objects):
        for k, row in enumerate(rows):
            objects[k] = row
    return _bad_objects(yh, d, keep, edit, count=len(rows))


FAILED_UPLOADS = {
    "vertex index out of range": (_bad_index, b"out of range"),
    "object names shape num_shapes": (_bad_shape_named, b"references a missing shape or material"),
    "object names material num_materials": (_bad_material_named, b"references a missing shape or material"),
    "color_tex is num_textures + 1": (_bad_color_tex, b"references a missing texture"),
    "texture of zero width": (_bad_empty_texture, b"is empty"),
    "no lights": (_bad_no_lights, b"scene has no lights (the path sampler needs at least one)"),
    "more than YH_MAX_LIGHTS lights": (_bad_too_many_lights, b"more than 16 lights: object"),
}


@pytest.mark.parametrize("case", list(FAILED_UPLOADS))
def test_a_failed_upload_leaves_a_context_without_a_scene(yh, case):
    """yh_upload_scene replaces the device arrays of the previous scene as it goes (round 6: the records and the trees are made on the device): a call that
    fails half-way — one bad description per case, each refused at another exit behind the point where the previous scene is dropped — must leave a context
    that refuses to render ("before yh_upload_scene"), never one whose scene table points at freed arrays; and a good upload afterwards renders as a fresh
    context does."""
    import ctypes as C
    make_bad, text = FAILED_UPLOADS[case]
    c = yh.Context(0)
    sf = yh.SceneFile(scene_path("hair-curls", scale=0.05))
    c.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=48)
    c.init_state(p)
    c.trace_samples(2)
    want = c.download()
    keep = []  # (the arrays the bad description points at)
    bad = make_bad(yh, sf.desc.contents, keep)
    assert c.lib.yh_upload_scene(c.h, C.byref(bad)) == yh.YH_E_INVALID and text in c.lib.yh_last_error(c.h), c.lib.yh_last_error(c.h)
    assert c.lib.yh_trace_samples(c.h, 1) == yh.YH_E_STATE and b"before" in c.lib.yh_last_error(c.h)
    assert c.lib.yh_init_state(c.h, p) == yh.YH_E_STATE
    c.upload_scene(sf.desc)
    c.init_state(p)
    c.trace_samples(2)
    assert np.array_equal(c.download(), want)
    c.close(), sf.close()


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_reference_selftests_pass_on_device(ctx, which):
    """white_furnace, white_furnace_sampled, sampling_weights, sampling_consistency
    (ext.cpp:555-693): same seed, counts and thresholds; 'TEST FAILED!' -> YH_E_SELFTEST."""
    ok, worst = ctx.selftest(which)
    assert ok, f"TEST FAILED! self-test {which}: worst deviation {worst}"
    assert worst < [0.05, 0.01, 0.001, 0.05][which]


# ---------------------------------------------------------------------------------------------
# scenes: closest hits, images
# ---------------------------------------------------------------------------------------------
IDS = [f"{n}-{'-'.join(map(str, k.values()))}" for n, k in GOLDEN_SCENES]


@pytest.mark.parametrize("name,kw", GOLDEN_SCENES, ids=IDS)
def test_closest_hits_bit_exact(ctx, oracle, yh, name, kw):
    """Camera rays and jittered rays over the rendered scenes. The edges of the segment, triangle and box tests — rays built on a
    threshold and a float to either side of it — are tests/test_hits_unit.py's."""
    g = golden(f"scene_{scene_tag(name, kw)}.npz")
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc)
    obj, elem, uv, dist = ctx.intersect(g["rays"])
    assert np.array_equal(obj, g["object"]) and np.array_equal(elem, g["element"])
    assert np.array_equal(uv, g["uv"]) and np.array_equal(dist, g["distance"])
    assert 0.2 < np.mean(obj >= 0) < 0.95
    # many more rays against the oracle, including axis-aligned and zero directions
    rng = np.random.default_rng(5)
    m = 100000
    rays = np.repeat(g["rays"], m // len(g["rays"]) + 1, axis=0)[:m].copy()
    rays[:, :3] += rng.normal(0, 0.3, (m, 3)).astype(np.float32)
    rays[:6, 3:6] = [[1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0, 0], [0, 1, 1], [-1, 0, 0]]
    rays[6:1000, 7] = rng.uniform(0.5, 30, 994)  # finite tmax
    osc = oracle.scene(sf.desc)
    ho, hg = osc.intersect(rays), ctx.intersect(rays)
    for a, b in zip(ho, hg):
        assert np.array_equal(a, b)
    osc.close(), sf.close()


@pytest.mark.parametrize("name,kw", [GOLDEN_SCENES[1], GOLDEN_SCENES[4]], ids=[IDS[1], IDS[4]])
def test_crowded_waves_test_their_leaves_together(ctx, oracle, yh, name, kw):
    """The one-lane traversal deals the segments of a wave's line leaves one per lane (csrc/dev_lane.h: lane_step, COOP) and keeps the tests
    that do not fit the 64 lanes for the next step. Random rays rarely crowd a wave; here every wave's 64 rays are THE SAME ray (or the same
    up to an ulp of the origin), so all its lanes reach the same leaves in the same steps — up to 256 tests per step for 64 lanes — and every
    leaf is split over steps. Closest hits must still be the oracle's, bit for bit (and the quad kernel's)."""
    g = golden(f"scene_{scene_tag(name, kw)}.npz")
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc)
    base = g["rays"][g["object"] >= 0][:1100]
    assert len(base) >= 64
    base = np.tile(base, (1100 // len(base) + 1, 1))[:1100]
    rays = np.repeat(base, 64, axis=0).copy()          # 64 consecutive rays = one wave's lanes (k_intersect_lanes hands rays out in order)
    odd = np.arange(len(rays)) % 64 >= 48               # a quarter of each wave an ulp off: not all lanes in perfect step
    rays[odd, 0] = np.nextafter(rays[odd, 0], np.float32(np.inf))
    assert len(rays) >= 65536                           # the one-lane kernel (host/batch_api.cpp)
    osc = oracle.scene(sf.desc)
    ho, hg = osc.intersect(rays), ctx.intersect(rays)
    for a, b in zip(ho, hg):
        assert np.array_equal(a, b)
    assert np.mean(hg[0] >= 0) > 0.9
    os.environ["YHAIR_INTERSECT"] = "quad"
    try:
        hq = ctx.intersect(rays)
    finally:
        del os.environ["YHAIR_INTERSECT"]
    for a, b in zip(hq, hg):
        assert np.array_equal(a, b)
    osc.close(), sf.close()


@pytest.mark.parametrize("name,kw", GOLDEN_SCENES, ids=IDS)
def test_images_match_reference_statistically(ctx, yh, name, kw):
    g = golden(f"scene_{scene_tag(name, kw)}.npz")
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc)
    res = g["img_1"].shape[0]
    p = yh.TraceParams.default(resolution=res)
    assert ctx.init_state(p) == (g["img_1"].shape[1], g["img_1"].shape[0])
    # initial per-pixel streams are exact (pt.cpp:1942-1945)
    rng0 = ctx.download_rng()
    assert np.array_equal(rng0[:, 1], g["rng_1"][:, 1])
    # --- 1 spp -------------------------------------------------------------------------------
    ctx.trace_samples(1)
    img = ctx.download()
    ref = g["img_1"]
    assert np.isfinite(img).all()
    close = _rel(img[..., :3], ref[..., :3]).max(axis=2) < 1e-3
    assert close.mean() >= BAR_1SPP, f"only {close.mean():.3f} of pixels within rel 1e-3 at 1 spp"
    hit = ref[..., 3] > 0
    assert np.mean(img[..., 3] == ref[..., 3]) > 0.999  # primary visibility is exact
    # camera rays that escape: bit-identical under a constant environment; with the lat-long
    # sky texture the lookup goes through atan2 / acos, so the bilinear weights move by an ulp
    if name == "sphere-hairblock":
        assert np.array_equal(img[~hit], ref[~hit])
    else:
        assert np.mean(_rel(img[~hit][:, :3], ref[~hit][:, :3]).max(axis=1) < 1e-3) > 0.99
    # rng state after one sample agrees for the pixels whose path did not diverge
    rng1 = ctx.download_rng()
    assert np.mean(rng1[:, 0] == g["rng_1"][:, 0]) >= BAR_1SPP
    # --- 16 spp ------------------------------------------------------------------------------
    ctx.init_state(p)
    ctx.trace_samples(16)
    img16 = ctx.download()
    floor = _relrmse(g["img_16_seed12345"], g["img_16"])      # seed-to-seed noise floor
    err = _relrmse(img16, g["img_16"])
    assert err <= 0.5 * floor, f"relRMSE {err:.4f} vs seed floor {floor:.4f}"
    assert abs(img16[..., :3].mean() - g["img_16"][..., :3].mean()) <= 0.01 * g["img_16"][..., :3].mean()
    sf.close()


@pytest.mark.parametrize("res,bounces,clamp,seed", [(50, 1, 100.0, 961748941), (37, 16, 1.0, 7), (64, 3, 100.0, 2 ** 40 + 5),
                                                    (41, 64, 0.25, 961748941)])
def test_trace_params_follow_the_oracle(ctx, oracle, yh, res, bounces, clamp, seed):
    """trace_params (yocto_pathtrace.h:188-197) beyond the defaults: image sizes that are not a
    multiple of the 8x8 tile or the 4x4 work item, one bounce (no Russian roulette), long paths
    (roulette after bounce 3), an active clamp, 64-bit seeds. Compared with the oracle rendered
    here with the same parameters."""
    name, kw = "lobes", dict(scale=0.05)
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc)
    osc = oracle.scene(sf.desc)
    p = yh.TraceParams.default(res, bounces, clamp, seed)
    w, h = ctx.init_state(p)
    ctx.trace_samples(1)
    img, ref = ctx.download(), osc.render(p, 1)
    assert img.shape == ref.shape == (h, w, 4)
    close = _rel(img[..., :3], ref[..., :3]).max(axis=2) < 1e-3
    assert close.mean() >= BAR_1SPP and np.isfinite(img).all()
    assert img[..., :3].max() <= clamp * (1 + 1e-6)
    ctx.init_state(p)
    ctx.trace_samples(16)
    img16, ref16 = ctx.download(), osc.render(p, 16)
    other = osc.render(yh.TraceParams.default(res, bounces, clamp, seed + 1), 16)
    assert _relrmse(img16, ref16) <= 0.5 * _relrmse(other, ref16)
    osc.close(), sf.close()


SHADER_SCENES = [("sphere-hairblock", dict(scale=0.05, zoom=True)), ("hair-curls", dict(scale=0.05)),
                 ("lobes", dict(scale=0.05)), ("textured", dict(scale=0.05))]


@pytest.mark.parametrize("shader", ["naive", "eyelight", "normal"])
@pytest.mark.parametrize("name,kw", SHADER_SCENES, ids=[n for n, _ in SHADER_SCENES])
def test_other_shaders_match_reference(ctx, oracle, yh, name, kw, shader):
    """shader_type naive / eyelight / normal (pt.cpp:1514-1672) against the reference's own images
    (tests/golden/shaders.npz) and, for the noise floor, the oracle at another seed."""
    g = golden("shaders.npz")
    tag = scene_tag(name, kw)
    ref1, ref8 = g[f"{tag}|{shader}|1"], g[f"{tag}|{shader}|8"]
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=ref1.shape[0], shader=shader)
    assert ctx.init_state(p) == (ref1.shape[1], ref1.shape[0])
    ctx.trace_samples(1)
    img = ctx.download()
    assert np.isfinite(img).all()
    assert np.mean(img[..., 3] == ref1[..., 3]) > 0.999
    close = _rel(img[..., :3], ref1[..., :3]).max(axis=2) < 1e-3
    if shader == "normal":  # no sampling beyond the camera ray: only rounding of the normal differs
        assert close.mean() >= 0.97, f"{close.mean():.3f}"
        assert np.abs(img[..., :3] - ref1[..., :3]).max() < 2e-2   # a hit that flips between neighbouring hairs
    else:
        assert close.mean() >= BAR_1SPP, f"only {close.mean():.3f} of pixels within rel 1e-3 at 1 spp"
    ctx.init_state(p)
    ctx.trace_samples(8)
    img8 = ctx.download()
    if shader == "normal":
        assert _relrmse(img8, ref8) < 2e-3
    else:
        osc = oracle.scene(sf.desc)
        other = osc.render(yh.TraceParams.default(resolution=ref1.shape[0], shader=shader, seed=777), 8)
        assert _relrmse(img8, ref8) <= 0.5 * _relrmse(other, ref8)
        osc.close()
    with pytest.raises(Exception):  # the instrumented kernel exists for the path shader only
        ctx.trace_samples_counted(1)
    sf.close()


@pytest.mark.parametrize("exact", [False, True], ids=["fast-bsdf", "exact-bsdf"])
@pytest.mark.parametrize("which", ["sloth", "bold-man", "straight-hair", "curly-hair", "hair-curls", "sphere-hairblock"])
def test_reference_scene_files_render_like_the_reference(ctx, yh, which, exact):
    """The reference's own scene files (verbatim JSON, stand-in geometry) through loader, upload and
    k_trace, against the reference's images of the same files (tests/golden/refscenes.npz) — with the
    default BSDF arithmetic (inside 1e-4 of the reference's values) and with yh_trace_params::hair_exact
    (IEEE divisions, library log / sin / cos, the reference's double asin: csrc/exact.hip)."""
    g = golden("refscenes.npz")
    ref1, ref8, other = g[f"{which}|1"], g[f"{which}|8"], g[f"{which}|8_seed777"]
    sf = yh.SceneFile(scene_path("ref-" + which, scale=0.05))
    ctx.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=48, hair_exact=exact)
    assert ctx.init_state(p) == (ref1.shape[1], ref1.shape[0])
    ctx.trace_samples(1)
    img = ctx.download()
    assert np.isfinite(img).all()
    assert np.mean(img[..., 3] == ref1[..., 3]) > 0.995
    close = _rel(img[..., :3], ref1[..., :3]).max(axis=2) < 1e-3
    assert close.mean() >= BAR_1SPP, f"only {close.mean():.3f} of pixels within rel 1e-3 at 1 spp"
    # 8 spp against the seed-to-seed floor (0.5 x floor), the SAME bar for both arithmetics. Until round 4
    # the default arithmetic had a relaxed bar of 0.75 (measured 0.52-0.62 on the reference's sphere-hairblock: light hair,
    # colour 0.8, eight-bounce paths, each bounce a chance to leave the reference's path). Since the chain that ends in the
    # SAMPLED DIRECTION is kept in the exact forms (csrc/dev_hair.h: YH_DIR_EXACT; only the lobes' values stay fast) it
    # measures 0.21 there, as the exact arithmetic does (0.23): profiles/r04/direction_chain_ab.txt
    ctx.init_state(p)
    ctx.trace_samples(8)
    assert ctx.launch_shape() == 0 or not exact
    bar = 0.5
    err, floor = _relrmse(ctx.download(), ref8), _relrmse(other, ref8)
    assert err <= bar * floor, f"{which}: relRMSE {err:.4f} vs {bar} x seed floor {floor:.4f}"
    sf.close()


def test_unknown_shader_is_rejected(ctx, yh):
    sf = yh.SceneFile(scene_path("lobes", scale=0.05))
    ctx.upload_scene(sf.desc)
    with pytest.raises(Exception, match="sampler unknown"):  # pt.cpp:1669
        ctx.init_state(yh.TraceParams.default(resolution=32, shader=7))
    sf.close()


def test_sample_batching_and_sharding_do_not_change_pixels(ctx, yh):
    """1x16 spp == 16x1 spp == 4+12 spp bitwise, and every shard of a 2- and 3-way tile split
    reproduces exactly the pixels of the single-GPU image."""
    sf = yh.SceneFile(scene_path("sphere-hairblock", scale=0.05, zoom=True))
    ctx.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=72)
    ctx.set_shard(0, 1)
    ctx.init_state(p)
    ctx.trace_samples(16)
    full = ctx.download()
    ctx.init_state(p)
    for _ in range(16):
        ctx.trace_samples(1)
    assert np.array_equal(ctx.download(), full)
    ctx.init_state(p)
    ctx.trace_samples(4), ctx.trace_samples(0), ctx.trace_samples(12)
    assert np.array_equal(ctx.download(), full)
    import yhair_dist
    for world in (2, 3):
        acc = np.zeros_like(full)
        for rank in range(world):
            ctx.set_shard(rank, world)
            ctx.init_state(p)
            ctx.trace_samples(16)
            part = ctx.download()
            assert ctx.shard_pixels(rank, world) == yhair_dist.shard_pixels(72, 72, rank, world)
            owned = np.zeros(full.shape[:2], bool)
            tx, _ = yhair_dist.tiles_xy(72, 72)
            for t in yhair_dist.shard_tiles(72, 72, rank, world):
                owned[(t // tx) * 8:(t // tx) * 8 + 8, (t % tx) * 8:(t % tx) * 8 + 8] = True
            assert np.array_equal(part[owned], full[owned])
            assert not part[~owned].any()
            acc += part
        assert np.array_equal(acc, full)
    ctx.set_shard(0, 1)
    sf.close()


def test_pack_unpack_tiles_on_device(ctx, yh):
    import torch
    import yhair_dist
    sf = yh.SceneFile(scene_path("sphere-hairblock", scale=0.02))
    ctx.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=50)  # 50 is not a multiple of 8: ragged edge tiles
    ctx.set_shard(0, 1)
    w, h = ctx.init_state(p)
    ctx.trace_samples(2)
    full = ctx.download()
    image = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    for rank in range(3):
        ctx.set_shard(rank, 3)
        ctx.init_state(p)
        ctx.trace_samples(2)
        n = ctx.shard_pixels(rank, 3)
        packed = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        assert ctx.pack_tiles_device(packed.data_ptr(), n) == n
        assert np.array_equal(packed.cpu().numpy(), yhair_dist.pack_tiles_host(ctx.download(), rank, 3))
        ctx.unpack_tiles_device(packed.data_ptr(), rank, 3, image.data_ptr())
    assert np.array_equal(image.cpu().numpy(), full)
    ctx.set_shard(0, 1)
    sf.close()


def test_work_counters_match_oracle_on_identical_paths(ctx, oracle, yh):
    """Where no path can diverge (1 bounce) the instrumented kernel counts the same rays and
    shading events as the reference algorithm. Node visits are fewer (4-wide nodes: one visit
    tests four reference boxes); primitive tests can only be equal or slightly more (a child box
    is accepted with the ray extent current at its parent, before nearer hits shrink it)."""
    sf = yh.SceneFile(scene_path("sphere-hairblock", scale=0.02))
    ctx.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=64, bounces=1)
    ctx.init_state(p)
    wc = ctx.trace_samples_counted(2).as_dict()
    osc = oracle.scene(sf.desc)
    _, owc = osc.render(p, 2, want_counts=True)
    owc = owc.as_dict()
    for k in ("samples", "rays", "hair_shades", "surf_shades", "env_lookups", "env_samples"):
        assert wc[k] == owc[k], k
    assert 0 < wc["nodes"] < owc["nodes"], (wc, owc)
    assert owc["seg_tests"] <= wc["seg_tests"] <= 1.15 * owc["seg_tests"], (wc["seg_tests"], owc["seg_tests"])
    assert owc["tri_tests"] <= wc["tri_tests"] <= 1.15 * owc["tri_tests"], (wc["tri_tests"], owc["tri_tests"])
    osc.close(), sf.close()


@pytest.mark.parametrize("name", ["hair-curls", "textured"])
def test_cli_matches_the_library(ctx, yh, tmp_path, name):
    """yscenetrace (the reference's command line on the C++ mirror of its API) writes the same
    pixels yh_download returns, in the reference's .pfm layout (top row first, rgb) — also for a
    scene whose materials, textures and texture coordinates go through the mirror's setters."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "yocto-hair_amd", "yscenetrace")
    scene = scene_path(name, scale=0.05)
    out = str(tmp_path / "cli.pfm")
    r = subprocess.run([exe, scene, "-r", "48", "-s", "6", "-o", out, "--spp-per-launch", "4"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    head = b"PF\n48 48\n-1\n"
    assert raw.startswith(head)
    cli = np.frombuffer(raw[len(head):], np.float32).reshape(48, 48, 3)
    sf = yh.SceneFile(scene)
    ctx.upload_scene(sf.desc)
    ctx.set_shard(0, 1)
    ctx.init_state(yh.TraceParams.default(resolution=48))
    ctx.trace_samples(6)
    assert np.array_equal(cli, ctx.download()[..., :3])
    # --shader,-t as in the reference (cli.cpp:213): the other shaders go through the same mirror
    r = subprocess.run([exe, scene, "-r", "48", "-s", "3", "-t", "eyelight", "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    cli = np.frombuffer(open(out, "rb").read()[len(head):], np.float32).reshape(48, 48, 3)
    ctx.init_state(yh.TraceParams.default(resolution=48, shader="eyelight"))
    ctx.trace_samples(3)
    assert np.array_equal(cli, ctx.download()[..., :3])
    # reference CLI behaviour: unknown shaders and bad scenes exit(1) with the message
    r = subprocess.run([exe, scene, "-t", "whitted"], capture_output=True, text=True)
    assert r.returncode == 1 and "unknown shader" in r.stdout
    r = subprocess.run([exe, str(tmp_path / "missing.json")], capture_output=True, text=True)
    assert r.returncode == 1 and "file not found" in r.stdout
    sf.close()


def test_async_launch_equals_the_blocking_call(ctx, yh):
    """yh_trace_samples_async + yh_synchronize (what a caller overlapping the render with its own work uses,
    e.g. the preview of apps/ysceneitraces/ysceneitraces.cpp:255-300) leaves the same pixels and RNG states as
    the blocking yh_trace_samples, launch for launch."""
    sf = yh.SceneFile(scene_path("straight-hair", scale=0.05))
    ctx.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=72)
    ctx.init_state(p)
    ctx.trace_samples(3), ctx.trace_samples(5)
    ref = (ctx.download(), ctx.download_rng())
    ctx.init_state(p)
    ctx.trace_samples_async(3)
    ctx.trace_samples_async(5)  # queued behind the first on the context's stream
    ctx.synchronize()
    assert ctx.last_trace_ms()[0] > 0
    assert np.array_equal(ctx.download(), ref[0]) and np.array_equal(ctx.download_rng(), ref[1])
    sf.close()


@pytest.mark.parametrize("n", [2, 3, 4])
def test_single_process_gather_over_contexts(yh, n):
    """yscenetrace --gpus N in one process: N contexts, context i renders shard (i, N), yh_gather_framebuffer
    brings the packed tiles to context 0 and un-interleaves them. On this one-GPU box the contexts share the
    device, so the payload moves by device-to-device copies instead of the RCCL gather; sharding, packing,
    the padded shard capacity and the un-interleave are the same code. Bit-identical to one context."""
    sf = yh.SceneFile(scene_path("hair-curls", scale=0.05))
    p = yh.TraceParams.default(resolution=100)  # 13 x 13 tiles: ragged edge, shards of unequal size
    one = yh.Context(0)
    one.upload_scene(sf.desc)
    one.init_state(p)
    one.trace_samples(4)
    ref = one.download()
    ctxs = [one] + [yh.Context(0) for _ in range(n - 1)]
    for i, c in enumerate(ctxs):
        if i:
            c.upload_scene(sf.desc)
        c.set_shard(i, n)
        c.init_state(p)
        c.trace_samples(4)
    img = yh.gather_framebuffer(ctxs)
    assert np.array_equal(img, ref)
    # a context that holds the wrong shard is refused
    ctxs[1].set_shard(0, n)
    ctxs[1].init_state(p)
    with pytest.raises(yh.YhError):
        yh.gather_framebuffer(ctxs)
    for c in ctxs:
        c.close()
    sf.close()


def test_cli_gpus_and_preview(ctx, yh, tmp_path):
    """yscenetrace --devices 0,0,0 (three contexts, tile-sharded, gathered) writes the pixels of the one-GPU run;
    ysceneitraces (the reference's progressive caller, headless) renders the resolution / pratio preview, then
    its samples through the stop-flag overload, and stops early when the flag is set."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scene = scene_path("straight-hair", scale=0.05)
    head = b"PF\n60 60\n-1\n"

    def pfm(path, w=60):
        raw = open(path, "rb").read()
        hd = f"PF\n{w} {w}\n-1\n".encode()
        assert raw.startswith(hd)
        return np.frombuffer(raw[len(hd):], np.float32).reshape(w, w, 3)

    exe = os.path.join(root, "yocto-hair_amd", "yscenetrace")
    a, b = str(tmp_path / "one.pfm"), str(tmp_path / "three.pfm")
    for out, extra in ((a, []), (b, ["--devices", "0,0,0"])):
        r = subprocess.run([exe, scene, "-r", "60", "-s", "5", "-o", out] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    assert "on 3 GPU(s)" in r.stdout
    assert np.array_equal(pfm(a), pfm(b))
    # the progressive caller
    exe = os.path.join(root, "yocto-hair_amd", "ysceneitraces")
    out, prev = str(tmp_path / "it.pfm"), str(tmp_path / "prev.pfm")
    r = subprocess.run([exe, scene, "-r", "60", "-s", "5", "--pratio", "4", "-o", out, "--preview-image", prev], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "preview: 15x15 at 1 spp upscaled to 60x60" in r.stdout and "render: 5 of 5 samples" in r.stdout
    assert np.array_equal(pfm(out), pfm(a))  # five one-sample launches = one five-sample launch
    sf = yh.SceneFile(scene)
    ctx.upload_scene(sf.desc)
    ctx.set_shard(0, 1)
    ctx.init_state(yh.TraceParams.default(resolution=15))
    ctx.trace_samples(1)
    small = ctx.download()[..., :3]
    assert np.array_equal(pfm(prev), np.repeat(np.repeat(small, 4, axis=0), 4, axis=1))
    # a flag set at once stops the render within a launch: far fewer samples than asked for, exit code 0
    r = subprocess.run([exe, scene, "-r", "60", "-s", "100000", "-o", out, "--stop-after-ms", "0"], capture_output=True, text=True)
    assert r.returncode == 0 and "(stopped)" in r.stdout, r.stdout + r.stderr
    done = int(r.stdout.split("render: ")[1].split(" of ")[0])
    assert done < 1000
    sf.close()


def test_full_size_properties(ctx, yh):
    """BASELINE.json's full C1 size (720x720, 1.6 M segments): properties that do not need the
    oracle — determinism, finiteness, energy bounds, background pixels = environment."""
    sf = yh.SceneFile(scene_path("sphere-hairblock", scale=1.0))
    ctx.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=720)
    assert ctx.init_state(p) == (720, 720)
    ctx.trace_samples(4)
    a = ctx.download()
    ctx.init_state(p)
    ctx.trace_samples(4)
    assert np.array_equal(ctx.download(), a)  # run-to-run bit determinism
    assert np.isfinite(a).all() and a.min() >= 0 and a[..., :3].max() <= 100.0  # clamp (pt.cpp:1684)
    bg = a[..., 3] == 0
    assert 0.3 < bg.mean() < 0.95
    assert np.array_equal(a[bg][:, :3], np.ones((bg.sum(), 3), np.float32))  # constant env (1,1,1)
    sf.close()


# ---------------------------------------------------------------------------------------------
# round 2: per-pixel k-sigma bar, launch shapes, BASELINE configs C2-C4 at full size
# ---------------------------------------------------------------------------------------------
HAIR_GOLDEN = [(n, k) for n, k in GOLDEN_SCENES if n in ("sphere-hairblock", "straight-hair", "curly-hair", "hair-curls")
               and not k.get("dof")]


def _k_sigma_share(ctx, osc, yh, res, spp, ref_img, seeds=(961748941, 12345, 777, 31337, 2024, 99)):
    """Share of pixels with |gpu - ref| <= K_SIGMA sqrt(var_ref + var_gpu), the variances of an spp-sample
    pixel mean estimated from renders at independent seeds on both sides."""
    gpu, ref = [], []
    for sd in seeds:
        p = yh.TraceParams.default(resolution=res, seed=sd)
        ctx.init_state(p)
        ctx.trace_samples(spp)
        gpu.append(ctx.download()[..., :3])
        ref.append(osc.render(p, spp)[..., :3] if sd != seeds[0] or ref_img is None else ref_img[..., :3])
    gpu, ref = np.stack(gpu), np.stack(ref)
    var = gpu.var(axis=0, ddof=1) + ref.var(axis=0, ddof=1)
    delta = np.abs(gpu[0] - ref[0])
    # pixels without variance (background under a constant environment) must agree to rounding
    ok = delta <= K_SIGMA * np.sqrt(var) + 1e-3 * np.abs(ref[0]) + 1e-6
    return float(ok.all(axis=2).mean()), float(np.sqrt(np.mean(delta ** 2)) / ref[0].mean())


@pytest.mark.parametrize("name,kw", HAIR_GOLDEN, ids=[f"{n}-{'-'.join(map(str, k.values()))}" for n, k in HAIR_GOLDEN])
def test_per_pixel_error_within_k_sigma(ctx, oracle, yh, name, kw):
    """16 spp against the reference's golden image, 64 spp against the oracle (bit-identical to the
    reference): >= 99 % of pixels within K_SIGMA standard errors."""
    g = golden(f"scene_{scene_tag(name, kw)}.npz")
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc)
    osc = oracle.scene(sf.desc)
    res = g["img_16"].shape[0]
    share16, err16 = _k_sigma_share(ctx, osc, yh, res, 16, g["img_16"])
    assert share16 >= 0.99, f"16 spp: {share16:.4f} of pixels within {K_SIGMA} sigma (relRMSE {err16:.4f})"
    share64, err64 = _k_sigma_share(ctx, osc, yh, res, 64, None, seeds=(961748941, 12345, 777, 31337))
    assert share64 >= 0.99, f"64 spp: {share64:.4f} of pixels within {K_SIGMA} sigma (relRMSE {err64:.4f})"
    osc.close(), sf.close()


@pytest.mark.parametrize("exact", [False, True], ids=["fast-bsdf", "exact-bsdf"])
@pytest.mark.parametrize("name,kw", [("straight-hair", dict(scale=0.05)), ("curly-hair", dict(scale=0.05)), ("hair-curls", dict(scale=0.05))],
                         ids=["straight-hair", "curly-hair", "hair-curls"])
def test_dense_hair_has_no_mean_shift_at_high_spp(ctx, oracle, yh, name, kw, exact):
    """The bias estimator of tools/parity_vs_spp.py as a test. The path-following ratio relRMSE(gpu, ref) / seed floor GROWS with
    the sample count on dense hair — what per-pixel stream decorrelation predicts (a device path that leaves the reference's shifts every later draw
    of that pixel's one PCG32 stream) and what a small bias of the fast BSDF arithmetic would also look like. What tells them apart: decorrelated
    estimates have the same MEAN. At 512 spp (32 x the spp of the path-following bar) the mean radiance over the pixels that see the model, two seeds
    pooled, must agree with the oracle's within 3 standard errors of the difference (pixels are independent streams: SE = std of the per-pixel
    differences / sqrt(n)) — for the default arithmetic and for the exact one; a bias of 0.5 % of the radiance would be ~ 5 SE here."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from parity_vs_spp import mean_shift
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc)
    osc = oracle.scene(sf.desc)
    res, spp = 48, 512
    gpu, ref = [], []
    for sd in (961748941, 12345):
        p = yh.TraceParams.default(resolution=res, seed=sd, hair_exact=exact)
        ctx.init_state(p)
        ctx.trace_samples(spp)
        gpu.append(ctx.download().astype(np.float64))
        ref.append(osc.render(yh.TraceParams.default(resolution=res, seed=sd), spp).astype(np.float64))
    mask = (ref[0][..., 3] > 0) & (ref[1][..., 3] > 0)
    assert mask.sum() > 500, "the check image should mostly see hair"
    ms = mean_shift((gpu[0][..., :3] + gpu[1][..., :3]) / 2, (ref[0][..., :3] + ref[1][..., :3]) / 2, mask)
    lum = ms["luminance"]
    assert lum["se"] < 5e-3, f"the estimator is too noisy to say anything: SE {lum['se']:.2e}"
    assert abs(lum["rel_shift"]) <= 3.0 * lum["se"], f"mean radiance over {ms['pixels']} pixels differs by {lum['rel_shift']:+.3e} = {lum['shift_in_se']:+.2f} standard errors ({lum['se']:.2e})"
    for c in "rgb":
        assert abs(ms[c]["rel_shift"]) <= 4.0 * ms[c]["se"], f"channel {c}: {ms[c]['rel_shift']:+.3e} against SE {ms[c]['se']:.2e}"
    osc.close(), sf.close()


@pytest.mark.parametrize("name,kw", [("sphere-hairblock", dict(scale=0.05, zoom=True)), ("straight-hair", dict(scale=0.05)),
                                     ("hair-curls", dict(scale=0.05)), ("lobes", dict(scale=0.05)),
                                     ("lights-unit", dict(scale=0.05, biglight=True))],
                         ids=["sphere-hairblock", "straight-hair", "hair-curls", "lobes", "big-light"])
def test_launch_shapes_and_kernels_render_identical_pixels(ctx, yh, name, kw, monkeypatch):
    """The host picks the integrator kernel — k_trace with a quad per path at 512 x 4 or at 256 x 5 (single-predicate
    line test), with an OCTET per path over 8-wide nodes (chain-bound launches), or the one-lane-per-path k_stream
    (csrc/stream.hip) — by measurement, so which kernel a render runs depends on history. Every choice must give
    the same bits: YHAIR_SHAPE forces each."""
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=88)
    images = {}
    for shape in ("0", "1", "3", "4", "5", "6", "7", "8"):  # k_trace 512 x 4, 256 x 5, k_stream, k_trace with octets, quads + octets side by side, sixteen lanes per path, octets with leaf pairs, sixteen lanes with leaf groups (2: a developer build only)
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


def test_stream_reports_print_without_changing_the_render(ctx, yh, monkeypatch, capfd):
    """The developer reports of a k_stream launch (host/stream_report.cpp: YHAIR_ST_WAVELOG's wave log, YHAIR_ST_PROF's tables of the
    instrumented build) on the device: two launches with both switched on print their lines — one wave log per launch, the correlation
    with the previous launch from the second on, the ten branch lines of each table — and render the bits and leave the RNG states of
    the same two launches without them."""
    sf = yh.SceneFile(scene_path("sphere-hairblock", scale=0.02))
    ctx.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=40)
    monkeypatch.setenv("YHAIR_SHAPE", "3")

    def render(reports):
        ctx.init_state(p)
        if reports:  # (after yh_init_state: its probe launch of a new image would report too)
            capfd.readouterr()
            monkeypatch.setenv("YHAIR_ST_WAVELOG", "1")
            monkeypatch.setenv("YHAIR_ST_PROF", "1")
        shapes = []
        for n in (2, 3):
            ctx.trace_samples(n)
            shapes.append(ctx.launch_shape())
        return ctx.download(), ctx.download_rng(), shapes

    plain = render(False)
    reported = render(True)
    err = capfd.readouterr().err
    monkeypatch.delenv("YHAIR_ST_WAVELOG"), monkeypatch.delenv("YHAIR_ST_PROF"), monkeypatch.delenv("YHAIR_SHAPE")
    assert plain[2] == [3, 3] and reported[2] == [3, 3]
    assert plain[0][..., 3].max() > 0
    assert np.array_equal(reported[0], plain[0]), "the reports change the pixels"
    assert np.array_equal(reported[1], plain[1]), "the reports change the RNG states"
    lines = err.splitlines()
    logs = [i for i, l in enumerate(lines) if l.startswith("[yhair] k_stream wave log: ")]
    assert len(logs) == 2, err
    # (a launch prints its correlation line above its wave-log line)
    assert any("correlation of the waves' ends with the previous launch's:" in l for l in lines[logs[0] + 1:logs[1]]), err
    branches = [l.split()[2] for l in lines if l.startswith("[yhair]   branch ")]
    assert branches == 2 * ["step", "pop", "scene", "enter", "fetch", "node", "line-leaf", "tri-leaf", "push", "2nd-seg"], err
    sf.close()


@pytest.mark.parametrize("name,kw", [("sphere-hairblock", dict(scale=0.05, zoom=True)), ("straight-hair", dict(scale=0.05))],
                         ids=["sphere-hairblock", "straight-hair"])
def test_kernel_trials_are_cut_off_a_long_request(ctx, yh, name, kw, monkeypatch):
    """yh_trace_samples starts a long request with 32-sample launches of the kernels the image has not timed yet
    (host/launch_plan.cpp: pick_launch_shape). The samples count like any others: one 150-sample request renders the bits of
    a single launch of one kernel, in more than one launch; once every candidate is timed a request is one launch again."""
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=90)  # (a size no other test uses: no timings kept from an earlier image)
    monkeypatch.setenv("YHAIR_SHAPE", "0")
    ctx.init_state(p)
    ctx.trace_samples(150)
    assert ctx.last_trace_ms()[1] == 1
    base = (ctx.download(), ctx.download_rng())
    monkeypatch.delenv("YHAIR_SHAPE")
    ctx.init_state(p)
    ctx.trace_samples(150)
    ms, launches = ctx.last_trace_ms()
    assert 3 <= launches <= 5 and ms > 0, launches  # the settling launch, two or three trials, then the rest (150 samples hold at most four 32-sample launches)
    assert np.array_equal(ctx.download(), base[0]) and np.array_equal(ctx.download_rng(), base[1])
    # up to four candidates (a chain-bound image: quads, octets without and with leaf pairs, sixteen lanes), each tried
    # twice when it ties with the best, fresh item costs may change the reading: the trials end within a few requests
    for _ in range(6):
        ctx.trace_samples(150)
        assert ctx.last_trace_ms()[1] <= 4
        if ctx.last_trace_ms()[1] == 1:
            break
    ctx.trace_samples(150)
    assert ctx.last_trace_ms()[1] == 1
    assert ctx.launch_shape() in (0, 1, 3, 4, 6, 7, 8)
    sf.close()


FULL_CONFIGS = [
    ("C1", "sphere-hairblock", dict(scale=1.0), 720),
    ("C2-beta_m0.1", "straight-hair", dict(scale=1.0, beta_m=0.1), 720),
    ("C2-beta_m0.25", "straight-hair", dict(scale=1.0, beta_m=0.25), 720),
    ("C2-beta_m0.6", "straight-hair", dict(scale=1.0, beta_m=0.6), 720),
    ("C3", "curly-hair", dict(scale=1.0), 1280),
    ("C4", "hair-curls", dict(scale=1.0), 1280),
]


@pytest.mark.parametrize("tag,name,kw,res", FULL_CONFIGS, ids=[c[0] for c in FULL_CONFIGS])
def test_baseline_configs_at_full_size(ctx, oracle, yh, tag, name, kw, res):
    """BASELINE.json configs[1..4] with their full geometry (1.6 M / 3.2 M / 4 x 1.0 M segments): (1) at the
    config's resolution, the size-independent properties of test_full_size_properties; (2) the same
    geometry at 96 x 96 against the oracle with ALL THREE image bars of the golden scenes: 1 spp within 1e-3,
    16 spp relRMSE <= 0.5 x the seed-to-seed floor, 16 spp per-pixel error within K_SIGMA standard errors;
    (3) (round 4) the oracle AT THE CONFIG'S OWN RESOLUTION — the very camera rays of the config: 720^2 / 1280^2 —
    all three bars again: 1 spp within 1e-3 with identical alpha, 8 spp relRMSE <= 0.5 x the floor, 8 spp per-pixel error
    within K_SIGMA standard errors over four seeds (the oracle on the box's host threads: seconds per render)."""
    sf = yh.SceneFile(scene_path(name, **kw))
    d = sf.desc.contents
    segments = sum(d.shapes[i].num_lines for i in range(d.num_shapes))
    assert segments >= 1_000_000
    ctx.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=res)
    assert ctx.init_state(p) == (res, res)
    ctx.trace_samples(1), ctx.trace_samples(2)
    a = ctx.download()
    ctx.init_state(p)
    ctx.trace_samples(3)
    assert np.array_equal(ctx.download(), a)                       # determinism; 1 + 2 spp == 3 spp
    assert np.isfinite(a).all() and a.min() >= 0 and a[..., :3].max() <= 100.0 * (1 + 1e-6)
    hit = a[..., 3] > 0
    assert 0.05 < hit.mean() < 0.98
    # camera rays that escape see the sky texture times the environment's emission (C1: a constant environment):
    # bounded by its brightest texel, and never black
    env = d.environments[0]
    n_tex = env.tex_width * env.tex_height
    emission = np.array(list(env.emission), np.float32)
    texmax = (np.ctypeslib.as_array(env.texels, (n_tex, 3)).max(axis=0) if n_tex else np.ones(3, np.float32)) * emission
    assert (a[~hit][:, :3] <= texmax * (1 + 1e-5)).all() and a[~hit][:, :3].max(axis=1).min() > 0
    # (2) full geometry, 96 x 96, against the oracle
    osc = oracle.scene(sf.desc)
    q = yh.TraceParams.default(resolution=96)
    ctx.init_state(q)
    ctx.trace_samples(1)
    g1, r1 = ctx.download(), osc.render(q, 1)
    assert np.mean(g1[..., 3] == r1[..., 3]) > 0.999
    close = _rel(g1[..., :3], r1[..., :3]).max(axis=2) < 1e-3
    assert close.mean() >= BAR_1SPP, f"{tag}: only {close.mean():.3f} of pixels within rel 1e-3 at 1 spp"
    ctx.init_state(q)
    ctx.trace_samples(16)
    g16, r16 = ctx.download(), osc.render(q, 16)
    other = osc.render(yh.TraceParams.default(resolution=96, seed=12345), 16)
    err, floor = _relrmse(g16, r16), _relrmse(other, r16)
    assert err <= 0.5 * floor, f"{tag}: relRMSE {err:.4f} vs seed floor {floor:.4f}"
    share, _ = _k_sigma_share(ctx, osc, yh, 96, 16, r16, seeds=(961748941, 12345, 777, 31337))
    assert share >= 0.99, f"{tag}: {share:.4f} of pixels within {K_SIGMA} sigma at 16 spp"
    # (3) the config's own image size against the oracle
    ctx.init_state(p)
    ctx.trace_samples(1)
    g1, r1 = ctx.download(), osc.render(p, 1)
    assert np.array_equal(g1[..., 3], r1[..., 3]), f"{tag}: primary visibility differs at {res}^2"
    close = _rel(g1[..., :3], r1[..., :3]).max(axis=2) < 1e-3
    assert close.mean() >= BAR_1SPP, f"{tag}: only {close.mean():.3f} of the {res}^2 pixels within rel 1e-3 at 1 spp"
    ctx.init_state(p)
    ctx.trace_samples(8)
    g8, r8 = ctx.download(), osc.render(p, 8)
    other8 = osc.render(yh.TraceParams.default(resolution=res, seed=12345), 8)
    err, floor = _relrmse(g8, r8), _relrmse(other8, r8)
    assert err <= 0.5 * floor, f"{tag} at {res}^2: relRMSE {err:.4f} vs seed floor {floor:.4f}"
    share, _ = _k_sigma_share(ctx, osc, yh, res, 8, r8, seeds=(961748941, 12345, 777, 31337))
    assert share >= 0.99, f"{tag} at {res}^2: {share:.4f} of pixels within {K_SIGMA} sigma at 8 spp"
    osc.close(), sf.close()


@pytest.mark.parametrize("biglight", [False, True], ids=["small-lights-in-lds", "big-light-through-the-bvh"])
def test_light_sampling_matches_oracle_at_unit_level(ctx, oracle, yh, biglight):
    """a20 (sample_lights / sample_lights_pdf, pt.cpp:1283-1358) isolated from the BSDF: a scene whose
    only surfaces are diffuse (no hair, so no libm-driven divergence before the light code runs) under
    two area lights and the textured sky, at 1 bounce: every radiance value is emission + one
    MIS-weighted light / BRDF sample, i.e. sample_lights, the env-CDF upper_bound and both pdf branches.
    Both light paths of the kernels: quads of two triangles (their records staged in LDS, no traversal) and,
    with `biglight`, an 18-triangle light that is sampled and intersected through memory (GENERAL variants)."""
    sf = yh.SceneFile(scene_path("lights-unit", scale=0.05, biglight=biglight))
    ctx.upload_scene(sf.desc)
    osc = oracle.scene(sf.desc)
    for bounces, spp in ((2, 4), (8, 4)):
        p = yh.TraceParams.default(resolution=96, bounces=bounces)
        ctx.init_state(p)
        ctx.trace_samples(spp)
        img, rng = ctx.download(), ctx.download_rng()
        ref, rref = osc.render(p, spp, want_rng=True)
        # diffuse-only paths: every draw count and nearly every value follows the reference exactly
        assert np.mean(rng[:, 0] == rref[:, 0]) > 0.995
        close = _rel(img[..., :3], ref[..., :3]).max(axis=2) < 1e-3
        assert close.mean() > 0.99, f"bounces {bounces}: {close.mean():.4f}"
        assert (ref[..., 3] > 0).mean() > 0.3
    osc.close(), sf.close()


# ---------------------------------------------------------------------------------------------
# round 3: the collective executed for real (a world of one), the bare `bench.py --gpus N`, the kernel choice pinned
# ---------------------------------------------------------------------------------------------
def _small_render(ctx, yh, res=100, spp=4):
    sf = yh.SceneFile(scene_path("sphere-hairblock", scale=0.05, zoom=True))
    ctx.upload_scene(sf.desc)
    ctx.set_shard(0, 1)
    w, h = ctx.init_state(yh.TraceParams.default(resolution=res))  # 100 is not a multiple of 8: ragged edge tiles
    ctx.trace_samples(spp)
    return sf, w, h, ctx.download()


def test_rccl_gather_executes_on_a_world_of_one(ctx, yh, monkeypatch):
    """yh_gather_framebuffer's RCCL branch (librccl dlopen + dlsym signatures, ncclCommInitAll, the grouped
    ncclGather on the context's stream, k_unpack behind it) on the one GPU a test box has: YHAIR_GATHER=rccl
    makes a communicator of one rank. The image must be the bits of yh_download."""
    sf, w, h, want = _small_render(ctx, yh)
    monkeypatch.setenv("YHAIR_GATHER", "rccl")
    got = yh.gather_framebuffer([ctx])
    assert got.shape == want.shape and np.array_equal(got, want)
    got2 = yh.gather_framebuffer([ctx])  # the communicator is reused
    assert np.array_equal(got2, want)
    monkeypatch.delenv("YHAIR_GATHER")
    assert np.array_equal(yh.gather_framebuffer([ctx]), want)  # (the copy branch, for comparison)
    sf.close()


def test_torch_nccl_gather_executes_on_a_world_of_one(ctx, yh):
    """bench.py's collective path — init_process_group("nccl") = RCCL, dist.gather of the packed tiles, the
    un-interleave on the context's stream — with one rank: yhair_dist.gather_framebuffer(force_collective=True)."""
    import socket
    import torch
    import torch.distributed as dist
    import yhair_dist
    sf, w, h, want = _small_render(ctx, yh)
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        n = ctx.shard_pixels(0, 1)
        packed = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ctx.pack_tiles_device(packed.data_ptr(), n)
        image = yhair_dist.gather_framebuffer(packed, w, h, 0, 1, ctx=ctx, force_collective=True)
        torch.cuda.synchronize()
        assert np.array_equal(image.cpu().numpy(), want)
    finally:
        dist.destroy_process_group()
    sf.close()


def _bench(args, timeout=600):
    import json
    import subprocess
    env = dict(os.environ, YHAIR_SCENES=SCENES)
    env.pop("YHAIR_SHAPE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]  # rank 0 prints ONE JSON line
    return json.loads(lines[0])


def test_bench_runs_as_a_bare_command_with_two_ranks():
    """`python bench.py --gpus 2` with no launcher around it: the script starts its two ranks itself (they share
    device 0 on a one-GPU box, so the gather goes through gloo), renders the same image as one rank, and prints one line.
    The shard check and the other scaling mode are --full's; a plain run leaves out whatever the headline figure does not need."""
    common = ["--scale", "0.05", "--resolution", "96", "--steps", "2", "--warmup", "1", "--spp-per-step", "4", "--no-cpu-baseline"]
    one = _bench(["--gpus", "1"] + common)
    two = _bench(["--gpus", "2", "--full"] + common)
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2 and two["scaling"] == "strong"
    assert "projected_strong_scaling" not in one["config"] and one["roofline"]["kernel_counts_per_sample"] is None  # plain
    assert two["config"]["image_mean_rgb"] == one["config"]["image_mean_rgb"]  # pixels do not depend on the shard
    assert "weak_scaling" in two["config"] and two["value"] > 0
    # the N > 1 line carries its own parity statement: the gathered image against rank 0's render of the whole image, bitwise
    assert two["parity"]["bitwise_equal"] is True and two["parity"]["differing_pixels"] == 0 and two["parity"]["collective_ranks"] == 2
    assert two["config"]["collective_ranks"] == 2 and two["roofline"]["launches_in_timed_steps"] == two["steps"]
    forced = _bench(["--gpus", "1", "--force-collective"] + common)  # the nccl process group with one rank
    assert forced["config"]["collective"].startswith("nccl") and forced["config"]["image_mean_rgb"] == one["config"]["image_mean_rgb"]


# The kernel every full-size config settles on (round 4: ties between candidates within 5 % of the fastest are decided by a
# fixed order — k_stream, the dense quad shape, the side-by-side launch, ... — not by the noise of the last 32-sample launch)
PINNED = {"C1": 5, "C2-beta_m0.25": 3, "C3": 3, "C4": 1}


@pytest.mark.parametrize("tag,name,kw,res", [c for c in FULL_CONFIGS if c[0] in PINNED], ids=list(PINNED))
def test_kernel_choice_is_stable_on_the_baseline_configs(yh, tag, name, kw, res, monkeypatch):
    """Which kernel the timing trials settle on, three times over from a fresh context (no trial record carried
    over, neither the process's nor the one on disk: YHAIR_NO_TRIAL_CACHE): the same kernel every time, and the one
    the round's profiles were taken on."""
    monkeypatch.setenv("YHAIR_NO_TRIAL_CACHE", "1")
    monkeypatch.delenv("YHAIR_SHAPE", raising=False)
    sf = yh.SceneFile(scene_path(name, **kw))
    chosen = []
    for _ in range(3):
        c = yh.Context(0)
        c.upload_scene(sf.desc)
        c.init_state(yh.TraceParams.default(resolution=res))
        c.trace_samples(32 * 8)  # settling launch, trials (twice on a tie), then the chosen kernel
        assert not c.trials_pending()
        c.trace_samples(64)
        assert c.last_trace_ms()[1] == 1  # no trial left: one launch
        chosen.append(c.launch_shape())
        c.close()
    assert chosen == [PINNED[tag]] * 3, f"{tag}: kernels chosen {chosen}, expected {PINNED[tag]}"
    sf.close()


def test_kernel_trials_persist_on_disk(yh, tmp_path, monkeypatch):
    """The trial record of an image is kept in YHAIR_CACHE_DIR/trials_v2.txt — for callers that opted in (YHAIR_CACHE_DIR or
    yh_set_trial_cache_dir: a library call writes no file unasked) — keyed by device, build, scene, image size, shard and bounces: a second PROCESS that renders the same image runs no trial at all —
    its first request is one launch of the kernel the first process settled on — and renders the same pixels."""
    import json
    import subprocess
    code = (
        "import sys, json, hashlib; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import torch, make_scenes, yhair_capi as yh\n"
        "sf = yh.SceneFile(make_scenes.ensure_scene('straight-hair', %r, scale=0.25))\n"
        "c = yh.Context(0); c.upload_scene(sf.desc); c.init_state(yh.TraceParams.default(resolution=256))\n"
        "pending0 = c.trials_pending(); c.trace_samples(640); first = c.last_trace_ms()[1]\n"
        "c.trace_samples(64)\n"
        "print(json.dumps(dict(pending0=pending0, first_launches=first, launches=c.last_trace_ms()[1], shape=c.launch_shape(), pending=c.trials_pending(),"
        " trials={str(k): v for k, v in c.kernel_trials().items()}, md5=hashlib.md5(c.download().tobytes()).hexdigest())))\n"
    ) % (os.path.join(ROOT, "yocto-hair_amd", "python"), os.path.join(ROOT, "tools"), SCENES)
    env = dict(os.environ, YHAIR_CACHE_DIR=str(tmp_path))
    for k in ("YHAIR_SHAPE", "YHAIR_NO_TRIAL_CACHE", "YHAIR_NO_DISK_CACHE", "YHAIR_NO_TRIALS"):
        env.pop(k, None)
    runs = []
    for _ in range(2):
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        runs.append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]))
    a, b = runs
    assert os.path.exists(tmp_path / "trials_v2.txt")
    assert a["first_launches"] > 1 and not a["pending"]        # the first process ran its trials inside the first request
    assert not b["pending0"] and b["first_launches"] == 1       # the second found the record: no trial, one launch
    assert b["shape"] == a["shape"] and b["trials"] == a["trials"] and b["md5"] == a["md5"]
    # switched off: the record is neither read nor written
    env2 = dict(env, YHAIR_NO_DISK_CACHE="1", YHAIR_CACHE_DIR=str(tmp_path / "unused"))
    out = subprocess.run([sys.executable, "-c", code], env=env2, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not os.path.exists(tmp_path / "unused")
    c = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert c["first_launches"] > 1 and c["md5"] == a["md5"]
    # OPT-IN (round 5): a library caller that names no directory gets no file, wherever HOME points
    home = tmp_path / "home"
    home.mkdir()
    env3 = {k: v for k, v in env.items() if k not in ("YHAIR_CACHE_DIR", "XDG_CACHE_HOME")}
    env3["HOME"] = str(home)
    out = subprocess.run([sys.executable, "-c", code], env=env3, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["first_launches"] > 1 and d["md5"] == a["md5"] and not any(f for _, _, fs in os.walk(home) for f in fs if f.startswith("trials_"))
    # ... and yh_set_trial_cache_dir is the call that opts in (what the command lines do)
    code2 = code.replace("c = yh.Context(0)", "yh.set_trial_cache_dir(%r); c = yh.Context(0)" % str(tmp_path / "api"))
    out = subprocess.run([sys.executable, "-c", code2], env=env3, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and os.path.exists(tmp_path / "api" / "trials_v2.txt"), out.stderr[-2000:]


def test_blocking_launch_after_an_async_one_across_a_kernel_switch(ctx, yh, monkeypatch):
    """A blocking yh_trace_samples right behind yh_trace_samples_async without yh_synchronize, with a kernel switch
    in between (the hand-out list is rewritten for the new kernel): the queued launch must not see the new list."""
    sf = yh.SceneFile(scene_path("straight-hair", scale=0.05))
    ctx.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=120)
    monkeypatch.setenv("YHAIR_SHAPE", "0")
    ctx.init_state(p)
    ctx.trace_samples(40)
    want = (ctx.download(), ctx.download_rng())
    for first, second in (("0", "3"), ("3", "1"), ("1", "0")):
        monkeypatch.setenv("YHAIR_SHAPE", first)
        ctx.init_state(p)
        ctx.trace_samples_async(30)
        monkeypatch.setenv("YHAIR_SHAPE", second)  # the next launch runs another kernel: work items re-dealt
        ctx.trace_samples(10)
        ctx.synchronize()
        assert np.array_equal(ctx.download(), want[0]) and np.array_equal(ctx.download_rng(), want[1]), (first, second)
    sf.close()


def test_launch_deadline_poisons_the_context(yh, monkeypatch):
    """yh_trace_samples waits for its launch with a deadline (YHAIR_LAUNCH_TIMEOUT_S; host/deadline.h). With a
    deadline no real launch can meet, the call returns YH_E_DEVICE with a message instead of blocking, and the context refuses
    every further launch — init_state, trace, download; a fresh context is unaffected. (The wait logic itself, with an event
    that never signals, is tests/test_abi.py::test_launch_deadline_logic on the CPU.)"""
    sf = yh.SceneFile(scene_path("straight-hair", scale=0.05))
    c = yh.Context(0)
    c.upload_scene(sf.desc)
    c.init_state(yh.TraceParams.default(resolution=256))
    c.trace_samples(2)
    monkeypatch.setenv("YHAIR_LAUNCH_TIMEOUT_S", "1e-9")
    with pytest.raises(yh.YhError, match="did not complete within"):
        c.trace_samples(64)
    monkeypatch.delenv("YHAIR_LAUNCH_TIMEOUT_S")
    for call in (lambda: c.trace_samples(1), lambda: c.init_state(yh.TraceParams.default(resolution=64)), c.download, c.synchronize):
        with pytest.raises(yh.YhError, match="exceeded its deadline"):
            call()
    c.close()  # frees nothing (the device may still be running the launch), returns at once
    c2 = yh.Context(0)
    c2.upload_scene(sf.desc)
    c2.init_state(yh.TraceParams.default(resolution=64))
    c2.trace_samples(4)
    assert c2.download()[..., 3].max() > 0
    c2.close()
    sf.close()


def test_octet_kernel_is_chosen_for_a_chain_bound_shard_and_renders_the_same_pixels(yh, monkeypatch):
    """C1's geometry at 360 x 360: a few hundred expensive work items for thousands of resident waves — the launch is
    bound by the chain of one path (what one GPU of several sees of the metric's image). The octet kernel (eight
    lanes per path, 8-wide nodes) is then a trial candidate and must win (measured 0.75 x the quad kernel's time),
    with the quad kernel's bits."""
    monkeypatch.delenv("YHAIR_SHAPE", raising=False)
    monkeypatch.setenv("YHAIR_NO_TRIAL_CACHE", "1")
    sf = yh.SceneFile(scene_path("sphere-hairblock", scale=1.0))
    c = yh.Context(0)
    c.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=360)
    c.init_state(p)
    c.trace_samples(32 * 7)
    c.trace_samples(64)
    assert c.launch_shape() in (4, 6, 7, 8), c.launch_shape()  # eight or sixteen lanes per path
    got = (c.download(), c.download_rng())
    monkeypatch.setenv("YHAIR_SHAPE", "0")
    c.init_state(p)
    c.trace_samples(32 * 7 + 64)
    assert np.array_equal(c.download(), got[0]) and np.array_equal(c.download_rng(), got[1])
    c.close(), sf.close()


def test_another_shard_is_another_image_for_the_kernel_trials(yh, monkeypatch):
    """yh_set_shard with another (rank, world) makes the context plan and time its kernels afresh: a quarter of the
    image is bound by other things than the whole (bench.py's projected strong scaling renders shard 0 of N on the
    context that rendered the full image)."""
    monkeypatch.delenv("YHAIR_SHAPE", raising=False)
    monkeypatch.setenv("YHAIR_NO_TRIAL_CACHE", "1")
    sf = yh.SceneFile(scene_path("sphere-hairblock", scale=0.05, zoom=True))
    c = yh.Context(0)
    c.upload_scene(sf.desc)
    p = yh.TraceParams.default(resolution=160)
    c.init_state(p)
    c.trace_samples(200)
    assert c.kernel_trials()  # the full image has timed its candidates
    c.set_shard(0, 4)
    c.init_state(p)
    assert not c.kernel_trials()  # the shard starts over
    c.trace_samples(200)
    assert c.kernel_trials()
    c.set_shard(0, 4)  # the same shard again: its record stays
    c.init_state(p)
    assert c.kernel_trials()
    c.close(), sf.close()


@pytest.mark.parametrize("res,shard", [(720, (0, 1)), (733, (0, 1)), (1200, (1, 3))], ids=["720", "733-ragged", "1200-shard-1-of-3"])
def test_stream_shares_render_the_quad_kernels_pixels(ctx, yh, res, shard, monkeypatch):
    """Round 5: when the resident waves hold the whole image at once (C2's 720 x 720), k_stream hands every wave its OWN share of
    the work list, sized by the speed of the wave's hardware slot and corrected launch after launch from the waves' begin / end
    stamps (host/launch_plan.cpp: deal_shares_by_speed). Which wave renders which pixel must not show: four launches (the
    hand-out is re-planned after launches 1, 2 and 4, each time from the measured stamps) give the quad kernel's image and RNG
    states bit for bit — on the config's image, on a size that is not a multiple of the tile, and on a shard of it."""
    sf = yh.SceneFile(scene_path("straight-hair", scale=0.25))
    ctx.upload_scene(sf.desc)
    ctx.set_shard(*shard)
    got = {}
    for shape in ("1", "3"):
        monkeypatch.setenv("YHAIR_SHAPE", shape)
        ctx.init_state(yh.TraceParams.default(resolution=res))
        for n in (3, 2, 1, 2, 1):
            ctx.trace_samples(n)
        mid = (ctx.download(), ctx.download_rng())
        ctx.trace_samples_counted(1)  # the instrumented (quad) launch behind a shared-out k_stream list: it must get a plain list of its own
        ctx.trace_samples(2)          # ... and k_stream its shares back
        got[shape] = mid + (ctx.download(), ctx.download_rng())
    monkeypatch.delenv("YHAIR_SHAPE")
    ctx.set_shard(0, 1)
    assert got["1"][0][..., 3].max() > 0
    for k in range(4):
        assert np.array_equal(got["1"][k], got["3"][k]), k
    sf.close()


@pytest.mark.parametrize("name,kw,general", [("sphere-hairblock", dict(scale=0.05, zoom=True), False), ("lobes", dict(scale=0.05), True)],
                         ids=["sphere-hairblock", "lobes"])
def test_counted_launches_fall_back_to_a_shape_with_an_instrumented_build(ctx, yh, name, kw, general, monkeypatch):
    """The instrumented build (yh_trace_samples_counted) exists for the quad shapes and, on plain scenes only, for the octets and the
    sixteen lanes without leaf pairs / groups (csrc/yh_device.h: yhd_shapes). Under every forced YHAIR_SHAPE a counted launch runs the
    table's fallback where it has none — k_stream the quad shape the dense / sparse reading picks, the others 512 x 4 — and the next
    launch the forced shape again, on a list of its own; pixels and RNG states are the quad kernel's."""
    sf = yh.SceneFile(scene_path(name, **kw))
    ctx.upload_scene(sf.desc)
    ctx.set_shard(0, 1)
    p = yh.TraceParams.default(resolution=88)
    fallback = {"0": {0}, "1": {1}, "3": {0, 1}, "4": {4}, "5": {0}, "6": {6}, "7": {0}, "8": {0}}
    if general:
        fallback.update({s: {0} for s in "45678"})
    got = {}
    for shape in ("0", "1", "3", "4", "5", "6", "7", "8"):
        monkeypatch.setenv("YHAIR_SHAPE", shape)
        ctx.init_state(p)
        ctx.trace_samples_counted(1)
        assert ctx.launch_shape() in fallback[shape], f"forced {shape}: the counted launch ran shape {ctx.launch_shape()}"
        ctx.trace_samples(3)
        assert ctx.launch_shape() == int(shape)
        got[shape] = (ctx.download(), ctx.download_rng())
    monkeypatch.delenv("YHAIR_SHAPE")
    assert got["0"][0][..., 3].max() > 0
    for shape, (img, rng) in got.items():
        assert np.array_equal(img, got["0"][0]), f"shape {shape} renders different pixels"
        assert np.array_equal(rng, got["0"][1]), f"shape {shape} leaves different RNG states"
    sf.close()


@pytest.mark.parametrize("res", [100, 61, 7])
def test_every_launch_shape_on_ragged_image_sizes(ctx, yh, res, monkeypatch):
    """Image sizes that are not multiples of the 8x8 tile, down to less than one tile: every kernel (quads, octets with
    and without leaf pairs, sixteen lanes, side by side, k_stream) renders the quad kernel's bits on the partial tiles too."""
    sf = yh.SceneFile(scene_path("sphere-hairblock", scale=0.05, zoom=True))
    ctx.upload_scene(sf.desc)
    ctx.set_shard(0, 1)
    ref = None
    for shape in ("0", "4", "6", "7", "8", "5", "3", "1"):
        monkeypatch.setenv("YHAIR_SHAPE", shape)
        ctx.init_state(yh.TraceParams.default(resolution=res))
        ctx.trace_samples(5), ctx.trace_samples(3)
        got = (ctx.download(), ctx.download_rng())
        ref = ref or got
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), f"shape {shape} at {res} x {res}"
    monkeypatch.delenv("YHAIR_SHAPE")
    sf.close()
