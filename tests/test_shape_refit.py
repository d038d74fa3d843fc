"""yh_refit_shape / yh_refit_shape_device: a vertex edit of ONE shape kept in the tree the shape has — the records written again in
their leaf slots, the boxes of the 4- / 8- / 16-wide nodes recomputed bottom-up in place (unit/refit.hip, one launch per level), no
tree built, the traversal array where it was; yh_shape_refit_growth; the unit-level yh_bvh_refit_wide / _gpu; the Python binding,
the C++ mirror's opt-in (set_shape_refit) and ysceneitraces --sway.

The yardstick stays a FRESH context that got yh_upload_scene of the edited description (tests/test_shape_edits.py): images as
uint32 with RNG states at 48 x 48, 2 spp, 256 rays of yh_intersect_batch and (plain scenes) yh_intersect_plain_batch forms 0 and 1,
256 rows of yh_lights_batch in both forms, yh_scene_once.

Two kinds of edit. Where the edited description has the reference tree of the shape's last build (the identity, `_double`, edits
of tangents or texcoords alone) EVERYTHING is the same bits (_check); the radius-only edit is held to the same, although it does
not keep the tree (test_what_the_same_tree_edits_do_to_the_reference_tree says why it can be). After a general deformation (`_sway`, the squashed
sphere) the refitted tree is another tree over the same primitives: every ray's distance is the same bits, and object, element and
uv may differ only where two primitives lie at bit-equal closest distance (_check_refit) — at most TIE_RAYS of the 256 rays and
TIE_PIXELS of the 2 304 pixels. That cap is a condition on the INPUT: the CPU half counts, for the same rays, those with two
primitives of the hit object at the bit-equal closest distance, by brute force with the oracle's intersection functions on rays
taken into the object's frame by a float32 restatement of unit/object_math.h (checked against the oracle's own closest hit, bit for
bit), and fails the choice of rays if there are more.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path
from test_scene_edits import _fresh, _same  # noqa: F401
from test_object_edits import (CROWD, FIELD, HAIRBLOCK, INSTANCE_SHAPES, _bits, _check, _compose, _differs, _fresh_results, _rays_at, _results, _rotation,
                               _translation)
from test_shape_edits import (HAIRBLOCK_BIG, RES, SIZES, SWAY_A, TEXTURED, ARGUMENT_REFUSALS, Reshaped, _argument_refusals, _chosen_sway, _description_of, _double,  # noqa: F401
                              _edited, _on_device, _prim_boxes, _refused_by_its_result, _sway, _tangents, _textured_with_the_floors_own_quad, _torch_tangents,
                              _wide_counts, refusal_baseline, scenes)

F, I32 = np.float32, np.int32
PKG = os.path.join(ROOT, "yocto-hair_amd")
WIDTHS = (4, 8, 16)
UNIT_SIZES = (1, 2, 5, 17, 300, 5000)  # 1: a root that is a leaf; the others have partly empty nodes
TIE_RAYS, TIE_PIXELS = 2, 23           # of 256 rays; 1 % of the 2 304 pixels
SWAYS = SWAY_A[:2]


# ---------------------------------------------------------------------------------------------
# the unit level: wide trees over random segment boxes
# ---------------------------------------------------------------------------------------------
def _segment_boxes(n, seed=3):
    rng = np.random.default_rng(seed + n)
    a = rng.uniform(-1, 1, (n, 3)).astype(F)
    b = (a + rng.normal(0, 0.05, (n, 3))).astype(F)
    r = rng.uniform(0.001, 0.01, (n, 1)).astype(F)
    return np.ascontiguousarray(np.concatenate([np.minimum(a, b) - r, np.maximum(a, b) + r], 1), F)


def _leaf_order(yh, boxes):
    n = len(boxes)
    nodes, prims = np.zeros((2 * n + 1, 8), F), np.zeros(n, I32)
    assert yh.load().yh_bvh_build(n, yh.fptr(boxes), yh.fptr(nodes), yh.iptr(prims)) >= 1
    return prims


def _device_form(yh, boxes, width):
    """yh_bvh_build_wide's slots as the device's collapse writes them: a child's ref is its first slot, the 4-wide form carries the
    occupied bits in bits 8-11 of the axes word (include/yhair.h: yh_bvh_build_wide_gpu)."""
    lib, n = yh.load(), len(boxes)
    count = lib.yh_bvh_build_wide(n, yh.fptr(boxes), width, None)
    slots = np.zeros((count, width, 8), F)
    assert lib.yh_bvh_build_wide(n, yh.fptr(boxes), width, yh.fptr(slots)) == count
    w = slots.view(np.uint32)
    ref = w[..., 6]
    internal = (ref != 0xFFFFFFFF) & ((ref & 0x80000000) == 0)
    ref[internal] *= width
    if width == 4:
        occupied = ((ref != 0xFFFFFFFF).astype(np.uint32) << np.arange(4, dtype=np.uint32)).sum(1, dtype=np.uint32)
        w[..., 7] = (w[..., 7] & 0xFF) | (occupied[:, None] << 8)
    return slots


def _numpy_refit(slots, leaf_boxes, width):
    """The bottom-up union, written here: a leaf slot's box from its primitives, an internal slot's from the child node's occupied
    slots. (np.minimum / np.maximum: the test boxes hold no signed zeros, so the order of a union does not matter.)"""
    out = slots.copy()
    w = out.view(np.uint32)
    for node in range(len(out) - 1, -1, -1):
        for s in range(width):
            ref = int(w[node, s, 6])
            if ref == 0xFFFFFFFF:
                continue
            if ref & 0x80000000:
                start, num = ref & 0x07FFFFFF, (ref >> 27) & 7
                b = leaf_boxes[start:start + num]
            else:
                child = out[ref // width]
                b = child[child.view(np.uint32)[:, 6] != 0xFFFFFFFF][:, :6]
            out[node, s, :3], out[node, s, 3:6] = b[:, :3].min(0), b[:, 3:6].max(0)
    return out


def _unit_case(yh, n, width):
    """boxes, leaf order, the tree over them, and the three sets of new boxes with what a refit must give for each."""
    boxes = _segment_boxes(n)
    prims = _leaf_order(yh, boxes)
    slots = _device_form(yh, boxes, width)
    moved = (boxes + np.random.default_rng(n).normal(0, 0.2, (n, 1, 3)).astype(F).repeat(2, 1).reshape(n, 6)).astype(F)
    assert np.array_equal(_leaf_order(yh, boxes * F(2)), prims), "doubling is exact: the same tree"
    return boxes, prims, slots, [("same", boxes, slots), ("doubled", boxes * F(2), _device_form(yh, boxes * F(2), width)),
                                 ("displaced", moved, _numpy_refit(slots, moved[prims], width))]


NEW_ENTRIES = ("yh_refit_shape", "yh_refit_shape_device", "yh_shape_refit_growth", "yh_bvh_refit_wide", "yh_bvh_refit_wide_gpu")


def test_library_exports_header_declares_and_binding_lists_the_entry_points(yh):
    lib = yh.load()
    header = open(os.path.join(ROOT, "include", "yhair.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libyhair.so")], capture_output=True, text=True, check=True).stdout
    for name in NEW_ENTRIES:
        assert hasattr(lib, name) and f" T {name}\n" in exported, name
        assert name in yh.EXPORTS
    for line in ("int yh_refit_shape(yh_context* ctx, int shape, const yh_shape* now);", "int yh_refit_shape_device(yh_context* ctx, int shape, const yh_shape* now);",
                 "int yh_shape_refit_growth(const yh_context* ctx, int shape, float growth[3]);",
                 "int yh_bvh_refit_wide(int n, const float* boxes, const int* primitives, int width, float* slots);",
                 "int yh_bvh_refit_wide_gpu(yh_context* ctx, int n, const float* boxes, const int* primitives, int width, float* slots);"):
        assert line in header, line
    for method in ("refit_shape", "refit_shape_device", "shape_refit_growth", "bvh_refit_wide_gpu"):
        assert callable(getattr(yh.Context, method))
    assert callable(yh.bvh_refit_wide)
    shape, growth = yh.Shape(), (C.c_float * 3)()
    # where the update answers a NULL context with YH_E_INVALID, so do these
    assert lib.yh_update_shape(None, 0, C.byref(shape)) == lib.yh_refit_shape(None, 0, C.byref(shape)) == yh.YH_E_INVALID
    assert lib.yh_update_shape_device(None, 0, None) == lib.yh_refit_shape_device(None, 0, None) == yh.YH_E_INVALID
    assert lib.yh_shape_nodes(None, 0, None, None, None) == lib.yh_shape_refit_growth(None, 0, growth) == yh.YH_E_INVALID
    boxes, prims, slots = _segment_boxes(5), np.arange(5, dtype=I32), np.zeros((1, 4, 8), F)
    assert lib.yh_bvh_refit_wide_gpu(None, 5, yh.fptr(boxes), yh.iptr(prims), 4, yh.fptr(slots)) == yh.YH_E_INVALID
    assert lib.yh_bvh_refit_wide(5, yh.fptr(boxes), yh.iptr(prims), 5, yh.fptr(slots)) == yh.YH_E_INVALID       # no such width
    assert lib.yh_bvh_refit_wide(5, yh.fptr(boxes), None, 4, yh.fptr(slots)) == yh.YH_E_INVALID


EMPTY = 0xFFFFFFFF


def _leaf(start, num):
    return 0xC0000000 | (num << 27) | start


@pytest.mark.parametrize("case", ["leaf-past-the-primitives", "leaf-without-its-tag", "child-out-of-order", "child-between-nodes", "child-past-n-nodes", "primitive-out-of-range"])
def test_host_refit_refuses_what_is_no_tree(yh, case):
    """Each refusal of yhh::wide_levels on its own: the arrays hold every node a reference can name before the check refuses (three
    nodes; `child-past-n-nodes`: n + 1), every other slot is empty, and the same arrays with the one word put right are accepted —
    so the word is the only possible reason. A refused call leaves the slots as they were."""
    lib, n = yh.load(), 5
    boxes, prims = _segment_boxes(n), np.arange(n, dtype=I32)
    nodes = 3 if case != "child-past-n-nodes" else n + 1
    slots = np.zeros((nodes, 4, 8), F)
    refs = slots.view(np.uint32)[..., 6]
    refs[...] = EMPTY
    if case == "child-past-n-nodes":  # a chain of n + 1 nodes, each the only child of the one before: more nodes than a tree over n primitives has
        for k in range(n):
            refs[k, 0] = 4 * (k + 1)
        refs[n, 0] = _leaf(0, 1)
        wrong, right = (n - 1, 0, 4 * n), _leaf(0, 1)
    else:
        refs[0, 0], refs[0, 2], refs[1, 0], refs[2, 1] = 4, 8, _leaf(0, 2), _leaf(2, 3)  # a root with two children, a leaf each
        wrong, right = {"leaf-past-the-primitives": ((2, 1, _leaf(4, 2)), _leaf(4, 1)),    # primitives 4 and 5 of 5
                        "leaf-without-its-tag": ((1, 0, _leaf(0, 2) & ~0x40000000), _leaf(0, 2)),
                        "child-out-of-order": ((0, 0, 8), 4),                              # node 2 where node 1 is due
                        "child-between-nodes": ((0, 0, 5), 4),
                        "primitive-out-of-range": (None, None)}[case]
    if wrong is None:
        prims[3] = n
    else:
        refs[wrong[:2]] = wrong[2]
    before = slots.tobytes()
    assert lib.yh_bvh_refit_wide(n, yh.fptr(boxes), yh.iptr(prims), 4, yh.fptr(slots)) == yh.YH_E_INVALID
    assert slots.tobytes() == before
    if wrong is None:
        prims[3] = 3
    else:
        refs[wrong[:2]] = right
    assert lib.yh_bvh_refit_wide(n, yh.fptr(boxes), yh.iptr(prims), 4, yh.fptr(slots)) == (n if case == "child-past-n-nodes" else 3)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n", UNIT_SIZES)
def test_host_refit_of_a_wide_tree(yh, n, width):
    boxes, prims, slots, cases = _unit_case(yh, n, width)
    words = slots.view(np.uint32)
    assert n > 1 or (len(slots) == 1 and (words[0, 0, 6] & 0xC0000000) == 0xC0000000), "n = 1: a root that is a leaf"
    assert n == 1 or (words[..., 6] == 0xFFFFFFFF).any(), "partly empty nodes"
    for name, new, want in cases:
        count, got = yh.bvh_refit_wide(new, prims, width, slots)
        assert count == len(slots), name
        assert np.array_equal(got.view(np.uint32)[..., 6:], words[..., 6:]), f"{name}: ref and axes words are not written"
        assert got.tobytes() == want.tobytes(), f"{name}: {np.count_nonzero((got.view(np.uint32) != want.view(np.uint32)).any(-1))} slots differ"
    assert cases[2][2].tobytes() != slots.tobytes(), "the displacement moved the boxes"


# ---------------------------------------------------------------------------------------------
# the CPU half of the general deformations: how many of the 256 rays meet a tie
# ---------------------------------------------------------------------------------------------
def _inverse_frame(f):
    """inverse(frame, non_rigid = true), unit/object_math.h in float32."""
    x, y, z, o = (np.asarray(f[3 * k:3 * k + 3], F) for k in range(4))

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)

    def dot(a, b):
        return F(F(a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])
    c0, c1, c2 = cross(y, z), cross(z, x), cross(x, y)
    s = F(1) / dot(x, cross(y, z))
    rx, ry, rz = np.array([c0[0], c1[0], c2[0]], F) * s, np.array([c0[1], c1[1], c2[1]], F) * s, np.array([c0[2], c1[2], c2[2]], F) * s
    ro = -(rx * o[0] + ry * o[1] + rz * o[2])
    return rx, ry, rz, ro


def _tied_rays(yh, oracle, d, shape, rays):
    """Of `rays`, those whose closest hit lies in an object that names `shape` and has a second primitive of that object at the
    bit-equal distance. The brute force's closest distance must be the oracle's own, bit for bit."""
    A = d.arrays(shape)
    osc = oracle.scene(d.ptr)
    obj, elem, _, dist = osc.intersect(rays)
    osc.close()
    lines = A["lines"] is not None
    idx = A["lines"] if lines else A["triangles"]
    P = [A["positions"][idx[:, k]] for k in range(idx.shape[1])]
    if lines:
        r = A["radius"] if A["radius"] is not None else np.full(len(A["positions"]), 0.001, F)
        R = [r[idx[:, 0]], r[idx[:, 1]]]
    tied, in_shape = [], 0
    for k in range(len(rays)):
        if elem[k] < 0 or d.objects[int(obj[k])].shape != shape:
            continue
        in_shape += 1
        rx, ry, rz, ro = _inverse_frame(d.objects[int(obj[k])].frame[:])
        o, v = rays[k, :3], rays[k, 3:6]
        local = np.concatenate([rx * o[0] + ry * o[1] + rz * o[2] + ro, rx * v[0] + ry * v[1] + rz * v[2], rays[k, 6:8]]).astype(F)
        tiled = np.ascontiguousarray(np.broadcast_to(local, (len(idx), 8)))
        hit, _, t = oracle.intersect_line(tiled, P[0], P[1], R[0], R[1]) if lines else oracle.intersect_triangle(tiled, P[0], P[1], P[2])
        t = t[hit != 0]
        assert len(t) and _bits(t.min()) == _bits(dist[k]), f"ray {k}: the brute force's closest distance is not the oracle's"
        if np.count_nonzero(_bits(t) == _bits(dist[k])) > 1:
            tied.append(k)
    return tied, in_shape


def _general_cases(yh, scenes):
    """name -> (base description, shape, edited description, plain): the general deformations of the GPU half."""
    out = {}
    for size in SIZES:
        base = Reshaped(yh, scenes(*SIZES[size]).desc)
        s = base.shape_of(True)
        for a in SWAYS:
            out[f"{size}-sway-{a}"] = (base, s, _edited(yh, scenes(*SIZES[size]).desc, s, _sway(base.arrays(s), a)), True)
    base = Reshaped(yh, scenes(*HAIRBLOCK).desc)
    s = base.shape_of(False)
    out["squash"] = (base, s, Reshaped(yh, scenes(*HAIRBLOCK).desc).set(yh, s, positions=base.arrays(s)["positions"] * np.array([1, 0.5, 1], F)), True)
    for name, scene in (("field", FIELD), ("crowd", CROWD)):
        base = Reshaped(yh, scenes(*scene).desc)
        s = base.shape_of(True)
        out[f"{name}-sway-{SWAYS[1]}"] = (base, s, _edited(yh, scenes(*scene).desc, s, _sway(base.arrays(s), SWAYS[1])), False)
    return out


GENERAL = [f"{size}-sway-{a}" for size in SIZES for a in SWAYS] + ["squash", f"field-sway-{SWAYS[1]}", f"crowd-sway-{SWAYS[1]}"]


def _rays_at_shape(d, shape, n=256, seed=11):
    """n rays from 0.2 units away through the midpoints of random elements of `shape`, in the objects that name it, object by
    object in turn: field and crowd are mostly floor and balls, and the rays of _rays_at hardly meet their hair."""
    A = d.arrays(shape)
    idx = A["lines"] if A["lines"] is not None else A["triangles"]
    rng = np.random.default_rng(seed)
    mid = A["positions"][idx[rng.integers(0, len(idx), n)]].astype(np.float64).mean(1)
    named = [o for o in range(d.n) if d.objects[o].shape == shape]
    f = np.array([d.objects[named[k % len(named)]].frame[:] for k in range(n)], np.float64).reshape(n, 4, 3)
    target = (f[:, :3] * mid[:, :, None]).sum(1) + f[:, 3]
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    o = target - 0.2 * v  # (from close by, in any direction: in `field` the floor hides most tufts from the camera)
    return np.concatenate([o, v, np.full((n, 1), 1e-4), np.full((n, 1), 3.4e38)], axis=1).astype(F)


INSTANCED = ("field", "crowd")  # the cases whose GPU half also traces _rays_at_shape
AIMED_FLOOR = 64                # of those 256 rays, how many must end in the edited shape


@pytest.mark.parametrize("case", GENERAL)
def test_the_rays_of_the_general_cases_meet_few_ties(yh, oracle, scenes, case):
    """The cap of the GPU half is a condition on its rays: at most TIE_RAYS of them may have two primitives at the closest distance,
    and enough of them must end in the edited shape for the comparison to say something about the refitted tree."""
    base, s, new, _ = _general_cases(yh, scenes)[case]
    tied, in_shape = _tied_rays(yh, oracle, new, s, _rays_at(new.d))
    print(f"{case}: {in_shape} of 256 rays end in the edited shape, {len(tied)} of them at a tie {tied}")
    assert len(tied) <= TIE_RAYS, "choose other rays: this is the input's fault, not the kernel's"
    if not case.startswith(INSTANCED):
        assert in_shape >= 16, "the rays do not meet the edited shape"
        return
    tied, in_shape = _tied_rays(yh, oracle, new, s, _rays_at_shape(new, s))
    print(f"{case}: {in_shape} of the 256 rays aimed at the hair end in it, {len(tied)} of them at a tie {tied}")
    assert in_shape >= AIMED_FLOOR, "the aimed rays do not meet the edited shape"
    assert len(tied) <= TIE_RAYS, "choose other rays: this is the input's fault, not the kernel's"


# ---------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------
def _check_refit(got, want, what):
    """The contract after a general deformation: distances the same bits; object, element or uv differ only at a bit-equal distance,
    on at most TIE_RAYS rays; pixels (with their RNG states) differ on at most TIE_PIXELS; lights and scene_once the same bits."""
    batches = [("yh_intersect_batch", got["hits"], want["hits"])]
    if "plain" in want:
        batches += [(f"yh_intersect_plain_batch form {form}", got["plain"][form], want["plain"][form]) for form in (0, 1)]
    for name, a, b in batches:
        assert np.array_equal(_bits(a[3]), _bits(b[3])), f"{what}: {name}: {np.count_nonzero(_bits(a[3]) != _bits(b[3]))} distances differ from a fresh upload's"
        other = (a[0] != b[0]) | (a[1] != b[1]) | (_bits(a[2]) != _bits(b[2])).any(1)
        print(f"{what}: {name}: {np.count_nonzero(other)} of {len(other)} rays differ in object, element or uv at a bit-equal distance")
        assert np.count_nonzero(other) <= TIE_RAYS, f"{what}: {name}"
    (img, rng), (wimg, wrng) = got["image"], want["image"]
    assert wimg[..., 3].max() > 0 and img.shape == wimg.shape
    pixels = (img.view(np.uint32) != wimg.view(np.uint32)).any(-1).reshape(-1) | (rng != wrng).any(-1).reshape(-1)
    print(f"{what}: {np.count_nonzero(pixels)} of {pixels.size} pixels differ from a fresh upload's (0 expected)")
    assert np.count_nonzero(pixels) <= TIE_PIXELS, what
    for form in (0, 1):
        assert np.array_equal(_bits(got["lights"][form]), _bits(want["lights"][form])), f"{what}: yh_lights_batch form {form} differs from a fresh upload's"
    assert got["once"] == want["once"], what


_AIMED = {}


def _check_aimed(ctx, yh, key, new, s, exact, what):
    """Closest hits of the rays aimed at the edited shape (field, crowd) against a fresh upload's, once per description: the same
    bits (`exact`), or the rule of _check_refit."""
    rays = _rays_at_shape(new, s)
    if key not in _AIMED:
        forced = os.environ.pop("YHAIR_SHAPE", None)  # (the yardstick under the host's own choice, as _fresh_results takes it)
        fresh = yh.Context(0)
        try:
            fresh.upload_scene(new.ptr)
            _AIMED[key] = fresh.intersect(rays)
        finally:
            fresh.close()
            if forced is not None:
                os.environ["YHAIR_SHAPE"] = forced
    a, b = ctx.intersect(rays), _AIMED[key]
    in_shape = sum(1 for k in range(len(rays)) if b[1][k] >= 0 and new.objects[int(b[0][k])].shape == s)
    other = (a[0] != b[0]) | (a[1] != b[1]) | (_bits(a[2]) != _bits(b[2])).any(1)
    print(f"{what}: {in_shape} of {len(rays)} aimed rays end in the edited shape; {np.count_nonzero(other)} differ in object, element or uv")
    assert in_shape >= AIMED_FLOOR, what
    assert np.array_equal(_bits(a[3]), _bits(b[3])), f"{what}: {np.count_nonzero(_bits(a[3]) != _bits(b[3]))} distances of the aimed rays differ from a fresh upload's"
    assert np.count_nonzero(other) <= (0 if exact else TIE_RAYS), what


# ---- 1. the kernel against the host's restatement ----
@pytest.mark.gpu
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n", UNIT_SIZES + (40000,))
def test_device_refit_of_a_wide_tree_is_the_hosts(ctx, yh, n, width):
    """Slot for slot; 40 000 primitives: every level but the top ones has more than one workgroup of 128 nodes."""
    boxes, prims, slots, cases = _unit_case(yh, n, width) if n <= 5000 else (None,) * 4
    if cases is None:
        boxes = _segment_boxes(n)
        prims, slots = _leaf_order(yh, boxes), _device_form(yh, boxes, width)
        moved = (boxes + np.random.default_rng(n).normal(0, 0.2, (n, 1, 3)).astype(F).repeat(2, 1).reshape(n, 6)).astype(F)
        cases = [("same", boxes, slots), ("displaced", moved, None)]
    built_n, built = ctx.lib.yh_bvh_build_wide_gpu(ctx.h, n, yh.fptr(boxes), width, None), np.zeros_like(slots)
    assert built_n == len(slots) and ctx.lib.yh_bvh_build_wide_gpu(ctx.h, n, yh.fptr(boxes), width, yh.fptr(built)) == built_n
    assert built.tobytes() == slots.tobytes(), "the device form the host tests restate"
    for name, new, want in cases:
        hc, host = yh.bvh_refit_wide(new, prims, width, slots)
        dc, dev = ctx.bvh_refit_wide_gpu(new, prims, width, slots)
        assert hc == dc == len(slots), name
        assert dev.tobytes() == host.tobytes(), f"{name}: {np.count_nonzero((dev.view(np.uint32) != host.view(np.uint32)).any(-1))} slots differ from the host's"
        assert want is None or dev.tobytes() == want.tobytes(), name


# ---- 2. edits whose refit is a fresh upload bit for bit (the first function and the CPU test need no GPU) ----
def _same_tree_edit(A, edit):
    if edit == "identity":
        return dict(A)
    if edit == "double":
        return _double(A)
    if edit == "tangents":
        return dict(A, normals=np.ascontiguousarray(A["normals"][:, [1, 2, 0]] * F(-1)))
    assert edit == "radius"
    return dict(A, radius=A["radius"] * F(0.75))


def test_what_the_same_tree_edits_do_to_the_reference_tree(yh, oracle, scenes):
    """`double` and `tangents` keep the reference's tree of the hair. A radius edit does NOT, on either size (a centre is the mean of
    rounded sums, and among tens of thousands of segments one crosses a split whatever the factor): its refit is bit for bit a fresh
    upload's only because none of the 256 rays meets a tie — counted here, cap 0 — and as long as no path of the image does."""
    for size in SIZES:
        base = Reshaped(yh, scenes(*SIZES[size]).desc)
        s = base.shape_of(True)
        A = base.arrays(s)
        order = _leaf_order(yh, _prim_boxes(A))
        for edit in ("double", "tangents"):
            assert np.array_equal(_leaf_order(yh, _prim_boxes(_same_tree_edit(A, edit))), order) and _wide_counts(yh, _same_tree_edit(A, edit)) == _wide_counts(yh, A), edit
        new = _edited(yh, scenes(*SIZES[size]).desc, s, _same_tree_edit(A, "radius"))
        kept = np.array_equal(_leaf_order(yh, _prim_boxes(new.arrays(s))), order)
        tied, in_shape = _tied_rays(yh, oracle, new, s, _rays_at(new.d))
        print(f"{size}: the radius edit keeps the leaf order: {kept}; {in_shape} of 256 rays end in the hair, {len(tied)} at a tie")
        assert in_shape >= 16 and not tied, "choose other rays: this is the input's fault, not the kernel's"


@pytest.mark.gpu
@pytest.mark.parametrize("edit", ["identity", "double", "tangents", "radius"])
@pytest.mark.parametrize("size", list(SIZES))
def test_refit_that_keeps_the_tree_renders_the_bits_of_a_fresh_upload(ctx, yh, scenes, size, edit):
    sf = scenes(*SIZES[size])
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    A = base.arrays(s)
    E = _same_tree_edit(A, edit)
    new = _edited(yh, sf.desc, s, E)
    ctx.upload_scene(base.ptr)
    nodes = ctx.shape_nodes(s)
    assert ctx.shape_refit_growth(s) == [1.0, 1.0, 1.0]
    ctx.refit_shape(s, new.shapes[s])
    assert ctx.shape_nodes(s) == nodes, "a refit never moves or grows anything"
    growth = ctx.shape_refit_growth(s)
    print(f"{size} {edit}: growth {growth}")
    assert (growth == [1.0, 1.0, 1.0]) == (edit in ("identity", "tangents")), "exactly 1.0 only where the boxes are reproduced"
    key = {"identity": f"shape-{size}-base", "double": f"shape-{size}-double"}.get(edit, f"refit-{size}-{edit}")
    got = _results(ctx, yh, new.d, True)
    _check(got, _fresh_results(yh, key, new.d, True), f"{size} {edit}")
    if edit != "identity":
        assert _differs(got, _fresh_results(yh, f"shape-{size}-base", base.d, True)), "the edit changed nothing"


@pytest.mark.gpu
def test_refit_doubles_with_a_radius_where_the_upload_had_none(ctx, yh, scenes):
    sf = scenes(*HAIRBLOCK)
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    base.set(yh, s, radius=None)
    A = base.arrays(s)
    assert A["radius"] is None
    new = Reshaped(yh, sf.desc).set(yh, s, **{k: v for k, v in _double(A).items() if v is not None})
    ctx.upload_scene(base.ptr)
    nodes = ctx.shape_nodes(s)
    ctx.refit_shape(s, new.shapes[s])
    assert ctx.shape_nodes(s) == nodes and ctx.shape_refit_growth(s) != [1.0, 1.0, 1.0]
    _check(_results(ctx, yh, new.d, True), _fresh_results(yh, "shape-noradius-double", new.d, True), "radius 0.001 -> 0.002")


@pytest.mark.gpu
def test_refit_with_other_texcoords_on_textureds_quad(ctx, yh, scenes):
    """The triangle case: two units per test record, per-vertex rows."""
    sf = scenes(*TEXTURED)
    base, own = _textured_with_the_floors_own_quad(yh, sf)
    new, _ = _textured_with_the_floors_own_quad(yh, sf)
    uv = base.arrays(own)["texcoords"]
    new.set(yh, own, texcoords=(uv * F(0.5) + F(0.25))[:, ::-1])
    ctx.upload_scene(base.ptr)
    before, nodes = _results(ctx, yh, base.d, False), ctx.shape_nodes(own)
    ctx.refit_shape(own, new.shapes[own])
    assert ctx.shape_nodes(own) == nodes and ctx.shape_refit_growth(own) == [1.0, 1.0, 1.0]
    got = _results(ctx, yh, new.d, False)
    _check(got, _fresh_results(yh, "shape-textured-uv", new.d), "texcoords")
    assert _differs(got, before), "the edit changed nothing"


# ---- 3. general deformations: another tree over the same primitives ----
@pytest.mark.gpu
@pytest.mark.parametrize("case", GENERAL[:-1])
def test_refit_after_a_deformation_hits_what_a_fresh_upload_hits(ctx, yh, scenes, case):
    base, s, new, plain = _general_cases(yh, scenes)[case]
    if case.startswith("field"):
        assert sum(base.objects[o].shape == s for o in range(base.n)) == 256
    ctx.upload_scene(base.ptr)
    nodes, before = ctx.shape_nodes(s), _results(ctx, yh, base.d, plain)
    ctx.refit_shape(s, new.shapes[s])
    assert ctx.shape_nodes(s) == nodes
    growth = ctx.shape_refit_growth(s)
    print(f"{case}: growth {growth}")
    got, want = _results(ctx, yh, new.d, plain), _fresh_results(yh, "refit-" + case, new.d, plain)
    _check_refit(got, want, case)
    if case.startswith(INSTANCED):
        _check_aimed(ctx, yh, "refit-" + case, new, s, False, case)
    assert _differs(got, before), "the edit changed nothing"
    ctx.update_shape(s, new.shapes[s])  # the same arrays through the build: the reference's tree again
    assert ctx.shape_refit_growth(s) == [1.0, 1.0, 1.0]
    _check(_results(ctx, yh, new.d, plain), want, case + ", then yh_update_shape")


# ---- 4. crowd under every launch shape ----
@pytest.mark.gpu
@pytest.mark.parametrize("edit", ["double", "sway"])
@pytest.mark.parametrize("shape", INSTANCE_SHAPES)
def test_crowd_hair_is_refitted_under_every_launch_shape(ctx, yh, scenes, shape, edit, monkeypatch):
    sf = scenes(*CROWD)
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    new = _edited(yh, sf.desc, s, _double(base.arrays(s))) if edit == "double" else _general_cases(yh, scenes)[GENERAL[-1]][2]
    monkeypatch.setenv("YHAIR_SHAPE", shape)
    ctx.upload_scene(base.ptr)
    nodes = ctx.shape_nodes(s)
    ctx.refit_shape(s, new.shapes[s])
    assert ctx.shape_nodes(s) == nodes
    got = _results(ctx, yh, new.d, False)
    assert ctx.launch_shape() == int(shape)
    if edit == "double":
        _check(got, _fresh_results(yh, "refit-crowd-double", new.d), f"crowd double, shape {shape}")
    else:
        _check_refit(got, _fresh_results(yh, "refit-" + GENERAL[-1], new.d), f"crowd sway, shape {shape}")
    _check_aimed(ctx, yh, "refit-crowd-" + edit, new, s, edit == "double", f"crowd {edit}, shape {shape}")


# ---- 5. the device form ----
@pytest.mark.gpu
@pytest.mark.parametrize("edit", ["double", "sway"])
@pytest.mark.parametrize("size", list(SIZES))
def test_device_form_refits_from_torch_tensors(ctx, yh, scenes, size, edit):
    import torch
    sf = scenes(*SIZES[size])
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    T = _on_device(base.arrays(s))
    ctx.upload_scene(base.ptr)
    nodes = ctx.shape_nodes(s)
    if edit == "double":
        T = dict(T, positions=T["positions"] * 2, radius=T["radius"] * 2)
    else:
        p = T["positions"].clone()
        p[:, 0] += SWAYS[1] * p[:, 1] * p[:, 1]
        T = dict(T, positions=p, normals=_torch_tangents(p, T["lines"]))
    ctx.refit_shape_device(s, T["positions"], normals=T["normals"], radius=T["radius"], lines=T["lines"])
    torch.cuda.synchronize()
    new = _description_of(yh, sf.desc, s, T)
    assert ctx.shape_nodes(s) == nodes
    got, want = _results(ctx, yh, new.d, True), _fresh_results(yh, f"refit-{size}-{edit}-torch", new.d, True)
    (_check if edit == "double" else _check_refit)(got, want, f"device form, {size} {edit}")
    assert _differs(got, _fresh_results(yh, f"shape-{size}-base", base.d, True)), "the edit changed nothing"


@pytest.mark.gpu
def test_device_form_refits_the_squashed_sphere(ctx, yh, scenes):
    """A triangle shape with texcoords and no radius: the per-vertex rows are written from the caller's device arrays."""
    import torch
    sf = scenes(*HAIRBLOCK)
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(False)
    T = _on_device(base.arrays(s))
    T = dict(T, positions=(T["positions"] * torch.tensor([1, 0.5, 1], device="cuda")).contiguous(), texcoords=T["texcoords"].flip(1).contiguous())
    ctx.upload_scene(base.ptr)
    nodes = ctx.shape_nodes(s)
    ctx.refit_shape_device(s, T["positions"], normals=T["normals"], triangles=T["triangles"], texcoords=T["texcoords"])
    new = _description_of(yh, sf.desc, s, T)
    assert ctx.shape_nodes(s) == nodes
    got = _results(ctx, yh, new.d, True)
    _check_refit(got, _fresh_results(yh, "shape-squash-torch", new.d, True), "device form, squash")
    assert _differs(got, _fresh_results(yh, "shape-host-built-base", base.d, True)), "the edit changed nothing"
    with pytest.raises(yh.YhError, match="positions"):
        ctx.refit_shape_device(s, None, triangles=T["triangles"])


# ---- 6. growth ----
@pytest.mark.gpu
def test_growth_is_above_one_after_a_sway_deterministic_and_the_same_in_both_forms(ctx, yh, scenes):
    sf = scenes(*HAIRBLOCK_BIG)
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    A = base.arrays(s)
    small, large = (_edited(yh, sf.desc, s, _sway(A, a)) for a in SWAYS)
    seen = []
    for run in range(2):
        ctx.upload_scene(base.ptr)
        ctx.refit_shape(s, small.shapes[s])
        g_small = ctx.shape_refit_growth(s)
        ctx.refit_shape(s, large.shapes[s])
        seen.append((g_small, ctx.shape_refit_growth(s)))
    print(f"growth after a = {SWAYS[0]}: {seen[0][0]}, after a = {SWAYS[1]}: {seen[0][1]}")
    assert seen[0] == seen[1], "the same sums from run to run"
    assert all(g > 1.0 for g in seen[0][1]), "the larger sway grows the boxes of all three widths"
    T = _on_device(large.arrays(s))
    ctx.upload_scene(base.ptr)
    ctx.refit_shape_device(s, T["positions"], normals=T["normals"], radius=T["radius"], lines=T["lines"])
    assert ctx.shape_refit_growth(s) == seen[0][1], "host form and device form"
    ctx.update_shape(s, large.shapes[s])
    assert ctx.shape_refit_growth(s) == [1.0, 1.0, 1.0], "a build is the new yardstick"


# ---- 7. interplay ----
@pytest.mark.gpu
def test_refit_then_object_and_camera_edits(ctx, yh, scenes):
    sf = scenes(*HAIRBLOCK)
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    final = _edited(yh, sf.desc, s, _sway(base.arrays(s), SWAYS[1]))
    hair = final.index(lines=True)[0]
    final.objects[hair].frame[:] = _compose(_translation(-0.3, 0.2, 0.25), _compose(final.objects[hair].frame[:], _rotation((1, 1, 0.3), 30)))
    final.camera.aperture, final.camera.focus = 0.1, 4.0
    ctx.upload_scene(base.ptr)
    ctx.refit_shape(s, final.shapes[s])
    ctx.update_objects(hair, final.rows(yh, hair, 1))
    ctx.update_camera(final.camera)
    _check_refit(_results(ctx, yh, final.d, True), _fresh_results(yh, "refit-interplay", final.d, True), "refit, objects, camera")


@pytest.mark.gpu
def test_refit_of_a_shape_that_lives_in_appended_room(ctx, yh, scenes):
    sf = scenes(*HAIRBLOCK)
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    A = base.arrays(s)
    a = _chosen_sway(yh, "host-built", A)[0]
    swy = _edited(yh, sf.desc, s, _sway(A, a))
    dbl = _edited(yh, sf.desc, s, _double(_sway(A, a)))
    ctx.upload_scene(base.ptr)
    off0 = ctx.shape_nodes(s)[0]
    ctx.update_shape(s, swy.shapes[s])
    nodes = ctx.shape_nodes(s)
    assert nodes[0] != off0, "the update appended a width"
    ctx.refit_shape(s, dbl.shapes[s])
    assert ctx.shape_nodes(s) == nodes
    _check(_results(ctx, yh, dbl.d, True), _fresh_results(yh, "refit-appended-double", dbl.d, True), "double in appended room")


# ---- 8. refusals: those of yh_update_shape that apply ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", ARGUMENT_REFUSALS)
def test_refused_arguments_leave_the_context_rendering(ctx, yh, scenes, refusal_baseline, name):
    calls, _keep = _argument_refusals(yh, scenes(*HAIRBLOCK))
    index, shape = calls[name]
    ctx.upload_scene(scenes(*HAIRBLOCK).desc)
    ctx.set_shard(0, 1)
    ctx.init_state(yh.TraceParams.default(resolution=RES))
    ctx.trace_samples(2)
    assert ctx.lib.yh_refit_shape(ctx.h, index, C.byref(shape) if shape is not None else None) == yh.YH_E_INVALID, name
    assert ctx.lib.yh_last_error(ctx.h).decode().startswith("yh_refit_shape:"), ctx.lib.yh_last_error(ctx.h)
    ctx.trace_samples(2)  # the image state is still there, and the scene is the earlier one
    _same((ctx.download(), ctx.download_rng()), refusal_baseline, name)
    assert ctx.scene_once() == refusal_baseline[2]
    assert ctx.shape_refit_growth(0) == [1.0, 1.0, 1.0]


@pytest.mark.gpu
def test_an_out_of_range_index_is_refused_in_the_device_form(ctx, yh, scenes):
    import torch
    base = Reshaped(yh, scenes(*HAIRBLOCK).desc)
    s = base.shape_of(True)
    T = _on_device(base.arrays(s))
    T["lines"][7, 0] = base.shapes[s].num_vertices
    torch.cuda.synchronize()
    _refused_by_its_result(ctx, yh, base, lambda: ctx.refit_shape_device(s, T["positions"], normals=T["normals"], radius=T["radius"], lines=T["lines"]),
                           "yh_refit_shape_device", ["vertex index out of range"])


@pytest.mark.gpu
def test_normals_where_the_upload_had_none_are_refused(ctx, yh, scenes):
    sf = scenes(*HAIRBLOCK)
    base = Reshaped(yh, sf.desc)
    s = base.shape_of(True)
    base.set(yh, s, normals=None)
    with_normals = Reshaped(yh, sf.desc)
    _refused_by_its_result(ctx, yh, base, lambda: ctx.refit_shape(s, with_normals.shapes[s]), "yh_refit_shape", ["normals"])


@pytest.mark.gpu
def test_the_shape_of_an_emitter_is_refused(ctx, yh, scenes):
    sf = scenes(*CROWD)
    base = Reshaped(yh, sf.desc)
    light = base.index(emissive=True)[0]
    s = base.objects[light].shape
    new = Reshaped(yh, sf.desc).set(yh, s, positions=base.arrays(s)["positions"] * F(1.5))
    _refused_by_its_result(ctx, yh, base, lambda: ctx.refit_shape(s, new.shapes[s]), "yh_refit_shape", ["emits"])


@pytest.mark.gpu
def test_call_order(yh, scenes):
    base = Reshaped(yh, scenes(*HAIRBLOCK).desc)
    s = base.shape_of(True)
    c = yh.Context(0)
    growth = (C.c_float * 3)()
    assert c.lib.yh_refit_shape(c.h, s, C.byref(base.shapes[s])) == yh.YH_E_STATE  # before an upload
    assert c.lib.yh_refit_shape_device(c.h, s, C.byref(base.shapes[s])) == yh.YH_E_STATE
    assert c.lib.yh_shape_refit_growth(c.h, s, growth) == yh.YH_E_STATE
    c.upload_scene(base.ptr)
    c.init_state(yh.TraceParams.default(resolution=RES))
    c.trace_samples(1)
    c.refit_shape(s, base.shapes[s])  # (an edit that changes no value is an edit all the same)
    assert c.lib.yh_trace_samples(c.h, 1) == yh.YH_E_STATE
    c.init_state(yh.TraceParams.default(resolution=RES))
    c.trace_samples(1)
    c.close()


# ---- 9. the mirror and the command line ----
def _compile_mirror_test(tmp_path):
    exe = str(tmp_path / "mirror_shape_refit")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "host"), "-Wno-class-memaccess", os.path.join(ROOT, "tests", "cpp", "test_mirror_shape_refit.cpp"),
                           "-o", exe, "-L" + PKG, "-lyhair", "-Wl,-rpath," + PKG, "-lpthread"])
    return exe


def test_mirror_keeps_its_classification_with_the_refit_opt_in(built, tmp_path):
    """set_shape_refit changes which call a vertex edit becomes, never how an edit is classified: checked by the C++ program."""
    exe = _compile_mirror_test(tmp_path)
    r = subprocess.run([exe, "--classify"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


@pytest.mark.gpu
def test_mirror_passes_vertex_edits_on_as_refits_with_both_opt_ins(built, tmp_path):
    """set_positions on the hair after an init_state: with set_shape_edits and set_shape_refit the growth is no longer 1, with
    set_shape_edits alone it is 1 (a build), with set_shape_refit alone a second upload."""
    exe = _compile_mirror_test(tmp_path)
    r = subprocess.run([exe, scene_path(*HAIRBLOCK[:1], **HAIRBLOCK[1])], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("refit", [True, False])
def test_ysceneitraces_sways(built, tmp_path, refit):
    out = str(tmp_path / "sway.hdr")
    cmd = [os.path.join(PKG, "ysceneitraces"), scene_path(*HAIRBLOCK[:1], **HAIRBLOCK[1]), "--resolution", "64", "--samples", "2", "--sway", "2", "-o", out]
    r = subprocess.run(cmd + (["--sway-refit"] if refit else []), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    steps = [line for line in r.stdout.splitlines() if line.startswith("sway step")]
    print(r.stdout)
    assert len(steps) == 2 and all("edit to preview" in s and (" refit" in s) == refit for s in steps), r.stdout
