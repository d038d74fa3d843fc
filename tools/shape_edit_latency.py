"""Latency of a vertex edit of the hair against a whole upload (profiles/edits/shape_edit_latency.txt).

    python tools/shape_edit_latency.py [--scene sphere-hairblock] [--scale 1.0] [--calls 10] [--upload-only]

One process, the HIP runtime warm (one untimed call of each kind first), wall-clock around the blocking calls. The edit is the
tests' `sway` (x += a * y^2, tangents recomputed) of the scene's hair shape, with the first a of --sway that makes a width outgrow its room:
    upload            yh_upload_scene of the edited description
    edit, growing     yh_update_shape on a freshly uploaded scene (the upload is not timed): widths that outgrow their room are appended
    edit, in place    yh_update_shape alternating between the swayed and the loaded arrays once the room is there
    device, growing / in place    the same through yh_update_shape_device, the arrays being torch tensors on the GPU
--upload-only measures the first line alone (an older build of the library, named by YHAIR_LIB, has no more than that).
"""
import argparse
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np
import torch  # noqa: F401  (first: torch's bundled HIP runtime must be the one libyhair.so binds to)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "yocto-hair_amd", "python"))
import make_scenes  # noqa: E402
import yhair_capi as yh  # noqa: E402

F = np.float32


def tangents(p, lines):
    d = p[lines[:, 1]] - p[lines[:, 0]]
    t = np.zeros_like(p)
    np.add.at(t, lines[:, 0], d), np.add.at(t, lines[:, 1], d)
    return (t / np.maximum(np.linalg.norm(t, axis=1, keepdims=True), F(1e-20))).astype(F)


def timed(fn, calls, before=None):
    out = []
    for k in range(calls + 1):  # (the first call warms up and is dropped)
        if before:
            before(k)
        t0 = time.perf_counter()
        fn(k)
        out.append((time.perf_counter() - t0) * 1e3)
    return out[1:]


def report(what, ms):
    print(f"  {what:<34s} median {np.median(ms):9.2f} ms   range {min(ms):9.2f} .. {max(ms):9.2f} ms   ({len(ms)} calls)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sphere-hairblock")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--sway", type=float, nargs="+", default=[0.05, 0.1, 0.2, 0.4, 0.8], help="x += a * y^2: the first a that grows a node count is measured")
    ap.add_argument("--upload-only", action="store_true")
    args = ap.parse_args()
    scenes = tempfile.TemporaryDirectory(prefix="yhair_latency_")
    sf = yh.SceneFile(make_scenes.ensure_scene(args.scene, scenes.name, scale=args.scale))
    src = sf.desc.contents
    hair = next(i for i in range(src.num_shapes) if src.shapes[i].num_lines > 0)
    sh = src.shapes[hair]
    nv, nl = sh.num_vertices, sh.num_lines
    pos0 = np.ctypeslib.as_array(sh.positions, (nv, 3)).copy()
    nrm0 = np.ctypeslib.as_array(sh.normals, (nv, 3)).copy()
    lines = np.ctypeslib.as_array(sh.lines, (nl, 2)).copy()

    def swayed_by(a):
        p = pos0.copy()
        p[:, 0] += F(a) * p[:, 1] * p[:, 1]
        return p, tangents(p, lines)

    def edited_by(a):
        """(the swayed shape, the description with it, the arrays they point into)"""
        p, n = swayed_by(a)
        shape = yh.Shape.from_buffer_copy(sh)
        shape.positions, shape.normals = yh.fptr(p), yh.fptr(n)
        shapes = (yh.Shape * src.num_shapes)(*[yh.Shape.from_buffer_copy(src.shapes[i]) for i in range(src.num_shapes)])
        shapes[hair] = shape
        desc = yh.SceneDesc.from_buffer_copy(src)
        desc.shapes = C.cast(shapes, C.POINTER(yh.Shape))
        return shape, desc, (p, n, shapes)

    loaded = yh.Shape.from_buffer_copy(sh)
    swayed, edited, keep = edited_by(args.sway[0])
    print(f"{args.scene} at scale {args.scale}: {nl} segments in the edited shape, {src.num_shapes} shapes, {src.num_objects} objects, {src.num_textures} textures; "
          f"library {os.path.relpath(yh.LIB_PATH, ROOT)}", flush=True)
    ctx = yh.Context(0)
    report("upload of the edited description", timed(lambda k: ctx.upload_scene(C.pointer(edited)), args.calls))
    if args.upload_only:
        return
    # the first sway of the list under which one of the three node counts outgrows its room
    for a in args.sway:
        swayed, edited, keep = edited_by(a)
        ctx.upload_scene(sf.desc)
        off0, cnt0, _ = ctx.shape_nodes(hair)
        ctx.update_shape(hair, swayed)
        off1, cnt1, room1 = ctx.shape_nodes(hair)
        grown = [w for w, o0, o1 in zip((4, 8, 16), off0, off1) if o0 != o1]
        print(f"  sway a = {a}: wide nodes {cnt0} -> {cnt1}; widths appended: {grown}", flush=True)
        if grown:
            break
    else:
        raise SystemExit("no sway of the list grows a node count: the growing case is not measured")
    pos1, nrm1 = keep[0], keep[1]
    report("edit, growing", timed(lambda k: ctx.update_shape(hair, swayed), args.calls, before=lambda k: ctx.upload_scene(sf.desc)))
    report("edit, in place", timed(lambda k: ctx.update_shape(hair, loaded if k % 2 == 0 else swayed), args.calls))
    assert ctx.shape_nodes(hair)[0] == off1, "the alternating edits were to stay in place"
    T = {k: torch.from_numpy(v).cuda() for k, v in dict(pos0=pos0, nrm0=nrm0, pos1=pos1, nrm1=nrm1, lines=lines).items()}
    radius = torch.from_numpy(np.ctypeslib.as_array(sh.radius, (nv,)).copy()).cuda() if sh.radius else None

    def device_edit(which):
        ctx.update_shape_device(hair, T["pos" + which], normals=T["nrm" + which], radius=radius, lines=T["lines"])
    report("device form, growing", timed(lambda k: device_edit("1"), args.calls, before=lambda k: ctx.upload_scene(sf.desc)))
    report("device form, in place", timed(lambda k: device_edit("0" if k % 2 == 0 else "1"), args.calls))
    ctx.close()


if __name__ == "__main__":
    main()
