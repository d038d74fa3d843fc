"""Latency of the edits that change the light list (yh_set_light_edits) against the upload they replace
(profiles/edits/light_edit_latency.txt).

    python tools/light_edit_latency.py [--scale 1.0] [--calls 10] [--grid 100]

One process, the HIP runtime warm (one untimed call of each kind first), wall-clock around the blocking calls, medians and ranges of
--calls calls. The yardstick is yh_upload_scene_maps of the same description, timed in the same process.
  sphere-hairblock at --scale, with a quad of two triangles above the hair under the `arealight` material the scene carries (no object of
      it uses that material: its light is the constant sky): the area light's material off and on (yh_update_materials, alternating), and a vertex edit of its quad
      through the four forms (yh_update_shape / _device, yh_refit_shape / _device, alternating between two stretches).
  lights-unit with its second light a grid of 2 x --grid x --grid triangles (about 20 000): the same vertex edits. The light's area cdf
      is ONE float chain in element order inside one wavefront (unit/light_list.hip): this is where that chain's cost shows, next to
      yh_triangle_cdf_gpu of the same triangles (which adds the copies of the arrays) and the host's loop (yh_triangle_cdf).
"""
import argparse
import ctypes as C
import os
import sys
import tempfile

import numpy as np
import torch  # noqa: F401  (first: torch's bundled HIP runtime must be the one libyhair.so binds to)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "yocto-hair_amd", "python"))
import make_scenes  # noqa: E402
import yhair_capi as yh  # noqa: E402
from shape_edit_latency import report, timed  # noqa: E402

F, I32 = np.float32, np.int32
STRETCH = ((1.5, 0.75), (1.25, 1.5))


QUAD = (np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0.5, 0.5, 0], [-0.5, 0.5, 0]], F), np.array([[0, 1, 2], [2, 3, 0]], I32))


def own_copy(desc, quad_light=False):
    """The description with material and shape arrays of its own (the geometry they point to is shared); quad_light: with QUAD as one
    more shape and, above the scene and facing down, one more object under the first material that emits."""
    src = desc.contents
    d = yh.SceneDesc.from_buffer_copy(src)
    materials = (yh.Material * src.num_materials)(*[yh.Material.from_buffer_copy(src.materials[i]) for i in range(src.num_materials)])
    rows = [yh.Shape.from_buffer_copy(src.shapes[i]) for i in range(src.num_shapes)]
    if quad_light:
        quad = yh.Shape()
        quad.num_vertices, quad.num_triangles, quad.positions, quad.triangles = 4, 2, yh.fptr(QUAD[0]), yh.iptr(QUAD[1])
        rows.append(quad)
        objects = [yh.Object.from_buffer_copy(src.objects[i]) for i in range(src.num_objects)] + [yh.Object()]
        objects[-1].frame[:] = [1, 0, 0, 0, 0, 1, 0, -1, 0, 0.3, 2.5, -0.3]
        objects[-1].shape = src.num_shapes
        objects[-1].material = next(i for i in range(src.num_materials) if any(src.materials[i].emission[:]))
        d.keep_objects = (yh.Object * len(objects))(*objects)
        d.objects, d.num_objects = C.cast(d.keep_objects, C.POINTER(yh.Object)), len(objects)
    shapes = (yh.Shape * len(rows))(*rows)
    d.materials, d.shapes, d.num_shapes = C.cast(materials, C.POINTER(yh.Material)), C.cast(shapes, C.POINTER(yh.Shape)), len(rows)
    return d, materials, shapes


def emitter(d):
    """(object, material row, shape) of the first object whose material emits."""
    for o in range(d.num_objects):
        if any(d.materials[d.objects[o].material].emission[:]):
            return o, d.objects[o].material, d.objects[o].shape
    raise SystemExit("the scene has no area light")


def grid(n):
    """2 n^2 triangles on (n + 1)^2 vertices in the XY plane, facing +z (tools/make_scenes.py: the grid light, finer)."""
    v = np.array([(-2 + 4 * i / n, -2 + 4 * j / n, 0.0) for j in range(n + 1) for i in range(n + 1)], F)
    t = []
    for j in range(n):
        for i in range(n):
            a, b, c, e = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i, (j + 1) * (n + 1) + i + 1
            t += [(a, b, c), (e, c, b)]
    return v, np.array(t, I32), np.tile(np.array([0, 0, 1], F), (len(v), 1))


def vertex_edits(ctx, s, shape, pos0, normals, triangles, calls):
    """The four forms on shape `s`, alternating between the two stretches of its positions."""
    keep, shapes, T = [], [], []
    for sx, sy in STRETCH:
        p = (pos0 * np.array([sx, sy, 1], F)).astype(F)
        sh = yh.Shape.from_buffer_copy(shape)
        sh.positions = yh.fptr(p)
        keep.append(p), shapes.append(sh), T.append(torch.from_numpy(p).cuda())
    t_nrm = torch.from_numpy(normals).cuda() if normals is not None else None
    t_tri = torch.from_numpy(triangles).cuda()
    report("yh_update_shape", timed(lambda k: ctx.update_shape(s, shapes[k % 2]), calls))
    report("yh_update_shape_device", timed(lambda k: ctx.update_shape_device(s, T[k % 2], normals=t_nrm, triangles=t_tri), calls))
    report("yh_refit_shape", timed(lambda k: ctx.refit_shape(s, shapes[k % 2]), calls))
    report("yh_refit_shape_device", timed(lambda k: ctx.refit_shape_device(s, T[k % 2], normals=t_nrm, triangles=t_tri), calls))


def arrays_of(sh):
    nv, nt = sh.num_vertices, sh.num_triangles
    return (np.ctypeslib.as_array(sh.positions, (nv, 3)).copy(), np.ctypeslib.as_array(sh.normals, (nv, 3)).copy() if sh.normals else None,
            np.ctypeslib.as_array(sh.triangles, (nt, 3)).copy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--grid", type=int, default=100)
    args = ap.parse_args()
    scenes = tempfile.TemporaryDirectory(prefix="yhair_latency_")
    ctx = yh.Context(0)
    ctx.set_light_edits(True)

    # ---- sphere-hairblock: a toggle of the area light, a vertex edit of its quad ----
    sf = yh.SceneFile(make_scenes.ensure_scene("sphere-hairblock", scenes.name, scale=args.scale))
    d, materials, shapes = own_copy(sf.desc, quad_light=True)
    _, row, s = emitter(d)
    segments = sum(d.shapes[i].num_lines for i in range(d.num_shapes))
    print(f"sphere-hairblock at scale {args.scale}: {segments} hair segments, {d.num_objects} objects; the light: {d.shapes[s].num_triangles} triangles", flush=True)
    report("yh_upload_scene_maps (yardstick)", timed(lambda k: ctx.upload_scene(C.pointer(d), sf.maps), args.calls))
    on, off = yh.Material.from_buffer_copy(materials[row]), yh.Material.from_buffer_copy(materials[row])
    off.emission[:] = [0, 0, 0]
    report("yh_update_materials, light off / on", timed(lambda k: ctx.update_materials(row, [off if k % 2 == 0 else on]), args.calls))
    ctx.update_materials(row, [on])
    vertex_edits(ctx, s, shapes[s], *arrays_of(shapes[s]), args.calls)
    print(f"  light list: {ctx.light_list()}", flush=True)
    sf.close()

    # ---- lights-unit with a fine grid as its second light: the cost of the cdf chain ----
    sf = yh.SceneFile(make_scenes.ensure_scene("lights-unit", scenes.name, scale=0.05, biglight=True))
    d, materials, shapes = own_copy(sf.desc)
    s = next(i for i in range(d.num_shapes) if d.shapes[i].num_triangles == 18)
    pos, tri, nrm = grid(args.grid)
    shapes[s].num_vertices, shapes[s].num_triangles = len(pos), len(tri)
    shapes[s].positions, shapes[s].normals, shapes[s].triangles = yh.fptr(pos), yh.fptr(nrm), yh.iptr(tri)
    shapes[s].texcoords = C.cast(None, yh.c_float_p)
    print(f"lights-unit, the second light a grid of {len(tri)} triangles", flush=True)
    report("yh_upload_scene_maps (yardstick)", timed(lambda k: ctx.upload_scene(C.pointer(d), sf.maps), args.calls))
    vertex_edits(ctx, s, shapes[s], pos, nrm, tri, args.calls)
    report("yh_triangle_cdf_gpu (with copies)", timed(lambda k: ctx.triangle_cdf_gpu(pos, tri), args.calls))
    report("yh_triangle_cdf (host loop)", timed(lambda k: yh.triangle_cdf(pos, tri), args.calls))
    print(f"  light list: {ctx.light_list()}", flush=True)
    sf.close()
    ctx.close()


if __name__ == "__main__":
    main()
