"""What yh_upload_scene lays out, as a caller can read it: where every shape's wide nodes sit in the traversal array (yh_shape_nodes), the
light list (yh_light_list), and the two forms the scene table settles on (yh_scene_once, yh_lights_const_env), for a handful of small
scenes. tests/test_upload_layout.py holds an upload to the file this writes, exactly: a change of the layout has to be made on purpose.

    python tools/upload_layout.py --commit <hash> [--out tests/golden/upload_layout.json]

writes the file from the library in place (YHAIR_LIB names another build); needs the GPU. --commit is recorded in the file's header.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "yocto-hair_amd", "python"))
import make_instance_goldens as mig  # noqa: E402
import make_scenes  # noqa: E402

# (name in the file, scene, its options, uploaded with its maps)
SCENES = [
    ("sphere-hairblock", "sphere-hairblock", dict(scale=0.02), False),
    ("lights-unit", "lights-unit", dict(scale=0.05, biglight=True), False),
    ("fur-field", mig.SCENE, mig.SCENE_KW, False),  # 339 objects: the scene level is walked as wide nodes
    ("hits-unit", "hits-unit", dict(variant="four"), False),
    ("maps", "maps", dict(), True),  # textures and maps (tests/test_material_maps.py)
]
GOLDEN = os.path.join(ROOT, "tests", "golden", "upload_layout.json")


def layout(ctx, yh, path, with_maps):
    """Uploads the scene at `path` and returns what the four entry points say, as json-ready lists."""
    sf = yh.SceneFile(path)
    ctx.upload_scene(sf.desc, sf.maps if with_maps else None)
    out = {
        "yh_shape_nodes": [dict(zip(("offset", "count", "room"), ctx.shape_nodes(i))) for i in range(sf.desc.contents.num_shapes)],
        "yh_light_list": [list(map(int, row)) for row in ctx.light_list()],
        "yh_scene_once": ctx.scene_once(),
        "yh_lights_const_env": ctx.lights_const_env(),
    }
    sf.close()
    return out


def layouts(ctx, yh, scene_dir):
    return {tag: layout(ctx, yh, make_scenes.ensure_scene(name, scene_dir, **kw), with_maps) for tag, name, kw, with_maps in SCENES}


if __name__ == "__main__":
    import tempfile

    import torch  # noqa: F401  (first: torch's bundled HIP runtime must be the one libyhair.so binds to)
    import yhair_capi as yh

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="yhair_layout_") as scenes:
        ctx = yh.Context(0)
        doc = {"header": f"written by tools/upload_layout.py from the library of commit {a.commit}; offsets in 32-byte units; "
                         "yh_light_list rows: object or -1, environment or -1, cdf entries, in the LDS light table",
               "scenes": layouts(ctx, yh, scenes)}
        ctx.close()
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(a.out)
