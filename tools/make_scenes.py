#!/usr/bin/env python3
"""Procedural stand-ins for the four hair models the reference does not ship.

`hair-block.ply`, `straight-hair.ply`, `curly-hair.ply` and `hair-curl.ply` are
git-ignored in the reference (tests/.gitignore:7-10; they live on Google Drive,
README.md:14,70), so EVERY config of BASELINE.json runs on synthetic hair
written in the reference's PLY layout (vertex `x y z nx ny nz radius` where
nx ny nz is the curve TANGENT, element `line` with `list uchar int
vertex_indices`; libs/yocto/yocto_shape.cpp:4855-4878, yocto_ply.h:1145-1161).

The scene JSONs written here are the bench variants SURVEY.md 8(d) specifies
(aspect 1.0 where the metric wants a square image, `eumelanin 1.3` instead of
`color` on the hair block, beta_m / beta_n / alpha overrides). The same files
feed the reference (oracle/_ref), the CPU oracle and the GPU path.

Geometry is deterministic: numpy Generator(PCG64) seeded 7.
"""
import argparse
import json
import os
import shutil

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "assets")
IDENT = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


def write_hair_ply(path, pos, r_root, r_tip):
    """pos: (S, V, 3) float strand polylines. Tangents = normalised central differences,
    radius tapered linearly root -> tip."""
    S, V, _ = pos.shape
    assert V <= 255, "list length is a uchar in the reference reader"
    tang = np.empty_like(pos)
    tang[:, 1:-1] = pos[:, 2:] - pos[:, :-2]
    tang[:, 0] = pos[:, 1] - pos[:, 0]
    tang[:, -1] = pos[:, -1] - pos[:, -2]
    tang /= np.maximum(np.linalg.norm(tang, axis=2, keepdims=True), 1e-20)
    t = np.linspace(0.0, 1.0, V, dtype=np.float32)[None, :, None]
    radius = (r_root * (1 - t) + r_tip * t).astype(np.float32) * np.ones((S, 1, 1), np.float32)
    verts = np.concatenate([pos, tang, radius], axis=2).astype("<f4").reshape(S * V, 7)
    idx = np.arange(S * V, dtype="<i4").reshape(S, V)
    lines = np.empty(S, dtype=[("n", "u1"), ("i", "<i4", (V,))])
    lines["n"] = V
    lines["i"] = idx
    header = ("ply\nformat binary_little_endian 1.0\ncomment synthetic hair (tools/make_scenes.py)\n"
              f"element vertex {S * V}\nproperty float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\nproperty float radius\n"
              f"element line {S}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode())
        f.write(verts.tobytes())
        f.write(lines.tobytes())
    return S * (V - 1)


def gen_hair_block(strands=100_000, segments=16, seed=7):
    """strands rooted uniformly on local [-.5,.5]^2, growing along
    local +z to z=1 with a helical wobble of amplitude U(0,0.02)."""
    rng = np.random.default_rng(seed)
    root = rng.uniform(-0.5, 0.5, (strands, 2)).astype(np.float32)
    amp = rng.uniform(0.0, 0.02, (strands, 1)).astype(np.float32)
    phase = rng.uniform(0.0, 2 * np.pi, (strands, 1)).astype(np.float32)
    turns = rng.uniform(1.0, 3.0, (strands, 1)).astype(np.float32)
    t = np.linspace(0.0, 1.0, segments + 1, dtype=np.float32)[None, :]
    ang = phase + 2 * np.pi * turns * t
    x = root[:, :1] + amp * t * np.cos(ang)
    y = root[:, 1:] + amp * t * np.sin(ang)
    z = np.broadcast_to(t, x.shape)
    return np.stack([x, y, z], axis=2).astype(np.float32)


def _scalp_roots(rng, strands, radius=4.5, centre=(0.0, 12.0, 0.0)):
    """Roots on the upper/back part of a scalp sphere (object space), face side left bare."""
    pts = []
    n = 0
    while n < strands:
        v = rng.normal(size=(strands * 2, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        keep = (v[:, 1] > -0.25) & ~((v[:, 2] < -0.45) & (v[:, 1] < 0.55))
        v = v[keep]
        pts.append(v)
        n += len(v)
    d = np.concatenate(pts)[:strands].astype(np.float32)
    return d, (np.asarray(centre, np.float32) + radius * d).astype(np.float32)


def gen_head_hair(strands=50_000, segments=32, curly=False, seed=7):
    """C2 (straight, 2 lines per span) / C3 (helical, 4 lines per span): strands leave the
    scalp along its normal and bend under gravity down to y ~ 2.5."""
    rng = np.random.default_rng(seed)
    d, root = _scalp_roots(rng, strands)
    length = rng.uniform(8.5, 10.5, (strands, 1)).astype(np.float32)
    t = np.linspace(0.0, 1.0, segments + 1, dtype=np.float32)[None, :, None]
    s = t * length[:, None, :]
    # outward for ~1.2 units, then blend to straight down; slight per-strand sway
    blend = (1 - np.exp(-s / 1.2)).astype(np.float32)
    out_dir = d[:, None, :]
    down = np.array([0, -1, 0], np.float32)[None, None, :]
    sway = rng.normal(0, 0.06, (strands, 1, 3)).astype(np.float32)
    sway[:, :, 1] = 0
    # integrate direction along the strand
    direction = (1 - blend) * out_dir + blend * (down + sway)
    direction /= np.linalg.norm(direction, axis=2, keepdims=True)
    step = (length / segments)[:, None, :]
    pos = root[:, None, :] + np.concatenate(
        [np.zeros((strands, 1, 3), np.float32), np.cumsum(direction[:, :-1] * step, axis=1)], axis=1)
    if curly:
        amp = rng.uniform(0.10, 0.28, (strands, 1, 1)).astype(np.float32)
        turns = rng.uniform(5.0, 9.0, (strands, 1, 1)).astype(np.float32)
        phase = rng.uniform(0, 2 * np.pi, (strands, 1, 1)).astype(np.float32)
        ang = phase + 2 * np.pi * turns * t
        grow = np.minimum(1.0, 4 * t).astype(np.float32)  # no curl right at the root
        ex = np.array([1, 0, 0], np.float32)[None, None, :]
        ez = np.array([0, 0, 1], np.float32)[None, None, :]
        pos = pos + amp * grow * (np.cos(ang) * ex + np.sin(ang) * ez)
    return pos.astype(np.float32)


def gen_hair_curl(strands=10_000, segments=100, seed=7):
    """C4: one curl bundle following a vertical helix (axis y from ~11 down to ~1)."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, segments + 1, dtype=np.float32)[None, :]
    off_r = 0.35 * np.sqrt(rng.uniform(0, 1, (strands, 1))).astype(np.float32)
    off_a = rng.uniform(0, 2 * np.pi, (strands, 1)).astype(np.float32)
    jitter = rng.uniform(-0.15, 0.15, (strands, 1)).astype(np.float32)
    turns = 4.0
    ang = 2 * np.pi * turns * t + jitter
    helix_r = 0.55 * (0.6 + 0.4 * t)
    y = 11.0 - 10.0 * t + 0.15 * off_r * np.sin(off_a)
    x = helix_r * np.cos(ang) + off_r * np.cos(off_a + 1.5 * ang)
    z = helix_r * np.sin(ang) + off_r * np.sin(off_a + 1.5 * ang)
    return np.stack([x, np.broadcast_to(y, x.shape), z], axis=2).astype(np.float32)


def _dump(scene, out_json):
    with open(out_json, "w") as f:
        json.dump(scene, f, indent=2)


def _prep(outdir, name):
    d = os.path.join(outdir, name)
    os.makedirs(os.path.join(d, "shapes"), exist_ok=True)
    os.makedirs(os.path.join(d, "textures"), exist_ok=True)
    return d


def make_sphere_hairblock(outdir, scale=1.0, name="sphere-hairblock", zoom=False, hair=None, dof=False):
    """C0/C1: variant of tests/sphere-hairblock/sphere-hairblock.json: aspect 1.0 and hair
    material {eumelanin 1.3} (the committed `color` would override melanin, ext.cpp:131-138)."""
    d = _prep(outdir, name)
    shutil.copy(os.path.join(ASSETS, "sphere.ply"), os.path.join(d, "shapes", "sphere.ply"))
    nseg = write_hair_ply(os.path.join(d, "shapes", "hair-block.ply"),
                          gen_hair_block(max(64, int(100_000 * scale))), 0.004, 0.001)
    cam = {"lens": 0.05, "aperture": 0.0, "aspect": 1.0, "lookat": [-0.5, 1.5, 5, 0.25, 0.5, 0, 0, 1, 0]}
    if zoom:  # SURVEY.md appendix B.3 "hair fills frame"
        cam = {"lens": 0.22, "aperture": 0.0, "aspect": 1.0, "lookat": [-0.5, 1.5, 5, 0.5, 0.5, -0.5, 0, 1, 0]}
    if dof:  # thin-lens branch of sample_camera (pt.cpp:211-229) and the portrait branch of init_state (pt.cpp:1933-1939)
        cam = {"lens": 0.085, "aperture": 0.12, "aspect": 0.75, "lookat": [-0.5, 1.5, 5, 0.4, 0.5, -0.3, 0, 1, 0]}
    scene = {
        "asset": {"copyright": "synthetic hair block; sphere from the reference's test assets"},
        "cameras": {"default": cam},
        "environments": {"sky": {"emission": [1, 1, 1]}},
        "objects": {
            "sphere": {"frame": [1, 0, 0, 0, 1, 0, 0, 0, 1, -0.5, 0, 0], "shape": "sphere", "material": "diffuse"},
            "hairblock": {"frame": [1, 0, 0, 0, 0, 1, 0, -1, 0, 0.5, 1, -0.5], "shape": "hair-block", "material": "hair"},
        },
        "materials": {
            "diffuse": {"color": [0.8, 0.4, 0.05]},
            "hair": hair if hair is not None else {"eumelanin": 1.3},
            "arealight": {"emission": [20, 20, 20]},
        },
    }
    _dump(scene, os.path.join(d, name + ".json"))
    return os.path.join(d, name + ".json"), nseg


LOBE_MATERIALS = {
    # one sphere per lobe combination of pt.cpp:405-471
    "plastic": {"color": [0.8, 0.2, 0.2], "specular": 1.0, "roughness": 0.2},
    "roughmetal": {"color": [0.9, 0.7, 0.3], "metallic": 1.0, "roughness": 0.3},
    "mirror": {"color": [0.9, 0.9, 0.9], "metallic": 1.0, "roughness": 0.0},
    "polish": {"color": [0.0, 0.0, 0.0], "specular": 1.0, "roughness": 0.0},
    "frosted": {"color": [0.9, 1.0, 0.9], "specular": 1.0, "transmission": 1.0, "thin": True, "roughness": 0.1},
    "pane": {"color": [1.0, 1.0, 1.0], "specular": 1.0, "transmission": 1.0, "thin": True, "roughness": 0.0, "ior": 1.33},
    "veil": {"color": [0.2, 0.8, 0.3], "opacity": 0.5},
    "mixed": {"color": [0.5, 0.6, 0.9], "specular": 0.5, "metallic": 0.3, "transmission": 0.4, "thin": True,
              "roughness": 0.15, "opacity": 0.9},
}


def make_lobes(outdir, scale=1.0, name="lobes"):
    """Rank-1 widening scene: eight spheres (specular / metal / delta / thin transmission /
    opacity materials), the hair block, one area light and a constant environment."""
    d = _prep(outdir, name)
    shutil.copy(os.path.join(ASSETS, "sphere.ply"), os.path.join(d, "shapes", "sphere.ply"))
    shutil.copy(os.path.join(ASSETS, "arealight.ply"), os.path.join(d, "shapes", "arealight.ply"))
    nseg = write_hair_ply(os.path.join(d, "shapes", "hair-block.ply"),
                          gen_hair_block(max(64, int(100_000 * scale))), 0.004, 0.001)
    objects = {
        "hairblock": {"frame": [1, 0, 0, 0, 0, 1, 0, -1, 0, 1.6, 1, -0.5], "shape": "hair-block", "material": "hair"},
        "floor": {"frame": [2, 0, 0, 0, 0, -2, 0, 2, 0, 0.3, 0, 0], "shape": "arealight", "material": "floor"},
        "light": {"lookat": [0.3, 5, 2, 0.3, 0.5, 0, 0, 1, 0], "shape": "arealight", "material": "arealight"},
    }
    materials = {"hair": {"eumelanin": 1.3}, "floor": {"color": [0.6, 0.6, 0.6]}, "arealight": {"emission": [12, 12, 12]}}
    for k, (mname, mat) in enumerate(LOBE_MATERIALS.items()):
        x, z = -1.5 + 0.85 * (k % 4), (0.45 if k < 4 else -0.55)
        sz = 0.7
        objects["ball%d" % k] = {"frame": [sz, 0, 0, 0, sz, 0, 0, 0, sz, x, 0.0, z], "shape": "sphere", "material": mname}
        materials[mname] = mat
    scene = {
        "asset": {"copyright": "synthetic; sphere and quad from the reference's test assets"},
        "cameras": {"default": {"lens": 0.05, "aperture": 0.0, "aspect": 1.0, "lookat": [0.2, 2.6, 5.2, 0.2, 0.35, 0, 0, 1, 0]}},
        "environments": {"sky": {"emission": [0.5, 0.5, 0.5]}},
        "objects": objects,
        "materials": materials,
    }
    _dump(scene, os.path.join(d, name + ".json"))
    return os.path.join(d, name + ".json"), nseg


VOLUME_MATERIALS = {
    # closed transmissive objects = homogeneous volumes (pt.cpp:498-533)
    "glass": {"color": [0.92, 0.97, 0.95], "specular": 1.0, "transmission": 1.0, "thin": False, "roughness": 0.0,
              "trdepth": 0.5},
    "roughglass": {"color": [0.95, 0.85, 0.7], "specular": 1.0, "transmission": 1.0, "thin": False, "roughness": 0.15,
                   "trdepth": 0.3},
    # the sloth body / bold-man skin recipe (tests/sloth/sloth.json:90-103), texture replaced by a colour
    "skin": {"color": [0.823, 0.516, 0.257], "specular": 1.0, "transmission": 1.0, "thin": False, "roughness": 0.5,
             "scattering": [0.823, 0.516, 0.257], "scanisotropy": -0.8, "trdepth": 0.001},
    "jade": {"color": [0.3, 0.7, 0.4], "specular": 1.0, "transmission": 0.8, "thin": False, "roughness": 0.2,
             "scattering": [0.5, 0.9, 0.6], "scanisotropy": 0.4, "trdepth": 0.05, "opacity": 0.95},
}


def make_volumes(outdir, scale=1.0, name="volumes"):
    """Rank-2 widening scene: four closed spheres with a medium inside (clear and rough glass,
    skin-like and jade-like subsurface scattering), the hair block, one area light."""
    d = _prep(outdir, name)
    shutil.copy(os.path.join(ASSETS, "sphere.ply"), os.path.join(d, "shapes", "sphere.ply"))
    shutil.copy(os.path.join(ASSETS, "arealight.ply"), os.path.join(d, "shapes", "arealight.ply"))
    nseg = write_hair_ply(os.path.join(d, "shapes", "hair-block.ply"),
                          gen_hair_block(max(64, int(100_000 * scale))), 0.004, 0.001)
    objects = {
        "hairblock": {"frame": [1, 0, 0, 0, 0, 1, 0, -1, 0, 1.6, 1, -0.5], "shape": "hair-block", "material": "hair"},
        "floor": {"frame": [2, 0, 0, 0, 0, -2, 0, 2, 0, 0.3, 0, 0], "shape": "arealight", "material": "floor"},
        "light": {"lookat": [0.3, 5, 2, 0.3, 0.5, 0, 0, 1, 0], "shape": "arealight", "material": "arealight"},
    }
    materials = {"hair": {"eumelanin": 0.3}, "floor": {"color": [0.6, 0.6, 0.6]}, "arealight": {"emission": [12, 12, 12]}}
    for k, (mname, mat) in enumerate(VOLUME_MATERIALS.items()):
        objects["ball%d" % k] = {"frame": [0.8, 0, 0, 0, 0.8, 0, 0, 0, 0.8, -1.5 + 0.95 * k, 0.0, 0.3], "shape": "sphere",
                                 "material": mname}
        materials[mname] = mat
    scene = {
        "asset": {"copyright": "synthetic; sphere and quad from the reference's test assets"},
        "cameras": {"default": {"lens": 0.05, "aperture": 0.0, "aspect": 1.0, "lookat": [0.2, 2.2, 5.0, 0.2, 0.4, 0, 0, 1, 0]}},
        "environments": {"sky": {"emission": [0.5, 0.5, 0.5]}},
        "objects": objects,
        "materials": materials,
    }
    _dump(scene, os.path.join(d, name + ".json"))
    return os.path.join(d, name + ".json"), nseg


def _write_uv_quad(path, half=2.0, tiles=2.0):
    """A quad in the XY plane (normal +z) with texture coordinates that run past [0, 1] (tiling)."""
    verts = [(-half, -half, 0, 0, 0, 1, 0, 0), (half, -half, 0, 0, 0, 1, tiles, 0),
             (-half, half, 0, 0, 0, 1, 0, tiles), (half, half, 0, 0, 0, 1, tiles, tiles)]
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                "property float nx\nproperty float ny\nproperty float nz\nproperty float u\nproperty float v\n"
                "element face 1\nproperty list uchar int vertex_indices\nend_header\n")
        for v in verts:
            f.write(" ".join(repr(float(x)) for x in v) + "\n")
        f.write("4 0 1 3 2\n")


def make_textured(outdir, scale=1.0, name="textured"):
    """Colour textures: the sloth scene's floor.png as color_tex on a tiled
    floor with texture coordinates, as emission_tex on a light, as scattering_tex inside a volume
    (the bold-man recipe), sky.hdr as a float colour texture on a sphere without texture coordinates."""
    d = _prep(outdir, name)
    shutil.copy(os.path.join(ASSETS, "sphere.ply"), os.path.join(d, "shapes", "sphere.ply"))
    shutil.copy(os.path.join(ASSETS, "floor.png"), os.path.join(d, "textures", "floor.png"))
    shutil.copy(os.path.join(ASSETS, "sky.hdr"), os.path.join(d, "textures", "sky.hdr"))
    _write_uv_quad(os.path.join(d, "shapes", "uvquad.ply"))
    nseg = write_hair_ply(os.path.join(d, "shapes", "hair-block.ply"),
                          gen_hair_block(max(64, int(100_000 * scale))), 0.004, 0.001)
    objects = {
        "hairblock": {"frame": [1, 0, 0, 0, 0, 1, 0, -1, 0, 1.4, 1, -0.5], "shape": "hair-block", "material": "hair"},
        "floor": {"frame": [2, 0, 0, 0, 0, -2, 0, 2, 0, 0.3, 0, 0], "shape": "uvquad", "material": "floor"},
        "light": {"lookat": [0.3, 5, 2, 0.3, 0.5, 0, 0, 1, 0], "shape": "uvquad", "material": "panel"},
        "ball0": {"frame": [0.8, 0, 0, 0, 0.8, 0, 0, 0, 0.8, -1.3, 0.0, 0.3], "shape": "sphere", "material": "marble"},
        "ball1": {"frame": [0.8, 0, 0, 0, 0.8, 0, 0, 0, 0.8, -0.3, 0.0, 0.3], "shape": "sphere", "material": "skin"},
        "ball2": {"frame": [0.8, 0, 0, 0, 0.8, 0, 0, 0, 0.8, 0.7, 0.0, 0.3], "shape": "sphere", "material": "glazed"},
    }
    materials = {
        "hair": {"eumelanin": 0.3},
        "floor": {"color": [0.7, 0.7, 0.7], "color_tex": "floor"},
        "panel": {"emission": [14, 14, 14], "emission_tex": "floor"},
        "marble": {"color": [0.9, 0.9, 0.9], "color_tex": "sky", "specular": 1.0, "roughness": 0.1},
        "skin": {"color": [0.8, 0.8, 0.8], "color_tex": "floor", "specular": 1.0, "transmission": 1.0, "thin": False,
                 "roughness": 0.5, "scattering": [1.0, 1.0, 1.0], "scattering_tex": "floor", "scanisotropy": -0.8,
                 "trdepth": 0.001},
        "glazed": {"color": [0.9, 0.8, 0.7], "color_tex": "floor", "emission": [0.2, 0.2, 0.2], "emission_tex": "sky",
                   "transmission": 0.5, "thin": True, "roughness": 0.2, "specular": 1.0},
    }
    scene = {
        "asset": {"copyright": "synthetic; sphere, floor.png and sky.hdr from the reference's test assets"},
        "cameras": {"default": {"lens": 0.05, "aperture": 0.0, "aspect": 1.0, "lookat": [0.2, 2.2, 5.0, 0.2, 0.4, 0, 0, 1, 0]}},
        "environments": {"sky": {"emission": [0.5, 0.5, 0.5]}},
        "objects": objects,
        "materials": materials,
    }
    _dump(scene, os.path.join(d, name + ".json"))
    return os.path.join(d, name + ".json"), nseg


def write_png(path, img):
    """8-bit PNG from a uint8 array (H, W) grey or (H, W, 3) RGB: one IDAT of zlib-compressed rows with filter 0."""
    import struct
    import zlib
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    ctype = 0 if img.ndim == 2 else 2
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 9)) + chunk(b"IEND", b""))


def _write_plain_quad(path, half=0.6):
    """A quad in the XY plane without normals or texture coordinates (texcoord = element uv, zero tangents)."""
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                "element face 1\nproperty list uchar int vertex_indices\nend_header\n")
        for x, y in ((-half, -half), (half, -half), (-half, half), (half, half)):
            f.write(f"{x!r} {y!r} 0.0\n")
        f.write("4 0 1 3 2\n")


def _map_textures(d, seed=11, n=32):
    """The maps of make_maps, seeded: grey scalar maps, one scalar map stored as RGB (read as grey with stb's weights
    by the reference's scalar loader) and a tangent-space normal map of bumps. Returns {name: mean of the map in [0, 1]}."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:n, 0:n].astype(np.float64) / n
    maps = {
        "spec": 0.15 + 0.85 * (0.5 + 0.5 * np.sin(2 * np.pi * 3 * x) * np.cos(2 * np.pi * 2 * y)),
        "rough": np.clip(0.05 + 0.9 * (((x * 4).astype(int) + (y * 4).astype(int)) % 2) + 0.05 * rng.random((n, n)), 0, 1),
        "holes": np.where(np.hypot((x * 4) % 1 - 0.5, (y * 4) % 1 - 0.5) < 0.3, 0.1, 1.0) * (0.9 + 0.1 * rng.random((n, n))),
    }
    means = {}
    for k, v in maps.items():
        b = np.round(np.clip(v, 0, 1) * 255).astype(np.uint8)
        write_png(os.path.join(d, "textures", k + ".png"), b)
        means[k] = float(b.mean() / 255)
    metal = np.stack([0.3 + 0.7 * x, 0.6 + 0.3 * y, 0.2 + 0.6 * rng.random((n, n))], axis=2)
    mb = np.round(np.clip(metal, 0, 1) * 255).astype(np.uint8)
    write_png(os.path.join(d, "textures", "metal.png"), mb)
    grey = (mb[..., 0].astype(int) * 77 + mb[..., 1].astype(int) * 150 + mb[..., 2].astype(int) * 29) >> 8
    means["metal"] = float(grey.mean() / 255)
    h = 0.5 * np.sin(2 * np.pi * 4 * x) * np.sin(2 * np.pi * 3 * y) + 0.1 * rng.random((n, n))
    gx, gy = np.gradient(h, axis=1) * n / 8, np.gradient(h, axis=0) * n / 8
    nrm = np.stack([-gx, -gy, np.ones_like(h)], axis=2)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    write_png(os.path.join(d, "textures", "bumps.png"), np.round((nrm * 0.5 + 0.5) * 255).astype(np.uint8))
    return means


MAP_KINDS = ("specular", "metallic", "roughness", "opacity", "normal")


def make_maps(outdir, scale=1.0, name="maps", only="", notrans=False, flat=False):
    """Scalar and normal maps (pt.cpp:329-347, 413-424): one material per map plus one with all of them, on the
    reference's uv sphere, the tiled uv quad, a quad without texture coordinates (normal map on zero tangents) and
    a small hair block under an opacity map, lit by an area light. A transmission_tex that changes no pixel.
    only=<kind of MAP_KINDS>: that map alone (the others dropped); notrans: without the transmission_tex;
    flat: every scalar map replaced by its mean as a constant factor and no normal map (the speed twin)."""
    d = _prep(outdir, name)
    shutil.copy(os.path.join(ASSETS, "sphere.ply"), os.path.join(d, "shapes", "sphere.ply"))
    shutil.copy(os.path.join(ASSETS, "arealight.ply"), os.path.join(d, "shapes", "arealight.ply"))
    _write_uv_quad(os.path.join(d, "shapes", "uvquad.ply"), tiles=3.0)
    _write_plain_quad(os.path.join(d, "shapes", "plainquad.ply"))
    nseg = write_hair_ply(os.path.join(d, "shapes", "hair-block.ply"),
                          gen_hair_block(max(64, int(20_000 * scale))), 0.004, 0.001)
    means = _map_textures(d)
    tex_of = {"specular": "spec", "metallic": "metal", "roughness": "rough", "opacity": "holes", "normal": "bumps"}
    materials = {
        "specmap": {"color": [0.8, 0.3, 0.2], "specular": 1.0, "roughness": 0.15, "specular_tex": "spec"},
        "metalmap": {"color": [0.9, 0.7, 0.3], "metallic": 1.0, "roughness": 0.3, "metallic_tex": "metal"},
        "roughmap": {"color": [0.7, 0.7, 0.7], "specular": 1.0, "roughness": 0.9, "roughness_tex": "rough"},
        "normalmap": {"color": [0.6, 0.6, 0.9], "specular": 0.5, "roughness": 0.3, "normal_tex": "bumps"},
        "flatnormal": {"color": [0.5, 0.8, 0.5], "normal_tex": "bumps"},
        "hairop": {"eumelanin": 0.8, "opacity_tex": "holes"},
        "allmaps": {"color": [0.7, 0.5, 0.8], "specular": 1.0, "metallic": 0.6, "roughness": 0.5, "opacity": 0.9995,
                    "specular_tex": "spec", "metallic_tex": "metal", "roughness_tex": "rough", "opacity_tex": "holes",
                    "normal_tex": "bumps", "transmission_tex": "rough"},
        "arealight": {"emission": [30, 30, 30]},
    }
    for mname, m in materials.items():
        for kind in MAP_KINDS:
            key = kind + "_tex"
            if key not in m:
                continue
            if flat:
                t = m.pop(key)
                if kind == "opacity":
                    m["opacity"] = m.get("opacity", 1.0) * means[t]
                elif kind != "normal":
                    m[kind] = m.get(kind, 1.0 if kind == "specular" else 0.0) * means[t]
            elif only and kind != only:
                m.pop(key)
        if notrans or flat:
            m.pop("transmission_tex", None)
    objects = {
        "floor": {"frame": [2, 0, 0, 0, 0, -2, 0, 2, 0, 0.0, -0.8, 0], "shape": "uvquad", "material": "roughmap"},
        "ball0": {"frame": [0.6, 0, 0, 0, 0.6, 0, 0, 0, 0.6, -1.3, 0.0, 0.3], "shape": "sphere", "material": "specmap"},
        "ball1": {"frame": [0.6, 0, 0, 0, 0.6, 0, 0, 0, 0.6, 0.0, 0.0, 0.3], "shape": "sphere", "material": "metalmap"},
        "ball2": {"frame": [0.6, 0, 0, 0, 0.6, 0, 0, 0, 0.6, 1.3, 0.0, 0.3], "shape": "sphere", "material": "normalmap"},
        "ball3": {"frame": [0.6, 0, 0, 0, 0.6, 0, 0, 0, 0.6, -0.65, 1.2, -0.6], "shape": "sphere", "material": "allmaps"},
        "panel": {"frame": [0.8, 0, 0.6, 0, 1, 0, -0.6, 0, 0.8, 0.8, 1.2, -0.8], "shape": "plainquad", "material": "flatnormal"},
        "hairblock": {"frame": [0.8, 0, 0, 0, 0, 0.8, 0, -0.8, 0, 1.6, 0.9, 0.2], "shape": "hair-block", "material": "hairop"},
        "light": {"lookat": [0.0, 4, 3, 0.0, 0.0, 0, 0, 1, 0], "shape": "arealight", "material": "arealight"},
    }
    scene = {
        "asset": {"copyright": "synthetic; sphere and arealight from the reference's test assets, maps generated (seeded)"},
        "cameras": {"default": {"lens": 0.05, "aperture": 0.0, "aspect": 1.0, "lookat": [0.0, 1.6, 5.5, 0.0, 0.4, 0, 0, 1, 0]}},
        "environments": {"sky": {"emission": [0.3, 0.3, 0.3]}},
        "objects": objects,
        "materials": materials,
    }
    _dump(scene, os.path.join(d, name + ".json"))
    return os.path.join(d, name + ".json"), nseg


def make_crowd(outdir, scale=1.0, name="crowd", count=70):
    """Many objects: a scene-level BVH several levels deep (the BASELINE configs have at most six
    objects) and more objects than the kernel stages in LDS, so the in-memory fallback of the scene
    level runs. `count` small spheres of four materials on a jittered grid around the hair block."""
    d = _prep(outdir, name)
    shutil.copy(os.path.join(ASSETS, "sphere.ply"), os.path.join(d, "shapes", "sphere.ply"))
    shutil.copy(os.path.join(ASSETS, "arealight.ply"), os.path.join(d, "shapes", "arealight.ply"))
    nseg = write_hair_ply(os.path.join(d, "shapes", "hair-block.ply"),
                          gen_hair_block(max(64, int(100_000 * scale))), 0.004, 0.001)
    rng = np.random.default_rng(11)
    objects = {
        "hairblock": {"frame": [1, 0, 0, 0, 0, 1, 0, -1, 0, 0.0, 1, -0.5], "shape": "hair-block", "material": "hair"},
        "light": {"lookat": [0.3, 6, 2, 0.3, 0.5, 0, 0, 1, 0], "shape": "arealight", "material": "arealight"},
    }
    mats = ["red", "gold", "glass", "veil"]
    side = int(np.ceil(np.sqrt(count)))
    for k in range(count):
        x = -3.0 + 6.0 * (k % side) / max(1, side - 1) + rng.uniform(-0.1, 0.1)
        z = -2.5 + 5.0 * (k // side) / max(1, side - 1) + rng.uniform(-0.1, 0.1)
        sz = float(rng.uniform(0.15, 0.3))
        a = float(rng.uniform(0, 2 * np.pi))
        c, sn = float(np.cos(a)) * sz, float(np.sin(a)) * sz  # rotated about y and scaled: a non-trivial inverse frame
        objects["ball%03d" % k] = {"frame": [c, 0, -sn, 0, sz, 0, sn, 0, c, float(x), 0.0, float(z)], "shape": "sphere",
                                   "material": mats[k % len(mats)]}
    materials = {"hair": {"eumelanin": 1.3}, "arealight": {"emission": [15, 15, 15]},
                 "red": {"color": [0.8, 0.2, 0.2]}, "gold": {"color": [0.9, 0.7, 0.3], "metallic": 1.0, "roughness": 0.25},
                 "glass": {"color": [0.95, 0.97, 1.0], "specular": 1.0, "transmission": 1.0, "thin": False, "roughness": 0.0,
                           "trdepth": 0.3},
                 "veil": {"color": [0.2, 0.7, 0.3], "opacity": 0.6}}
    scene = {
        "asset": {"copyright": "synthetic; sphere and quad from the reference's test assets"},
        "cameras": {"default": {"lens": 0.035, "aperture": 0.0, "aspect": 1.0, "lookat": [0.5, 3.5, 7.0, 0.0, 0.3, 0, 0, 1, 0]}},
        "environments": {"sky": {"emission": [0.6, 0.6, 0.6]}},
        "objects": objects,
        "materials": materials,
    }
    _dump(scene, os.path.join(d, name + ".json"))
    return os.path.join(d, name + ".json"), nseg


def write_instance_ply(path, frames, ascii=False, order=None):
    """frames: (N, 12) float32 rows `xx xy xz yx yy yz zx zy zz ox oy oz` -> instances/<name>.ply in the reference's layout
    (element `instance`, twelve float properties; yocto_sceneio.cpp:848-898). order: the header's property order."""
    names = ["xx", "xy", "xz", "yx", "yy", "yz", "zx", "zy", "zz", "ox", "oy", "oz"]
    order = list(order) if order is not None else list(range(12))
    frames = np.asarray(frames, np.float32).reshape(-1, 12)
    header = (f"ply\nformat {'ascii' if ascii else 'binary_little_endian'} 1.0\ncomment instances (tools/make_scenes.py)\n"
              f"element instance {len(frames)}\n" + "".join(f"property float {names[k]}\n" for k in order) + "end_header\n")
    with open(path, "wb") as f:
        f.write(header.encode())
        if ascii:
            for row in frames[:, order]:
                f.write((" ".join(repr(float(v)) for v in row) + "\n").encode())
        else:
            f.write(frames[:, order].astype("<f4").tobytes())


def compose_frames(a, b):
    """a * b of two frames in float32 with the reference's operation order (yocto_math.h:2871-2873: rotation(a) * rotation(b),
    rotation(a) * b.o + a.o, a matrix times a vector being a.x * v.x + a.y * v.y + a.z * v.z): a (N, 12), b (12,)."""
    a = np.asarray(a, np.float32).reshape(-1, 12)
    b = np.asarray(b, np.float32)
    out = np.empty_like(a)
    for c in range(4):
        for k in range(3):
            v = (a[:, k] * b[3 * c] + a[:, 3 + k] * b[3 * c + 1]) + a[:, 6 + k] * b[3 * c + 2]
            out[:, 3 * c + k] = v + a[:, 9 + k] if c == 3 else v
    return out


def _field_frames(rng, n, extent, lo, hi):
    """n frames on a jittered grid over [-extent, extent]^2 (y = 0): rotated about y, scaled differently along each axis
    and sheared a little, so that their inverse is not the transpose."""
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    cell = 2.0 * extent / side
    x = -extent + cell * (k % side + 0.5) + rng.uniform(-0.3, 0.3, n) * cell
    z = -extent + cell * (k // side + 0.5) + rng.uniform(-0.3, 0.3, n) * cell
    a = rng.uniform(0, 2 * np.pi, n)
    sx, sy, sz = (rng.uniform(lo, hi, n) for _ in range(3))
    tx, tz = rng.uniform(-0.15, 0.15, n), rng.uniform(-0.15, 0.15, n)
    zero = np.zeros(n)
    return np.stack([sx * np.cos(a), zero, -sx * np.sin(a), sy * tx, sy, sy * tz, sz * np.sin(a), zero, sz * np.cos(a),
                     x, zero, z], axis=1).astype(np.float32)


def make_fur_field(outdir, scale=1.0, name="fur-field", count=2048, expanded=False):
    """Instances (yocto_sceneio.cpp:848-867,1198-1217; yscenetrace.cpp:150-181): one small hair tuft with `count` frames and
    one sphere with count/8 frames, from two instance files, both objects with a frame of their own (so that
    instance * object and object * instance differ); a floor, one area light that is not instanced, a constant
    environment. expanded: the same scene with one JSON object per frame, named so that the alphabetical order keeps
    every copy in its object's place — what a reader without instances can load."""
    d = _prep(outdir, name)
    shutil.copy(os.path.join(ASSETS, "sphere.ply"), os.path.join(d, "shapes", "sphere.ply"))
    shutil.copy(os.path.join(ASSETS, "arealight.ply"), os.path.join(d, "shapes", "arealight.ply"))
    nseg = write_hair_ply(os.path.join(d, "shapes", "tuft.ply"), gen_hair_block(max(32, int(600 * scale)), 8), 0.02, 0.005)
    rng = np.random.default_rng(23)
    side = int(np.ceil(np.sqrt(count)))
    extent = max(1.0, 0.15 * side)
    tufts = _field_frames(rng, count, extent, 0.25, 0.45)
    pebbles = _field_frames(rng, max(1, count // 8), extent, 0.08, 0.2)
    objects = {
        "floor": {"frame": [0.6 * extent, 0, 0, 0, 0, -0.6 * extent, 0, 0.6 * extent, 0, 0, 0, 0], "shape": "arealight", "material": "floor"},
        "light": {"lookat": [0.3 * extent, 2.5 * extent + 3, 0.8 * extent, 0, 0, 0, 0, 1, 0], "shape": "arealight",
                  "material": "arealight"},
        "pebble": {"frame": [0.8, 0, 0.6, 0, 1, 0, -0.6, 0, 0.8, 0, 0.4, 0], "shape": "sphere", "material": "stone",
                   "instance": "pebbles"},
        "tuft": {"frame": [0.6, 0, 0, 0, 0, 0.6, 0, -0.6, 0, 0.02, 0, -0.03], "shape": "tuft", "material": "fur",
                 "instance": "tufts"},
    }
    if expanded:
        for oname, frames in (("pebble", pebbles), ("tuft", tufts)):
            o = objects.pop(oname)
            o.pop("instance")
            for k, fr in enumerate(compose_frames(frames, o["frame"])):
                objects["%s#%05d" % (oname, k)] = dict(o, frame=[float(v) for v in fr])
    else:
        os.makedirs(os.path.join(d, "instances"), exist_ok=True)
        write_instance_ply(os.path.join(d, "instances", "tufts.ply"), tufts)
        write_instance_ply(os.path.join(d, "instances", "pebbles.ply"), pebbles)
    power = 5.0 * max(1.0, extent * extent / 4)
    scene = {
        "asset": {"copyright": "synthetic; sphere and quad from the reference's test assets"},
        "cameras": {"default": {"lens": 0.035, "aperture": 0.0, "aspect": 1.0,
                                "lookat": [0.4 * extent, 0.9 * extent + 0.6, 2.0 * extent + 1.0, 0.0, 0.1, 0, 0, 1, 0]}},
        "environments": {"sky": {"emission": [0.9, 0.9, 0.9]}},
        "objects": objects,
        "materials": {"fur": {"eumelanin": 0.8}, "stone": {"color": [0.55, 0.5, 0.45], "specular": 0.5, "roughness": 0.4},
                      "floor": {"color": [0.35, 0.45, 0.25]}, "arealight": {"emission": [power, power, power]}},
    }
    _dump(scene, os.path.join(d, name + ".json"))
    return os.path.join(d, name + ".json"), nseg * count


def make_fur_field_expanded(outdir, scale=1.0, name="fur-field-expanded", count=2048):
    return make_fur_field(outdir, scale, name, count, expanded=True)


def _head_scene(outdir, name, shape, pos, emission, lights, hair_mat):
    d = _prep(outdir, name)
    shutil.copy(os.path.join(ASSETS, "sky.hdr"), os.path.join(d, "textures", "sky.hdr"))
    nseg = write_hair_ply(os.path.join(d, "shapes", shape + ".ply"), pos, 0.006, 0.003)
    objects = {"hair": {"frame": [-1, 0, 0, 0, 1, 0, 0, 0, -1, 0, 0, 0], "shape": shape, "material": "brown"}}
    materials = {"brown": hair_mat}
    if lights:
        shutil.copy(os.path.join(ASSETS, "arealight_straight.ply"), os.path.join(d, "shapes", "arealight.ply"))
        objects["arealight1"] = {"lookat": [-5, 20, 10, 0, 9.5, 0, 0, 1, 0], "shape": "arealight", "material": "arealight"}
        objects["arealight2"] = {"lookat": [5, 20, 10, 0, 9.5, 0, 0, 1, 0], "shape": "arealight", "material": "arealight"}
        materials["arealight"] = {"emission": [20, 20, 20]}
    scene = {
        "asset": {"copyright": "synthetic head of hair; sky.hdr from the reference's test assets"},
        "cameras": {"default": {"lens": 0.05, "aperture": 0.0, "aspect": 1.0, "lookat": [0, 15, 23, 0, 9.5, 0, 0, 1, 0]}},
        "environments": {"sky": {"emission": emission, "emission_tex": "sky", "frame": IDENT}},
        "objects": objects,
        "materials": materials,
    }
    _dump(scene, os.path.join(d, name + ".json"))
    return os.path.join(d, name + ".json"), nseg


def make_straight_hair(outdir, scale=1.0, beta_m=0.3, name=None):
    """C2: variant of tests/straight-hair/straight-hair.json with a beta_m override."""
    name = name or ("straight-hair" if beta_m == 0.3 else f"straight-hair-bm{beta_m:g}")
    mat = {"eumelanin": 1.3}
    if beta_m != 0.3:
        mat["beta_m"] = beta_m
    return _head_scene(outdir, name, "straight-hair", gen_head_hair(max(64, int(50_000 * scale)), 32, False),
                       [1, 1, 1], True, mat)


def make_curly_hair(outdir, scale=1.0, name="curly-hair"):
    """C3: tests/curly-hair/curly-hair.json (environment only, emission 2.5)."""
    return _head_scene(outdir, name, "curly-hair", gen_head_hair(max(64, int(50_000 * scale)), 64, True),
                       [2.5, 2.5, 2.5], False, {"eumelanin": 1.3})


def make_hair_curls(outdir, scale=1.0, name="hair-curls", beta_n=0.9, alpha=2):
    """C4: variant of tests/hair-curls/hair-curls.json: aspect 1.0, beta_n 0.9, alpha 2 on the
    four hair materials; one curl shape instanced four times."""
    d = _prep(outdir, name)
    shutil.copy(os.path.join(ASSETS, "sky.hdr"), os.path.join(d, "textures", "sky.hdr"))
    shutil.copy(os.path.join(ASSETS, "arealight.ply"), os.path.join(d, "shapes", "arealight.ply"))
    nseg = write_hair_ply(os.path.join(d, "shapes", "hair-curl.ply"),
                          gen_hair_curl(max(64, int(10_000 * scale))), 0.008, 0.004)
    ov = {"beta_n": beta_n, "alpha": alpha}
    objects = {}
    for nm, x in (("black", -3.75), ("red", -1.25), ("brown", 1.25), ("blonde", 3.75)):
        objects[nm] = {"frame": [1, 0, 0, 0, 1, 0, 0, 0, 1, x, 0, 0], "shape": "hair-curl", "material": nm}
    objects["arealight1"] = {"lookat": [-8, 10, 5, -6.5, 3.5, 0, 0, 1, 0], "shape": "arealight", "material": "arealight"}
    objects["arealight2"] = {"lookat": [0, 10, 5, -1.5, 3.5, 0, 0, 1, 0], "shape": "arealight", "material": "arealight"}
    scene = {
        "asset": {"copyright": "synthetic curl bundle; sky.hdr / arealight.ply from the reference's test assets"},
        "cameras": {"default": {"lens": 0.05, "aperture": 0.0, "aspect": 1.0, "lookat": [-4, 5.9, 20, -4, 5.9, 0, 0, 1, 0]}},
        "environments": {"sky": {"emission": [2, 2, 2], "emission_tex": "sky", "frame": IDENT}},
        "objects": objects,
        "materials": {
            "black": dict(eumelanin=8, **ov), "red": dict(pheomelanin=2, **ov),
            "brown": dict(eumelanin=1.3, **ov), "blonde": dict(eumelanin=0.3, **ov),
            "arealight": {"emission": [20, 20, 20]},
        },
    }
    _dump(scene, os.path.join(d, name + ".json"))
    return os.path.join(d, name + ".json"), nseg * 4


# ---------------------------------------------------------------------------------------------
# The reference's OWN scene descriptions (tests/golden/ref_scenes/*.json: data files of the
# reference's test directory, verbatim) with stand-ins for the models it does not distribute
# (tests/.gitignore there): synthetic hair by shape name, the reference's sphere for every mesh,
# a uv quad for the floor; textures it does ship (sky.hdr, floor.png) under their own names.
# ---------------------------------------------------------------------------------------------
REF_SCENES = os.path.join(ROOT, "tests", "golden", "ref_scenes")


def make_reference_scene(outdir, scale=1.0, name=None, which="sloth"):
    d = _prep(outdir, name)
    with open(os.path.join(REF_SCENES, which + ".json")) as f:
        scene = json.load(f)
    shapes, textures = set(), set()
    for o in scene.get("objects", {}).values():
        if "shape" in o:
            shapes.add(o["shape"])
    for group in ("materials", "environments"):
        for m in scene.get(group, {}).values():
            textures.update(v for k, v in m.items() if k.endswith("_tex"))
    nseg = 0
    for sh in sorted(shapes):
        dst = os.path.join(d, "shapes", sh + ".ply")
        if sh == "hair-block":
            nseg += write_hair_ply(dst, gen_hair_block(max(64, int(100_000 * scale))), 0.004, 0.001)
        elif sh == "straight-hair":
            nseg += write_hair_ply(dst, gen_head_hair(max(64, int(50_000 * scale)), 32, False), 0.006, 0.003)
        elif sh == "curly-hair":
            nseg += write_hair_ply(dst, gen_head_hair(max(64, int(50_000 * scale)), 64, True), 0.006, 0.003)
        elif sh == "hair-curl":
            nseg += write_hair_ply(dst, gen_hair_curl(max(64, int(10_000 * scale))), 0.008, 0.004)
        elif "hair" in sh:  # sloth's fur patches
            nseg += write_hair_ply(dst, gen_hair_curl(max(64, int(4_000 * scale)), 40), 0.008, 0.004)
        elif sh == "arealight":
            shutil.copy(os.path.join(ASSETS, "arealight_straight.ply" if which == "straight-hair" else "arealight.ply"), dst)
        elif sh == "floor":
            _write_uv_quad(dst, half=12.0, tiles=6.0)
        else:
            shutil.copy(os.path.join(ASSETS, "sphere.ply"), dst)
    for t in sorted(textures):
        if t in ("floor", "texture1"):
            shutil.copy(os.path.join(ASSETS, "floor.png"), os.path.join(d, "textures", t + ".png"))
        else:
            shutil.copy(os.path.join(ASSETS, "sky.hdr"), os.path.join(d, "textures", t + ".hdr"))
    shutil.copy(os.path.join(REF_SCENES, which + ".json"), os.path.join(d, name + ".json"))  # verbatim
    return os.path.join(d, name + ".json"), nseg


def _ref_maker(which):
    return lambda outdir, scale=1.0, name=None: make_reference_scene(outdir, scale, name or ("ref-" + which), which)


def _write_grid_light(path, n=3):
    """The reference's arealight quad (-2..2 in x and y, z = 0, facing +z) as an n x n grid: 2 n^2 triangles — an area
    light too big for the kernels' LDS light table (> 4 triangles), i.e. one sampled and intersected through memory."""
    verts = [(-2 + 4 * i / n, -2 + 4 * j / n, 0.0) for j in range(n + 1) for i in range(n + 1)]
    faces = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i, (j + 1) * (n + 1) + i + 1
            faces += [(a, b, c), (d, c, b)]
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {len(verts)}\nproperty float x\nproperty float y\nproperty float z\n"
                f"property float nx\nproperty float ny\nproperty float nz\nelement face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n")
        for v in verts:
            f.write(f"{v[0]:.9g} {v[1]:.9g} {v[2]:.9g} 0 0 1\n")
        for t in faces:
            f.write(f"3 {t[0]} {t[1]} {t[2]}\n")


def make_lights_unit(outdir, scale=1.0, name="lights-unit", biglight=False):
    """Light sampling in isolation (pt.cpp:1283-1358): diffuse spheres and a floor — no hair, so no
    libm-driven path divergence ahead of the light code — under two area lights (the uniform light
    pick, triangle CDF, the 100-step area pdf walk through both quads) and the textured sky (texel CDF
    upper_bound, texel pdf)."""
    d = _prep(outdir, name)
    shutil.copy(os.path.join(ASSETS, "sphere.ply"), os.path.join(d, "shapes", "sphere.ply"))
    shutil.copy(os.path.join(ASSETS, "arealight.ply"), os.path.join(d, "shapes", "arealight.ply"))
    shutil.copy(os.path.join(ASSETS, "sky.hdr"), os.path.join(d, "textures", "sky.hdr"))
    objects = {
        "floor": {"frame": [3, 0, 0, 0, 0, -3, 0, 3, 0, 0.0, 0, 0], "shape": "arealight", "material": "floor"},
        "ball0": {"frame": [1, 0, 0, 0, 1, 0, 0, 0, 1, -0.7, 0.0, 0.2], "shape": "sphere", "material": "red"},
        "ball1": {"frame": [0.6, 0, 0, 0, 0.6, 0, 0, 0, 0.6, 0.8, 0.0, 0.6], "shape": "sphere", "material": "white"},
        # one light behind the other as seen from the floor: the area pdf walk crosses both quads
        "light1": {"lookat": [0.5, 4, 1.5, 0.0, 0.5, 0, 0, 1, 0], "shape": "arealight", "material": "arealight"},
        "light2": {"lookat": [1.0, 8, 3.0, 0.0, 0.5, 0, 0, 1, 0], "shape": "gridlight" if biglight else "arealight", "material": "arealight2"},
    }
    if biglight:  # the second light as an 18-triangle mesh: the light code that goes through the BVH (GENERAL kernel variants)
        _write_grid_light(os.path.join(d, "shapes", "gridlight.ply"))
    scene = {
        "asset": {"copyright": "synthetic; sphere, quad and sky.hdr from the reference's test assets"},
        "cameras": {"default": {"lens": 0.05, "aperture": 0.0, "aspect": 1.0, "lookat": [0.0, 2.4, 5.5, 0.0, 0.5, 0, 0, 1, 0]}},
        "environments": {"sky": {"emission": [1.5, 1.5, 1.5], "emission_tex": "sky", "frame": IDENT}},
        "objects": objects,
        "materials": {"floor": {"color": [0.7, 0.7, 0.7]}, "red": {"color": [0.8, 0.2, 0.2]}, "white": {"color": [0.9, 0.9, 0.9]},
                      "arealight": {"emission": [10, 10, 10]}, "arealight2": {"emission": [30, 25, 20]}},
    }
    _dump(scene, os.path.join(d, name + ".json"))
    return os.path.join(d, name + ".json"), 0


def rotation_frame(axis, degrees):
    """A frame (x, y, z axes, origin 0) that rotates about `axis` by `degrees`, as float32-exact JSON numbers."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    return [float(np.float32(v)) for v in R.T.reshape(-1)] + [0.0, 0.0, 0.0]


ENV_ROT = rotation_frame((1, 2, 3), 40)       # the sky of envs-unit
ENV_ROT_SMALL = rotation_frame((3, -1, 2), 110)  # its small png environments
ENV_LOOKAT = [1.0, 2.0, 3.0, 0.0, 0.5, -1.0, 0.0, 1.0, 0.0]


def _write_env_png(path, w, h, seed=23):
    """An 8-bit RGB environment map: seeded noise, its top third black (a flat stretch at the head of the texel cdf)
    and one texel at 255."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    img = rng.integers(20, 120, (h, w, 3), dtype=np.uint8)
    img[: h // 3] = 0
    img[h - 1 - h // 4, (2 * w) // 3] = 255
    write_png(path, img)


def _write_fan_light(path, n, degenerate=False):
    """A fan of n triangles of different areas around the origin in the XY plane (z = 0, facing +z), without normals;
    degenerate: two rim vertices coincide, so one triangle has no area (a tie in the light's area cdf)."""
    rim = []
    for k in range(n + 1):
        th, r = 0.3 + k * 4.4 / n, 1.0 + 0.35 * ((5 * k) % 3)
        rim.append((r * np.cos(th), r * np.sin(th), 0.0))
    if degenerate:
        rim[2] = rim[1]
    with open(path, "w") as f:
        f.write(f"ply\nformat ascii 1.0\nelement vertex {n + 2}\nproperty float x\nproperty float y\nproperty float z\n"
                f"element face {n}\nproperty list uchar int vertex_indices\nend_header\n")
        for v in [(0.0, 0.0, 0.0)] + rim:
            f.write(f"{v[0]:.9g} {v[1]:.9g} {v[2]:.9g}\n")
        for k in range(n):
            f.write(f"3 0 {k + 1} {k + 2}\n")


def make_envs_unit(outdir, scale=1.0, name="envs-unit", variant="rot"):
    """The light and environment tables at their edges, on the diffuse-only stage of make_lights_unit (no hair: paths follow
    the oracle draw for draw). `variant`:
      rot        sky.hdr in a frame rotated about (1, 2, 3) by 40 degrees
      lookat     the same texture placed with "lookat" (next to a "frame" that it overrides)
      multi      four environments in name order: constant | textured with emission 0 (no light) | rotated sky.hdr | rotated 67x63 png
      tex-WxH    one rotated W x H png environment (_write_env_png)
      lights-N   ONE emitter, a fan of N triangles in an object frame with non-uniform scale, under a constant sky; N = 4 has
                 a triangle without area"""
    d = _prep(outdir, name)
    shutil.copy(os.path.join(ASSETS, "sphere.ply"), os.path.join(d, "shapes", "sphere.ply"))
    shutil.copy(os.path.join(ASSETS, "arealight.ply"), os.path.join(d, "shapes", "arealight.ply"))
    objects = {
        "floor": {"frame": [3, 0, 0, 0, 0, -3, 0, 3, 0, 0.0, 0, 0], "shape": "arealight", "material": "floor"},
        "ball0": {"frame": [1, 0, 0, 0, 1, 0, 0, 0, 1, -0.7, 0.0, 0.2], "shape": "sphere", "material": "red"},
        "ball1": {"frame": [0.6, 0, 0, 0, 0.6, 0, 0, 0, 0.6, 0.8, 0.0, 0.6], "shape": "sphere", "material": "white"},
    }
    materials = {"floor": {"color": [0.7, 0.7, 0.7]}, "red": {"color": [0.8, 0.2, 0.2]}, "white": {"color": [0.9, 0.9, 0.9]},
                 "arealight": {"emission": [10, 10, 10]}, "arealight2": {"emission": [30, 25, 20]}}
    sky = lambda: shutil.copy(os.path.join(ASSETS, "sky.hdr"), os.path.join(d, "textures", "sky.hdr"))  # noqa: E731
    if variant.startswith("lights-"):
        n = int(variant[7:])
        _write_fan_light(os.path.join(d, "shapes", "fanlight.ply"), n, degenerate=(n == 4))
        objects["light1"] = {"frame": [1.5, 0, 0, 0, 0, 0.7, 0, -1.2, 0, 0.2, 3.0, 0.5], "shape": "fanlight", "material": "arealight"}
        envs = {"sky": {"emission": [0.5, 0.5, 0.5]}}
    else:
        objects["light1"] = {"lookat": [0.5, 4, 1.5, 0.0, 0.5, 0, 0, 1, 0], "shape": "arealight", "material": "arealight"}
        objects["light2"] = {"lookat": [1.0, 8, 3.0, 0.0, 0.5, 0, 0, 1, 0], "shape": "arealight", "material": "arealight2"}
        if variant == "rot":
            sky()
            envs = {"sky": {"emission": [1.5, 1.5, 1.5], "emission_tex": "sky", "frame": ENV_ROT}}
        elif variant == "lookat":
            sky()
            envs = {"sky": {"emission": [1.5, 1.5, 1.5], "emission_tex": "sky", "frame": ENV_ROT, "lookat": ENV_LOOKAT}}
        elif variant == "multi":
            sky()
            _write_env_png(os.path.join(d, "textures", "small.png"), 67, 63)
            envs = {"a-constant": {"emission": [0.3, 0.4, 0.5]},
                    "b-black": {"emission": [0, 0, 0], "emission_tex": "small", "frame": ENV_ROT_SMALL},
                    "c-sky": {"emission": [1.5, 1.5, 1.5], "emission_tex": "sky", "frame": ENV_ROT},
                    "d-small": {"emission": [2, 2, 2], "emission_tex": "small", "frame": ENV_ROT_SMALL}}
        elif variant.startswith("tex-"):
            w, h = (int(v) for v in variant[4:].split("x"))
            _write_env_png(os.path.join(d, "textures", "small.png"), w, h)
            envs = {"sky": {"emission": [2, 2, 2], "emission_tex": "small", "frame": ENV_ROT_SMALL}}
        else:
            raise ValueError(f"envs-unit: unknown variant {variant!r}")
    scene = {
        "asset": {"copyright": "synthetic; sphere, quad and sky.hdr from the reference's test assets"},
        "cameras": {"default": {"lens": 0.05, "aperture": 0.0, "aspect": 1.0, "lookat": [0.0, 2.4, 5.5, 0.0, 0.5, 0, 0, 1, 0]}},
        "environments": envs, "objects": objects, "materials": materials,
    }
    _dump(scene, os.path.join(d, name + ".json"))
    return os.path.join(d, name + ".json"), 0


SCENE_ONCE_VARIANTS = ("one", "disjoint", "overlap", "tie", "full", "five")


def make_scene_once(outdir, scale=1.0, name="scene-once", variant="disjoint"):
    """Small scenes for the scene level of the plain kernels (csrc/dev_trace.h: the scene level resolved once per ray): the
    hair block of sphere-hairblock at 256 strands with
      one       nothing else;
      disjoint  the sphere beside it (sphere-hairblock's layout);
      overlap   the block pushed into the sphere, whose frame is sheared and scaled differently along each axis (non-rigid);
      tie       two COINCIDENT quads of two objects cutting through the block (every hit on them is an exact-t tie);
      full      the sphere and two small area lights: four objects, a full leaf of the scene tree;
      five      those and a floor quad: five objects, a scene tree of more than one node.
    No material has a lobe beyond diffuse / hair and every light is a small one: the plain kernel variants render them."""
    assert variant in SCENE_ONCE_VARIANTS, variant
    d = _prep(outdir, name)
    for a in ("sphere", "arealight"):
        shutil.copy(os.path.join(ASSETS, a + ".ply"), os.path.join(d, "shapes", a + ".ply"))
    nseg = write_hair_ply(os.path.join(d, "shapes", "hair-block.ply"), gen_hair_block(max(64, min(512, int(256 * scale)))), 0.004, 0.001)
    hair_frame = [1, 0, 0, 0, 0, 1, 0, -1, 0, 0.5, 1, -0.5]
    sphere_frame = [1, 0, 0, 0, 1, 0, 0, 0, 1, -0.5, 0, 0]
    if variant == "overlap":
        hair_frame = [1, 0, 0, 0, 0, 1, 0, -1, 0, -0.3, 0.8, -0.5]
        sphere_frame = [1.3, 0, 0, 0, 0.7, 0, 0.2, 0, 1.1, -0.5, 0, 0]
    objects = {"hairblock": {"frame": hair_frame, "shape": "hair-block", "material": "hair"}}
    if variant in ("disjoint", "overlap", "full", "five"):
        objects["sphere"] = {"frame": sphere_frame, "shape": "sphere", "material": "diffuse"}
    quad = [0.25, 0, 0, 0, 0, -0.25, 0, 0.25, 0, 0.4, 0.4, -0.5]  # the 4 x 4 quad as a unit square facing +y, inside the block
    if variant == "tie":
        objects["quad-a"] = {"frame": quad, "shape": "arealight", "material": "floor"}
        objects["quad-b"] = {"frame": quad, "shape": "arealight", "material": "floor2"}
    if variant in ("full", "five"):
        objects["light1"] = {"lookat": [0.5, 4, 1.5, 0.0, 0.5, 0, 0, 1, 0], "shape": "arealight", "material": "arealight"}
        objects["light2"] = {"lookat": [1.0, 8, 3.0, 0.0, 0.5, 0, 0, 1, 0], "shape": "arealight", "material": "arealight2"}
    if variant == "five":
        objects["floor"] = {"frame": [1, 0, 0, 0, 0, -1, 0, 1, 0, 0.0, -1.2, 0], "shape": "arealight", "material": "floor"}
    scene = {
        "asset": {"copyright": "synthetic hair block; sphere and quad from the reference's test assets"},
        "cameras": {"default": {"lens": 0.05, "aperture": 0.0, "aspect": 1.0, "lookat": [-0.5, 1.5, 5, 0.25, 0.5, 0, 0, 1, 0]}},
        "environments": {"sky": {"emission": [1, 1, 1]}},
        "objects": objects,
        "materials": {"diffuse": {"color": [0.8, 0.4, 0.05]}, "hair": {"eumelanin": 1.3}, "floor": {"color": [0.7, 0.7, 0.7]},
                      "floor2": {"color": [0.2, 0.3, 0.8]}, "arealight": {"emission": [10, 10, 10]}, "arealight2": {"emission": [30, 25, 20]}},
    }
    _dump(scene, os.path.join(d, name + ".json"))
    return os.path.join(d, name + ".json"), nseg


HITS_UNIT_VARIANTS = ("four", "six", "far", "deep", "ties")
HITS_CHAIN_SEGMENTS = 44
_Q = 1.0 / 1024  # the grid of hits-unit: every coordinate, radius and frame entry is a multiple of 2^-10 below 2^6


def _hits_strands():
    """Shape `strands` of hits-unit: (positions (V, 3), radius (V,), polylines: lists of vertex indices), float64 on the 2^-10 grid.
    Strand 0 lies along x; 1 and 2 cross at a shared joint; 3 has a segment of zero length; 4 and 5 are the same strand twice; the
    rest are seeded, 4-8 segments each, their radii tapering, every third to exactly 0 at the tip."""
    rng = np.random.default_rng(7)
    pos, rad, lines = [], [], []

    def strand(p, r):
        lines.append(list(range(len(pos), len(pos) + len(p))))
        pos.extend(p), rad.extend(r)
    strand([(-1 + 0.5 * k, 0.25, 0.25) for k in range(5)], [32 * _Q, 28 * _Q, 24 * _Q, 20 * _Q, 16 * _Q])
    cross = (0.5, -0.5, -0.5)
    strand([(0.5, -1 + 0.25 * k, -0.5) for k in range(5)], [16 * _Q] * 5)          # along y, `cross` its third vertex
    strand([(0.5, -0.5, -1 + 0.25 * k) for k in range(5)], [24 * _Q, 20 * _Q, 16 * _Q, 12 * _Q, 8 * _Q])  # along z, `cross` its third vertex
    assert pos[7] == cross and pos[12] == cross
    strand([(-0.5, -0.75, 0.5), (-0.5, -0.5, 0.5), (-0.5, -0.5, 0.5), (-0.25, -0.25, 0.5), (-0.25, 0.0, 0.75)], [16 * _Q] * 5)
    twin = [(-0.75, 0.5, -0.75 + 0.25 * k) for k in range(5)]
    strand(twin, [20 * _Q, 16 * _Q, 12 * _Q, 8 * _Q, 0.0])
    strand(twin, [20 * _Q, 16 * _Q, 12 * _Q, 8 * _Q, 0.0])
    for s in range(26):
        n = int(rng.integers(4, 9))
        p = rng.integers(-896, 897, 3).astype(np.float64)
        step = rng.integers(-192, 193, (n, 3)).astype(np.float64)
        step[np.abs(step).sum(1) == 0] = (64, 0, 0)
        pts = np.clip(np.concatenate([[p], p + np.cumsum(step, 0)]), -1024, 1024) * _Q
        r0 = int(rng.integers(12, 33))
        r1 = 0 if s % 3 == 0 else int(rng.integers(2, 12))
        strand([tuple(v) for v in pts], [((r0 * (n - k) + r1 * k) // n) * _Q for k in range(n + 1)])
    return np.array(pos, np.float64), np.array(rad, np.float64), lines


def _hits_tris():
    """Shape `tris` of hits-unit, in the plane z = 0: an 8 x 8 grid of squares over [-1, 1]^2 (128 triangles, shared edges and
    vertices), then a triangle without area, a sliver of aspect 2^10 and the grid's triangle 37 once more (a coincident pair)."""
    verts = [(-1 + 0.25 * i, -1 + 0.25 * j, 0.0) for j in range(9) for i in range(9)]
    tris = []
    for j in range(8):
        for i in range(8):
            a, b, c, d = 9 * j + i, 9 * j + i + 1, 9 * (j + 1) + i, 9 * (j + 1) + i + 1
            tris += [(a, b, c), (d, c, b)]
    k = len(verts)
    verts += [(0.25, 1.25, 0.0), (0.5, 1.25, 0.0), (0.75, 1.25, 0.0), (-1.0, 1.25, 0.0), (0.0, 1.25, 0.0), (-0.5, 1.25 + _Q, 0.0)]
    tris += [(k, k + 1, k + 2), (k + 3, k + 4, k + 5), tris[37]]
    return np.array(verts, np.float64), np.array(tris, np.int32)


def _hits_chain(n=HITS_CHAIN_SEGMENTS):
    """Shape `chain` of hits-unit (variant `deep`): n separate segments along x, the k-th from 0.75 c to 1.25 c with radius c / 8 at
    both ends, c = 2^k 2^-20 (its centroid). Every box holds a stretch of the x axis, and the middle split of the centroids' range
    takes the largest one or two away from all the others: the tree is as deep as the shape has segments, nearly."""
    c = 2.0 ** (np.arange(n) - 20.0)
    pos = np.zeros((2 * n, 3))
    pos[0::2, 0], pos[1::2, 0] = 0.75 * c, 1.25 * c
    return pos, np.repeat(c / 8, 2), [[2 * k, 2 * k + 1] for k in range(n)]


def _hits_ties():
    """The shapes of variant `ties` of hits-unit, on the 2^-10 grid: primitives that are there many times over, so that one ray meets
    bit-equal hits in different leaves of a shape's tree (identical centroids: the builder halves them by index, split_middle's fall-back,
    every node's axis x). name -> dict(positions, radius, polylines | triangles, twin, canon): twin[k] = the first primitive with k's very
    record (same vertices in the same order: the same arithmetic, the same t as bits), canon[k] = the first with k's geometry in any
    vertex order (the same box, another record).
      stack    ONE tapering segment along x 64 times, copies 0, 31 and 63 with their ends swapped: 16 leaves of four, one full 16-wide node
      sheaf    a four-segment strand along z six times, the fourth of them listed from its tip: 24 segments
      plates   ONE triangle in the plane z = 0 32 times, copies 5, 18 and 31 with their vertices rotated: 8 leaves of four, one full 8-wide node;
               then a small one below it 8 times, so that the shape's box is larger than the 32's: a ray along z through a lower vertex of the
               large one lies on a face of the shape's box in x alone, and on faces of the boxes of all 32 in x and y
      rungs    four sites along y, a segment along x at each, there 4, 8, 9 and 16 times: 1, 2, 3 and 4 leaves"""
    out = {}

    def lines_shape(name, strands):  # strands: (points, radii, reversed)
        pos, rad, poly, key = [], [], [], []
        for pts, rr, rev in strands:
            idx = list(range(len(pos), len(pos) + len(pts)))
            pos.extend(pts), rad.extend(rr)
            poly.append(idx[::-1] if rev else idx)
            seg = [(tuple(pts[k]), rr[k], tuple(pts[k + 1]), rr[k + 1]) for k in range(len(pts) - 1)]
            key += [(b, rb, a, ra) for a, ra, b, rb in seg[::-1]] if rev else seg
        twin = [key.index(k) for k in key]
        canon = [min(key.index(k) if k in key else len(key), key.index(k[2:] + k[:2]) if k[2:] + k[:2] in key else len(key)) for k in key]
        out[name] = dict(positions=np.array(pos, np.float64), radius=np.array(rad, np.float64), polylines=poly, twin=np.array(twin), canon=np.array(canon))
    seg = ([(-0.5, 0.0, 0.0), (0.5, 0.0, 0.0)], [24 * _Q, 16 * _Q])
    lines_shape("stack", [(*seg, k in (0, 31, 63)) for k in range(64)])
    strand = ([(0.0, 0.0, -1 + 0.5 * k) for k in range(5)], [20 * _Q, 16 * _Q, 12 * _Q, 8 * _Q, 4 * _Q])
    lines_shape("sheaf", [(*strand, k == 3) for k in range(6)])
    lines_shape("rungs", [([(-0.25, y, 0.0), (0.25, y, 0.0)], [16 * _Q, 16 * _Q], False) for y, n in ((-3.0, 4), (-1.0, 8), (1.0, 9), (3.0, 16)) for _ in range(n)])
    verts, tris, turns = [], [], []
    for k in range(32):
        verts += [(-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.0, 0.5, 0.0)]
        turn = {5: 1, 18: 2, 31: 1}.get(k, 0)
        tris.append(tuple(3 * k + (j + turn) % 3 for j in range(3))), turns.append(turn)
    for k in range(32, 40):
        verts += [(-0.25, -1.5, 0.0), (0.25, -1.5, 0.0), (0.0, -1.0, 0.0)]
        tris.append((3 * k, 3 * k + 1, 3 * k + 2)), turns.append(3)
    out["plates"] = dict(positions=np.array(verts, np.float64), radius=np.zeros(len(verts)), triangles=np.array(tris, np.int32),
                         twin=np.array([turns.index(t) for t in turns]),
                         canon=np.array([0] * 32 + [32] * 8))
    return out


def hits_unit_geometry(variant="four"):
    """The scene hits-unit as arrays, for the tests that aim rays at it: a list of objects in the scene's object order, each a dict
    of name, shape, frame (12 float32: x, y, z axes and origin), positions (V, 3) and radius (V,) as float32, lines (S, 2) or
    triangles (T, 3)."""
    assert variant in HITS_UNIT_VARIANTS, variant
    sp, sr, sl = _hits_strands()
    tp, tt = _hits_tris()
    cp, cr, cl = _hits_chain()
    shapes = {"strands": dict(positions=sp, radius=sr, lines=np.array([(l[k], l[k + 1]) for l in sl for k in range(len(l) - 1)], np.int32)),
              "tris": dict(positions=tp, radius=np.zeros(len(tp)), triangles=tt),
              "chain": dict(positions=cp, radius=cr, lines=np.array(cl, np.int32))}
    if variant == "ties":
        for name, t in _hits_ties().items():
            prims = dict(triangles=t["triangles"]) if "triangles" in t else dict(lines=np.array([(l[k], l[k + 1]) for l in t["polylines"] for k in range(len(l) - 1)], np.int32))
            shapes[name] = dict(positions=t["positions"], radius=t["radius"], twin=t["twin"], canon=t["canon"], **prims)
    rot = rotation_frame((1, 2, 3), 40)
    objects = [("a-strands", "strands", IDENT[:9] + [0, 0, 0]),
               ("b-sheared", "strands", [1.5, 0.25, 0, 0, 0.75, 0.5, 0, 0, 1.25, 3, 0, 0]),
               ("c-tris", "tris", IDENT[:9] + [0, 0, 0]),  # (through the strands of a-strands: world space is both objects' own)
               ("d-rotated", "tris", rot[:9] + [3, 0, -1.5])]
    if variant in ("six", "far"):
        objects += [("e-mirrored", "strands", [-1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 3, 0]),
                    ("f-tris2", "tris", [2, 0, 0, 0, 2, 0, 0, 0, 0.5, 3, 3.5, 0.5])]
    if variant == "ties":  # (translations on the grid: object space is world space moved, exactly)
        objects += [("g-stack", "stack", IDENT[:9] + [0, -4, 0]), ("h-sheaf", "sheaf", IDENT[:9] + [3, -4, 0]),
                    ("i-plates", "plates", IDENT[:9] + [0, -4, 3]), ("j-rungs", "rungs", IDENT[:9] + [-4, 0, 0])]
    if variant == "deep":  # (first by name: where it shares a leaf of the scene tree, the others are entered after it)
        objects = [("a-chain", "chain", [2.0 ** -19, 0, 0, 0, 2.0 ** -19, 0, 0, 0, 2.0 ** -19, -8, 0, -0.75])] + objects
    out = []
    for k, (name, shape, frame) in enumerate(objects):
        frame = np.array(frame, np.float64)
        if variant == "far":
            frame[9:] += (65536, -2048, 8192) if name == "f-tris2" else (4096, -2048, 8192)
        sh = shapes[shape]
        out.append(dict(name=name, shape=shape, frame=frame.astype(np.float32), positions=sh["positions"].astype(np.float32),
                        radius=sh["radius"].astype(np.float32), **{k2: sh[k2] for k2 in ("lines", "triangles", "twin", "canon") if k2 in sh}))
    return out


def _write_f32_ply(path, positions, radius=None, polylines=None, triangles=None):
    """A binary float32 PLY in the reference's layout: lines with tangents and radii, or bare triangles."""
    positions = np.asarray(positions, "<f4")
    header = f"ply\nformat binary_little_endian 1.0\ncomment hits-unit (tools/make_scenes.py)\nelement vertex {len(positions)}\nproperty float x\nproperty float y\nproperty float z\n"
    body = b""
    if polylines is not None:
        tang = np.zeros_like(positions)
        for l in polylines:
            p = positions[l].astype(np.float64)
            t = np.gradient(p, axis=0)
            t[np.linalg.norm(t, axis=1) == 0] = (1, 0, 0)
            tang[l] = t / np.linalg.norm(t, axis=1, keepdims=True)
        header += f"property float nx\nproperty float ny\nproperty float nz\nproperty float radius\nelement line {len(polylines)}\nproperty list uchar int vertex_indices\n"
        verts = np.concatenate([positions, tang, np.asarray(radius, "<f4")[:, None]], axis=1).astype("<f4")
        body = b"".join(bytes([len(l)]) + np.asarray(l, "<i4").tobytes() for l in polylines)
    else:
        header += f"element face {len(triangles)}\nproperty list uchar int vertex_indices\n"
        verts = positions
        body = b"".join(b"\x03" + np.asarray(t, "<i4").tobytes() for t in triangles)
    with open(path, "wb") as f:
        f.write((header + "end_header\n").encode() + verts.tobytes() + body)


def make_hits_unit(outdir, scale=1.0, name="hits-unit", variant="four"):
    """Closest hits at the edges of segments, triangles and boxes (tests/hit_cases.py aims the rays): geometry on the 2^-10 grid, so
    that a ray built on an edge is on it exactly in float32. Shapes: `strands` and `tris` (_hits_strands, _hits_tris). `variant`:
      four   strands | strands in a scaled and sheared frame | tris (an axis-aligned flat box) | tris in a rigid rotation: a scene level of one leaf
      six    those, strands mirrored and a second, scaled tris: a scene tree of more than one node
      far    six, every frame moved by (2^12, -2^11, 2^13) and the last object out to x = 2^16
      deep   a `chain` (_hits_chain, off the grid: powers of two from 2^-21 to 2^24, in a frame that scales them by 2^-19, its small
             end at (-8, 0, -0.75)) and four: a shape tree deep enough that a ray along it fills the traversal stacks past their LDS
             windows, on its way to the objects of `four` behind
      ties   four and four shapes whose primitives are there many times over (_hits_ties): bit-equal hits in different leaves, slots
             and wide nodes, so that visiting order and the merge across a group's leaves decide who wins
    Hair and diffuse materials only: the plain kernel variants take the scenes."""
    d = _prep(outdir, name)
    sp, sr, sl = _hits_strands()
    tp, tt = _hits_tris()
    _write_f32_ply(os.path.join(d, "shapes", "strands.ply"), sp, sr, polylines=sl)
    _write_f32_ply(os.path.join(d, "shapes", "tris.ply"), tp, triangles=tt)
    if variant == "deep":
        cp, cr, cl = _hits_chain()
        _write_f32_ply(os.path.join(d, "shapes", "chain.ply"), cp, cr, polylines=cl)
    if variant == "ties":
        for shape, t in _hits_ties().items():
            _write_f32_ply(os.path.join(d, "shapes", shape + ".ply"), t["positions"], t["radius"], polylines=t.get("polylines"), triangles=t.get("triangles"))
    geo = hits_unit_geometry(variant)
    objects = {o["name"]: {"frame": [float(v) for v in o["frame"]], "shape": o["shape"],
                           "material": "hair" if o["shape"] != "tris" else "diffuse"} for o in geo}
    shift = geo[0]["frame"][9:].astype(np.float64)
    eye, at = shift + (1.5, 1.0, 9.0), shift + (1.5, 1.0, 0.0)
    scene = {
        "asset": {"copyright": "synthetic (tools/make_scenes.py)"},
        "cameras": {"default": {"lens": 0.05, "aperture": 0.0, "aspect": 1.0, "lookat": [float(v) for v in (*eye, *at)] + [0, 1, 0]}},
        "environments": {"sky": {"emission": [1, 1, 1]}},
        "objects": objects,
        "materials": {"diffuse": {"color": [0.8, 0.4, 0.05]}, "hair": {"eumelanin": 1.3}},
    }
    _dump(scene, os.path.join(d, name + ".json"))
    return os.path.join(d, name + ".json"), sum(len(o.get("lines", ())) for o in geo)


MAKERS = {
    "hits-unit": make_hits_unit,
    "scene-once": make_scene_once,
    "lights-unit": make_lights_unit,
    "envs-unit": make_envs_unit,
    "sphere-hairblock": make_sphere_hairblock,
    "straight-hair": make_straight_hair,
    "curly-hair": make_curly_hair,
    "hair-curls": make_hair_curls,
    "lobes": make_lobes,
    "volumes": make_volumes,
    "textured": make_textured,
    "crowd": make_crowd,
    "maps": make_maps,
    "fur-field": make_fur_field,
    "fur-field-expanded": make_fur_field_expanded,
}


for _w in ("sloth", "bold-man", "straight-hair", "curly-hair", "hair-curls", "sphere-hairblock"):
    MAKERS["ref-" + _w] = _ref_maker(_w)


def ensure_scene(name, outdir, scale=1.0, **kw):
    """Builds the scene once per (name, scale, overrides) under outdir and returns the JSON path."""
    tag = name if scale == 1.0 else f"{name}-x{scale:g}"
    for k, v in sorted(kw.items()):
        tag += (f"-{k}{v:g}" if isinstance(v, (int, float)) and not isinstance(v, bool) else
                f"-{k}-{v}" if isinstance(v, str) and v else (f"-{k}" if v else ""))
    path = os.path.join(outdir, tag, tag + ".json")
    if not os.path.exists(path):
        MAKERS[name](outdir, scale=scale, name=tag, **kw)
    return path


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "scenes"))
    ap.add_argument("--scale", type=float, default=1.0, help="strand-count multiplier")
    ap.add_argument("scenes", nargs="*", default=list(MAKERS))
    a = ap.parse_args()
    for s in a.scenes:
        p = ensure_scene(s, a.out, a.scale)
        print(p)
