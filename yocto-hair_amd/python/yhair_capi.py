"""ctypes binding of include/yhair.h (the product's C ABI, libyhair.so).

Plumbing only: no arithmetic of the hot path happens in Python. The same
structures are handed to the CPU oracle (oracle/libyh_oracle.so) by the tests,
which is why the struct mirrors live here and the oracle loader lives in
tests/ (tests/oracle_capi.py) — the product never imports the oracle.
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIB_PATH = os.environ.get("YHAIR_LIB", os.path.join(ROOT, "yocto-hair_amd", "libyhair.so"))

YH_OK, YH_E_INVALID, YH_E_DEVICE, YH_E_STATE, YH_E_IO, YH_E_SELFTEST = 0, -1, -2, -3, -4, -5
YH_HAIR_BRDF_FLOATS = 30
HAIR_SHADE_FLOATS = 15
SURFACE_BSDF_FLOATS = 29
VOLUME_FLOATS = 24
QUAD_FORMS_FLOATS = 12
# yh_path_ends_batch: the operations and, per operation, the floats in, ints in, floats out, ints out of a row (include/yhair.h: YH_PATH_*)
PATH_BEGIN, PATH_CONTINUE, PATH_END = 0, 1, 2
PATH_OPS = {"begin": PATH_BEGIN, "continue": PATH_CONTINUE, "end": PATH_END}
PATH_ROWS = {PATH_BEGIN: (17, 4, 12, 3), PATH_CONTINUE: (3, 2, 3, 2), PATH_END: (8, 1, 4, 0)}
INTERSECT_FORMS = 7  # yh_intersect_plain_batch: forms 0 .. 6
INTERSECT_TABLE_IN_MEMORY = 16  # ... and, on forms 3 .. 6, the scene level read from memory
# yh_point_batch: the columns of a row (include/yhair.h: YH_POINT_*)
POINT_FLOATS = 53
POINT_COLUMNS = {"position": slice(0, 3), "normal": slice(3, 6), "shading_normal": slice(6, 9), "texcoord": slice(9, 11),
                 "color_tex": slice(11, 14), "emission_tex": slice(14, 17), "emission_tex_x": slice(17, 18),
                 "scattering_tex": slice(18, 21), "emission": slice(21, 24), "bsdf": slice(24, 46), "density": slice(46, 49),
                 "scatter": slice(49, 52), "anisotropy": slice(52, 53)}
(LOBE_DIFFUSE, LOBE_SPECULAR, LOBE_METAL, LOBE_TRANSMISSION, LOBE_REFRACTION, LOBE_DELTA_SPECULAR,
 LOBE_DELTA_METAL, LOBE_DELTA_TRANSMISSION, LOBE_DELTA_REFRACTION) = range(9)
LOBE_COUNT = 9

c_float_p = C.POINTER(C.c_float)
c_int_p = C.POINTER(C.c_int)


class Shape(C.Structure):
    _fields_ = [("num_vertices", C.c_int), ("positions", c_float_p), ("normals", c_float_p),
                ("radius", c_float_p), ("num_lines", C.c_int), ("lines", c_int_p),
                ("num_triangles", C.c_int), ("triangles", c_int_p), ("texcoords", c_float_p)]


class Texture(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("is_byte", C.c_int), ("pixels", C.c_void_p)]


class Material(C.Structure):
    _fields_ = [("emission", C.c_float * 3), ("color", C.c_float * 3), ("specular", C.c_float),
                ("metallic", C.c_float), ("roughness", C.c_float), ("transmission", C.c_float),
                ("opacity", C.c_float), ("ior", C.c_float), ("thin", C.c_int),
                ("sigma_a", C.c_float * 3), ("beta_m", C.c_float), ("beta_n", C.c_float),
                ("alpha", C.c_float), ("eta", C.c_float), ("eumelanin", C.c_float),
                ("pheomelanin", C.c_float), ("scattering", C.c_float * 3), ("scanisotropy", C.c_float),
                ("trdepth", C.c_float), ("emission_tex", C.c_int), ("color_tex", C.c_int),
                ("scattering_tex", C.c_int)]


class MaterialMaps(C.Structure):
    """yh_material_maps: a material's scalar and normal maps, 1-based into SceneDesc.textures, 0 = none."""
    _fields_ = [("specular_tex", C.c_int), ("metallic_tex", C.c_int), ("roughness_tex", C.c_int),
                ("transmission_tex", C.c_int), ("opacity_tex", C.c_int), ("normal_tex", C.c_int)]


class Object(C.Structure):
    _fields_ = [("frame", C.c_float * 12), ("shape", C.c_int), ("material", C.c_int)]


class Environment(C.Structure):
    _fields_ = [("frame", C.c_float * 12), ("emission", C.c_float * 3), ("tex_width", C.c_int),
                ("tex_height", C.c_int), ("texels", c_float_p)]


class Camera(C.Structure):
    _fields_ = [("frame", C.c_float * 12), ("lens", C.c_float), ("film", C.c_float * 2),
                ("focus", C.c_float), ("aperture", C.c_float)]


class SceneDesc(C.Structure):
    _fields_ = [("num_shapes", C.c_int), ("shapes", C.POINTER(Shape)),
                ("num_materials", C.c_int), ("materials", C.POINTER(Material)),
                ("num_objects", C.c_int), ("objects", C.POINTER(Object)),
                ("num_environments", C.c_int), ("environments", C.POINTER(Environment)),
                ("camera", Camera), ("num_textures", C.c_int), ("textures", C.POINTER(Texture))]


SHADER_NAMES = ["naive", "path", "eyelight", "normal"]  # shader_type, yocto_pathtrace.h:177-199


class TraceParams(C.Structure):
    _fields_ = [("resolution", C.c_int), ("bounces", C.c_int), ("clamp", C.c_float),
                ("seed", C.c_uint64), ("shader", C.c_int), ("hair_exact", C.c_int)]

    @staticmethod
    def default(resolution=720, bounces=8, clamp=100.0, seed=961748941, shader="path", hair_exact=False):
        return TraceParams(resolution, bounces, clamp, seed, SHADER_NAMES.index(shader) if isinstance(shader, str) else shader,
                           1 if hair_exact else 0)


GBUFFER_CENTRE, GBUFFER_NEXT_SAMPLE = 0, 1
GBUFFER_MODES = {"centre": GBUFFER_CENTRE, "next": GBUFFER_NEXT_SAMPLE}
# the planes of yh_gbuffer in the struct's order: name, numpy dtype, components per pixel
GBUFFER_PLANES = (("object", np.int32, 1), ("element", np.int32, 1), ("material", np.int32, 1), ("uv", np.float32, 2),
                  ("distance", np.float32, 1), ("position", np.float32, 3), ("normal", np.float32, 3), ("tangent", np.float32, 3),
                  ("texcoord", np.float32, 2), ("albedo", np.float32, 3), ("ray", np.float32, 6))


class GBuffer(C.Structure):
    _fields_ = [(n, c_int_p if t is np.int32 else c_float_p) for n, t, _ in GBUFFER_PLANES]


DENOISE_MAX_ITERATIONS = 6


class DenoiseParams(C.Structure):
    """yh_denoise_params (include/yhair.h: DENOISE)."""
    _fields_ = [("iterations", C.c_int), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_position", C.c_float),
                ("demodulate", C.c_int), ("match_object", C.c_int)]

    def copy(self, **changes):
        q = DenoiseParams.from_buffer_copy(self)
        for k, v in changes.items():
            setattr(q, k, v)
        return q


class TemporalParams(C.Structure):
    """yh_temporal_params (include/yhair.h: TEMPORAL)."""
    _fields_ = [("max_history", C.c_int), ("sigma_position", C.c_float), ("match_object", C.c_int)]

    def copy(self, **changes):
        q = TemporalParams.from_buffer_copy(self)
        for k, v in changes.items():
            setattr(q, k, v)
        return q


VARIANCE_MAX_STEPS = 1024


class VarianceParams(C.Structure):
    """yh_variance_params (include/yhair.h: VARIANCE)."""
    _fields_ = [("iterations", C.c_int), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_position", C.c_float),
                ("demodulate", C.c_int), ("match_object", C.c_int), ("epsilon", C.c_float), ("min_steps", C.c_int)]

    def copy(self, **changes):
        q = VarianceParams.from_buffer_copy(self)
        for k, v in changes.items():
            setattr(q, k, v)
        return q


class WorkCounts(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("samples", "rays", "nodes", "seg_tests", "tri_tests",
                                          "hair_shades", "surf_shades", "env_lookups",
                                          "env_samples", "cyc_trace", "cyc_shade", "ticks_tile",
                                          "wave_iters", "wave_steps", "lane_steps", "lane_iters", "cyc_geom", "cyc_sample",
                                          "cyc_eval", "cyc_rest")] + [("branch", C.c_uint64 * 10)]

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "branch"}
        names = ("node", "line", "tri", "enter", "scene")
        for k, nm in enumerate(names):
            d["trips_" + nm], d["lanes_" + nm] = int(self.branch[2 * k]), int(self.branch[2 * k + 1])
        return d

    def bytes_per_sample(self, spp_per_launch, env_textured=True):
        """algorithmic bytes per sample of the reference algorithm. The environment's texels count for a
        TEXTURED environment only (the oracle counts every eval_environment, yh_oracle.cpp; a constant one reads nothing)."""
        s = max(1, self.samples)
        return (32 * self.nodes + 44 * self.seg_tests + 52 * self.tri_tests +
                104 * self.hair_shades + (48 * self.env_lookups if env_textured else 0) + 88 * self.env_samples) / s \
            + 32.0 / spp_per_launch


def fptr(a):
    return a.ctypes.data_as(c_float_p)


def iptr(a):
    return a.ctypes.data_as(c_int_p)


def hair_material_rows(mats12):
    """(n,12) float rows [sigma_a3 beta_m beta_n alpha eta color3 eumelanin pheomelanin]
    (yocto_extension.h:86-95 order) -> ctypes array of yh_material."""
    mats12 = np.ascontiguousarray(mats12, dtype=np.float32).reshape(-1, 12)
    arr = (Material * len(mats12))()
    for i, r in enumerate(mats12):
        m = arr[i]
        m.sigma_a[:] = r[0:3].tolist()
        m.beta_m, m.beta_n, m.alpha, m.eta = map(float, r[3:7])
        m.color[:] = r[7:10].tolist()
        m.eumelanin, m.pheomelanin = float(r[10]), float(r[11])
        m.opacity, m.ior, m.thin, m.trdepth = 1.0, 1.5, 1, 0.01
    return arr


def volume_material_rows(rows10):
    """(n, 10) float rows [color3 transmission thin trdepth scattering3 scanisotropy] -> ctypes array of yh_material
    (a non-hair material otherwise at its defaults: no specular, no metal, roughness 1, opacity 1, ior 1.5)."""
    rows10 = np.ascontiguousarray(rows10, dtype=np.float32).reshape(-1, 10)
    arr = (Material * len(rows10))()
    for i, r in enumerate(rows10):
        m = arr[i]
        m.color[:] = r[0:3].tolist()
        m.transmission, m.thin, m.trdepth = float(r[3]), int(r[4] != 0), float(r[5])
        m.scattering[:] = r[6:9].tolist()
        m.scanisotropy = float(r[9])
        m.opacity, m.ior, m.roughness = 1.0, 1.5, 1.0
    return arr


_SIGS = {
    "yh_create": (C.c_void_p, [C.c_int]),
    "yh_destroy": (None, [C.c_void_p]),
    "yh_last_error": (C.c_char_p, [C.c_void_p]),
    "yh_version": (C.c_char_p, []),
    "yh_upload_scene": (C.c_int, [C.c_void_p, C.POINTER(SceneDesc)]),
    "yh_upload_scene_maps": (C.c_int, [C.c_void_p, C.POINTER(SceneDesc), C.POINTER(MaterialMaps)]),
    "yh_update_camera": (C.c_int, [C.c_void_p, C.POINTER(Camera)]),
    "yh_update_materials": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Material)]),
    "yh_update_environments": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Environment)]),
    "yh_update_objects": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Object)]),
    "yh_update_shape": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Shape)]),
    "yh_update_shape_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Shape)]),
    "yh_refit_shape": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Shape)]),
    "yh_refit_shape_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Shape)]),
    "yh_shape_refit_growth": (C.c_int, [C.c_void_p, C.c_int, c_float_p]),
    "yh_shape_nodes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), c_int_p, c_int_p]),
    "yh_set_light_edits": (C.c_int, [C.c_void_p, C.c_int]),
    "yh_light_list": (C.c_int, [C.c_void_p, c_int_p, c_int_p, c_int_p, c_int_p, C.c_int]),
    "yh_triangle_cdf": (C.c_int, [C.c_int, c_float_p, C.c_int, c_int_p, c_float_p]),
    "yh_triangle_cdf_gpu": (C.c_int, [C.c_void_p, C.c_int, c_float_p, C.c_int, c_int_p, c_float_p]),
    "yh_download_display": (C.c_int, [C.c_void_p, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_uint8)]),
    "yh_init_state": (C.c_int, [C.c_void_p, C.POINTER(TraceParams)]),
    "yh_image_size": (C.c_int, [C.c_void_p, c_int_p, c_int_p]),
    "yh_set_shard": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "yh_trace_samples": (C.c_int, [C.c_void_p, C.c_int]),
    "yh_trace_samples_async": (C.c_int, [C.c_void_p, C.c_int]),
    "yh_synchronize": (C.c_int, [C.c_void_p]),
    "yh_download": (C.c_int, [C.c_void_p, c_float_p]),
    "yh_pack_tiles_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "yh_unpack_tiles_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "yh_gather_framebuffer": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, c_float_p]),
    "yh_shard_pixels": (C.c_int64, [C.c_void_p, C.c_int, C.c_int]),
    "yh_download_rng": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "yh_trace_gbuffer": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(GBuffer)]),
    "yh_trace_gbuffer_device": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(GBuffer)]),
    "yh_denoise_default_params": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams)]),
    "yh_denoise_image_device": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.c_void_p, C.POINTER(GBuffer), C.c_void_p]),
    "yh_denoise": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), c_float_p, c_float_p]),
    "yh_denoise_display": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.c_float, C.c_int, C.c_int, C.POINTER(C.c_uint8)]),
    "yh_atrous_filter": (C.c_int, [C.c_int, C.c_int, C.POINTER(DenoiseParams), c_float_p, c_int_p, c_float_p, c_float_p, c_float_p, c_float_p]),
    "yh_atrous_filter_gpu": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(DenoiseParams), c_float_p, c_int_p, c_float_p, c_float_p,
                                       c_float_p, c_float_p]),
    "yh_atrous_level_ms": (C.c_int, [C.c_void_p, c_float_p, C.c_int]),
    "yh_temporal_default_params": (C.c_int, [C.c_void_p, C.POINTER(TemporalParams)]),
    "yh_temporal_accumulate_device": (C.c_int, [C.c_void_p, C.POINTER(TemporalParams), C.c_void_p, C.c_int, C.POINTER(GBuffer), C.c_void_p]),
    "yh_temporal_accumulate": (C.c_int, [C.c_void_p, C.POINTER(TemporalParams), c_float_p, C.c_int, C.POINTER(GBuffer), c_float_p]),
    "yh_temporal_display": (C.c_int, [C.c_void_p, C.POINTER(TemporalParams), C.POINTER(DenoiseParams), C.c_float, C.c_int, C.c_int, C.POINTER(C.c_uint8)]),
    "yh_temporal_reset": (C.c_int, [C.c_void_p]),
    "yh_temporal_lengths": (C.c_int, [C.c_void_p, c_int_p]),
    "yh_reproject": (C.c_int, [C.c_int, C.c_int, C.POINTER(TemporalParams), c_float_p, C.c_int, c_int_p, c_float_p, c_float_p, c_int_p, c_int_p, c_float_p,
                               C.POINTER(Camera), C.POINTER(Camera), C.c_int, c_float_p, c_float_p, c_int_p, c_float_p, c_int_p]),
    "yh_reproject_gpu": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(TemporalParams), c_float_p, C.c_int, c_int_p, c_float_p, c_float_p, c_int_p, c_int_p,
                                   c_float_p, C.POINTER(Camera), C.POINTER(Camera), C.c_int, c_float_p, c_float_p, c_int_p, c_float_p, c_int_p]),
    "yh_variance_default_params": (C.c_int, [C.c_void_p, C.POINTER(VarianceParams)]),
    "yh_temporal_accumulate_variance_device": (C.c_int, [C.c_void_p, C.POINTER(TemporalParams), C.POINTER(VarianceParams), C.c_void_p, C.c_int, C.POINTER(GBuffer),
                                                         C.c_void_p, C.c_void_p]),
    "yh_temporal_accumulate_variance": (C.c_int, [C.c_void_p, C.POINTER(TemporalParams), C.POINTER(VarianceParams), c_float_p, C.c_int, C.POINTER(GBuffer),
                                                  c_float_p, c_float_p]),
    "yh_denoise_variance_image_device": (C.c_int, [C.c_void_p, C.POINTER(VarianceParams), C.c_void_p, C.c_void_p, C.POINTER(GBuffer), C.c_void_p, C.c_void_p]),
    "yh_denoise_variance_image": (C.c_int, [C.c_void_p, C.POINTER(VarianceParams), c_float_p, c_float_p, C.POINTER(GBuffer), c_float_p, c_float_p]),
    "yh_svgf_display": (C.c_int, [C.c_void_p, C.POINTER(TemporalParams), C.POINTER(VarianceParams), C.c_float, C.c_int, C.c_int, C.POINTER(C.c_uint8)]),
    "yh_temporal_steps": (C.c_int, [C.c_void_p, c_int_p]),
    "yh_reproject_moments": (C.c_int, [C.c_int, C.c_int, C.POINTER(TemporalParams), c_float_p, C.c_int, c_int_p, c_float_p, c_float_p, c_float_p, c_int_p, c_int_p,
                                       c_float_p, c_float_p, c_int_p, C.POINTER(Camera), C.POINTER(Camera), C.c_int, c_float_p, c_float_p, c_int_p, c_float_p, c_int_p,
                                       c_float_p, c_int_p]),
    "yh_reproject_moments_gpu": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(TemporalParams), c_float_p, C.c_int, c_int_p, c_float_p, c_float_p, c_float_p, c_int_p,
                                           c_int_p, c_float_p, c_float_p, c_int_p, C.POINTER(Camera), C.POINTER(Camera), C.c_int, c_float_p, c_float_p, c_int_p, c_float_p,
                                           c_int_p, c_float_p, c_int_p]),
    "yh_variance_spatial": (C.c_int, [C.c_int, C.c_int, C.POINTER(TemporalParams), C.c_int, c_float_p, c_int_p, c_int_p, c_float_p, c_float_p]),
    "yh_variance_spatial_gpu": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(TemporalParams), C.c_int, c_float_p, c_int_p, c_int_p, c_float_p, c_float_p]),
    "yh_atrous_variance_filter": (C.c_int, [C.c_int, C.c_int, C.POINTER(VarianceParams), c_float_p, c_float_p, c_int_p, c_float_p, c_float_p, c_float_p, c_float_p,
                                            c_float_p]),
    "yh_atrous_variance_filter_gpu": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(VarianceParams), c_float_p, c_float_p, c_int_p, c_float_p, c_float_p,
                                                c_float_p, c_float_p, c_float_p]),
    "yh_trace_samples_counted": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(WorkCounts)]),
    "yh_last_trace_ms": (C.c_int, [C.c_void_p, c_float_p, c_int_p]),
    "yh_launch_shape": (C.c_int, [C.c_void_p]),
    "yh_tile_costs": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int]),
    "yh_item_costs": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int]),
    "yh_kernel_trials": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int]),
    "yh_trials_pending": (C.c_int, [C.c_void_p]),
    "yh_set_trial_cache_dir": (C.c_int, [C.c_char_p]),
    "yh_default_trial_cache_dir": (C.c_char_p, []),
    "yh_hair_brdf_batch": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Material), c_float_p,
                                     c_float_p, c_float_p, c_float_p]),
    "yh_curves_to_lines": (C.c_int, [C.c_void_p, C.c_int, c_float_p, c_float_p, c_float_p, C.c_int, c_float_p,
                                     c_float_p, c_float_p, c_int_p]),
    "yh_bvh_build_gpu": (C.c_int, [C.c_void_p, C.c_int, c_float_p, c_float_p, c_int_p]),
    "yh_bvh_build": (C.c_int, [C.c_int, c_float_p, c_float_p, c_int_p]),
    "yh_bvh_build_wide": (C.c_int, [C.c_int, c_float_p, C.c_int, c_float_p]),
    "yh_bvh_build_wide_gpu": (C.c_int, [C.c_void_p, C.c_int, c_float_p, C.c_int, c_float_p]),
    "yh_bvh_refit_wide": (C.c_int, [C.c_int, c_float_p, c_int_p, C.c_int, c_float_p]),
    "yh_bvh_refit_wide_gpu": (C.c_int, [C.c_void_p, C.c_int, c_float_p, c_int_p, C.c_int, c_float_p]),
    "yh_surface_lobe_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p, c_float_p, c_float_p, c_float_p,
                                        c_float_p, c_float_p]),
    "yh_surface_bsdf_batch": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Material), c_float_p, c_float_p, c_float_p,
                                        c_float_p, c_float_p]),
    "yh_hair_eval_batch": (C.c_int, [C.c_void_p, C.c_int, c_float_p, c_float_p, c_float_p, c_float_p]),
    "yh_hair_sample_batch": (C.c_int, [C.c_void_p, C.c_int, c_float_p, c_float_p, c_float_p, c_float_p]),
    "yh_hair_pdf_batch": (C.c_int, [C.c_void_p, C.c_int, c_float_p, c_float_p, c_float_p, c_float_p]),
    "yh_hair_eval_pdf_batch": (C.c_int, [C.c_void_p, C.c_int, c_float_p, c_float_p, c_float_p, c_float_p]),
    "yh_hair_shade_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Material), c_float_p, c_float_p, c_float_p,
                                      c_float_p, c_float_p, c_float_p, c_float_p]),
    "yh_intersect_batch": (C.c_int, [C.c_void_p, C.c_int, c_float_p, c_int_p, c_int_p, c_float_p, c_float_p]),
    "yh_intersect_plain_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p, c_int_p, c_int_p, c_float_p, c_float_p]),
    "yh_intersect_plain_form": (C.c_int, [C.c_int]),
    "yh_scene_once": (C.c_int, [C.c_void_p]),
    "yh_lights_const_env": (C.c_int, [C.c_void_p]),
    "yh_shade_regions": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]),
    "yh_set_count_bound": (C.c_int, [C.c_void_p, C.c_int]),
    "yh_lights_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_float_p, c_float_p, c_float_p, c_float_p]),
    "yh_volume_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(Material), c_float_p, c_float_p, c_float_p, c_float_p,
                                  c_float_p, c_float_p]),
    "yh_point_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_int_p, c_int_p, c_float_p, c_float_p, c_float_p]),
    "yh_quad_forms_batch": (C.c_int, [C.c_void_p, C.c_int, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p]),
    "yh_path_ends_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_float_p, c_int_p, C.POINTER(C.c_uint64), c_float_p, c_int_p,
                                     C.POINTER(C.c_uint64)]),
    "yh_selftest": (C.c_int, [C.c_void_p, C.c_int, c_float_p]),
    "yh_scene_load": (C.c_void_p, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]),
    "yh_scene_get": (C.POINTER(SceneDesc), [C.c_void_p]),
    "yh_scene_get_maps": (C.POINTER(MaterialMaps), [C.c_void_p]),
    "yh_scene_free": (None, [C.c_void_p]),
    "yh_save_image": (C.c_int, [C.c_char_p, C.c_int, C.c_int, c_float_p, C.c_char_p, C.c_int]),
}
EXPORTS = tuple(_SIGS)

_lib = None


def load(path=None):
    """Loads libyhair.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is None or path:
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise RuntimeError(f"{p} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback for the product path)")
        lib = C.CDLL(p)
        for name, (res, args) in _SIGS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                if "YHAIR_LIB" in os.environ:  # developer A/B against an older build (tools/_ab/): it may lack newer entry points
                    continue
                raise
            fn.restype, fn.argtypes = res, args
        if path:
            return lib
        _lib = lib
    return _lib


class YhError(RuntimeError):
    pass


def _refit_args(boxes, primitives, slots):
    return (np.ascontiguousarray(boxes, np.float32).reshape(-1, 6), np.ascontiguousarray(primitives, np.int32),
            np.array(slots, np.float32, copy=True, order="C"))


def bvh_refit_wide(boxes, primitives, width, slots):
    """yh_bvh_refit_wide (host, no GPU): arguments and result as Context.bvh_refit_wide_gpu."""
    boxes, primitives, out = _refit_args(boxes, primitives, slots)
    n = load().yh_bvh_refit_wide(len(boxes), fptr(boxes), iptr(primitives), width, fptr(out))
    if n < 0:
        raise YhError(f"yhair error {n}: yh_bvh_refit_wide")
    return n, out


def _cdf_args(positions, triangles):
    positions = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    triangles = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    return positions, triangles, np.zeros(len(triangles), np.float32)


def triangle_cdf(positions, triangles):
    """yh_triangle_cdf (host, no GPU): the area cdf of a triangle shape, one float32 chain in element order."""
    positions, triangles, out = _cdf_args(positions, triangles)
    rc = load().yh_triangle_cdf(len(positions), fptr(positions), len(triangles), iptr(triangles), fptr(out))
    if rc != YH_OK:
        raise YhError(f"yhair error {rc}: yh_triangle_cdf")
    return out


def denoise_default_params(ctx=None):
    """yh_denoise_default_params: the defaults, sigma_position from the scene `ctx` (a Context) has uploaded, 0 without one."""
    p = DenoiseParams()
    rc = load().yh_denoise_default_params(ctx.h if ctx is not None else None, C.byref(p))
    if rc != YH_OK:
        raise YhError(f"yhair error {rc}: yh_denoise_default_params")
    return p


def _filter_args(rgba, object, normal, position, albedo):
    rgba = np.ascontiguousarray(rgba, np.float32)
    h, w = rgba.shape[:2]
    object = np.ascontiguousarray(object, np.int32) if object is not None else None
    planes = [np.ascontiguousarray(a, np.float32) if a is not None else None for a in (normal, position, albedo)]
    assert rgba.shape == (h, w, 4) and (object is None or object.shape == (h, w)) and all(a is None or a.shape == (h, w, 3) for a in planes)
    held = [rgba, object] + planes
    ptrs = [fptr(rgba), iptr(object) if object is not None else None] + [fptr(a) if a is not None else None for a in planes]
    return w, h, held, ptrs, np.zeros((h, w, 4), np.float32)


def atrous_filter(params, rgba, object, normal=None, position=None, albedo=None):
    """yh_atrous_filter (host, no GPU): the a-trous filter of yh_denoise on (H, W, 4) rgba, (H, W) object ids and (H, W, 3) planes."""
    w, h, held, ptrs, out = _filter_args(rgba, object, normal, position, albedo)
    rc = load().yh_atrous_filter(w, h, C.byref(params), *ptrs, fptr(out))
    if rc != YH_OK:
        raise YhError(f"yhair error {rc}: yh_atrous_filter")
    return out


def temporal_default_params(ctx=None):
    """yh_temporal_default_params: the defaults, sigma_position from the scene `ctx` (a Context) has uploaded, 0 without one."""
    p = TemporalParams()
    rc = load().yh_temporal_default_params(ctx.h if ctx is not None else None, C.byref(p))
    if rc != YH_OK:
        raise YhError(f"yhair error {rc}: yh_temporal_default_params")
    return p


def camera_of(floats17):
    """A Camera from the 17 floats frame (12), lens, film (2), focus, aperture."""
    a = np.ascontiguousarray(floats17, np.float32).reshape(17)
    return Camera.from_buffer_copy(a.tobytes())


def _reproject_args(rgba, samples, object, position, history, camera, prev_camera, frames, prev_frames, usable):
    """The arguments of yh_reproject after (w, h, params): history = None or (rgba, length, object, position) of the previous step;
    cameras = Camera or 17 floats; frames / prev_frames (n, 12) or None; usable (n,) or None."""
    rgba = np.ascontiguousarray(rgba, np.float32)
    h, w = rgba.shape[:2]
    object, position = np.ascontiguousarray(object, np.int32), np.ascontiguousarray(position, np.float32)
    assert rgba.shape == (h, w, 4) and object.shape == (h, w) and position.shape == (h, w, 3)
    held = [rgba, object, position]
    hist = [None] * 4
    if history is not None:
        hr, hl, ho, hp = history
        hist = [np.ascontiguousarray(hr, np.float32), np.ascontiguousarray(hl, np.int32), np.ascontiguousarray(ho, np.int32), np.ascontiguousarray(hp, np.float32)]
        assert hist[0].shape == (h, w, 4) and hist[1].shape == (h, w) and hist[2].shape == (h, w) and hist[3].shape == (h, w, 3)
    cams = [c if isinstance(c, Camera) or c is None else camera_of(c) for c in (camera, prev_camera)]
    n = 0
    fr = [None, None]
    if frames is not None:
        prev_frames = prev_frames if prev_frames is not None else frames  # (without a history they are not read)
        fr = [np.ascontiguousarray(frames, np.float32).reshape(-1, 12), np.ascontiguousarray(prev_frames, np.float32).reshape(-1, 12)]
        n = len(fr[0])
        assert fr[1].shape == fr[0].shape
    use = np.ascontiguousarray(usable, np.int32) if usable is not None else None
    assert use is None or use.shape == (n,)
    held += hist + cams + fr + [use]
    out, length = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.int32)
    opt = lambda a, f: f(a) if a is not None else None  # noqa: E731
    args = [fptr(rgba), int(samples), iptr(object), fptr(position), opt(hist[0], fptr), opt(hist[1], iptr), opt(hist[2], iptr), opt(hist[3], fptr),
            opt(cams[0], C.byref), opt(cams[1], C.byref), n, opt(fr[0], fptr), opt(fr[1], fptr), opt(use, iptr), fptr(out), iptr(length)]
    return w, h, held, args, out, length


def reproject(params, rgba, samples, object, position, history, camera, prev_camera=None, frames=None, prev_frames=None, usable=None):
    """yh_reproject (host, no GPU): one step of the temporal stage; returns (out_rgba, out_length), which with `object` and `position`
    are the next step's `history`."""
    w, h, held, args, out, length = _reproject_args(rgba, samples, object, position, history, camera, prev_camera, frames, prev_frames, usable)
    rc = load().yh_reproject(w, h, C.byref(params) if params is not None else None, *args)
    if rc != YH_OK:
        raise YhError(f"yhair error {rc}: yh_reproject")
    return out, length


# the variance stage (include/yhair.h: VARIANCE)
def variance_default_params(ctx=None):
    """yh_variance_default_params: the defaults, sigma_position from the scene `ctx` (a Context) has uploaded, 0 without one."""
    p = VarianceParams()
    rc = load().yh_variance_default_params(ctx.h if ctx is not None else None, C.byref(p))
    if rc != YH_OK:
        raise YhError(f"yhair error {rc}: yh_variance_default_params")
    return p


def _moment_args(rgba, samples, object, position, albedo, history, moment_history, camera, prev_camera, frames, prev_frames, usable):
    """The arguments of yh_reproject_moments after (w, h, params): _reproject_args' with albedo (H, W, 3) or None and
    moment_history = None or (moments (H, W, 2), steps (H, W)) of the previous step."""
    w, h, held, a, out, length = _reproject_args(rgba, samples, object, position, history, camera, prev_camera, frames, prev_frames, usable)
    albedo = np.ascontiguousarray(albedo, np.float32) if albedo is not None else None
    hm = [None, None]
    if moment_history is not None:
        hm = [np.ascontiguousarray(moment_history[0], np.float32), np.ascontiguousarray(moment_history[1], np.int32)]
        assert hm[0].shape == (h, w, 2) and hm[1].shape == (h, w)
    assert albedo is None or albedo.shape == (h, w, 3)
    moments, steps = np.zeros((h, w, 2), np.float32), np.zeros((h, w), np.int32)
    held += [albedo] + hm
    opt = lambda x, f: f(x) if x is not None else None  # noqa: E731
    args = a[:4] + [opt(albedo, fptr)] + a[4:8] + [opt(hm[0], fptr), opt(hm[1], iptr)] + a[8:] + [fptr(moments), iptr(steps)]
    return w, h, held, args, (out, length, moments, steps)


def reproject_moments(params, rgba, samples, object, position, albedo, history, moment_history, camera, prev_camera=None, frames=None, prev_frames=None,
                      usable=None):
    """yh_reproject_moments (host, no GPU): stage M; returns (out_rgba, out_length, out_moments, out_steps)."""
    w, h, held, args, outs = _moment_args(rgba, samples, object, position, albedo, history, moment_history, camera, prev_camera, frames, prev_frames, usable)
    rc = load().yh_reproject_moments(w, h, C.byref(params) if params is not None else None, *args)
    if rc != YH_OK:
        raise YhError(f"yhair error {rc}: yh_reproject_moments")
    return outs


def _spatial_args(moments, steps, object, position):
    moments, steps = np.ascontiguousarray(moments, np.float32), np.ascontiguousarray(steps, np.int32)
    object, position = np.ascontiguousarray(object, np.int32), np.ascontiguousarray(position, np.float32)
    h, w = steps.shape
    assert moments.shape == (h, w, 2) and object.shape == (h, w) and position.shape == (h, w, 3)
    out = np.zeros((h, w), np.float32)
    return w, h, [moments, steps, object, position], [fptr(moments), iptr(steps), iptr(object), fptr(position), fptr(out)], out


def variance_spatial(temporal_params, min_steps, moments, steps, object, position):
    """yh_variance_spatial (host, no GPU): stage S over a step's moments and steps; returns the (H, W) variance."""
    w, h, held, ptrs, out = _spatial_args(moments, steps, object, position)
    rc = load().yh_variance_spatial(w, h, C.byref(temporal_params), int(min_steps), *ptrs)
    if rc != YH_OK:
        raise YhError(f"yhair error {rc}: yh_variance_spatial")
    return out


def _vfilter_args(rgba, variance, object, normal, position, albedo):
    w, h, held, ptrs, out = _filter_args(rgba, object, normal, position, albedo)
    variance = np.ascontiguousarray(variance, np.float32)
    assert variance.shape == (h, w)
    out_variance = np.zeros((h, w), np.float32)
    return w, h, held + [variance], ptrs[:1] + [fptr(variance)] + ptrs[1:] + [fptr(out), fptr(out_variance)], (out, out_variance)


def atrous_variance_filter(params, rgba, variance, object, normal=None, position=None, albedo=None):
    """yh_atrous_variance_filter (host, no GPU): stage F; returns (out (H, W, 4), out_variance (H, W))."""
    w, h, held, ptrs, outs = _vfilter_args(rgba, variance, object, normal, position, albedo)
    rc = load().yh_atrous_variance_filter(w, h, C.byref(params), *ptrs)
    if rc != YH_OK:
        raise YhError(f"yhair error {rc}: yh_atrous_variance_filter")
    return outs


def set_trial_cache_dir(path=None, default=False):
    """yh_set_trial_cache_dir: opt in to the kernel-trial record on disk (process-wide). default=True: the directory the
    command lines use ($XDG_CACHE_HOME/yhair or ~/.cache/yhair); path=None without default: no file."""
    lib = load()
    if not hasattr(lib, "yh_set_trial_cache_dir"):  # an older developer build (YHAIR_LIB)
        return None
    d = lib.yh_default_trial_cache_dir() if default else (path.encode() if path else None)
    lib.yh_set_trial_cache_dir(d)
    return d.decode() if d else None


class SceneFile:
    """yh_scene_load / yh_scene_get / yh_scene_free."""

    def __init__(self, json_path, camera=""):
        lib = load()
        err = C.create_string_buffer(512)
        self.handle = lib.yh_scene_load(str(json_path).encode(), camera.encode(), err, 512)
        if not self.handle:
            raise YhError(err.value.decode())
        self.desc = lib.yh_scene_get(self.handle)
        # yh_scene_get_maps: one MaterialMaps per material (index it like desc.contents.materials)
        self.maps = lib.yh_scene_get_maps(self.handle)

    def close(self):
        if self.handle and load is not None:
            load().yh_scene_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass


def gather_framebuffer(contexts):
    """yh_gather_framebuffer: the full (H, W, 4) image of `contexts`, context i holding shard (i, len(contexts))."""
    lib = load()
    w, h = C.c_int(), C.c_int()
    contexts[0]._chk(lib.yh_image_size(contexts[0].h, C.byref(w), C.byref(h)))
    img = np.zeros((h.value, w.value, 4), np.float32)
    arr = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
    contexts[0]._chk(lib.yh_gather_framebuffer(arr, len(contexts), fptr(img)))
    return img


class Context:
    """One GPU context (yh_create ... yh_destroy). Raises when no GPU: no fallback."""

    def __init__(self, device=0):
        self.lib = load()
        self.h = self.lib.yh_create(device)
        if not self.h:
            raise YhError("yh_create failed: " + self.lib.yh_last_error(None).decode())

    def _chk(self, rc):
        if rc != YH_OK:
            raise YhError(f"yhair error {rc}: " + self.lib.yh_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.lib.yh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # whole path -----------------------------------------------------------
    def upload_scene(self, desc, maps=None):
        """yh_upload_scene, or yh_upload_scene_maps with `maps`: one MaterialMaps per material (a ctypes array or pointer,
        e.g. SceneFile.maps)."""
        if maps is None:
            self._chk(self.lib.yh_upload_scene(self.h, desc))
        else:
            self._chk(self.lib.yh_upload_scene_maps(self.h, desc, C.cast(maps, C.POINTER(MaterialMaps))))

    # edits of the uploaded scene that keep its shapes' trees (include/yhair.h): the image state is gone afterwards, call init_state again
    def update_camera(self, camera):
        """yh_update_camera: `camera` is a Camera (e.g. a copy of desc.contents.camera with fields changed)."""
        self._chk(self.lib.yh_update_camera(self.h, C.byref(camera) if camera is not None else None))

    def update_materials(self, first, materials):
        """yh_update_materials: rows [first, first + len(materials)) of the material table; `materials` is a ctypes array of
        Material, or a list of them."""
        if materials is not None and not isinstance(materials, C.Array):
            materials = (Material * len(materials))(*materials)
        self._chk(self.lib.yh_update_materials(self.h, first, len(materials) if materials is not None else 0, materials))

    def update_objects(self, first, objects):
        """yh_update_objects: rows [first, first + len(objects)) of the object list (frame and material; the shape stays); `objects`
        is a ctypes array of Object, or a list of them."""
        if objects is not None and not isinstance(objects, C.Array):
            objects = (Object * len(objects))(*objects)
        self._chk(self.lib.yh_update_objects(self.h, first, len(objects) if objects is not None else 0, objects))

    # vertex edits of one shape: its tree, records and nodes are made again, and the scene level; no other shape is touched
    def update_shape(self, index, shape):
        """yh_update_shape: `shape` is a Shape with HOST arrays and the uploaded shape's counts (e.g. a copy of
        desc.contents.shapes[index] with its pointers set to edited float32 / int32 numpy arrays, which the caller keeps alive)."""
        self._chk(self.lib.yh_update_shape(self.h, index, C.byref(shape) if shape is not None else None))

    @staticmethod
    def _device_shape(who, positions, normals, radius, lines, triangles, texcoords):
        """The Shape of the device forms: contiguous torch tensors on the context's device, checked; the current torch stream is
        synchronised, since the calls run on the context's own stream."""
        import torch

        def ptr(t, dtype, cols, what):
            if t is None:
                return None
            if not isinstance(t, torch.Tensor):
                raise YhError(f"{who}: {what} must be a torch tensor, not {type(t).__name__}")
            if not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or (cols and (t.dim() != 2 or t.shape[1] != cols)) or (not cols and t.dim() != 1):
                raise YhError(f"{who}: {what} must be a contiguous {dtype} tensor on the GPU" + (f" of shape (n, {cols})" if cols else " of shape (n,)"))
            return t.data_ptr()

        if positions is None:
            raise YhError(f"{who}: positions is None")
        s = Shape()
        s.positions = C.cast(ptr(positions, torch.float32, 3, "positions"), c_float_p)
        s.num_vertices = int(positions.shape[0])
        s.normals = C.cast(ptr(normals, torch.float32, 3, "normals"), c_float_p)
        s.radius = C.cast(ptr(radius, torch.float32, 0, "radius"), c_float_p)
        s.texcoords = C.cast(ptr(texcoords, torch.float32, 2, "texcoords"), c_float_p)
        s.lines = C.cast(ptr(lines, torch.int32, 2, "lines"), c_int_p)
        s.num_lines = int(lines.shape[0]) if lines is not None else 0
        s.triangles = C.cast(ptr(triangles, torch.int32, 3, "triangles"), c_int_p)
        s.num_triangles = int(triangles.shape[0]) if triangles is not None else 0
        torch.cuda.current_stream(positions.device).synchronize()
        return s

    def update_shape_device(self, index, positions, normals=None, radius=None, lines=None, triangles=None, texcoords=None):
        """yh_update_shape_device: contiguous torch tensors on the context's device — positions (n, 3), normals (n, 3), radius (n,),
        texcoords (n, 2) float32; lines (m, 2) or triangles (m, 3) int32. The current torch stream is synchronised before the call,
        which runs on the context's own stream."""
        s = self._device_shape("update_shape_device", positions, normals, radius, lines, triangles, texcoords)
        self._chk(self.lib.yh_update_shape_device(self.h, index, C.byref(s)))

    # the same edits kept in the tree the shape has: records and boxes again, nothing built (include/yhair.h: REFIT)
    def refit_shape(self, index, shape):
        """yh_refit_shape: arguments as update_shape."""
        self._chk(self.lib.yh_refit_shape(self.h, index, C.byref(shape) if shape is not None else None))

    def refit_shape_device(self, index, positions, normals=None, radius=None, lines=None, triangles=None, texcoords=None):
        """yh_refit_shape_device: arguments as update_shape_device."""
        s = self._device_shape("refit_shape_device", positions, normals, radius, lines, triangles, texcoords)
        self._chk(self.lib.yh_refit_shape_device(self.h, index, C.byref(s)))

    def shape_refit_growth(self, index):
        """yh_shape_refit_growth: for the 4-, 8- and 16-wide nodes of the shape, the half-area sum of their slot boxes now over the
        sum at the shape's last build (exactly 1.0 after an upload, an update and a refit that reproduces the boxes)."""
        g = (C.c_float * 3)()
        rc = self.lib.yh_shape_refit_growth(self.h, index, g)
        if rc != YH_OK:
            raise YhError(f"yhair error {rc}: yh_shape_refit_growth")
        return [float(v) for v in g]

    def shape_nodes(self, index):
        """yh_shape_nodes: (offsets, counts, room) of the shape's 4-, 8- and 16-wide nodes in the traversal array (32-byte units)."""
        off, cnt, room = (C.c_int64 * 3)(), (C.c_int * 3)(), (C.c_int * 3)()
        self._chk(self.lib.yh_shape_nodes(self.h, index, off, cnt, room))
        return list(off), list(cnt), list(room)

    # light edits (include/yhair.h: LIGHT EDITS): with the opt-in, the edits above make the light list again instead of refusing
    def set_light_edits(self, on=True):
        """yh_set_light_edits: emission toggles, an emitter's material on another object and vertex edits of an emitter's shape go
        through the update / refit calls (off by default)."""
        self._chk(self.lib.yh_set_light_edits(self.h, int(bool(on))))

    def light_list(self):
        """yh_light_list: [(object or -1, environment or -1, cdf entries, in the LDS light table)] in the kernels' order."""
        a = [(C.c_int * 16)() for _ in range(4)]
        n = self.lib.yh_light_list(self.h, *a, 16)
        self._chk(min(n, 0))
        return [(a[0][i], a[1][i], a[2][i], bool(a[3][i])) for i in range(n)]

    def triangle_cdf_gpu(self, positions, triangles):
        """yh_triangle_cdf_gpu: triangle_cdf by the kernel of the light edits (one wave, the sums one chain in element order)."""
        positions, triangles, out = _cdf_args(positions, triangles)
        self._chk(self.lib.yh_triangle_cdf_gpu(self.h, len(positions), fptr(positions), len(triangles), iptr(triangles), fptr(out)))
        return out

    def update_environments(self, environments):
        """yh_update_environments: frame and emission of every environment (a ctypes array of Environment, or a list)."""
        if environments is not None and not isinstance(environments, C.Array):
            environments = (Environment * len(environments))(*environments)
        self._chk(self.lib.yh_update_environments(self.h, len(environments) if environments is not None else 0, environments))

    def set_shard(self, rank, world):
        self._chk(self.lib.yh_set_shard(self.h, rank, world))

    def init_state(self, params):
        self._chk(self.lib.yh_init_state(self.h, C.byref(params)))
        w, h = C.c_int(), C.c_int()
        self._chk(self.lib.yh_image_size(self.h, C.byref(w), C.byref(h)))
        self.width, self.height = w.value, h.value
        return self.width, self.height

    def trace_samples(self, n):
        self._chk(self.lib.yh_trace_samples(self.h, n))

    def trace_samples_async(self, n):
        self._chk(self.lib.yh_trace_samples_async(self.h, n))

    def synchronize(self):
        self._chk(self.lib.yh_synchronize(self.h))

    def trace_samples_counted(self, n):
        wc = WorkCounts()
        self._chk(self.lib.yh_trace_samples_counted(self.h, n, C.byref(wc)))
        return wc

    def launch_shape(self):
        """The sample-loop kernel of the most recent launch (include/yhair.h: yh_launch_shape)."""
        return int(self.lib.yh_launch_shape(self.h))

    def last_trace_ms(self):
        ms, n = C.c_float(), C.c_int()
        self._chk(self.lib.yh_last_trace_ms(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def tile_costs(self):
        tx, ty = (self.width + 7) // 8, (self.height + 7) // 8
        out = np.zeros(tx * ty, np.uint32)
        self._chk(self.lib.yh_tile_costs(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32)), len(out)))
        return out.reshape(ty, tx)

    def kernel_trials(self):
        """{launch shape: (ms per sample of its fastest trial, number of trials)} for the shapes tried on this image."""
        ms, tr = (C.c_double * 16)(), (C.c_int * 16)()
        n = self.lib.yh_kernel_trials(self.h, ms, tr, 16)
        self._chk(min(n, 0))
        return {k: (round(ms[k], 5), tr[k]) for k in range(min(n, 16)) if tr[k] or ms[k]}

    def trials_pending(self):
        """True while a candidate kernel of this image still wants a 32-sample timing trial (include/yhair.h)."""
        n = self.lib.yh_trials_pending(self.h)
        self._chk(min(n, 0))
        return n > 0

    def item_costs(self):
        """Per work item (tile * 4 + quadrant) cost of the most recent launch."""
        w, h = C.c_int(), C.c_int()
        self._chk(self.lib.yh_image_size(self.h, C.byref(w), C.byref(h)))
        n = ((w.value + 7) // 8) * ((h.value + 7) // 8) * 4
        out = np.zeros(n, np.uint32)
        self._chk(self.lib.yh_item_costs(self.h, out.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return out

    def download(self):
        img = np.zeros((self.height, self.width, 4), np.float32)
        self._chk(self.lib.yh_download(self.h, fptr(img)))
        return img

    def download_display(self, exposure=0.0, filmic=False, srgb=True):
        """yh_download_display: the tone-mapped image as (H, W, 4) bytes, made on the device."""
        img = np.zeros((self.height, self.width, 4), np.uint8)
        self._chk(self.lib.yh_download_display(self.h, exposure, int(filmic), int(srgb), img.ctypes.data_as(C.POINTER(C.c_uint8))))
        return img

    def download_rng(self):
        rng = np.zeros((self.height * self.width, 2), np.uint64)
        self._chk(self.lib.yh_download_rng(self.h, rng.ctypes.data_as(C.POINTER(C.c_uint64))))
        return rng

    # the first-hit feature pass (include/yhair.h: yh_trace_gbuffer)
    def trace_gbuffer(self, mode=GBUFFER_CENTRE, planes=None):
        """yh_trace_gbuffer: a dict of numpy arrays, (H, W) or (H, W, components), for the planes named in `planes` (default: all of
        GBUFFER_PLANES). mode: GBUFFER_CENTRE / GBUFFER_NEXT_SAMPLE, or "centre" / "next"."""
        mode = GBUFFER_MODES.get(mode, mode)
        names = [n for n, _, _ in GBUFFER_PLANES] if planes is None else list(planes)
        g, out = GBuffer(), {}
        h, w = getattr(self, "height", 0), getattr(self, "width", 0)  # (before init_state: the call itself refuses)
        for n, t, c in GBUFFER_PLANES:
            if n in names:
                out[n] = np.zeros((h, w) + ((c,) if c > 1 else ()), t)
                setattr(g, n, iptr(out[n]) if t is np.int32 else fptr(out[n]))
        if len(out) != len(names):
            raise YhError("trace_gbuffer: unknown plane among " + ", ".join(names))
        self._chk(self.lib.yh_trace_gbuffer(self.h, mode, C.byref(g)))
        return out

    def trace_gbuffer_device(self, mode=GBUFFER_CENTRE, **planes):
        """yh_trace_gbuffer_device: writes the planes given by name (GBUFFER_PLANES) into contiguous torch tensors on the context's
        device, int32 / float32 with at least height x width x components elements; nothing is copied. The current torch stream is
        synchronised before the call, which runs on the context's own stream and returns when the planes are written."""
        import torch
        mode = GBUFFER_MODES.get(mode, mode)
        kinds = {n: (t, c) for n, t, c in GBUFFER_PLANES}
        g, device = GBuffer(), None
        for n, t in planes.items():
            if n not in kinds:
                raise YhError(f"trace_gbuffer_device: unknown plane {n}")
            if t is None:
                continue
            dtype = torch.int32 if kinds[n][0] is np.int32 else torch.float32
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() \
                    or t.numel() < self.height * self.width * kinds[n][1]:
                raise YhError(f"trace_gbuffer_device: {n} must be a contiguous {dtype} tensor on the GPU of at least "
                              f"{self.height} x {self.width} x {kinds[n][1]} elements")
            setattr(g, n, C.cast(t.data_ptr(), c_int_p if dtype == torch.int32 else c_float_p))
            device = t.device
        if device is not None:
            torch.cuda.current_stream(device).synchronize()
        self._chk(self.lib.yh_trace_gbuffer_device(self.h, mode, C.byref(g)))

    # the denoiser (include/yhair.h: DENOISE)
    def denoise_default_params(self):
        return denoise_default_params(self)

    def denoise(self, params=None, rgba=None):
        """yh_denoise: the denoised (H, W, 4) image of `rgba` (None: the context's own render); params None: the defaults."""
        params = params if params is not None else self.denoise_default_params()
        rgba = np.ascontiguousarray(rgba, np.float32) if rgba is not None else None
        out = np.zeros((getattr(self, "height", 0), getattr(self, "width", 0), 4), np.float32)
        assert rgba is None or rgba.shape == out.shape
        self._chk(self.lib.yh_denoise(self.h, C.byref(params), fptr(rgba) if rgba is not None else None, fptr(out)))
        return out

    def denoise_display(self, params=None, exposure=0.0, filmic=False, srgb=True):
        """yh_denoise_display: the own render, denoised and tone-mapped on the device, as (H, W, 4) bytes."""
        params = params if params is not None else self.denoise_default_params()
        img = np.zeros((getattr(self, "height", 0), getattr(self, "width", 0), 4), np.uint8)
        self._chk(self.lib.yh_denoise_display(self.h, C.byref(params), exposure, int(filmic), int(srgb), img.ctypes.data_as(C.POINTER(C.c_uint8))))
        return img

    def denoise_image_device(self, params, rgba_out, rgba_in=None, **guides):
        """yh_denoise_image_device: contiguous float32 torch tensors of (H, W, 4) on the context's device (rgba_in None: the own
        render); guides: object / normal / position / albedo tensors as trace_gbuffer_device fills them, none: traced by the call.
        The current torch stream is synchronised before the call, which runs on the context's own stream."""
        import torch
        kinds = {n: (t, c) for n, t, c in GBUFFER_PLANES}
        npix = self.height * self.width

        def ptr(t, dtype, comps, what):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or t.numel() < npix * comps:
                raise YhError(f"denoise_image_device: {what} must be a contiguous {dtype} tensor on the GPU of at least {self.height} x {self.width} x {comps} elements")
            return t.data_ptr()
        out_p = ptr(rgba_out, torch.float32, 4, "rgba_out")
        in_p = ptr(rgba_in, torch.float32, 4, "rgba_in") if rgba_in is not None else None
        g = GBuffer()
        for n, t in guides.items():
            if n not in kinds:
                raise YhError(f"denoise_image_device: unknown plane {n}")
            if t is not None:
                dtype = torch.int32 if kinds[n][0] is np.int32 else torch.float32
                setattr(g, n, C.cast(ptr(t, dtype, kinds[n][1], n), c_int_p if dtype == torch.int32 else c_float_p))
        torch.cuda.current_stream(rgba_out.device).synchronize()
        self._chk(self.lib.yh_denoise_image_device(self.h, C.byref(params), in_p, C.byref(g) if guides else None, out_p))

    def atrous_filter_gpu(self, form, params, rgba, object, normal=None, position=None, albedo=None):
        """yh_atrous_filter_gpu: atrous_filter's arrays through the device kernels (form 0: taps from memory, 1: from an LDS tile)."""
        w, h, held, ptrs, out = _filter_args(rgba, object, normal, position, albedo)
        self._chk(self.lib.yh_atrous_filter_gpu(self.h, form, w, h, C.byref(params), *ptrs, fptr(out)))
        return out

    def atrous_level_ms(self):
        """yh_atrous_level_ms: the event times of the last atrous_filter_gpu: [pack, level 0, level 1, ...]."""
        ms = (C.c_float * (1 + DENOISE_MAX_ITERATIONS))()
        n = self.lib.yh_atrous_level_ms(self.h, ms, len(ms))
        return [float(ms[k]) for k in range(max(n, 0))]

    # the temporal stage (include/yhair.h: TEMPORAL)
    def temporal_default_params(self):
        return temporal_default_params(self)

    def _host_guides(self, object, position):
        if object is None and position is None:
            return None, []
        g, held = GBuffer(), []
        if object is not None:
            held.append(np.ascontiguousarray(object, np.int32))
            g.object = iptr(held[-1])
        if position is not None:
            held.append(np.ascontiguousarray(position, np.float32))
            g.position = fptr(held[-1])
        return g, held

    def temporal_accumulate(self, params=None, rgba=None, samples=0, object=None, position=None, want_image=True):
        """yh_temporal_accumulate: the (H, W, 4) image `rgba` with `samples` samples in it (None: the context's own render) blended
        with the reprojected history; object / position: centre-mode planes (neither: traced by the call). Returns the accumulated
        image, or None with want_image False (the history is only updated). params None: the defaults."""
        params = params if params is not None else self.temporal_default_params()
        rgba = np.ascontiguousarray(rgba, np.float32) if rgba is not None else None
        out = np.zeros((getattr(self, "height", 0), getattr(self, "width", 0), 4), np.float32) if want_image else None
        assert rgba is None or out is None or rgba.shape == out.shape
        g, held = self._host_guides(object, position)
        self._chk(self.lib.yh_temporal_accumulate(self.h, C.byref(params), fptr(rgba) if rgba is not None else None, int(samples),
                                                  C.byref(g) if g is not None else None, fptr(out) if out is not None else None))
        return out

    def temporal_accumulate_device(self, params, rgba_out=None, rgba_in=None, samples=0, object=None, position=None):
        """yh_temporal_accumulate_device: contiguous torch tensors on the context's device, float32 (H, W, 4) images (rgba_in None: the
        own render; rgba_out None: the history is only updated), int32 (H, W) object and float32 (H, W, 3) position as
        trace_gbuffer_device fills them (neither: traced by the call). The current torch stream is synchronised before the call."""
        import torch
        npix = self.height * self.width

        def ptr(t, dtype, comps, what):
            if t is None:
                return None
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or t.numel() < npix * comps:
                raise YhError(f"temporal_accumulate_device: {what} must be a contiguous {dtype} tensor on the GPU of at least {self.height} x {self.width} x {comps} elements")
            return t.data_ptr()
        out_p, in_p = ptr(rgba_out, torch.float32, 4, "rgba_out"), ptr(rgba_in, torch.float32, 4, "rgba_in")
        g = None
        if object is not None or position is not None:
            g = GBuffer()
            if object is not None:
                g.object = C.cast(ptr(object, torch.int32, 1, "object"), c_int_p)
            if position is not None:
                g.position = C.cast(ptr(position, torch.float32, 3, "position"), c_float_p)
        torch.cuda.synchronize()
        self._chk(self.lib.yh_temporal_accumulate_device(self.h, C.byref(params), in_p, int(samples), C.byref(g) if g is not None else None, out_p))

    def temporal_display(self, params=None, denoise_params=None, exposure=0.0, filmic=False, srgb=True):
        """yh_temporal_display: the own render accumulated, filtered with `denoise_params` (None: no filter) and tone-mapped on the
        device, as (H, W, 4) bytes."""
        params = params if params is not None else self.temporal_default_params()
        img = np.zeros((getattr(self, "height", 0), getattr(self, "width", 0), 4), np.uint8)
        self._chk(self.lib.yh_temporal_display(self.h, C.byref(params), C.byref(denoise_params) if denoise_params is not None else None, exposure,
                                               int(filmic), int(srgb), img.ctypes.data_as(C.POINTER(C.c_uint8))))
        return img

    def temporal_reset(self):
        self._chk(self.lib.yh_temporal_reset(self.h))

    def temporal_lengths(self):
        """yh_temporal_lengths: the history's lengths as an (H, W) int32 array, or None without a history."""
        n = self.lib.yh_temporal_lengths(self.h, None)
        self._chk(min(n, 0))
        if n == 0:
            return None
        out = np.zeros(n, np.int32)
        self._chk(min(self.lib.yh_temporal_lengths(self.h, iptr(out)), 0))
        return out.reshape(self.height, self.width) if n == getattr(self, "height", 0) * getattr(self, "width", 0) else out

    def reproject_gpu(self, params, rgba, samples, object, position, history, camera, prev_camera=None, frames=None, prev_frames=None, usable=None):
        """yh_reproject_gpu: reproject's arrays through the device kernel."""
        w, h, held, args, out, length = _reproject_args(rgba, samples, object, position, history, camera, prev_camera, frames, prev_frames, usable)
        self._chk(self.lib.yh_reproject_gpu(self.h, w, h, C.byref(params) if params is not None else None, *args))
        return out, length

    # the variance stage (include/yhair.h: VARIANCE)
    def variance_default_params(self):
        return variance_default_params(self)

    def _variance_guides(self, planes):
        """A GBuffer of host arrays from {name: array or None}; None when no plane is given."""
        kinds = {n: (t, c) for n, t, c in GBUFFER_PLANES}
        g, held = GBuffer(), []
        for n, a in planes.items():
            if a is not None:
                held.append(np.ascontiguousarray(a, kinds[n][0]))
                setattr(g, n, iptr(held[-1]) if kinds[n][0] is np.int32 else fptr(held[-1]))
        return (g, held) if held else (None, held)

    def temporal_accumulate_variance(self, params=None, variance_params=None, rgba=None, samples=0, object=None, position=None, albedo=None):
        """yh_temporal_accumulate_variance: temporal_accumulate with the moment history beside the colour's (stages M and S); returns
        (accumulated image (H, W, 4), variance (H, W)). object / position / albedo: centre-mode planes (none: traced by the call)."""
        params = params if params is not None else self.temporal_default_params()
        variance_params = variance_params if variance_params is not None else self.variance_default_params()
        rgba = np.ascontiguousarray(rgba, np.float32) if rgba is not None else None
        h, w = getattr(self, "height", 0), getattr(self, "width", 0)
        out, var = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.float32)
        assert rgba is None or rgba.shape == out.shape
        g, held = self._variance_guides(dict(object=object, position=position, albedo=albedo))
        self._chk(self.lib.yh_temporal_accumulate_variance(self.h, C.byref(params), C.byref(variance_params), fptr(rgba) if rgba is not None else None,
                                                           int(samples), C.byref(g) if g is not None else None, fptr(out), fptr(var)))
        return out, var

    def denoise_variance_image(self, variance_params, rgba, variance=None, **guides):
        """yh_denoise_variance_image: stage F over the (H, W, 4) image `rgba`; variance None: the one the context kept from its last
        temporal_accumulate_variance; guides: object / normal / position / albedo host planes, none: traced by the call. Returns
        (filtered image, filtered variance)."""
        rgba = np.ascontiguousarray(rgba, np.float32)
        variance = np.ascontiguousarray(variance, np.float32) if variance is not None else None
        out, var = np.zeros_like(rgba), np.zeros(rgba.shape[:2], np.float32)
        g, held = self._variance_guides(guides)
        self._chk(self.lib.yh_denoise_variance_image(self.h, C.byref(variance_params), fptr(rgba), fptr(variance) if variance is not None else None,
                                                     C.byref(g) if g is not None else None, fptr(out), fptr(var)))
        return out, var

    def _device_call(self, what, tensors):
        """data_ptr()s of contiguous torch tensors on the GPU (None stays None): {name: (tensor, dtype name, comps)}"""
        import torch
        npix, ptrs = self.height * self.width, {}
        for n, (t, dtype, comps) in tensors.items():
            dtype = getattr(torch, dtype)
            if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or t.numel() < npix * comps):
                raise YhError(f"{what}: {n} must be a contiguous {dtype} tensor on the GPU of at least {self.height} x {self.width} x {comps} elements")
            ptrs[n] = t.data_ptr() if t is not None else None
        torch.cuda.synchronize()
        return ptrs

    def _device_guides(self, ptrs, names):
        if all(ptrs[n] is None for n in names):
            return None
        g = GBuffer()
        for n in names:
            if ptrs[n] is not None:
                setattr(g, n, C.cast(ptrs[n], c_int_p if n == "object" else c_float_p))
        return g

    def temporal_accumulate_variance_device(self, params, variance_params, rgba_out=None, variance_out=None, rgba_in=None, samples=0, object=None, position=None,
                                            albedo=None):
        """yh_temporal_accumulate_variance_device: contiguous torch tensors on the context's device, as temporal_accumulate_device takes
        them, with a float32 (H, W) variance_out and a float32 (H, W, 3) albedo."""
        p = self._device_call("temporal_accumulate_variance_device", dict(
            rgba_out=(rgba_out, "float32", 4), variance_out=(variance_out, "float32", 1), rgba_in=(rgba_in, "float32", 4), object=(object, "int32", 1),
            position=(position, "float32", 3), albedo=(albedo, "float32", 3)))
        g = self._device_guides(p, ("object", "position", "albedo"))
        self._chk(self.lib.yh_temporal_accumulate_variance_device(self.h, C.byref(params), C.byref(variance_params), p["rgba_in"], int(samples),
                                                                  C.byref(g) if g is not None else None, p["rgba_out"], p["variance_out"]))

    def denoise_variance_image_device(self, variance_params, rgba_out, rgba_in, variance_in=None, variance_out=None, object=None, normal=None, position=None,
                                      albedo=None):
        """yh_denoise_variance_image_device: contiguous torch tensors on the context's device (variance_in None: the context's own)."""
        p = self._device_call("denoise_variance_image_device", dict(
            rgba_out=(rgba_out, "float32", 4), rgba_in=(rgba_in, "float32", 4), variance_in=(variance_in, "float32", 1), variance_out=(variance_out, "float32", 1),
            object=(object, "int32", 1), normal=(normal, "float32", 3), position=(position, "float32", 3), albedo=(albedo, "float32", 3)))
        g = self._device_guides(p, ("object", "normal", "position", "albedo"))
        self._chk(self.lib.yh_denoise_variance_image_device(self.h, C.byref(variance_params), p["rgba_in"], p["variance_in"], C.byref(g) if g is not None else None,
                                                            p["rgba_out"], p["variance_out"]))

    def svgf_display(self, params=None, variance_params=None, exposure=0.0, filmic=False, srgb=True):
        """yh_svgf_display: the own render through stages M, S and F and the tone map, as (H, W, 4) bytes."""
        params = params if params is not None else self.temporal_default_params()
        variance_params = variance_params if variance_params is not None else self.variance_default_params()
        img = np.zeros((getattr(self, "height", 0), getattr(self, "width", 0), 4), np.uint8)
        self._chk(self.lib.yh_svgf_display(self.h, C.byref(params), C.byref(variance_params), exposure, int(filmic), int(srgb),
                                           img.ctypes.data_as(C.POINTER(C.c_uint8))))
        return img

    def temporal_steps(self):
        """yh_temporal_steps: the moment history's steps as an (H, W) int32 array, or None without a moment history."""
        n = self.lib.yh_temporal_steps(self.h, None)
        self._chk(min(n, 0))
        if n == 0:
            return None
        out = np.zeros(n, np.int32)
        self._chk(min(self.lib.yh_temporal_steps(self.h, iptr(out)), 0))
        return out.reshape(self.height, self.width) if n == getattr(self, "height", 0) * getattr(self, "width", 0) else out

    def reproject_moments_gpu(self, params, rgba, samples, object, position, albedo, history, moment_history, camera, prev_camera=None, frames=None,
                              prev_frames=None, usable=None):
        """yh_reproject_moments_gpu: reproject_moments' arrays through the device kernel."""
        w, h, held, args, outs = _moment_args(rgba, samples, object, position, albedo, history, moment_history, camera, prev_camera, frames, prev_frames, usable)
        self._chk(self.lib.yh_reproject_moments_gpu(self.h, w, h, C.byref(params) if params is not None else None, *args))
        return outs

    def variance_spatial_gpu(self, temporal_params, min_steps, moments, steps, object, position):
        """yh_variance_spatial_gpu: variance_spatial's arrays through the device kernel."""
        w, h, held, ptrs, out = _spatial_args(moments, steps, object, position)
        self._chk(self.lib.yh_variance_spatial_gpu(self.h, w, h, C.byref(temporal_params), int(min_steps), *ptrs))
        return out

    def atrous_variance_filter_gpu(self, form, params, rgba, variance, object, normal=None, position=None, albedo=None):
        """yh_atrous_variance_filter_gpu: atrous_variance_filter's arrays through the device kernels (form 0: taps from memory, 1: from an LDS tile)."""
        w, h, held, ptrs, outs = _vfilter_args(rgba, variance, object, normal, position, albedo)
        self._chk(self.lib.yh_atrous_variance_filter_gpu(self.h, form, w, h, C.byref(params), *ptrs))
        return outs

    def shard_pixels(self, rank, world):
        return int(self.lib.yh_shard_pixels(self.h, rank, world))

    def pack_tiles_device(self, dev_ptr, capacity):
        n = C.c_int64()
        self._chk(self.lib.yh_pack_tiles_device(self.h, C.c_void_p(dev_ptr), capacity, C.byref(n)))
        return n.value

    def unpack_tiles_device(self, packed_ptr, src_rank, world, image_ptr):
        self._chk(self.lib.yh_unpack_tiles_device(self.h, C.c_void_p(packed_ptr), src_rank, world,
                                                  C.c_void_p(image_ptr)))

    # unit level -----------------------------------------------------------
    def hair_brdf(self, mats12, v, normal, tangent):
        mats = hair_material_rows(mats12)
        n = len(mats)
        v = np.ascontiguousarray(v, np.float32)
        normal = np.ascontiguousarray(normal, np.float32)
        tangent = np.ascontiguousarray(tangent, np.float32)
        out = np.zeros((n, 30), np.float32)
        self._chk(self.lib.yh_hair_brdf_batch(self.h, n, mats, fptr(v), fptr(normal), fptr(tangent), fptr(out)))
        return out

    def _wowi(self, fn, brdf, a, b, width):
        brdf = np.ascontiguousarray(brdf, np.float32)
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        n = len(brdf)
        out = np.zeros((n, width) if width > 1 else (n,), np.float32)
        self._chk(fn(self.h, n, fptr(brdf), fptr(a), fptr(b), fptr(out)))
        return out

    def hair_eval(self, brdf, wo, wi):
        return self._wowi(self.lib.yh_hair_eval_batch, brdf, wo, wi, 3)

    def hair_sample(self, brdf, wo, rn):
        return self._wowi(self.lib.yh_hair_sample_batch, brdf, wo, rn, 3)

    def hair_pdf(self, brdf, wo, wi):
        return self._wowi(self.lib.yh_hair_pdf_batch, brdf, wo, wi, 1)

    def hair_shade(self, form, exact, materials, v, normal, tangent, wo, wi, rn2):
        """yh_hair_shade_batch: the hair path of a shaded hit on the upload's material rows (form 0: a quad per row, 1: a lane per
        row; exact: the exact arithmetic, form 0 only). materials: (n, 12) rows as for hair_brdf, or the ctypes array
        hair_material_rows makes of them. (n, HAIR_SHADE_FLOATS) = f [3], pdf at wi, the sampled direction [3], f [3], pdf at
        it, the four lobe pdfs."""
        mats = materials if isinstance(materials, C.Array) else hair_material_rows(materials)
        a = [np.ascontiguousarray(x, np.float32) for x in (v, normal, tangent, wo, wi, rn2)]
        n = len(mats)
        assert all(len(x) == n for x in a)
        out = np.zeros((n, HAIR_SHADE_FLOATS), np.float32)
        self._chk(self.lib.yh_hair_shade_batch(self.h, form, int(exact), n, mats, *(fptr(x) for x in a), fptr(out)))
        return out

    def curves_to_lines(self, P, width0, width1, base_vertex=0):
        """pbrt curves (n, 12) -> positions (5n, 3), tangents (5n, 3), radius (5n), lines (4n, 2)."""
        P = np.ascontiguousarray(P, np.float32).reshape(-1, 12)
        w0, w1 = np.ascontiguousarray(width0, np.float32), np.ascontiguousarray(width1, np.float32)
        n = len(P)
        pos, nrm = np.zeros((5 * n, 3), np.float32), np.zeros((5 * n, 3), np.float32)
        rad, lines = np.zeros(5 * n, np.float32), np.zeros((4 * n, 2), np.int32)
        self._chk(self.lib.yh_curves_to_lines(self.h, n, fptr(P), fptr(w0), fptr(w1), base_vertex, fptr(pos), fptr(nrm),
                                              fptr(rad), iptr(lines)))
        return pos, nrm, rad, lines

    def surface_lobe(self, kind, params8, normal, wo, wi, rn3):
        """One YH_LOBE_* kind (yocto_math.h:4427-4755): (n, 7) = f*|cos| [3], pdf, sampled incoming [3]."""
        a = [np.ascontiguousarray(x, np.float32) for x in (params8, normal, wo, wi, rn3)]
        out = np.zeros((len(a[0]), 7), np.float32)
        self._chk(self.lib.yh_surface_lobe_batch(self.h, kind, len(a[0]), *(fptr(x) for x in a), fptr(out)))
        return out

    def surface_bsdf(self, materials, normal, wo, wi, rn3):
        """eval_brdf + lobe dispatch of non-hair materials: (n, SURFACE_BSDF_FLOATS)."""
        a = [np.ascontiguousarray(x, np.float32) for x in (normal, wo, wi, rn3)]
        out = np.zeros((len(a[0]), SURFACE_BSDF_FLOATS), np.float32)
        self._chk(self.lib.yh_surface_bsdf_batch(self.h, len(a[0]), materials, *(fptr(x) for x in a), fptr(out)))
        return out

    def volume(self, form, tex, materials, normal, wo, wi, texval4, rn5):
        """yh_volume_batch: the homogeneous medium of a path on the upload's material rows (form 0: a quad per row, 1: a lane per
        row; tex 1: the density derived on the device from colour x texval[:, 0:3] and transmission x texval[:, 3]). materials:
        (n, 10) rows as for volume_material_rows, or the ctypes array it makes. rn5: rl, rd, max_distance, rx, ry.
        (n, VOLUME_FLOATS) = in_medium, density [3], scatter [3], anisotropy, distance, weight factor [3], distance pdf, the
        sampled direction [3], f [3], pdf at wi, f [3], pdf at the sampled direction."""
        mats = materials if isinstance(materials, C.Array) else volume_material_rows(materials)
        a = [np.ascontiguousarray(x, np.float32) for x in (normal, wo, wi, texval4, rn5)]
        n = len(mats)
        assert all(len(x) == n for x in a)
        out = np.zeros((n, VOLUME_FLOATS), np.float32)
        self._chk(self.lib.yh_volume_batch(self.h, form, tex, n, mats, *(fptr(x) for x in a), fptr(out)))
        return out

    def point(self, form, object, element, uv, outgoing):
        """yh_point_batch: the shading point of a hit on the uploaded scene with its maps (form 0: launch shape 0 on this scene, a quad
        per row; 1: the streaming kernel, a lane per row; 2: the 256-thread shape and shade_step). (n, POINT_FLOATS), the columns of
        POINT_COLUMNS."""
        object, element = np.ascontiguousarray(object, np.int32), np.ascontiguousarray(element, np.int32)
        uv, outgoing = np.ascontiguousarray(uv, np.float32).reshape(-1, 2), np.ascontiguousarray(outgoing, np.float32).reshape(-1, 3)
        n = len(object)
        assert len(element) == n and len(uv) == n and len(outgoing) == n
        out = np.zeros((n, POINT_FLOATS), np.float32)
        self._chk(self.lib.yh_point_batch(self.h, form, n, iptr(object), iptr(element), fptr(uv), fptr(outgoing), fptr(out)))
        return out

    def quad_forms(self, normal, rn2, a, b):
        """yh_quad_forms_batch: (n, QUAD_FORMS_FLOATS) = sample_hemisphere_cos_quad [3], sample_hemisphere_cos [3],
        quad_div(a, b) [3], a / b [3]."""
        x = [np.ascontiguousarray(v, np.float32) for v in (normal, rn2, a, b)]
        n = len(x[0])
        assert all(len(v) == n for v in x)
        out = np.zeros((n, QUAD_FORMS_FLOATS), np.float32)
        self._chk(self.lib.yh_quad_forms_batch(self.h, n, *(fptr(v) for v in x), fptr(out)))
        return out

    def path_ends(self, op, form, fin, iin, rng=None):
        """yh_path_ends_batch: the start and the end of a path, row by row (form 0: a quad per row, 1: a lane per row). op, or its
        name in PATH_OPS: PATH_BEGIN (fin (n, 17) the camera, iin (n, 4) i j w h, rng (n, 2) uint64), PATH_CONTINUE (fin (n, 3) the
        weight, iin (n, 2) bounce bounces, rng) or PATH_END (fin (n, 8) radiance clamp acc, iin (n, 1) hit). Returns (fout, iout,
        state): the rows of include/yhair.h, iout and state None for PATH_END."""
        op = PATH_OPS.get(op, op)
        nfi, nii, nfo, nio = PATH_ROWS[op]
        fin, iin = np.ascontiguousarray(fin, np.float32).reshape(-1, nfi), np.ascontiguousarray(iin, np.int32).reshape(-1, nii)
        n = len(fin)
        assert len(iin) == n
        u64 = C.POINTER(C.c_uint64)
        fout = np.zeros((n, nfo), np.float32)
        if op == PATH_END:
            self._chk(self.lib.yh_path_ends_batch(self.h, op, form, n, fptr(fin), iptr(iin), None, fptr(fout), None, None))
            return fout, None, None
        rng = np.ascontiguousarray(rng, np.uint64).reshape(-1, 2)
        assert len(rng) == n
        iout, state = np.zeros((n, nio), np.int32), np.zeros(n, np.uint64)
        self._chk(self.lib.yh_path_ends_batch(self.h, op, form, n, fptr(fin), iptr(iin), rng.ctypes.data_as(u64), fptr(fout), iptr(iout),
                                              state.ctypes.data_as(u64)))
        return fout, iout, state

    def bvh_refit_wide_gpu(self, boxes, primitives, width, slots):
        """yh_bvh_refit_wide_gpu: the refitted copy of `slots` (device form, as from yh_bvh_build_wide_gpu) under the new `boxes`
        (primitive order); `primitives` is the leaf order. Returns (node count, slots)."""
        boxes, primitives, out = _refit_args(boxes, primitives, slots)
        n = self.lib.yh_bvh_refit_wide_gpu(self.h, len(boxes), fptr(boxes), iptr(primitives), width, fptr(out))
        if n < 0:
            self._chk(n)
        return n, out

    def intersect(self, rays):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = len(rays)
        obj, elem = np.zeros(n, np.int32), np.zeros(n, np.int32)
        uv, dist = np.zeros((n, 2), np.float32), np.zeros(n, np.float32)
        self._chk(self.lib.yh_intersect_batch(self.h, n, fptr(rays), iptr(obj), iptr(elem), fptr(uv), fptr(dist)))
        return obj, elem, uv, dist

    def intersect_plain(self, form, rays):
        """yh_intersect_plain_batch: closest hits through the traversal of the plain 512-thread sample-loop kernels (form 0: a
        quad per ray, 1: an octet per ray), the scene level staged in LDS and walked as a launch on this scene walks it; forms 2-6:
        the traversal of the 256-thread launch shapes (2 the dense quad, 3 octet, 4 octet with leaf pairs, 5 sixteen lanes, 6 sixteen
        with leaf groups), and form | INTERSECT_TABLE_IN_MEMORY (3-6): their scene level read from memory."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        n = len(rays)
        obj, elem = np.zeros(n, np.int32), np.zeros(n, np.int32)
        uv, dist = np.zeros((n, 2), np.float32), np.zeros(n, np.float32)
        self._chk(self.lib.yh_intersect_plain_batch(self.h, form, n, fptr(rays), iptr(obj), iptr(elem), fptr(uv), fptr(dist)))
        return obj, elem, uv, dist

    def scene_once(self):
        """yh_scene_once: the object count when the plain 512-thread kernels resolve this scene's scene level once per ray, else 0."""
        rc = int(self.lib.yh_scene_once(self.h))
        if rc < 0:
            self._chk(rc)
        return rc

    def lights_const_env(self):
        """yh_lights_const_env: 1 when the plain 512-thread kernels take this scene's lights (constant environments only) from the kernel argument."""
        rc = int(self.lib.yh_lights_const_env(self.h))
        if rc < 0:
            self._chk(rc)
        return rc

    SHADE_REGIONS = ("regen", "miss", "fetch", "hair", "sample", "eval", "lights_pdf", "weight", "end")

    def shade_regions(self):
        """yh_shade_regions of the last trace_samples_counted: {region: (cycles, trips, lanes)}."""
        out = (C.c_uint64 * 27)()
        self.lib.yh_shade_regions(self.h, out, 27)
        return {nm: (int(out[3 * k]), int(out[3 * k + 1]), int(out[3 * k + 2])) for k, nm in enumerate(self.SHADE_REGIONS)}

    def set_count_bound(self, items):
        """yh_set_count_bound: trace_samples_counted counts the first `items` work items of the cost-ordered list only (0: all)."""
        self._chk(self.lib.yh_set_count_bound(self.h, int(items)))

    def lights(self, form, position, direction, rn4):
        """yh_lights_batch on the uploaded scene (form 0: a quad per row, 1: a lane per row): (n, 8) = sample_lights
        direction [3], sample_lights_pdf at it, sample_lights_pdf at `direction`, eval_environment(direction) [3]."""
        a = [np.ascontiguousarray(x, np.float32) for x in (position, direction, rn4)]
        n = len(a[0])
        out = np.zeros((n, 8), np.float32)
        self._chk(self.lib.yh_lights_batch(self.h, form, n, *(fptr(x) for x in a), fptr(out)))
        return out

    def selftest(self, which):
        worst = C.c_float()
        rc = self.lib.yh_selftest(self.h, which, C.byref(worst))
        if rc not in (YH_OK, YH_E_SELFTEST):
            self._chk(rc)
        return rc == YH_OK, worst.value
