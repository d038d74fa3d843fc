"""The variance stage without a GPU: the library exports its entry points, the header declares them, the binding lists them,
VarianceParams has the layout a C compiler gives yh_variance_params, the defaults without a context, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

ENTRIES = ("yh_variance_default_params", "yh_temporal_accumulate_variance_device", "yh_temporal_accumulate_variance", "yh_denoise_variance_image_device",
           "yh_denoise_variance_image", "yh_svgf_display", "yh_temporal_steps", "yh_reproject_moments", "yh_reproject_moments_gpu", "yh_variance_spatial",
           "yh_variance_spatial_gpu", "yh_atrous_variance_filter", "yh_atrous_variance_filter_gpu")
FIELDS = ["iterations", "sigma_luminance", "sigma_normal", "sigma_position", "demodulate", "match_object", "epsilon", "min_steps"]
F = np.float32


def test_library_header_and_binding_have_the_entry_points(yh):
    header = open(os.path.join(ROOT, "include", "yhair.h")).read()
    lib = yh.load()
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in yh.EXPORTS and hasattr(lib, name)
    section = header[header.index("VARIANCE ("):header.index("typedef struct yh_variance_params")]
    assert "an extension" in section and "Schied" in section and "#define YH_VARIANCE_MAX_STEPS 1024" in section
    for method in ("temporal_accumulate_variance", "temporal_accumulate_variance_device", "denoise_variance_image", "denoise_variance_image_device", "svgf_display",
                   "temporal_steps", "reproject_moments_gpu", "variance_spatial_gpu", "atrous_variance_filter_gpu", "variance_default_params"):
        assert callable(getattr(yh.Context, method))
    assert callable(yh.reproject_moments) and callable(yh.variance_spatial) and callable(yh.atrous_variance_filter) and yh.VARIANCE_MAX_STEPS == 1024


def test_struct_layout_is_the_headers(yh, tmp_path):
    assert [n for n, _ in yh.VarianceParams._fields_] == FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "yhair.h"\nint main(void) {\n  printf("%zu", sizeof(yh_variance_params));\n'
                   + "".join(f'  printf(" %zu", offsetof(yh_variance_params, {n}));\n' for n in FIELDS) + '  printf(" %d", YH_VARIANCE_MAX_STEPS);\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(yh.VarianceParams) == 32
    assert out[1:9] == [getattr(yh.VarianceParams, n).offset for n in FIELDS]
    assert out[9] == yh.VARIANCE_MAX_STEPS
    # ... beside the two structs that were there, which are as they were
    assert [n for n, _ in yh.DenoiseParams._fields_] == ["iterations", "sigma_color", "sigma_normal", "sigma_position", "demodulate", "match_object"]
    assert [n for n, _ in yh.TemporalParams._fields_] == ["max_history", "sigma_position", "match_object"]
    assert C.sizeof(yh.DenoiseParams) == 24 and C.sizeof(yh.TemporalParams) == 12


def test_defaults_without_a_context(yh):
    p, d = yh.variance_default_params(), yh.denoise_default_params()
    assert (p.sigma_normal, p.sigma_position, p.demodulate, p.match_object) == (d.sigma_normal, d.sigma_position, d.demodulate, d.match_object)
    assert 1 <= p.iterations <= yh.DENOISE_MAX_ITERATIONS and p.sigma_luminance > 0 and p.epsilon > 0 and p.min_steps >= 1
    assert yh.load().yh_variance_default_params(None, None) == yh.YH_E_INVALID


def test_null_context_is_refused(yh):
    lib = yh.load()
    t, v = yh.temporal_default_params(), yh.variance_default_params()
    assert lib.yh_temporal_accumulate_variance_device(None, C.byref(t), C.byref(v), None, 0, None, None, None) == yh.YH_E_INVALID
    assert lib.yh_temporal_accumulate_variance(None, C.byref(t), C.byref(v), None, 0, None, None, None) == yh.YH_E_INVALID
    assert lib.yh_denoise_variance_image_device(None, C.byref(v), None, None, None, None, None) == yh.YH_E_INVALID
    assert lib.yh_denoise_variance_image(None, C.byref(v), None, None, None, None, None) == yh.YH_E_INVALID
    assert lib.yh_svgf_display(None, C.byref(t), C.byref(v), 0.0, 0, 1, None) == yh.YH_E_INVALID
    assert lib.yh_temporal_steps(None, None) == yh.YH_E_INVALID
    assert lib.yh_variance_spatial_gpu(None, 1, 1, C.byref(t), 1, None, None, None, None, None) == yh.YH_E_INVALID
    assert lib.yh_atrous_variance_filter_gpu(None, 0, 1, 1, C.byref(v), *[None] * 8) == yh.YH_E_INVALID


def test_host_form_refusals_leave_the_outputs_alone(yh):
    """min_steps < 1, an epsilon that is not > 0, iterations outside 0 .. 6, a NULL image, variance, plane or output, a moment history given
    in part: YH_E_INVALID, and the output arrays as they were."""
    lib = yh.load()
    w, h = 4, 3
    rgba, var, ids, pl = np.ones((h, w, 4), F), np.ones((h, w), F), np.zeros((h, w), np.int32), np.ones((h, w, 3), F)
    out, out_var = np.full((h, w, 4), 7, F), np.full((h, w), 7, F)
    good = yh.VarianceParams(2, 1.0, 0.5, 0.5, 1, 1, 1e-4, 2)

    def filt(p=good, rgba=rgba, var=var, ids=ids, normal=pl, position=pl, albedo=pl, out=out):
        f = lambda a: yh.fptr(a) if a is not None else None  # noqa: E731
        return lib.yh_atrous_variance_filter(w, h, C.byref(p) if p is not None else None, f(rgba), f(var), yh.iptr(ids) if ids is not None else None, f(normal),
                                             f(position), f(albedo), f(out), yh.fptr(out_var))
    for bad in (good.copy(min_steps=0), good.copy(epsilon=0.0), good.copy(epsilon=-1.0), good.copy(epsilon=float("nan")), good.copy(iterations=-1),
                good.copy(iterations=7), None):
        assert filt(p=bad) == yh.YH_E_INVALID
    for missing in ("rgba", "var", "ids", "normal", "position", "albedo", "out"):
        assert filt(**{missing: None}) == yh.YH_E_INVALID, missing
    assert np.all(out == 7) and np.all(out_var == 7)
    assert filt(p=good.copy(sigma_normal=0.0, sigma_position=0.0, demodulate=0), normal=None, position=None, albedo=None) == yh.YH_OK
    assert not np.all(out == 7)
    t = yh.TemporalParams(4, 0.0, 1)
    mom, steps, sv = np.ones((h, w, 2), F), np.ones((h, w), np.int32), np.full((h, w), 7, F)
    for min_steps in (0, -2):
        assert lib.yh_variance_spatial(w, h, C.byref(t), min_steps, yh.fptr(mom), yh.iptr(steps), yh.iptr(ids), yh.fptr(pl), yh.fptr(sv)) == yh.YH_E_INVALID
    assert lib.yh_variance_spatial(w, h, None, 2, yh.fptr(mom), yh.iptr(steps), yh.iptr(ids), yh.fptr(pl), yh.fptr(sv)) == yh.YH_E_INVALID
    assert lib.yh_variance_spatial(w, h, C.byref(t), 2, yh.fptr(mom), None, yh.iptr(ids), yh.fptr(pl), yh.fptr(sv)) == yh.YH_E_INVALID
    assert np.all(sv == 7)
    cam = yh.camera_of(np.arange(17, dtype=F))
    o4, ol, om, os_ = np.full((h, w, 4), 7, F), np.full((h, w), 7, np.int32), np.full((h, w, 2), 7, F), np.full((h, w), 7, np.int32)
    head = [w, h, C.byref(t), yh.fptr(rgba), 2, yh.iptr(ids), yh.fptr(pl), None, yh.fptr(rgba), yh.iptr(steps), yh.iptr(ids), yh.fptr(pl)]
    tail = [C.byref(cam), C.byref(cam), 0, None, None, None, yh.fptr(o4), yh.iptr(ol), yh.fptr(om), yh.iptr(os_)]
    assert lib.yh_reproject_moments(*head, yh.fptr(mom), None, *tail) == yh.YH_E_INVALID, "moments without steps"
    assert lib.yh_reproject_moments(*head, None, yh.iptr(steps), *tail) == yh.YH_E_INVALID, "steps without moments"
    assert lib.yh_reproject_moments(*head, yh.fptr(mom), yh.iptr(steps), *tail[:-1], None) == yh.YH_E_INVALID, "no out_steps"
    assert np.all(o4 == 7) and np.all(ol == 7) and np.all(om == 7) and np.all(os_ == 7)
    assert lib.yh_reproject_moments(*head, None, None, *tail) == yh.YH_OK, "no moment history"
    assert (os_ == 1).all()
