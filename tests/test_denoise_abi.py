"""The denoiser without a GPU: the library exports its entry points, the header declares them, the binding lists them, DenoiseParams has
the layout a C compiler gives yh_denoise_params, the defaults without a context, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

ENTRIES = ("yh_denoise_default_params", "yh_denoise_image_device", "yh_denoise", "yh_denoise_display", "yh_atrous_filter",
           "yh_atrous_filter_gpu", "yh_atrous_level_ms")
F = np.float32


def test_library_header_and_binding_have_the_entry_points(yh):
    header = open(os.path.join(ROOT, "include", "yhair.h")).read()
    lib = yh.load()
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in yh.EXPORTS and hasattr(lib, name)
    assert re.search(r"#define YH_DENOISE_MAX_ITERATIONS 6\b", header) and yh.DENOISE_MAX_ITERATIONS == 6
    assert "Dammertz" in header and "an extension" in header[header.index("DENOISE ("):header.index("#define YH_DENOISE_MAX_ITERATIONS")]
    for method in ("denoise", "denoise_display", "denoise_image_device", "atrous_filter_gpu", "denoise_default_params"):
        assert callable(getattr(yh.Context, method))
    assert callable(yh.atrous_filter)


def test_struct_layout_is_the_headers(yh, tmp_path):
    names = [n for n, _ in yh.DenoiseParams._fields_]
    assert names == ["iterations", "sigma_color", "sigma_normal", "sigma_position", "demodulate", "match_object"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "yhair.h"\nint main(void) {\n  printf("%zu", sizeof(yh_denoise_params));\n'
                   + "".join(f'  printf(" %zu", offsetof(yh_denoise_params, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(yh.DenoiseParams) == 24
    assert out[1:] == [getattr(yh.DenoiseParams, n).offset for n in names]


def test_defaults_without_a_context(yh):
    p = yh.denoise_default_params()
    assert 1 <= p.iterations <= yh.DENOISE_MAX_ITERATIONS and p.sigma_color > 0 and p.sigma_normal > 0
    assert p.sigma_position == 0 and p.demodulate == 1 and p.match_object == 1
    assert yh.load().yh_denoise_default_params(None, None) == yh.YH_E_INVALID


def test_null_context_is_refused(yh):
    lib = yh.load()
    p = yh.denoise_default_params()
    buf = np.zeros(16, F)
    assert lib.yh_denoise_image_device(None, C.byref(p), None, None, None) == yh.YH_E_INVALID
    assert lib.yh_denoise(None, C.byref(p), None, yh.fptr(buf)) == yh.YH_E_INVALID
    assert lib.yh_denoise_display(None, C.byref(p), 0.0, 0, 1, None) == yh.YH_E_INVALID
    assert lib.yh_atrous_filter_gpu(None, 0, 1, 1, C.byref(p), yh.fptr(buf), None, None, None, None, yh.fptr(buf)) == yh.YH_E_INVALID
    assert lib.yh_atrous_level_ms(None, None, 0) == yh.YH_E_INVALID


def test_host_filter_refusals_leave_the_output_alone(yh):
    """iterations outside 0 .. 6, a NULL params / image / output, an empty image, a guide plane the parameters need: YH_E_INVALID, and the
    output array as it was."""
    lib = yh.load()
    w, h = 4, 3
    rgba, ids = np.ones((h, w, 4), F), np.zeros((h, w), np.int32)
    n, x, a = (np.ones((h, w, 3), F) for _ in range(3))
    out = np.full((h, w, 4), 7, F)

    def call(p, rgba_=rgba, ids_=ids, n_=n, x_=x, a_=a, out_=out, w_=w, h_=h):
        ptr = lambda v, f: f(v) if v is not None else None
        return lib.yh_atrous_filter(w_, h_, C.byref(p) if p is not None else None, ptr(rgba_, yh.fptr), ptr(ids_, yh.iptr), ptr(n_, yh.fptr),
                                    ptr(x_, yh.fptr), ptr(a_, yh.fptr), ptr(out_, yh.fptr))
    good = yh.DenoiseParams(2, 1.0, 1.0, 1.0, 1, 1)
    assert call(good) == yh.YH_OK
    out[:] = 7
    for it in (-1, 7, 1 << 20):
        assert call(good.copy(iterations=it)) == yh.YH_E_INVALID
    assert call(None) == yh.YH_E_INVALID
    assert call(good, rgba_=None) == yh.YH_E_INVALID
    assert call(good, out_=None) == yh.YH_E_INVALID
    assert call(good, w_=0) == yh.YH_E_INVALID and call(good, h_=-1) == yh.YH_E_INVALID
    for missing in ("ids_", "n_", "x_", "a_"):
        assert call(good, **{missing: None}) == yh.YH_E_INVALID, missing
    assert np.all(out == 7)
    # ... and each plane is needed only where its parameter reads it; with iterations = 0 none is
    assert call(good.copy(sigma_normal=0.0), n_=None) == yh.YH_OK
    assert call(good.copy(sigma_position=0.0), x_=None) == yh.YH_OK
    assert call(good.copy(demodulate=0), a_=None) == yh.YH_OK
    assert call(good.copy(iterations=0), ids_=None, n_=None, x_=None, a_=None) == yh.YH_OK
