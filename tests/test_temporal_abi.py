"""The temporal stage without a GPU: the library exports its entry points, the header declares them, the binding lists them,
TemporalParams has the layout a C compiler gives yh_temporal_params, the defaults without a context, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

ENTRIES = ("yh_temporal_default_params", "yh_temporal_accumulate_device", "yh_temporal_accumulate", "yh_temporal_display", "yh_temporal_reset",
           "yh_temporal_lengths", "yh_reproject", "yh_reproject_gpu")
F = np.float32


def test_library_header_and_binding_have_the_entry_points(yh):
    header = open(os.path.join(ROOT, "include", "yhair.h")).read()
    lib = yh.load()
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in yh.EXPORTS and hasattr(lib, name)
    section = header[header.index("TEMPORAL ("):header.index("typedef struct yh_temporal_params")]
    assert "an extension" in section and "Schied" in section
    for method in ("temporal_accumulate", "temporal_accumulate_device", "temporal_display", "temporal_reset", "temporal_lengths", "reproject_gpu",
                   "temporal_default_params"):
        assert callable(getattr(yh.Context, method))
    assert callable(yh.reproject) and callable(yh.temporal_default_params)


def test_struct_layout_is_the_headers(yh, tmp_path):
    names = [n for n, _ in yh.TemporalParams._fields_]
    assert names == ["max_history", "sigma_position", "match_object"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "yhair.h"\nint main(void) {\n  printf("%zu", sizeof(yh_temporal_params));\n'
                   + "".join(f'  printf(" %zu", offsetof(yh_temporal_params, {n}));\n' for n in names) + '  printf(" %zu", sizeof(yh_camera));\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(yh.TemporalParams) == 12
    assert out[1:4] == [getattr(yh.TemporalParams, n).offset for n in names]
    assert out[4] == C.sizeof(yh.Camera) == 17 * 4, "a camera is the 17 floats the projection reads"


def test_defaults_without_a_context(yh):
    p = yh.temporal_default_params()
    assert p.max_history >= 1 and p.sigma_position == 0 and p.match_object == 1
    assert yh.load().yh_temporal_default_params(None, None) == yh.YH_E_INVALID


def test_null_context_is_refused(yh):
    lib = yh.load()
    p = yh.temporal_default_params()
    assert lib.yh_temporal_accumulate_device(None, C.byref(p), None, 0, None, None) == yh.YH_E_INVALID
    assert lib.yh_temporal_accumulate(None, C.byref(p), None, 0, None, None) == yh.YH_E_INVALID
    assert lib.yh_temporal_display(None, C.byref(p), None, 0.0, 0, 1, None) == yh.YH_E_INVALID
    assert lib.yh_temporal_reset(None) == yh.YH_E_INVALID
    assert lib.yh_temporal_lengths(None, None) == yh.YH_E_INVALID
    assert lib.yh_reproject_gpu(None, *([1, 1, C.byref(p)] + [None, 1] + [None] * 8 + [0] + [None] * 5)) == yh.YH_E_INVALID


def test_host_form_refusals_leave_the_outputs_alone(yh):
    """max_history < 1, samples < 1, a NULL params / image / plane / camera / output, an empty image, a history or frames given in part:
    YH_E_INVALID, and the output arrays as they were."""
    lib = yh.load()
    w, h = 4, 3
    cam = yh.camera_of(np.arange(17, dtype=F))
    base = dict(w=w, h=h, p=yh.TemporalParams(8, 0.5, 1), rgba=np.ones((h, w, 4), F), samples=2, ids=np.zeros((h, w), np.int32), pos=np.ones((h, w, 3), F),
                hr=np.ones((h, w, 4), F), hl=np.ones((h, w), np.int32), hi=np.zeros((h, w), np.int32), hp=np.ones((h, w, 3), F), cam=cam, pcam=cam, n=1,
                fr=np.ones((1, 12), F), pf=np.ones((1, 12), F), use=np.ones(1, np.int32), out=np.full((h, w, 4), 7, F), length=np.full((h, w), 7, np.int32))

    def call(**changes):
        a = dict(base, **changes)
        ptr = lambda v: None if v is None else (C.byref(v) if isinstance(v, C.Structure) else yh.iptr(v) if v.dtype == np.int32 else yh.fptr(v))  # noqa: E731
        return lib.yh_reproject(a["w"], a["h"], ptr(a["p"]), ptr(a["rgba"]), a["samples"], ptr(a["ids"]), ptr(a["pos"]), ptr(a["hr"]), ptr(a["hl"]), ptr(a["hi"]),
                                ptr(a["hp"]), ptr(a["cam"]), ptr(a["pcam"]), a["n"], ptr(a["fr"]), ptr(a["pf"]), ptr(a["use"]), ptr(a["out"]), ptr(a["length"]))
    assert call() == yh.YH_OK
    base["out"][:], base["length"][:] = 7, 7
    for bad in (0, -1, (1 << 30) + 1):
        assert call(p=yh.TemporalParams(bad, 0.5, 1)) == yh.YH_E_INVALID
    for bad in (0, -3):
        assert call(samples=bad) == yh.YH_E_INVALID
    for missing in ("p", "rgba", "ids", "pos", "cam", "out", "length", "hr", "hi", "hp", "pcam", "pf"):
        assert call(**{missing: None}) == yh.YH_E_INVALID, missing
    assert call(w=0) == yh.YH_E_INVALID and call(h=-1) == yh.YH_E_INVALID and call(n=-1) == yh.YH_E_INVALID
    assert np.all(base["out"] == 7) and np.all(base["length"] == 7)
    # ... and what is optional: no history at all, no motion, every object usable
    assert call(hl=None, hr=None, hi=None, hp=None, pcam=None) == yh.YH_OK
    assert call(fr=None, pf=None, use=None) == yh.YH_OK
    assert call(use=None) == yh.YH_OK
