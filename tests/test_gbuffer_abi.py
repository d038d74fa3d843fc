"""The first-hit feature pass without a GPU: the library exports yh_trace_gbuffer / yh_trace_gbuffer_device, the header declares them,
the binding lists them, its GBuffer has the layout a C compiler gives yh_gbuffer, and a NULL context is refused."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

ENTRIES = ("yh_trace_gbuffer", "yh_trace_gbuffer_device")


def test_library_header_and_binding_have_the_entry_points(yh):
    header = open(os.path.join(ROOT, "include", "yhair.h")).read()
    lib = yh.load()
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(yh_context\* ctx, int mode, const yh_gbuffer\* out\);", header), name
        assert name in yh.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == [C.c_void_p, C.c_int, C.POINTER(yh.GBuffer)]
    assert (yh.GBUFFER_CENTRE, yh.GBUFFER_NEXT_SAMPLE) == (0, 1)
    assert re.search(r"#define YH_GBUFFER_CENTRE 0\b", header) and re.search(r"#define YH_GBUFFER_NEXT_SAMPLE 1\b", header)
    assert callable(yh.Context.trace_gbuffer) and callable(yh.Context.trace_gbuffer_device)


def test_struct_layout_is_the_headers(yh, tmp_path):
    """sizeof and every offsetof of yh_gbuffer as a C compiler sees the header, against the ctypes mirror."""
    names = [n for n, _, _ in yh.GBUFFER_PLANES]
    assert names == [n for n, _ in yh.GBuffer._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "yhair.h"\nint main(void) {\n  printf("%zu", sizeof(yh_gbuffer));\n'
                   + "".join(f'  printf(" %zu", offsetof(yh_gbuffer, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(yh.GBuffer) == 11 * C.sizeof(C.c_void_p)
    assert out[1:] == [getattr(yh.GBuffer, n).offset for n in names]


def test_null_context_is_refused(yh):
    lib = yh.load()
    g = yh.GBuffer()
    for name in ENTRIES:
        assert getattr(lib, name)(None, 0, C.byref(g)) == yh.YH_E_INVALID
        assert getattr(lib, name)(None, 0, None) == yh.YH_E_INVALID
