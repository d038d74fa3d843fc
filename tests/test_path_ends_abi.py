"""yh_path_ends_batch without a GPU: the library exports it, the header declares it, the binding lists it with the header's argument
types, the row sizes of the binding are the header's YH_PATH_* as a C compiler sees them, a YH_PATH_BEGIN row is a yh_camera field for
field, the oracle exports its counterpart, and a NULL context is refused."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

ENTRY = "yh_path_ends_batch"
MACROS = ("YH_PATH_BEGIN", "YH_PATH_CONTINUE", "YH_PATH_END", "YH_PATH_OPS", "YH_PATH_BEGIN_IN", "YH_PATH_BEGIN_OUT", "YH_PATH_CONTINUE_IN",
          "YH_PATH_CONTINUE_OUT", "YH_PATH_END_IN", "YH_PATH_END_OUT")


def test_library_header_and_binding_have_the_entry_point(yh, oracle):
    header = open(os.path.join(ROOT, "include", "yhair.h")).read()
    lib = yh.load()
    decl = r"\bint yh_path_ends_batch\(yh_context\* ctx, int op, int form, int n,\s+const float\* fin, const int\* iin, const uint64_t\* rng, float\* fout,\s+int\* iout, uint64_t\* state\);"
    assert re.search(decl, header)
    assert ENTRY in yh.EXPORTS and hasattr(lib, ENTRY)
    u64p = C.POINTER(C.c_uint64)
    assert getattr(lib, ENTRY).argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int, yh.c_float_p, yh.c_int_p, u64p, yh.c_float_p, yh.c_int_p, u64p]
    assert getattr(lib, ENTRY).restype == C.c_int
    assert callable(yh.Context.path_ends) and yh.PATH_OPS == {"begin": yh.PATH_BEGIN, "continue": yh.PATH_CONTINUE, "end": yh.PATH_END}
    oheader = open(os.path.join(ROOT, "oracle", "yh_oracle.h")).read()
    assert re.search(r"\bvoid yo_path_ends_batch\(int op, int n, const float\* fin, const int\* iin, const uint64_t\* rng, float\* fout, int\* iout,\s+uint64_t\* state\);", oheader)
    assert hasattr(oracle.lib, "yo_path_ends_batch") and callable(oracle.path_ends)
    launchers = open(os.path.join(ROOT, "yocto-hair_amd", "csrc", "launchers.h")).read()
    for name in ("yhk_path_ends_quads", "yhk_path_ends_lanes"):  # declared once, for both compilers
        assert len(re.findall(rf"\bint {name}\(", launchers)) == 1
        host = os.path.join(ROOT, "yocto-hair_amd", "host")
        assert not any(re.search(rf"\bint {name}\(", open(os.path.join(host, f)).read()) for f in os.listdir(host) if f.endswith((".cpp", ".h")))


def test_row_layout_is_the_headers(yh, tmp_path):
    """The YH_PATH_* values as a C compiler sees the header against the binding's; sizeof and offsetof of yh_camera against a
    YH_PATH_BEGIN row (frame[12], lens, film x, film y, focus, aperture: the 17 floats the kernels hold)."""
    fields = ("frame", "lens", "film", "focus", "aperture")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "yhair.h"\nint main(void) {\n'
                   + "".join(f'  printf("%d ", {m});\n' for m in MACROS) + '  printf("%zu", sizeof(yh_camera));\n'
                   + "".join(f'  printf(" %zu", offsetof(yh_camera, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    m = dict(zip(MACROS, out))
    assert (m["YH_PATH_BEGIN"], m["YH_PATH_CONTINUE"], m["YH_PATH_END"], m["YH_PATH_OPS"]) == (yh.PATH_BEGIN, yh.PATH_CONTINUE, yh.PATH_END, 3) == (0, 1, 2, 3)
    assert yh.PATH_ROWS == {yh.PATH_BEGIN: (m["YH_PATH_BEGIN_IN"], 4, m["YH_PATH_BEGIN_OUT"], 3), yh.PATH_CONTINUE: (m["YH_PATH_CONTINUE_IN"], 2, m["YH_PATH_CONTINUE_OUT"], 2),
                            yh.PATH_END: (m["YH_PATH_END_IN"], 1, m["YH_PATH_END_OUT"], 0)}
    size, offsets = out[len(MACROS)], out[len(MACROS) + 1:]
    assert size == C.sizeof(yh.Camera) == 4 * m["YH_PATH_BEGIN_IN"]
    assert offsets == [getattr(yh.Camera, f).offset for f in fields] == [0, 48, 52, 60, 64]


def test_null_context_is_refused(yh):
    import numpy as np
    lib = yh.load()
    u64p = C.POINTER(C.c_uint64)
    for op in (yh.PATH_BEGIN, yh.PATH_CONTINUE, yh.PATH_END):
        nfi, nii, nfo, nio = yh.PATH_ROWS[op]
        fin, iin, rng = np.zeros((1, nfi), np.float32), np.ones((1, nii), np.int32), np.ones((1, 2), np.uint64)
        fout, iout, state = np.zeros((1, nfo), np.float32), np.zeros((1, max(nio, 1)), np.int32), np.zeros(1, np.uint64)
        for form in (0, 1):
            assert lib.yh_path_ends_batch(None, op, form, 1, yh.fptr(fin), yh.iptr(iin), rng.ctypes.data_as(u64p), yh.fptr(fout), yh.iptr(iout),
                                          state.ctypes.data_as(u64p)) == yh.YH_E_INVALID
