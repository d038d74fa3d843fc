"""tools/codegen_diff.py: the step that splits an assembly listing into functions and drops what carries no code. Made-up listings, no compiler."""
import codegen_diff

LISTING = """
\t.text
\t.globl\t_Z5k_onePf
\t.p2align\t8
\t.type\t_Z5k_onePf,@function
_Z5k_onePf:                             ; @_Z5k_onePf
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0    ; a comment
\tv_mov_b32_e32 v1, 0
\ts_cbranch_scc1 .LBB{fn}_{blk}
; %bb.1:                                ; in Loop: Header=BB{fn}_{blk} Depth=1
\t.p2align\t6
\tv_add_f32_e32 v1, {addend}, v1
.LBB{fn}_{blk}:                         ; %the end
\ts_endpgm
\t.section\t.rodata,"a",@progbits
.Lfunc_end{fn}:
\t.size\t_Z5k_onePf, .Lfunc_end{fn}-_Z5k_onePf
\t.amdhsa_kernel _Z5k_onePf
\t\t.amdhsa_next_free_vgpr 2
\t.end_amdhsa_kernel
_ZN3yhd6helperEf:                       ; @_ZN3yhd6helperEf
\tv_mul_f32_e32 v0, v0, v0
\ts_setpc_b64 s[30:31]
.Lfunc_end{helper}:
"""


def functions(fn, blk, addend, helper, comment=""):
    return codegen_diff.split_functions(LISTING.format(fn=fn, blk=blk, addend=addend, helper=helper).replace("a comment", comment or "a comment"))


def test_labels_comments_and_directives_do_not_count():
    a, b = functions(0, 2, "1.0", 1), functions(7, 31, "1.0", 8, comment="another one entirely")
    assert set(a) == {"_Z5k_onePf", "_ZN3yhd6helperEf"}
    assert a == b
    assert a["_Z5k_onePf"] == [" s_load_dwordx2 s[0:1], s[4:5], 0x0", " v_mov_b32_e32 v1, 0", " s_cbranch_scc1 .L0", " v_add_f32_e32 v1, 1.0, v1", ".L0:", " s_endpgm"]
    assert codegen_diff.instruction_lines(a["_Z5k_onePf"]) == 5 and codegen_diff.instruction_lines(a["_ZN3yhd6helperEf"]) == 2
    rows = codegen_diff.compare({"csrc/kernels.hip": a}, {"unit/one.hip": b})  # ... and a function that moved is matched by its name
    assert [(r[0], r[1], r[2], r[3], r[5]) for r in rows] == [("SAME", 5, 5, "unit/one.hip", "csrc/kernels.hip"), ("SAME", 2, 2, "unit/one.hip", "csrc/kernels.hip")]


def test_one_changed_instruction_is_a_difference():
    a, b = functions(0, 2, "1.0", 1), functions(0, 2, "2.0", 1)
    assert a["_ZN3yhd6helperEf"] == b["_ZN3yhd6helperEf"] and a["_Z5k_onePf"] != b["_Z5k_onePf"]
    b["_Z3newv"] = [" s_endpgm"]
    rows = {r[4]: r[:4] for r in codegen_diff.compare({"unit/one.hip": a}, {"unit/one.hip": b})}
    assert rows == {"_Z5k_onePf": ("DIFF", 5, 5, "unit/one.hip"), "_ZN3yhd6helperEf": ("SAME", 2, 2, "unit/one.hip"), "_Z3newv": ("NEW_ONLY", None, 1, "unit/one.hip")}
