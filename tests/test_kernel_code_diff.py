"""tools/kernel_code_diff.py: the normaliser and the verdict on three short hand-written pieces of gfx950 assembly (no compiler, no GPU)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tools"))
import kernel_code_diff as kcd  # noqa: E402

KERNEL = """\
\t.globl\t_Z1kPf ; -- Begin function _Z1kPf
_Z1kPf: ; @_Z1kPf
; %bb.0:
\ts_load_dwordx2 s[0:1], s[0:1], 0x0
\tv_mov_b32_e32 {r}, 0
\tv_exp_f32_e32 {r}, {r}{more}
\ts_waitcnt lgkmcnt(0)
\tglobal_store_dword {r}, {r}, s[0:1] {comment}
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel _Z1kPf
\t\t.amdhsa_group_segment_fixed_size 128
\t\t.amdhsa_private_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 8
\t.end_amdhsa_kernel
\t.loc\t1 {line} 0
\t.set _Z1kPf.symbol, __hip_cuid_{cuid}
; Kernel info:
; NumVgprs: {vgpr}
; Occupancy: 8
"""


def kernel(r="v0", vgpr=1, cuid="0123abcd", comment="", line=7, more=""):
    asm = KERNEL.format(r=r, vgpr=vgpr, cuid=cuid, comment=comment, line=line, more=more)
    (name, text), = kcd.kernels(asm).items()
    assert name == "_Z1kPf" and text.startswith("_Z1kPf:") and text.rstrip().endswith("; Occupancy: 8")
    return text


def test_same_code_with_another_cuid_and_comments_is_identical():
    a, b = kernel(), kernel(cuid="fedc9876", comment="; 4-byte Folded Spill? no: a remark", line=99)
    assert a != b
    assert kcd.normalise(a) == kcd.normalise(b)
    assert not any(";" in t or t.startswith(".loc") for t in kcd.normalise(b))
    assert kcd.verdict(a, b) == ("identical", {})


def test_same_counts_in_other_registers_are_the_same_figures():
    a, b = kernel(), kernel(r="v1")                  # (the descriptor's count decides, not the names: next test)
    assert kcd.normalise(a) != kcd.normalise(b)
    assert kcd.verdict(a, b) == ("same figures", {})
    fa = kcd.figures(a)
    assert (fa["vgpr"], fa["sgpr"], fa["lds_bytes"], fa["private_bytes"], fa["occupancy"]) == (1, 8, 128, 0, 8)
    assert (fa["valu"], fa["valu_trans"], fa["salu"], fa["vmem"], fa["lds"], fa["wait_nop"], fa["branch"], fa["instructions"]) == (1, 1, 1, 1, 0, 1, 1, 6)


def test_one_more_vgpr_is_a_change_and_says_which_figure():
    a, b = kernel(), kernel(r="v1", vgpr=2)
    assert kcd.verdict(a, b) == ("changed", {"vgpr": (1, 2)})
    assert kcd.verdict(a, a.replace("fixed_size 128", "fixed_size 256")) == ("changed", {"lds_bytes": (128, 256)})
    # ... and so is one more instruction of a kind, in the same registers
    assert kcd.verdict(a, kernel(more="\n\tv_exp_f32_e32 v0, v0")) == ("changed", {"valu_trans": (1, 2)})
