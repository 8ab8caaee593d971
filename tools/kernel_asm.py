"""What the tools that read the compiler's gfx950 assembly share (isa_budget.py, kernel_code_diff.py): how a .hip file of csrc/ is
compiled to assembly -- with the Makefile's own HIPFLAGS, read from the Makefile, so the flags are stated once -- and how an
instruction is classified by kind.  Needs no GPU."""
import os, re, subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("lvd_gs-slam_amd", "csrc")


def hipflags(root=ROOT, extra=()):
    """(hipcc, flags) of the csrc/Makefile of the tree at `root`; `extra` stands where the Makefile has $(EXTRA)."""
    text = open(os.path.join(root, CSRC, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M).group(1).strip()
    flags = []
    for f in var("HIPFLAGS").split():
        if f == "$(EXTRA)": flags += list(extra)
        else: flags.append(f.replace("$(ARCH)", var("ARCH")))
    return os.environ.get("HIPCC", var("HIPCC")), flags


def compile_asm(src, root=ROOT, extra=()):
    """The device assembly of one .hip file (a path, or a name in csrc/) of the tree at `root`."""
    if not os.path.isabs(src) and not os.path.exists(src): src = os.path.join(root, CSRC, src)
    hipcc, flags = hipflags(root, extra)
    r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", src, "-o", "-"], capture_output=True, text=True)
    if r.returncode: raise SystemExit(r.stderr)
    return r.stdout


KINDS = ["valu", "valu_trans", "valu_dpp", "valu_xlane", "salu", "lds", "vmem", "branch", "wait_nop"]
DPP_WORDS = ("row_ror", "row_shr", "row_bcast", "quad_perm", "row_mirror", "row_half_mirror")


def kind(op):
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier")): return "wait_nop"
    if op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc")): return "branch"
    if op.startswith("s_"): return "salu"
    if op.startswith("ds_"): return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")): return "vmem"
    if op.startswith(("v_exp", "v_rcp", "v_log", "v_sqrt", "v_rsq", "v_sin", "v_cos")): return "valu_trans"
    if op.startswith(("v_permlane", "v_readlane", "v_writelane", "v_readfirstlane")): return "valu_xlane"
    if op.startswith("v_"): return "valu"
    return None


def line_kind(line):
    """(kind, opcode) of one line of assembly; None for labels, directives, comments and blank lines."""
    t = line.strip()
    if not t or t.startswith((";", ".")) or t.endswith(":"): return None
    op = t.split()[0]
    k = kind(op)
    if k is None: return None
    if k == "valu" and ("_dpp" in op or any(w in t for w in DPP_WORDS)): k = "valu_dpp"
    return k, op
