#!/usr/bin/env python3
"""Does a change to the source leave the code the chip runs alone?  Compiles the named .hip files (default: blend.hip) of two
trees to gfx950 assembly, each with its own Makefile's HIPFLAGS plus any EXTRA, and compares them kernel by kernel.  Needs no GPU;
a file takes seconds.

    python3 tools/kernel_code_diff.py <tree A> <tree B> [file.hip ...] [--extra=-DLVDGS_DIAG_FILL ... or EXTRA=... in the environment] [--markdown]

Verdict per kernel:
    identical     the same text once comments, .loc / .file / .ident lines and the __hip_cuid_* symbol are dropped;
    same figures  VGPR, SGPR, LDS, private segment and the instruction counts by kind (tools/kernel_asm.py) are all equal;
    changed       with the figures that differ.
Exit status 1 on any `changed` (a kernel present in one tree only counts as changed).  The tool compares and counts; it looks for
no particular instruction.  --markdown prints the table of profiles/blend_stages/README.md (A -> B)."""
import argparse, collections, os, re, subprocess, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_asm import KINDS, compile_asm, line_kind

RESOURCES = [("vgpr", r"\.amdhsa_next_free_vgpr\s+(\d+)"), ("sgpr", r"\.amdhsa_next_free_sgpr\s+(\d+)"),
             ("lds_bytes", r"\.amdhsa_group_segment_fixed_size\s+(\d+)"), ("private_bytes", r"\.amdhsa_private_segment_fixed_size\s+(\d+)")]


def normalise(asm):
    """The assembly without what differs between two builds of the same code."""
    out = []
    for line in asm.split("\n"):
        t = line.split(";")[0].strip()
        if not t or re.match(r"\.(loc|file|ident)\b", t): continue
        out.append(re.sub(r"__hip_cuid_\w+", "__hip_cuid", re.sub(r"\s+", " ", t)))
    return out


def kernels(asm):
    """{kernel symbol: its text, from its label to the end of the compiler's "Kernel info" note} of one file's assembly, in order."""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    starts = [(m.start(), m.group(1)) for m in re.finditer(r"^(\S+):", asm, re.M) if m.group(1) in names]
    ends = [s for s, _ in starts[1:]] + [len(asm)]
    out = collections.OrderedDict()
    for (s, name), e in zip(starts, ends):
        text = asm[s:e]
        note = re.search(r"^; Kernel info:\n(;.*\n)*", text, re.M)   # (what follows is the next function's header, or the file's tail)
        out[name] = text[:note.end()] if note else text
    return out


def figures(text):
    """Resources from the kernel descriptor, occupancy from the compiler's note, instruction counts by kind."""
    f = collections.OrderedDict()
    for key, pat in RESOURCES:
        m = re.search(pat, text)
        f[key] = int(m.group(1)) if m else None
    m = re.search(r";\s*Occupancy:\s*(\d+)", text)
    f["occupancy"] = int(m.group(1)) if m else None
    counts = collections.Counter(ko[0] for ko in map(line_kind, text.split("\n")) if ko)
    for k in KINDS: f[k] = counts[k]
    f["instructions"] = sum(counts.values())
    return f


def verdict(a, b):
    """('identical' | 'same figures' | 'changed', {figure: (a, b)} of the figures that differ) for one kernel's text in two builds."""
    if normalise(a) == normalise(b): return "identical", {}
    fa, fb = figures(a), figures(b)
    diff = {k: (fa[k], fb[k]) for k in fa if k != "occupancy" and k != "instructions" and fa[k] != fb[k]}
    return ("changed" if diff else "same figures"), diff


def demangle(names):
    try: return dict(zip(names, subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True).stdout.split("\n")))
    except (OSError, subprocess.CalledProcessError): return {n: n for n in names}


def short(name):
    name = re.sub(r"^void ", "", name).replace("lvdgs::(anonymous namespace)::", "").replace("lvdgs::", "")
    return re.sub(r"\((\w|::|[ ,*&()])*\)$", "", name)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a"); ap.add_argument("tree_b"); ap.add_argument("files", nargs="*", default=["blend.hip"])
    ap.add_argument("--extra", action="append", default=[], help="a flag where the Makefile has $(EXTRA); may be repeated")
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    args.extra = args.extra or os.environ.get("EXTRA", "").split()   # (as `make EXTRA=...` would be given it)
    changed = 0
    for f in args.files:
        ka, kb = (kernels(compile_asm(f, root=os.path.abspath(t), extra=args.extra)) for t in (args.tree_a, args.tree_b))
        names = list(ka) + [n for n in kb if n not in ka]
        pretty = demangle(names)
        print(f"{'### ' if args.markdown else ''}{f}{' ' + ' '.join(args.extra) if args.extra else ''}: {len(names)} kernels\n")
        if args.markdown:
            print("| kernel | VGPR | SGPR | LDS | scratch | occupancy | instructions | verdict |\n|---|---|---|---|---|---|---|---|")
        tally = collections.Counter()
        for n in names:
            if n not in ka or n not in kb:
                v, diff = "changed", {"present": (n in ka, n in kb)}
            else:
                v, diff = verdict(ka[n], kb[n])
            tally[v] += 1
            changed += v == "changed"
            if args.markdown and n in ka and n in kb:
                fa, fb = figures(ka[n]), figures(kb[n])
                note = "".join(f"; {k} {x} -> {y}" for k, (x, y) in diff.items() if k in KINDS)
                print(f"| `{short(pretty[n])}` | " + " | ".join(f"{fa[k]} -> {fb[k]}" for k in ("vgpr", "sgpr", "lds_bytes", "private_bytes", "occupancy", "instructions")) + f" | {v}{note} |")
            else:
                print(f"{v:13s} {short(pretty[n])}" + "".join(f"  {k}: {x} -> {y}" for k, (x, y) in diff.items()))
        print("\n" + ", ".join(f"{c} {v}" for v, c in tally.items()) + "\n")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
