#!/usr/bin/env python3
"""Register budget of the per-Gaussian kernels from hipcc's device assembly (no GPU needed).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -S --cuda-device-only X.hip -o X.s
    kernel_table.py X.s [Y.s ...]                   markdown table: registers, spills, scratch, LDS, instruction lines per kernel
    kernel_table.py --same PARENT.s X.s [Y.s ...]   every kernel of X.s, Y.s ...: same metadata and same instruction lines as in PARENT.s?

Reads the kernels' metadata and counts / compares lines (comments, directives and blank lines left out; the per-file numbering of
the branch labels removed); it does not look at what the instructions are."""
import re, sys

FIELDS = [("vgpr", ".vgpr_count"), ("vgpr spills", ".vgpr_spill_count"), ("sgpr", ".sgpr_count"), ("sgpr spills", ".sgpr_spill_count"),
          ("scratch B", ".private_segment_fixed_size"), ("LDS B", ".group_segment_fixed_size")]

def kernels(path):
    text = open(path).read()
    out = {}
    for block in text.split("\n  - .agpr_count:")[1:]:   # one entry of amdhsa.kernels each
        meta = {k: int(re.search(r"^\s+" + re.escape(k) + r":\s+(\d+)", block, re.M).group(1)) for _, k in FIELDS}
        name = re.search(r"^\s+\.name:\s+(\S+)", block, re.M).group(1)
        body = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M).group(1)
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].strip()) for l in body.split("\n")]
        lines = [l for l in lines if l and not (l.startswith(".") and not l.endswith(":"))]
        meta["instructions"] = sum(not l.endswith(":") for l in lines)
        out[name] = (meta, lines)
    return out

def short(name):
    m = re.match(r"_ZN5lvdgs12_GLOBAL__N_1(\d+)", name)
    return name[m.end():m.end() + int(m.group(1))] + ("<" + name[m.end() + int(m.group(1)):] + ">" if "ILi" in name else "") if m else name

if sys.argv[1] == "--same":
    parent, bad = kernels(sys.argv[2]), 0
    for path in sys.argv[3:]:
        for name, (meta, lines) in kernels(path).items():
            same = name in parent and parent[name] == (meta, lines)
            bad += not same
            print(("identical  " if same else "DIFFERENT  ") + f"{meta['instructions']:5d} lines  {short(name)}  ({path.split('/')[-1]})")
    sys.exit(1 if bad else 0)
cols = [f for f, _ in FIELDS] + ["instructions"]
print("| kernel | " + " | ".join(cols) + " |\n|---|" + "---|" * len(cols))
for path in sys.argv[1:]:
    for name, (meta, _) in kernels(path).items():
        print(f"| `{short(name)}` | " + " | ".join(str(meta[k]) for k in [k for _, k in FIELDS] + ["instructions"]) + " |")
