#!/usr/bin/env python3
"""Static instruction counts of the kernels in a device assembly file.

    hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 --cuda-device-only -S \
        csrc/cg.hip -o cg.s
    python scripts/count_vector_ops.py cg.s k_cg_step2_hpILb0ELi3ELi3ELb0ELb1ELb0ELb0ELb1E

For every kernel whose (mangled) name contains the fragment it prints the number of
instructions and four counts, classified by the opcode's prefix alone:

    v_        vector ALU
    ds_       LDS
    global_   global memory accesses
    off       of the global accesses, those whose last operand is `off`: the address is a
              64-bit vector register pair, no scalar base

The counts are static: one per instruction in the kernel's text, whatever a loop or a
branch makes of it at run time.  DESIGN.md section 3 quotes them for the two loop kernels.
"""
import re
import sys

LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")


def kernels(path):
    """{symbol: [instruction lines]} for every global function of the file."""
    out, cur = {}, None
    for line in open(path):
        m = LABEL.match(line)
        if m and not m.group(1).startswith("."):
            cur = out.setdefault(m.group(1), [])
            continue
        if line.startswith(".Lfunc_end") or line.lstrip().startswith(".end_amdhsa_kernel"):
            cur = None
            continue
        if cur is None:
            continue
        s = line.split(";", 1)[0].strip()
        if not s or s.startswith(".") or LABEL.match(s):
            continue
        cur.append(s)
    return out


def count(lines):
    c = {"total": len(lines), "v_": 0, "ds_": 0, "global_": 0, "off": 0}
    for s in lines:
        op = s.split()[0]
        for prefix in ("v_", "ds_", "global_"):
            if op.startswith(prefix):
                c[prefix] += 1
        if op.startswith("global_") and "off" in s.replace(",", " ").split()[1:]:
            c["off"] += 1
    return c


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    found = 0
    for name, lines in kernels(argv[1]).items():
        if argv[2] not in name or not lines:
            continue
        found += 1
        c = count(lines)
        print(f"{name}\n  instructions {c['total']}  v_ {c['v_']}  ds_ {c['ds_']}  "
              f"global_ {c['global_']}  of those off {c['off']}")
    if not found:
        print(f"no kernel matching {argv[2]!r} in {argv[1]}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
