#!/usr/bin/env python3
"""Static instruction count per class of every kernel in hipcc ISA listings (make -C <pkg> asm):
vector ALU, scalar ALU, scalar memory, LDS, vector memory, branch, no-op, wait.  With two listing
directories, prints only the kernels whose counts differ (the check that a change confined to some
instantiations left every other kernel's instruction stream alone).
usage: python tools/asm_classes.py DIR [DIR_BEFORE] [--match SUBSTR]"""
import collections
import glob
import os
import re
import sys

CLASSES = ("valu", "salu", "smem", "lds", "vmem", "branch", "nop", "wait")


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op == "s_waitcnt":
        return "wait"
    if op == "s_nop":
        return "nop"
    if op.startswith("s_cbranch") or op in ("s_branch", "s_setpc_b64", "s_swappc_b64", "s_endpgm"):
        return "branch"
    if op.startswith(("s_load_", "s_buffer_load_", "s_memtime", "s_memrealtime")):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    return None


def count(d):
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        cur = None
        for l in open(path):
            m = re.match(r"^(_Z\w+):", l)
            if m:
                cur = out.setdefault((os.path.basename(path), m.group(1)), collections.Counter())
                continue
            if l.startswith(".Lfunc_end"):
                cur = None
                continue
            t = l.strip()
            if cur is None or not t or t[0] in ";.":
                continue
            c = classify(t.split()[0])
            if c:
                cur[c] += 1
    return out


def row(c):
    return " ".join(f"{k} {c[k]}" for k in CLASSES) + f" total {sum(c.values())}"


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    match = sys.argv[sys.argv.index("--match") + 1] if "--match" in sys.argv else ""
    if "--match" in sys.argv:
        args.remove(match)
    new = count(args[0])
    if len(args) == 1:
        for k, c in new.items():
            if match in k[1]:
                print(k[0], k[1], row(c))
        return 0
    old = count(args[1])
    changed = [k for k in sorted(set(new) | set(old)) if new.get(k) != old.get(k)]
    for k in changed:
        print(k[0], k[1])
        print("   before:", row(old[k]) if k in old else "-")
        print("   after: ", row(new[k]) if k in new else "-")
    print(f"{len(new)} kernels, {len(changed)} changed")
    return 0


if __name__ == "__main__":
    sys.exit(main())
