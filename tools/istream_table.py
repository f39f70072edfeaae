#!/usr/bin/env python3
"""Per-wave instruction stream of the small-batch codec kernels from one profiling run: for each
workload a `--kernel-trace --stats` pass (kt_<wl>/) and two separate `--pmc` passes
(pmc_<wl>/p1: SQ_WAVES and SQ_INSTS_VALU/SALU/SMEM/LDS/VMEM_RD/VMEM_WR/BRANCH; pmc_<wl>/p2:
SQ_WAVE_CYCLES, SQ_WAIT_ANY, SQ_WAIT_INST_ANY, SQ_ACTIVE_INST_ANY, SQ_ACTIVE_INST_SCA,
SQ_ACTIVE_INST_VALU) of tools/prof_driver.py.  SQ cycle counters are quad-cycles (x4 below).
usage: python tools/istream_table.py <run dir> > profiles/<name>.md"""
import collections
import csv
import os
import statistics
import sys

# workload: (decode tiles per wave (1008 B of stream), encode tiles per wave (1024 B))
WL = {"cfg1": (3.5, 4), "c4k_random": (5, 4), "c4k_zero": (2, 4), "c4k_random_q": (5, 4)}
INSTS = ("VALU", "SALU", "SMEM", "LDS", "VMEM_RD", "VMEM_WR", "BRANCH")


def kname(k):
    return k.split("(")[0].replace("void ", "").replace("rle::", "")


def pmc(path):
    vals = collections.defaultdict(lambda: collections.defaultdict(list))
    if os.path.exists(path):
        for r in csv.DictReader(open(path)):
            k = kname(r["Kernel_Name"])
            if k.startswith(("encode_kernel", "decode_kernel")):
                vals[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
    return {k: {c: statistics.mean(v) for c, v in d.items()} for k, d in vals.items()}


def main():
    d = sys.argv[1]
    rows_i, rows_c = [], []
    for wl, (dt, et) in WL.items():
        kt = os.path.join(d, f"kt_{wl}", "run_kernel_trace.csv")
        if not os.path.exists(kt):
            continue
        times = collections.defaultdict(list)
        for r in csv.DictReader(open(kt)):
            times[kname(r["Kernel_Name"])].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
        p1 = pmc(os.path.join(d, f"pmc_{wl}", "p1", "run_counter_collection.csv"))
        p2 = pmc(os.path.join(d, f"pmc_{wl}", "p2", "run_counter_collection.csv"))
        for k in sorted(p1):
            a, b = p1[k], p2.get(k, {})
            w = a["SQ_WAVES"]
            tiles = et if k.startswith("encode") else dt
            # the last 40 % of the launches: past the warm launches and the clock ramp
            t = times[k][-max(1, len(times[k]) * 2 // 5):]
            us = statistics.median(t)
            per = {c: a.get("SQ_INSTS_" + c, 0.0) / w for c in INSTS}
            # SQ_INSTS_SALU counts branches and waits with the scalar ALU ops; SMEM is separate
            tot = per["VALU"] + per["SALU"] + per["SMEM"] + per["LDS"] + per["VMEM_RD"] + per["VMEM_WR"]
            rows_i.append(f"| {wl} | {k} | {us:.2f} | {w:.0f} | " + " | ".join(f"{per[c]:.0f}" for c in INSTS) +
                          f" | {tot:.0f} | {tot / tiles:.0f} | {per['VALU'] / tiles:.0f} | {per['SALU'] / tiles:.0f} | "
                          f"{per['SALU'] / tot:.2f} |")
            if b:
                w2 = b["SQ_WAVES"]
                cyc = 4.0 * b["SQ_WAVE_CYCLES"] / w2
                rows_c.append(f"| {wl} | {k} | {cyc:.0f} | {cyc / tiles:.0f} | {cyc / tot:.2f} | "
                              f"{b['SQ_ACTIVE_INST_ANY'] / b['SQ_WAVE_CYCLES']:.2f} | "
                              f"{b['SQ_WAIT_INST_ANY'] / b['SQ_WAVE_CYCLES']:.2f} | "
                              f"{b['SQ_WAIT_ANY'] / b['SQ_WAVE_CYCLES']:.2f} | "
                              f"{4.0 * b['SQ_ACTIVE_INST_VALU'] / w2:.0f} | {4.0 * b['SQ_ACTIVE_INST_SCA'] / w2:.0f} |")
    print("| workload | kernel | µs | waves | " + " | ".join(INSTS) +
          " | issued / wave | issued / tile | VALU / tile | SALU / tile | SALU share |")
    print("|" + "---|" * (9 + len(INSTS)))
    print("\n".join(rows_i))
    print()
    print("| workload | kernel | cycles / wave | cycles / tile | cycles / issued instruction | ACTIVE_INST_ANY / WAVE_CYCLES | "
          "WAIT_INST_ANY / WAVE_CYCLES | WAIT_ANY / WAVE_CYCLES | VALU active cycles / wave | scalar active cycles / wave |")
    print("|" + "---|" * 10)
    print("\n".join(rows_c))


if __name__ == "__main__":
    main()
