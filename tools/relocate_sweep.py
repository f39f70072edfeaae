#!/usr/bin/env python3
"""Relocating stored streams: rle_relocate_batch_device against the streaming copy of the same bytes
and against what a caller had to do before, timed in one process on the same arenas (not bench.py;
DESIGN.md §4d quotes the table).

  r  relocation      rle_relocate_batch_device: the layout launch and the copy launch that follows the
                     per-file map on the device; sizes never leave the device
  m  plain copy      rle_copy_device of the same number of copied bytes, one contiguous range: the
                     ceiling of any relocation (no map, no gaps); the ratio r / m goes in the table
  h  host route      what a caller had to do before: d_len and d_want copied to the host with a
                     synchronise, the slots laid out there, d_new_off and d_new_cap uploaded, and one
                     hipMemcpyAsync device-to-device per file (the source offsets are the host's own
                     copy, at no cost)

Per shape (n streams of C bytes each, random bytes: a copy does not care): the streams packed in the
source arena; twice, with want = C (slots as tight as the streams) and with want = the worst-case slot
of an append of as many bytes again (rle_append_slot_bytes(C, C): gaps larger than the streams).
dst_cap is the layout's total: the room this relocation takes.  `reps` replicas of the source and of
every destination arena, device events around `reps` back-to-back calls (one per replica; h's copy to
the host makes each of its calls wait for the one before), a warm-up round, the forms alternating over
`rounds` rounds, median / min / max in us per call.  Before any timing the outputs are compared: r's
destination with h's, byte for byte over the poison, and r's with m's where the slots are tight.  A
form counts as faster or slower than another only when the medians differ by more than the two forms'
min-max spreads together.

usage: python tools/relocate_sweep.py [--rounds 7] [--sizes 4096,65536] [--out profiles/relocate.json]"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "c-filestorage-server-and-client_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rle_mi355x as R  # noqa: E402

SHAPES = ((1, 4096, 8), (64, 4096, 8), (4096, 4096, 8), (1, 65536, 8), (64, 65536, 8), (4096, 65536, 3),
          (1, 1 << 20, 8), (64, 1 << 20, 4))   # (n, C, reps)
POISON = 0xA5
D2D = 3   # hipMemcpyDeviceToDevice


def r16(x):
    return (x + 15) & ~15


def hip_runtime():
    """The HIP runtime this process already uses (torch's), for the host route's hipMemcpyAsync."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "no HIP runtime is loaded"
    hip = ctypes.CDLL(paths[0])
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    return hip


def shape(n, C, slots, reps, rounds, dev, hip):
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)   # noqa: E731
    assert C % 16 == 0
    want_h = [C if slots == "tight" else R.append_slot_bytes(C, C)] * n
    cap = r16(max(want_h[0], C))
    total = n * cap
    src = torch.randint(0, 256, (reps, n * C), dtype=torch.uint8, device=dev)
    soff_h = [i * C for i in range(n)]
    off, length, want = i64(soff_h), i64([C] * n), i64(want_h)
    dst = {k: torch.full((reps, total), POISON, dtype=torch.uint8, device=dev) for k in "rh"}
    dst["m"] = torch.full((reps, n * C), POISON, dtype=torch.uint8, device=dev)
    new_off = {k: torch.zeros(n, dtype=torch.int64, device=dev) for k in "rh"}
    new_cap = {k: torch.zeros(n, dtype=torch.int64, device=dev) for k in "rh"}
    d_total = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream()
    sp = ctypes.c_void_p(s.cuda_stream)

    def form_r(k):
        R.relocate_batch(src[k], off, length, dst["r"][k], new_off["r"], new_cap["r"], d_total, want=want,
                         status=status, dst_cap=total)

    def form_m(k):
        R.copy_device(dst["m"][k], src[k], n * C)

    def form_h(k):
        ln, wn = length.cpu().numpy(), want.cpu().numpy()            # the sizes through the host
        caps = (np.maximum(ln, wn) + 15) & ~15
        offs = np.cumsum(caps) - caps
        assert offs[-1] + caps[-1] <= total
        new_off["h"].copy_(torch.from_numpy(offs), non_blocking=True)
        new_cap["h"].copy_(torch.from_numpy(caps), non_blocking=True)
        d, sbase = dst["h"][k].data_ptr(), src[k].data_ptr()
        for i in range(n):
            rc = hip.hipMemcpyAsync(d + int(offs[i]), sbase + soff_h[i], int(ln[i]), D2D, sp)
            assert rc == 0, rc

    # the outputs first
    for fn in (form_r, form_m, form_h):
        fn(0)
    torch.cuda.synchronize()
    assert int(status.abs().sum().item()) == 0 and int(d_total.item()) == total
    assert torch.equal(new_off["r"], new_off["h"]) and torch.equal(new_cap["r"], new_cap["h"])
    assert torch.equal(dst["r"][0], dst["h"][0]), "r's destination differs from h's"
    assert torch.equal(dst["r"][0].view(n, cap)[:, :C], src[0].view(n, C)), "r is not the streams"
    assert bool((dst["r"][0].view(n, cap)[:, C:] == POISON).all()), "r wrote into a gap"
    assert torch.equal(dst["m"][0], src[0])

    forms = (("r", form_r), ("m", form_m), ("h", form_h))
    times = {name: [] for name, _ in forms}
    for rnd in range(rounds + 1):   # round 0 warms every form at this shape
        for name, fn in forms:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for k in range(reps):
                fn(k)
            e1.record(s)
            torch.cuda.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1) / reps * 1e3)
    room = total
    row = {"n": n, "C": C, "slots": slots, "want": want_h[0], "copied_bytes": n * C, "room_bytes": room,
           "span_bytes": R.relocate_span_bytes(room), "reps": reps, "rounds": rounds, "outputs_equal": True}
    for name in times:
        v = sorted(times[name])
        row[name] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2)}
    row["r_copy_GBps"] = round(2 * n * C / row["r"]["median_us"] / 1e3, 1)   # bytes read + bytes written
    spread = lambda f: row[f]["max_us"] - row[f]["min_us"]   # noqa: E731
    for other in "mh":
        d = row["r"]["median_us"] - row[other]["median_us"]
        sp_ = spread("r") + spread(other)
        row["r_over_" + other] = round(row["r"]["median_us"] / row[other]["median_us"], 3)
        row["r_minus_" + other + "_us"] = round(d, 2)
        row["r_spread_with_" + other + "_us"] = round(sp_, 2)
        row["r_vs_" + other] = "slower" if d > sp_ else ("faster" if -d > sp_ else "within the spread")
    return row


def size_name(c):
    return f"{c >> 20} MiB" if c >= 1 << 20 else f"{c >> 10} KiB"


def table(rows):
    out = ["| streams x C | slots | r | m | h | r / m | r / h |", "|---|---|---|---|---|---|---|"]
    cell = lambda r, k: f"{r[k]['median_us']:.1f} ({r[k]['min_us']:.1f}-{r[k]['max_us']:.1f})"   # noqa: E731
    for r in rows:
        out.append(f"| {r['n']} x {size_name(r['C'])} | {r['slots']} | {cell(r, 'r')} | {cell(r, 'm')} | {cell(r, 'h')} | "
                   f"{r['r_over_m']:.2f} {r['r_vs_m']} | {r['r_over_h']:.2f} {r['r_vs_h']} |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="", help="comma-separated stream sizes C to run (default: all)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "relocate.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "relocate_sweep.py measures on an MI355X"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    hip = hip_runtime()
    rows = []
    sizes = {int(c) for c in a.sizes.split(",") if c}
    for n, C, reps in SHAPES:
        if sizes and C not in sizes:
            continue
        for slots in ("tight", "worst-case"):
            rows.append(shape(n, C, slots, reps, a.rounds, dev, hip))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    res = {"tool": "tools/relocate_sweep.py", "device": torch.cuda.get_device_name(0), "library": R.version(),
           "forms": {"r": "rle_relocate_batch_device (layout launch + one copy launch)",
                     "m": "rle_copy_device of the same number of copied bytes, one contiguous range (the ceiling)",
                     "h": "d_len and d_want copied to the host with a synchronise, the slots laid out there, the "
                          "offsets and capacities uploaded, one hipMemcpyAsync device-to-device per file"},
           "slots": {"tight": "want = C", "worst-case": "want = rle_append_slot_bytes(C, C)"},
           "timing": "device events around `reps` back-to-back calls (one per replica of the arenas), forms "
                     "alternating over `rounds` rounds after a warm-up round; us per call of n streams; median (min-max)",
           "rows": rows, "table": table(rows).split("\n")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(table(rows))


if __name__ == "__main__":
    main()
