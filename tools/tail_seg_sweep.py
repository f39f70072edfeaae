#!/usr/bin/env python3
"""The tail scan of streams that stay compressed in device memory: the one-wave scan against its
segmented form, timed in one process on the same streams (not bench.py; DESIGN.md §4b quotes the
table).

  b  tail scan             rle_tail_batch_device: one wave per stream walks all of its tiles
  s  segmented tail scan   rle_tail_batch_device_seg: the stream cut into segments, several waves per
                           stream (plan, map, summary, scan)
  d  segmented decode      rle_decode_batch_device_seg of the same streams: the same plan, map and
                           summary launches (s launches the decode's own summary kernel), the decode's
                           scan, and its write pass on top -- what the whole decode costs where s
                           only parses

Per shape (n streams of U content bytes each, one synthetic kind): content generated and encoded on
the device, `reps` replicas of the stream arena so that back-to-back launches do not read what the
launch before left in the caches, device events around `reps` back-to-back launches (one per
replica), a warm-up round, the forms alternating over `rounds` rounds, median / min / max.  Before
any timing the tail words, decoded lengths and status words of b and s are compared.

usage: python tools/tail_seg_sweep.py [--rounds 7] [--n 64] [--out profiles/tail_seg.json]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "c-filestorage-server-and-client_amd")]
import torch  # noqa: E402

import rle_mi355x as R  # noqa: E402

KINDS = {"random": 1, "runs50": 2}
SHAPES = ((1, 1 << 20, 8), (64, 1 << 20, 4), (1, 1 << 16, 16), (4096, 4096, 8), (4096, 1 << 16, 3))   # (n, U, reps)


def r16(x):
    return (x + 15) & ~15


def shape(n, U, kind, reps, rounds, dev):
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)   # noqa: E731
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    kind_t = torch.full((n,), KINDS[kind], dtype=torch.int32, device=dev)
    us, cap = r16(U), r16(R.max_compressed_size(U))
    d_x = torch.zeros(n * us, dtype=torch.uint8, device=dev)
    x_off, len_u = ar * us, i64([U] * n)
    R.gen_synthetic(d_x, x_off, len_u, kind_t, ar)
    s_off = ar * cap
    rep = torch.zeros(reps, n * cap, dtype=torch.uint8, device=dev)
    len_c = torch.zeros(n, dtype=torch.int64, device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    R.encode_batch(d_x, x_off, len_u, rep[0], s_off, len_c, st)
    torch.cuda.synchronize()
    assert int(st.abs().sum().item()) == 0
    rep[1:].copy_(rep[0].expand(reps - 1, -1))
    total = int(len_c.sum().item())
    res = {f: [torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev)] for f in "bs"}
    st_d = torch.zeros(n, dtype=torch.int32, device=dev)
    ws_s = R.tail_seg_workspace(n, total, dev)
    ws_d = R.seg_workspace(n, total, dev)

    def form_b(k):
        R.tail_batch(rep[k], s_off, len_c, *res["b"])

    def form_s(k):
        R.tail_batch_seg(rep[k], s_off, len_c, *res["s"], total_in_bytes=total, ws=ws_s)

    def form_d(k):
        R.decode_batch_seg(rep[k], s_off, len_c, d_x, x_off, len_u, None, st_d, total_in_bytes=total, workspace=ws_d)

    # b and s give the same tail words, decoded lengths and status words
    form_b(0)
    form_s(reps - 1)
    form_d(0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(res["b"], res["s"])), "the forms' results differ"
    assert int(res["s"][2].abs().sum().item()) == 0 and bool((res["s"][1] == U).all())
    assert int((st_d & 0xFF).sum().item()) == 0

    forms = (("b", form_b), ("s", form_s), ("d", form_d))
    times = {name: [] for name, _ in forms}
    s = torch.cuda.current_stream()
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
    row = {"n": n, "U": U, "kind": kind, "stream_bytes": total, "segment_bytes": R.seg_segment_bytes(total),
           "reps": reps, "rounds": rounds, "results_equal": True}
    for name in times:
        v = sorted(times[name])
        row[name] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2)}
    row["b_over_s"] = round(row["b"]["median_us"] / row["s"]["median_us"], 2)
    row["s_slowest_below_b_fastest"] = row["s"]["max_us"] < row["b"]["min_us"]
    row["b_slowest_below_s_fastest"] = row["b"]["max_us"] < row["s"]["min_us"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kinds", default="random,runs50")
    ap.add_argument("--n", type=int, default=0, help="only the shapes of this many streams")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tail_seg.json"))
    a = ap.parse_args()
    assert a.rounds >= 7, "at least 7 rounds"
    assert torch.cuda.is_available(), "tail_seg_sweep.py measures on an MI355X"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    rows = []
    for n, U, reps in SHAPES:
        if a.n and n != a.n:
            continue
        for kind in a.kinds.split(","):
            rows.append(shape(n, U, kind, reps, a.rounds, dev))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    res = {"tool": "tools/tail_seg_sweep.py", "device": torch.cuda.get_device_name(0), "library": R.version(),
           "forms": {"b": "rle_tail_batch_device",
                     "s": "rle_tail_batch_device_seg, total_in_bytes = the sum of the stream lengths",
                     "d": "rle_decode_batch_device_seg of the same streams (s's launches, the decode's scan, and "
                          "the write pass)"},
           "timing": "device events around `reps` back-to-back launches (one per replica of the stream arena), "
                     "forms alternating over `rounds` rounds after a warm-up round; us per launch of n streams",
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
