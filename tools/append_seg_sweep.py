#!/usr/bin/env python3
"""Large appends to streams that stay compressed in device memory: the one-wave append against its
segmented form, timed in one process on the same files (not bench.py; DESIGN.md §4b quotes the
table).

  b  append             rle_append_batch_device: one wave per file walks all of the new bytes
  s  segmented append   rle_append_batch_device_seg: the new bytes cut into segments, several waves
                        per file (plan, map, entry, summary, scan, write)
  e  segmented encode   rle_encode_batch_device_seg of the new bytes alone into a separate arena:
                        the same bytes with no splice, the floor for s

Per shape (n files of U old bytes each, A new bytes each, one synthetic kind): as tools/
append_sweep.py -- files generated and encoded on the device, `reps` replicas of the stream arena
because an append changes its file, device events around `reps` back-to-back launches (one per
replica), replicas restored untimed before every timing, a warm-up round, the forms alternating over
`rounds` rounds, median / min / max.  Before any timing the streams, lengths, decoded lengths and
tail words of b and s are compared.  s counts as faster than b only when the medians differ by more
than the two forms' min-max spreads together.

usage: python tools/append_seg_sweep.py [--rounds 7] [--n 64] [--out profiles/append_seg.json]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "c-filestorage-server-and-client_amd")]
import torch  # noqa: E402

import rle_mi355x as R  # noqa: E402

KINDS = {"random": 1, "runs50": 2}
SHAPES = ((1, 1 << 20, 8), (64, 1 << 20, 4), (1, 1 << 16, 16), (4096, 4096, 8))   # (n, A, reps)
OLD = 4096


def r16(x):
    return (x + 15) & ~15


def shape(n, U, A, kind, reps, rounds, dev):
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)   # noqa: E731
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    kind_t = torch.full((n,), KINDS[kind], dtype=torch.int32, device=dev)
    us, as_ = r16(U), r16(A)
    d_old = torch.zeros(n * us, dtype=torch.uint8, device=dev)
    d_new = torch.zeros(n * as_, dtype=torch.uint8, device=dev)
    old_off, new_off = ar * us, ar * as_
    len_u, len_a = i64([U] * n), i64([A] * n)
    R.gen_synthetic(d_old, old_off, len_u, kind_t, ar)
    R.gen_synthetic(d_new, new_off, len_a, kind_t, ar + n)
    cap = R.append_slot_bytes(R.max_compressed_size(U), A)
    assert cap
    s_off, caps = ar * cap, i64([cap] * n)
    base = torch.zeros(n * cap, dtype=torch.uint8, device=dev)
    base_len = torch.zeros(n, dtype=torch.int64, device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    R.encode_batch(d_old, old_off, len_u, base, s_off, base_len, st)
    base_tail = torch.zeros(n, dtype=torch.int64, device=dev)
    base_ulen = torch.zeros(n, dtype=torch.int64, device=dev)
    R.tail_batch(base, s_off, base_len, base_tail, base_ulen, st)
    torch.cuda.synchronize()
    assert int(st.abs().sum().item()) == 0 and bool((base_ulen == U).all())
    rep = torch.empty(reps, n * cap, dtype=torch.uint8, device=dev)
    lens = torch.empty(reps, n, dtype=torch.int64, device=dev)
    tails = torch.empty(reps, n, dtype=torch.int64, device=dev)
    ulens = torch.empty(reps, n, dtype=torch.int64, device=dev)
    e_cap = r16(R.max_compressed_size(A))
    out_e = torch.zeros(n * e_cap, dtype=torch.uint8, device=dev)
    e_off, len_e = ar * e_cap, torch.zeros(n, dtype=torch.int64, device=dev)
    st_b, st_s, st_e = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
    total = n * A
    ws_s = R.append_seg_workspace(n, total, dev)
    ws_e = R.seg_workspace(n, total, dev)

    def restore():
        rep.copy_(base.expand(reps, -1))
        lens.copy_(base_len.expand(reps, -1))
        tails.copy_(base_tail.expand(reps, -1))
        ulens.copy_(base_ulen.expand(reps, -1))

    def form_b(k):
        R.append_batch(rep[k], s_off, lens[k], caps, ulens[k], d_new, new_off, len_a, st_b, tail=tails[k])

    def form_s(k):
        R.append_batch_seg(rep[k], s_off, lens[k], caps, ulens[k], d_new, new_off, len_a, st_s, total_new_bytes=total,
                           workspace=ws_s, tail=tails[k])

    def form_e(k):
        R.encode_batch_seg(d_new, new_off, len_a, out_e, e_off, len_e, st_e, total_in_bytes=total, workspace=ws_e)

    # b and s give the same streams, lengths, decoded lengths and tail words
    restore()
    form_b(0)
    form_s(1)
    form_e(0)
    torch.cuda.synchronize()
    assert int(st_b.abs().sum().item()) == 0 and int(st_s.abs().sum().item()) == 0 and int(st_e.abs().sum().item()) == 0
    assert torch.equal(lens[0], lens[1]) and torch.equal(tails[0], tails[1]) and torch.equal(ulens[0], ulens[1])
    assert bool((ulens[1] == U + A).all())
    same = True
    step = max(1, (64 << 20) // cap)   # (in pieces: the masks are n x cap)
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        live = torch.arange(cap, device=dev)[None, :] < lens[0][lo:hi, None]
        vb, vs = (t.view(n, cap)[lo:hi] for t in (rep[0], rep[1]))
        same = same and bool(((vb == vs) | ~live).all())
    assert same, "the forms' streams differ"
    c_new = int(lens[0].sum().item())

    forms = (("b", form_b), ("s", form_s), ("e", form_e))
    times = {name: [] for name, _ in forms}
    s = torch.cuda.current_stream()
    for rnd in range(rounds + 1):   # round 0 warms every form at this shape
        for name, fn in forms:
            restore()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for k in range(reps):
                fn(k)
            e1.record(s)
            torch.cuda.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1) / reps * 1e3)
    row = {"n": n, "U": U, "A": A, "kind": kind, "segment_bytes": R.seg_segment_bytes(total),
           "new_stream_bytes": c_new, "encoded_new_bytes": int(len_e.sum().item()), "reps": reps, "rounds": rounds,
           "outputs_equal": True}
    for name in times:
        v = sorted(times[name])
        row[name] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2)}
    spread = lambda f: row[f]["max_us"] - row[f]["min_us"]   # noqa: E731
    row["b_over_s"] = round(row["b"]["median_us"] / row["s"]["median_us"], 2)
    row["s_over_e"] = round(row["s"]["median_us"] / row["e"]["median_us"], 2)
    row["spread_b_plus_s_us"] = round(spread("b") + spread("s"), 2)
    row["s_faster_than_b_beyond_spread"] = row["b"]["median_us"] - row["s"]["median_us"] > spread("b") + spread("s")
    row["s_slower_than_e_beyond_spread"] = row["s"]["median_us"] - row["e"]["median_us"] > spread("s") + spread("e")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kinds", default="random,runs50")
    ap.add_argument("--n", type=int, default=0, help="only the shapes of this many files (under a kernel trace)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "append_seg.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "append_seg_sweep.py measures on an MI355X"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    rows = []
    for n, A, reps in SHAPES:
        if a.n and n != a.n:
            continue
        for kind in a.kinds.split(","):
            rows.append(shape(n, OLD, A, kind, reps, a.rounds, dev))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    res = {"tool": "tools/append_seg_sweep.py", "device": torch.cuda.get_device_name(0), "library": R.version(),
           "forms": {"b": "rle_append_batch_device, tail words carried",
                     "s": "rle_append_batch_device_seg, tail words carried, total_new_bytes = n * A",
                     "e": "rle_encode_batch_device_seg of the new bytes alone (no splice)"},
           "timing": "device events around `reps` back-to-back launches (one per replica of the stream arena), "
                     "forms alternating over `rounds` rounds after a warm-up round; us per launch of n files",
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
