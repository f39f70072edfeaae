#!/usr/bin/env python3
"""Reading stored streams into a packed reply: rle_readn_batch_device against the aligned decode and
against what a caller had to do before, timed in one process on the same files (not bench.py;
DESIGN.md §4c quotes the table).

  p  packed reply    rle_readn_batch_device: the layout launch and the packed decode, straight into
                     the reply (header gaps left alone), lengths never leave the device
  d  aligned slots   rle_decode_batch_device of the same files into 16-byte aligned slots at offsets
                     the host knows: what byte-granular ends cost is p - d
  c  caller before   the device-to-host copy of d_ulen and the host cumsum, then d, then one device
                     gather of the slots into the packed reply

Per shape (n files of U decoded bytes each, one synthetic kind): files generated and encoded on the
device, decoded lengths from rle_tail_batch_device; every file's header is G = 49 bytes (20 + a path
of 29), so a file's row in the reply is G + U bytes, an odd number: the destinations take every phase
mod 16.  Equal lengths keep c's gather as cheap as a caller could make it: one strided device copy
(reply.view(n, G + U)[:, G:] = slots.view(n, slot)[:, :U]); its places come from the host cumsum all
the same and are checked against that stride.  `reps` replicas of the stream arena and of every
output arena, device events around `reps` back-to-back calls (one per replica; c's copy to the host
makes each of its calls wait for the one before), a warm-up round, the forms alternating over
`rounds` rounds, median / min / max in us per call.  Before any timing the outputs are compared: p's
reply with c's, byte for byte, and both with d's slots.  A form counts as faster or slower than
another only when the medians differ by more than the two forms' min-max spreads together.

usage: python tools/readn_pack_sweep.py [--rounds 7] [--out profiles/readn_pack.json]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "c-filestorage-server-and-client_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rle_mi355x as R  # noqa: E402

KINDS = {"random": 1, "runs50": 2}
SHAPES = ((64, 4096, 8), (4096, 4096, 8), (64, 65536, 8), (4096, 65536, 4))   # (n, U, reps)
GAP = 49
POISON = 0xA5


def r16(x):
    return (x + 15) & ~15


def shape(n, U, kind, reps, rounds, dev):
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)   # noqa: E731
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    kind_t = torch.full((n,), KINDS[kind], dtype=torch.int32, device=dev)
    slot, cslot, row = r16(U), r16(R.max_compressed_size(U)), GAP + U
    d_x = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    x_off, c_off, len_u = ar * slot, ar * cslot, i64([U] * n)
    R.gen_synthetic(d_x, x_off, len_u, kind_t, ar)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    base = torch.zeros(n * cslot, dtype=torch.uint8, device=dev)
    clen = torch.zeros(n, dtype=torch.int64, device=dev)
    R.encode_batch(d_x, x_off, len_u, base, c_off, clen, st)
    tail = torch.zeros(n, dtype=torch.int64, device=dev)
    ulen = torch.zeros(n, dtype=torch.int64, device=dev)
    R.tail_batch(base, c_off, clen, tail, ulen, st)
    torch.cuda.synchronize()
    assert int(st.abs().sum().item()) == 0 and bool((ulen == U).all())
    streams = base.expand(reps, -1).contiguous()                    # replicas of the stream arena
    gap = i64([GAP] * n)
    gap_h = np.full(n, GAP, np.int64)
    cap = n * row
    reply_p = torch.full((reps, cap), POISON, dtype=torch.uint8, device=dev)
    reply_c = torch.full((reps, cap), POISON, dtype=torch.uint8, device=dev)
    slots_d = torch.full((reps, n * slot), POISON, dtype=torch.uint8, device=dev)
    slots_c = torch.full((reps, n * slot), POISON, dtype=torch.uint8, device=dev)
    place = torch.zeros(n, dtype=torch.int64, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    sts = {name: torch.zeros(n, dtype=torch.int32, device=dev) for name in "pdc"}
    want_place = np.arange(n, dtype=np.int64) * row + GAP

    def form_p(k):
        R.readn_batch(streams[k], c_off, clen, ulen, gap, reply_p[k], place, total, sts["p"], out_cap=cap)

    def form_d(k):
        R.decode_batch(streams[k], c_off, clen, slots_d[k], x_off, ulen, None, sts["d"])

    def form_c(k):
        u = ulen.cpu().numpy()                      # the lengths through the host
        ends = np.cumsum(u + gap_h)
        assert ends[-1] <= cap and np.array_equal(ends - u, want_place)
        R.decode_batch(streams[k], c_off, clen, slots_c[k], x_off, ulen, None, sts["c"])
        reply_c[k].view(n, row)[:, GAP:] = slots_c[k].view(n, slot)[:, :U]   # the gather

    # the outputs first
    form_p(0)
    form_d(0)
    form_c(0)
    torch.cuda.synchronize()
    assert all(int(sts[k].abs().sum().item()) == 0 for k in "pdc")
    assert int(total.item()) == cap and np.array_equal(place.cpu().numpy(), want_place)
    assert torch.equal(reply_p[0], reply_c[0]), "p's reply differs from c's"
    assert bool((reply_p[0].view(n, row)[:, :GAP] == POISON).all()), "p wrote into a header gap"
    assert torch.equal(reply_p[0].view(n, row)[:, GAP:], slots_d[0].view(n, slot)[:, :U]), "p's contents differ from d's"
    assert torch.equal(slots_d[0].view(n, slot)[:, :U], d_x.view(n, slot)[:, :U]), "d is not the content"

    forms = (("p", form_p), ("d", form_d), ("c", form_c))
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
    row_ = {"n": n, "U": U, "kind": kind, "gap": GAP, "stream_bytes": int(clen.sum().item()), "reply_bytes": cap,
            "reps": reps, "rounds": rounds, "outputs_equal": True}
    for name in times:
        v = sorted(times[name])
        row_[name] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2)}
    spread = lambda f: row_[f]["max_us"] - row_[f]["min_us"]   # noqa: E731
    for other in "dc":
        d = row_["p"]["median_us"] - row_[other]["median_us"]
        sp = spread("p") + spread(other)
        row_["p_over_" + other] = round(row_["p"]["median_us"] / row_[other]["median_us"], 3)
        row_["p_minus_" + other + "_us"] = round(d, 2)
        row_["p_spread_with_" + other + "_us"] = round(sp, 2)
        row_["p_vs_" + other] = "slower" if d > sp else ("faster" if -d > sp else "within the spread")
    return row_


def table(rows):
    out = ["| files x U | kind | p | d | c | p / d | p / c |", "|---|---|---|---|---|---|---|"]
    cell = lambda r, k: f"{r[k]['median_us']:.1f} ({r[k]['min_us']:.1f}-{r[k]['max_us']:.1f})"   # noqa: E731
    for r in rows:
        out.append(f"| {r['n']} x {r['U'] >> 10} KiB | {r['kind']} | {cell(r, 'p')} | {cell(r, 'd')} | {cell(r, 'c')} | "
                   f"{r['p_over_d']:.2f} {r['p_vs_d']} | {r['p_over_c']:.2f} {r['p_vs_c']} |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kinds", default="random,runs50")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "readn_pack.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "readn_pack_sweep.py measures on an MI355X"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    rows = []
    for n, U, reps in SHAPES:
        for kind in a.kinds.split(","):
            rows.append(shape(n, U, kind, reps, a.rounds, dev))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    res = {"tool": "tools/readn_pack_sweep.py", "device": torch.cuda.get_device_name(0), "library": R.version(),
           "forms": {"p": "rle_readn_batch_device into a packed reply (49-byte header gaps)",
                     "d": "rle_decode_batch_device into 16-byte aligned slots",
                     "c": "d_ulen copied to the host and summed there, d, one strided device copy of the slots "
                          "into the packed reply"},
           "timing": "device events around `reps` back-to-back calls (one per replica of the arenas), forms "
                     "alternating over `rounds` rounds after a warm-up round; us per call of n files; median (min-max)",
           "rows": rows, "table": table(rows).split("\n")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(table(rows))


if __name__ == "__main__":
    main()
