#!/usr/bin/env python3
"""Reading large stored streams into a packed reply: rle_readn_batch_device_seg against the one-wave
rle_readn_batch_device and against the segmented decode into aligned slots, timed in one process on
the same files (not bench.py; DESIGN.md §4c "Segmented form" quotes the table).

  s  segmented packed   rle_readn_batch_device_seg: the layout launch, then plan, map, summary, packed
                        scan and packed write, several waves per stream, straight into the reply
  p  one-wave packed    rle_readn_batch_device: the layout launch and one wave per file
  a  aligned, segmented rle_decode_batch_device_seg of the same files into 16-byte aligned slots at
                        offsets the host knows: the floor; what byte-granular ends cost is s / a

Per shape (n files of U decoded bytes each, one synthetic kind): files generated and encoded on the
device, decoded lengths from rle_tail_batch_device; every file's header is G = 49 bytes, so a file's
row in the reply is G + U bytes, an odd number: the destinations take every phase mod 16.  `reps`
replicas of the stream arena and of every output arena, device events around `reps` back-to-back
calls (one per replica), a warm-up round, the forms alternating over `rounds` rounds, median / min /
max in us per call.  total_in_bytes is the streams' sum, read once before any timing; each segmented
form has a workspace of its own.  Before any timing the outputs are compared: s's reply with p's,
byte for byte, and both with a's slots and the content.  A form counts as faster or slower than
another only when the medians differ by more than the two forms' min-max spreads together.

usage: python tools/readn_pack_seg_sweep.py [--rounds 7] [--out profiles/readn_pack_seg.json]"""
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
SHAPES = ((1, 65536, 8), (1, 1 << 20, 8), (64, 65536, 8), (64, 1 << 20, 4), (4096, 4096, 8), (4096, 65536, 4))   # (n, U, reps)
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
    hint = int(clen.sum().item())
    streams = base.expand(reps, -1).contiguous()                    # replicas of the stream arena
    gap = i64([GAP] * n)
    cap = n * row
    reply_s = torch.full((reps, cap), POISON, dtype=torch.uint8, device=dev)
    reply_p = torch.full((reps, cap), POISON, dtype=torch.uint8, device=dev)
    slots_a = torch.full((reps, n * slot), POISON, dtype=torch.uint8, device=dev)
    place = {k: torch.zeros(n, dtype=torch.int64, device=dev) for k in "sp"}
    total = {k: torch.zeros(1, dtype=torch.int64, device=dev) for k in "sp"}
    sts = {name: torch.zeros(n, dtype=torch.int32, device=dev) for name in "spa"}
    ws_s, ws_a = R.decode_packed_seg_workspace(n, hint, dev), R.seg_workspace(n, hint, dev)
    want_place = np.arange(n, dtype=np.int64) * row + GAP

    def form_s(k):
        R.readn_batch_seg(streams[k], c_off, clen, ulen, gap, reply_s[k], place["s"], total["s"], sts["s"], out_cap=cap,
                          total_in_bytes=hint, ws=ws_s)

    def form_p(k):
        R.readn_batch(streams[k], c_off, clen, ulen, gap, reply_p[k], place["p"], total["p"], sts["p"], out_cap=cap)

    def form_a(k):
        R.decode_batch_seg(streams[k], c_off, clen, slots_a[k], x_off, ulen, None, sts["a"], total_in_bytes=hint,
                           workspace=ws_a)

    # the outputs first
    form_s(0)
    form_p(0)
    form_a(0)
    torch.cuda.synchronize()
    assert all(int(sts[k].abs().sum().item()) == 0 for k in "spa")
    for k in "sp":
        assert int(total[k].item()) == cap and np.array_equal(place[k].cpu().numpy(), want_place)
    assert torch.equal(reply_s[0], reply_p[0]), "s's reply differs from p's"
    assert bool((reply_s[0].view(n, row)[:, :GAP] == POISON).all()), "s wrote into a header gap"
    assert torch.equal(reply_s[0].view(n, row)[:, GAP:], slots_a[0].view(n, slot)[:, :U]), "s's contents differ from a's"
    assert torch.equal(slots_a[0].view(n, slot)[:, :U], d_x.view(n, slot)[:, :U]), "a is not the content"

    forms = (("s", form_s), ("p", form_p), ("a", form_a))
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
    row_ = {"n": n, "U": U, "kind": kind, "gap": GAP, "stream_bytes": hint, "reply_bytes": cap,
            "segment_bytes": R.seg_segment_bytes(hint), "reps": reps, "rounds": rounds, "outputs_equal": True}
    for name in times:
        v = sorted(times[name])
        row_[name] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2)}
    spread = lambda f: row_[f]["max_us"] - row_[f]["min_us"]   # noqa: E731
    for other in "pa":
        d = row_["s"]["median_us"] - row_[other]["median_us"]
        sp = spread("s") + spread(other)
        row_["s_over_" + other] = round(row_["s"]["median_us"] / row_[other]["median_us"], 3)
        row_["s_minus_" + other + "_us"] = round(d, 2)
        row_["s_spread_with_" + other + "_us"] = round(sp, 2)
        row_["s_vs_" + other] = "slower" if d > sp else ("faster" if -d > sp else "within the spread")
    return row_


def size_name(U):
    return f"{U >> 20} MiB" if U >= 1 << 20 else f"{U >> 10} KiB"


def table(rows):
    out = ["| files x U | kind | s | p | a | s / p | s / a |", "|---|---|---|---|---|---|---|"]
    cell = lambda r, k: f"{r[k]['median_us']:.1f} ({r[k]['min_us']:.1f}-{r[k]['max_us']:.1f})"   # noqa: E731
    for r in rows:
        out.append(f"| {r['n']} x {size_name(r['U'])} | {r['kind']} | {cell(r, 's')} | {cell(r, 'p')} | {cell(r, 'a')} | "
                   f"{r['s_over_p']:.2f} {r['s_vs_p']} | {r['s_over_a']:.2f} {r['s_vs_a']} |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kinds", default="random,runs50")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "readn_pack_seg.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "readn_pack_seg_sweep.py measures on an MI355X"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    rows = []
    for n, U, reps in SHAPES:
        for kind in a.kinds.split(","):
            rows.append(shape(n, U, kind, reps, a.rounds, dev))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    gate = [r for r in rows if r["U"] == 1 << 20]
    res = {"tool": "tools/readn_pack_seg_sweep.py", "device": torch.cuda.get_device_name(0), "library": R.version(),
           "forms": {"s": "rle_readn_batch_device_seg into a packed reply (49-byte header gaps)",
                     "p": "rle_readn_batch_device into the same reply, one wave per file",
                     "a": "rle_decode_batch_device_seg into 16-byte aligned slots"},
           "timing": "device events around `reps` back-to-back calls (one per replica of the arenas), forms "
                     "alternating over `rounds` rounds after a warm-up round; us per call of n files; median (min-max)",
           "gate": {"rule": "on 1 x 1 MiB and 64 x 1 MiB, s is faster than p by more than the two spreads together",
                    "holds": bool(gate) and all(r["s_vs_p"] == "faster" for r in gate)},
           "rows": rows, "table": table(rows).split("\n")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(table(rows))
    print("gate:", res["gate"])


if __name__ == "__main__":
    main()
