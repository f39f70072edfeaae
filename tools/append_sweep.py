#!/usr/bin/env python3
"""Appending to streams that stay compressed in device memory: the three ways a caller can do it,
timed in one process on the same files (not bench.py; DESIGN.md §4b quotes the table).

  a  scan + append      rle_tail_batch_device, then rle_append_batch_device
  b  append             rle_append_batch_device alone, tail words carried from the previous append
  c  decode, copy, encode   what the batched API offered before: rle_decode_batch_device of every
                        file, a device copy of the new bytes behind the decoded content,
                        rle_encode_batch_device of the whole

Per shape (n files, old content of U bytes each, A new bytes each, one synthetic kind): the files are
generated and encoded on the device, and `reps` replicas of the stream arena are made, because an
append changes its file: a timing is device events around `reps` back-to-back launches, one per
replica, and the replicas are restored (untimed) before the next timing.  Every shape is warmed, the
three forms alternate over `rounds` rounds, median and min are reported.  Before any timing the
three forms' streams and lengths are compared with each other.  The algorithmic bytes of each form
(what it must read and write, from the lengths) stand beside the times.

usage: python tools/append_sweep.py [--n 4096] [--reps 16] [--rounds 5] [--out profiles/append_batch.json]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "c-filestorage-server-and-client_amd")]
import torch  # noqa: E402

import rle_mi355x as R  # noqa: E402

KINDS = {"random": 1, "runs50": 2}


def r16(x):
    return (x + 15) & ~15


def shape(n, U, A, kind, reps, rounds, dev):
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)   # noqa: E731
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    kind_t = torch.full((n,), KINDS[kind], dtype=torch.int32, device=dev)
    # old content, new content (each file its own generator index), the decoded arena of form c
    us, as_ = r16(U + A), r16(A)
    d_dec = torch.zeros(n * us, dtype=torch.uint8, device=dev)
    d_new = torch.zeros(n * as_, dtype=torch.uint8, device=dev)
    dec_off, new_off = ar * us, ar * as_
    len_u, len_a, len_ua = i64([U] * n), i64([A] * n), i64([U + A] * n)
    R.gen_synthetic(d_dec, dec_off, len_u, kind_t, ar)
    R.gen_synthetic(d_new, new_off, len_a, kind_t, ar + n)
    # the stored streams: slots of the capacity an append may need
    cap = R.append_slot_bytes(R.max_compressed_size(U), A)
    assert cap and cap >= R.max_compressed_size(U + A)
    s_off, caps = ar * cap, i64([cap] * n)
    base = torch.zeros(n * cap, dtype=torch.uint8, device=dev)
    base_len = torch.zeros(n, dtype=torch.int64, device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    R.encode_batch(d_dec, dec_off, len_u, base, s_off, base_len, st)
    base_tail = torch.zeros(n, dtype=torch.int64, device=dev)
    base_ulen = torch.zeros(n, dtype=torch.int64, device=dev)
    R.tail_batch(base, s_off, base_len, base_tail, base_ulen, st)
    torch.cuda.synchronize()
    assert int(st.abs().sum().item()) == 0 and bool((base_ulen == U).all())
    rep = torch.empty(reps, n * cap, dtype=torch.uint8, device=dev)
    lens = torch.empty(reps, n, dtype=torch.int64, device=dev)
    tails = torch.empty(reps, n, dtype=torch.int64, device=dev)
    ulens = torch.empty(reps, n, dtype=torch.int64, device=dev)
    out_c = torch.zeros(n * cap, dtype=torch.uint8, device=dev)   # form c's new streams
    len_c = torch.zeros(n, dtype=torch.int64, device=dev)
    st_a, st_b, st_c = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))

    def restore():
        rep.copy_(base.expand(reps, -1))
        lens.copy_(base_len.expand(reps, -1))
        tails.copy_(base_tail.expand(reps, -1))
        ulens.copy_(base_ulen.expand(reps, -1))

    def form_a(k):
        R.tail_batch(rep[k], s_off, lens[k], tails[k], None, None)
        R.append_batch(rep[k], s_off, lens[k], caps, ulens[k], d_new, new_off, len_a, st_a, tail=tails[k])

    def form_b(k):
        R.append_batch(rep[k], s_off, lens[k], caps, ulens[k], d_new, new_off, len_a, st_b, tail=tails[k])

    def form_c(k):
        R.decode_batch(rep[k], s_off, lens[k], d_dec, dec_off, ulens[k], None, st_c)
        d_dec.view(n, us)[:, U:U + A].copy_(d_new.view(n, as_)[:, :A])
        R.encode_batch(d_dec, dec_off, len_ua, out_c, s_off, len_c, st_c)

    # the three forms give the same streams
    restore()
    form_c(2)
    form_a(0)
    form_b(1)
    torch.cuda.synchronize()
    assert int(st_a.abs().sum().item()) == 0 and int(st_b.abs().sum().item()) == 0 and int(st_c.abs().sum().item()) == 0
    assert torch.equal(lens[0], lens[1]) and torch.equal(lens[0], len_c) and torch.equal(tails[0], tails[1])
    assert bool((ulens[0] == U + A).all()) and bool((ulens[1] == U + A).all())
    same = True
    for lo in range(0, n, 256):   # (in pieces: the masks are n x cap)
        hi = min(n, lo + 256)
        live = torch.arange(cap, device=dev)[None, :] < lens[0][lo:hi, None]
        va, vb, vc = (t.view(n, cap)[lo:hi] for t in (rep[0], rep[1], out_c))
        same = same and bool(((va == vb) | ~live).all()) and bool(((va == vc) | ~live).all())
    assert same, "the forms' streams differ"
    c_old, c_new = int(base_len.sum().item()), int(len_c.sum().item())
    kept = int((base_tail & 0xFFFFFFFF).sum().item())   # the bytes below every old final token
    written = c_new - kept   # bytes from each old final token's offset to the new end
    nbytes = {
        "a": {"read": c_old + n * A, "write": written},
        "b": {"read": n * A, "write": written},
        "c": {"read": c_old + n * A + n * (U + A), "write": n * U + n * A + c_new},
    }

    times = {"a": [], "b": [], "c": []}
    s = torch.cuda.current_stream()
    for rnd in range(rounds + 1):   # round 0 warms every form at this shape
        for name, fn in (("a", form_a), ("b", form_b), ("c", form_c)):
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
    row = {"n": n, "U": U, "A": A, "kind": kind, "old_stream_bytes": c_old, "new_stream_bytes": c_new,
           "reps": reps, "rounds": rounds, "outputs_equal": True}
    for name in times:
        v = sorted(times[name])
        row[name] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2),
                     "read_bytes": nbytes[name]["read"], "write_bytes": nbytes[name]["write"]}
    row["c_over_b"] = round(row["c"]["median_us"] / row["b"]["median_us"], 2)
    row["c_over_a"] = round(row["c"]["median_us"] / row["a"]["median_us"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--old", default="4096,65536")
    ap.add_argument("--new", default="64,4096")
    ap.add_argument("--kinds", default="random,runs50")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "append_batch.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "append_sweep.py measures on an MI355X"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    rows = []
    for U in (int(v) for v in a.old.split(",")):
        for A in (int(v) for v in a.new.split(",")):
            for kind in a.kinds.split(","):
                rows.append(shape(a.n, U, A, kind, a.reps, a.rounds, dev))
                print(json.dumps(rows[-1]), flush=True)
                torch.cuda.empty_cache()
    res = {"tool": "tools/append_sweep.py", "device": torch.cuda.get_device_name(0), "library": R.version(),
           "forms": {"a": "rle_tail_batch_device + rle_append_batch_device",
                     "b": "rle_append_batch_device, tail words carried",
                     "c": "rle_decode_batch_device + strided device copy of the new bytes + rle_encode_batch_device"},
           "timing": "device events around `reps` back-to-back launches (one per replica of the stream arena), "
                     "forms alternating over `rounds` rounds after a warm-up round; us per launch of n files",
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
