#!/usr/bin/env python3
"""Large appends to streams that stay compressed in device memory: the one-wave append against its
segmented form (DESIGN.md §4b quotes the table; the method is tools/sweeplib.py's).

  b  append             rle_append_batch_device: one wave per file walks all of the new bytes
  s  segmented append   rle_append_batch_device_seg: the new bytes cut into segments, several waves
                        per file (plan, map, entry, summary, scan, write)
  e  segmented encode   rle_encode_batch_device_seg of the new bytes alone into a separate arena:
                        the same bytes with no splice, the floor for s

Per shape (n files of U old bytes each, A new bytes each, one synthetic kind): as tools/
append_sweep.py -- files generated and encoded on the device, the replicas of the stream arena
restored untimed before every timing.  Before any timing the streams, lengths, decoded lengths and
tail words of b and s are compared.  The row says whether s is faster than b, and slower than e,
by more than the two forms' min-max spreads together.

usage: python tools/append_seg_sweep.py [--rounds 7] [--n 64] [--shapes 2] [--out profiles/append_seg.json]"""
import sweeplib as S
import torch
from sweeplib import R

SHAPES = ((1, 1 << 20, 8), (64, 1 << 20, 4), (1, 1 << 16, 16), (4096, 4096, 8))   # (n, A, reps)
OLD = 4096
FORMS = {"b": "rle_append_batch_device, tail words carried",
         "s": "rle_append_batch_device_seg, tail words carried, total_new_bytes = n * A",
         "e": "rle_encode_batch_device_seg of the new bytes alone (no splice)"}
TIMING = S.timing_text("launch", "the stream arena", "files", cells=False)


def shape(a, s, kind, dev):
    (n, A, reps), U, rounds = s, OLD, a.rounds
    cap = R.append_slot_bytes(R.max_compressed_size(U), A)
    assert cap
    f = S.stored_files(n, U, kind, cap, dev)
    d_new, new_off, len_a = S.gen_files(n, A, kind, dev, index_base=n)
    s_off, caps = f.s_off, torch.full_like(len_a, cap)
    rep, lens, tails, ulens, restore = S.replicas(reps, f.streams, f.clen, f.tail, f.ulen)
    e_cap = S.r16(R.max_compressed_size(A))
    out_e = torch.zeros(n * e_cap, dtype=torch.uint8, device=dev)
    e_off, len_e = torch.arange(n, dtype=torch.int64, device=dev) * e_cap, torch.zeros(n, dtype=torch.int64, device=dev)
    st_b, st_s, st_e = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
    total = n * A
    ws_s = R.append_seg_workspace(n, total, dev)
    ws_e = R.seg_workspace(n, total, dev)

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
    assert S.same_streams(rep[0], rep[1], lens[0], cap), "the forms' streams differ"
    c_new = int(lens[0].sum().item())

    times = S.time_forms((("b", form_b), ("s", form_s), ("e", form_e)), reps, rounds, before=restore)
    row = {"n": n, "U": U, "A": A, "kind": kind, "segment_bytes": R.seg_segment_bytes(total),
           "new_stream_bytes": c_new, "encoded_new_bytes": int(len_e.sum().item()), "reps": reps, "rounds": rounds,
           "outputs_equal": True}
    row.update((name, S.stats(v)) for name, v in times.items())
    return judged(row)


def judged(row):
    """This tool's older row fields, from the shared verdicts of b against s and of s against e."""
    v = dict(row)
    S.verdict(v, "b", "s", 2)
    S.verdict(v, "s", "e", 2)
    row.update(b_over_s=v["b_over_s"], s_over_e=v["s_over_e"], spread_b_plus_s_us=v["b_spread_with_s_us"],
               s_faster_than_b_beyond_spread=v["b_vs_s"] == "slower", s_slower_than_e_beyond_spread=v["s_vs_e"] == "slower")
    return row


if __name__ == "__main__":
    S.main(__file__, shape, SHAPES, {"forms": FORMS, "timing": TIMING}, "append_seg.json",
           keep=lambda a, s: not a.n or s[0] == a.n,
           options=[("--n", dict(type=int, default=0, help="only the shapes of this many files (under a kernel trace)"))])
