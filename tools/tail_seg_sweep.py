#!/usr/bin/env python3
"""The tail scan of streams that stay compressed in device memory: the one-wave scan against its
segmented form (DESIGN.md §4b quotes the table; the method is tools/sweeplib.py's).

  b  tail scan             rle_tail_batch_device: one wave per stream walks all of its tiles
  s  segmented tail scan   rle_tail_batch_device_seg: the stream cut into segments, several waves per
                           stream (plan, map, summary, scan)
  d  segmented decode      rle_decode_batch_device_seg of the same streams: the same plan, map and
                           summary launches (s launches the decode's own summary kernel), the decode's
                           scan, and its write pass on top -- what the whole decode costs where s
                           only parses

Per shape (n streams of U content bytes each, one synthetic kind): content generated and encoded on
the device, replicas of the stream arena.  At least 7 rounds.  Before any timing the tail words,
decoded lengths and status words of b and s are compared.

usage: python tools/tail_seg_sweep.py [--rounds 7] [--n 64] [--shapes 0,2] [--out profiles/tail_seg.json]"""
import sweeplib as S
import torch
from sweeplib import R

SHAPES = ((1, 1 << 20, 8), (64, 1 << 20, 4), (1, 1 << 16, 16), (4096, 4096, 8), (4096, 1 << 16, 3))   # (n, U, reps)
FORMS = {"b": "rle_tail_batch_device",
         "s": "rle_tail_batch_device_seg, total_in_bytes = the sum of the stream lengths",
         "d": "rle_decode_batch_device_seg of the same streams (s's launches, the decode's scan, and "
              "the write pass)"}
TIMING = S.timing_text("launch", "the stream arena", "streams", cells=False)


def shape(a, s, kind, dev):
    (n, U, reps), rounds = s, a.rounds
    f = S.stored_files(n, U, kind, S.r16(R.max_compressed_size(U)), dev, tail=False)
    rep = f.streams.expand(reps, -1).contiguous()
    total = int(f.clen.sum().item())
    res = {k: [torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev)] for k in "bs"}
    st_d = torch.zeros(n, dtype=torch.int32, device=dev)
    ws_s = R.tail_seg_workspace(n, total, dev)
    ws_d = R.seg_workspace(n, total, dev)

    def form_b(k):
        R.tail_batch(rep[k], f.s_off, f.clen, *res["b"])

    def form_s(k):
        R.tail_batch_seg(rep[k], f.s_off, f.clen, *res["s"], total_in_bytes=total, ws=ws_s)

    def form_d(k):
        R.decode_batch_seg(rep[k], f.s_off, f.clen, f.x, f.x_off, f.len_u, None, st_d, total_in_bytes=total, workspace=ws_d)

    # b and s give the same tail words, decoded lengths and status words
    form_b(0)
    form_s(reps - 1)
    form_d(0)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(res["b"], res["s"])), "the forms' results differ"
    assert int(res["s"][2].abs().sum().item()) == 0 and bool((res["s"][1] == U).all())
    assert int((st_d & 0xFF).sum().item()) == 0

    times = S.time_forms((("b", form_b), ("s", form_s), ("d", form_d)), reps, rounds)
    row = {"n": n, "U": U, "kind": kind, "stream_bytes": total, "segment_bytes": R.seg_segment_bytes(total),
           "reps": reps, "rounds": rounds, "results_equal": True}
    row.update((name, S.stats(v)) for name, v in times.items())
    S.over(row, "b", "s")
    row["s_slowest_below_b_fastest"] = row["s"]["max_us"] < row["b"]["min_us"]
    row["b_slowest_below_s_fastest"] = row["b"]["max_us"] < row["s"]["min_us"]
    return row


if __name__ == "__main__":
    S.main(__file__, shape, SHAPES, {"forms": FORMS, "timing": TIMING}, "tail_seg.json", min_rounds=7,
           keep=lambda a, s: not a.n or s[0] == a.n,
           options=[("--n", dict(type=int, default=0, help="only the shapes of this many streams"))])
