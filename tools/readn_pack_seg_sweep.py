#!/usr/bin/env python3
"""Reading large stored streams into a packed reply: rle_readn_batch_device_seg against the one-wave
rle_readn_batch_device and against the segmented decode into aligned slots (DESIGN.md §4c
"Segmented form" quotes the table; the method is tools/sweeplib.py's).

  s  segmented packed   rle_readn_batch_device_seg: the layout launch, then plan, map, summary, packed
                        scan and packed write, several waves per stream, straight into the reply
  p  one-wave packed    rle_readn_batch_device: the layout launch and one wave per file
  a  aligned, segmented rle_decode_batch_device_seg of the same files into 16-byte aligned slots at
                        offsets the host knows: the floor; what byte-granular ends cost is s / a

Per shape (n files of U decoded bytes each, one synthetic kind): files generated and encoded on the
device, decoded lengths from rle_tail_batch_device; every file's header is G = 49 bytes, so a file's
row in the reply is G + U bytes, an odd number: the destinations take every phase mod 16.  Replicas
of the stream arena and of every output arena.  total_in_bytes is the streams' sum, read once before
any timing; each segmented form has a workspace of its own.  Before any timing the outputs are
compared: s's reply with p's, byte for byte, and both with a's slots and the content.

usage: python tools/readn_pack_seg_sweep.py [--rounds 7] [--shapes 1,3] [--out profiles/readn_pack_seg.json]"""
import numpy as np
import sweeplib as S
import torch
from sweeplib import R

SHAPES = ((1, 65536, 8), (1, 1 << 20, 8), (64, 65536, 8), (64, 1 << 20, 4), (4096, 4096, 8), (4096, 65536, 4))   # (n, U, reps)
GAP = 49
POISON = 0xA5
FORMS = {"s": "rle_readn_batch_device_seg into a packed reply (49-byte header gaps)",
         "p": "rle_readn_batch_device into the same reply, one wave per file",
         "a": "rle_decode_batch_device_seg into 16-byte aligned slots"}
TIMING = S.timing_text("call", "the arenas", "files")


def shape(a, s, kind, dev):
    (n, U, reps), rounds = s, a.rounds
    slot, row = S.r16(U), GAP + U
    f = S.stored_files(n, U, kind, S.r16(R.max_compressed_size(U)), dev)
    hint = int(f.clen.sum().item())
    streams = f.streams.expand(reps, -1).contiguous()                    # replicas of the stream arena
    gap = torch.full((n,), GAP, dtype=torch.int64, device=dev)
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
        R.readn_batch_seg(streams[k], f.s_off, f.clen, f.ulen, gap, reply_s[k], place["s"], total["s"], sts["s"],
                          out_cap=cap, total_in_bytes=hint, ws=ws_s)

    def form_p(k):
        R.readn_batch(streams[k], f.s_off, f.clen, f.ulen, gap, reply_p[k], place["p"], total["p"], sts["p"], out_cap=cap)

    def form_a(k):
        R.decode_batch_seg(streams[k], f.s_off, f.clen, slots_a[k], f.x_off, f.ulen, None, sts["a"], total_in_bytes=hint,
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
    assert torch.equal(slots_a[0].view(n, slot)[:, :U], f.x.view(n, slot)[:, :U]), "a is not the content"

    times = S.time_forms((("s", form_s), ("p", form_p), ("a", form_a)), reps, rounds)
    row_ = {"n": n, "U": U, "kind": kind, "gap": GAP, "stream_bytes": hint, "reply_bytes": cap,
            "segment_bytes": R.seg_segment_bytes(hint), "reps": reps, "rounds": rounds, "outputs_equal": True}
    row_.update((name, S.stats(v)) for name, v in times.items())
    for other in "pa":
        S.verdict(row_, "s", other)
    return row_


def table(rows):
    return S.table(["files x U", "kind", "s", "p", "a", "s / p", "s / a"], rows,
                   lambda r: [f"{r['n']} x {S.size_name(r['U'])}", r["kind"], *(S.cell(r, k) for k in "spa"),
                              S.ratio_cell(r, "s", "p"), S.ratio_cell(r, "s", "a")])


def gate(rows):
    big = [r for r in rows if r["U"] == 1 << 20]
    return {"gate": {"rule": "on 1 x 1 MiB and 64 x 1 MiB, s is faster than p by more than the two spreads together",
                     "holds": bool(big) and all(r["s_vs_p"] == "faster" for r in big)}}


if __name__ == "__main__":
    res = S.main(__file__, shape, SHAPES, {"forms": FORMS, "timing": TIMING}, "readn_pack_seg.json", extra=gate,
                 table=table)
    print("gate:", res["gate"])
