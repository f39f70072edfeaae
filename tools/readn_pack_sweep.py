#!/usr/bin/env python3
"""Reading stored streams into a packed reply: rle_readn_batch_device against the aligned decode and
against what a caller had to do before (DESIGN.md §4c quotes the table; the method is
tools/sweeplib.py's).

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
the same and are checked against that stride.  Replicas of the stream arena and of every output
arena; c's copy to the host makes each of its calls wait for the one before.  Before any timing the
outputs are compared: p's reply with c's, byte for byte, and both with d's slots.

usage: python tools/readn_pack_sweep.py [--rounds 7] [--shapes 0,1] [--out profiles/readn_pack.json]"""
import numpy as np
import sweeplib as S
import torch
from sweeplib import R

SHAPES = ((64, 4096, 8), (4096, 4096, 8), (64, 65536, 8), (4096, 65536, 4))   # (n, U, reps)
GAP = 49
POISON = 0xA5
FORMS = {"p": "rle_readn_batch_device into a packed reply (49-byte header gaps)",
         "d": "rle_decode_batch_device into 16-byte aligned slots",
         "c": "d_ulen copied to the host and summed there, d, one strided device copy of the slots "
              "into the packed reply"}
TIMING = S.timing_text("call", "the arenas", "files")


def shape(a, s, kind, dev):
    (n, U, reps), rounds = s, a.rounds
    slot, row = S.r16(U), GAP + U
    f = S.stored_files(n, U, kind, S.r16(R.max_compressed_size(U)), dev)
    streams = f.streams.expand(reps, -1).contiguous()                    # replicas of the stream arena
    gap = torch.full((n,), GAP, dtype=torch.int64, device=dev)
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
        R.readn_batch(streams[k], f.s_off, f.clen, f.ulen, gap, reply_p[k], place, total, sts["p"], out_cap=cap)

    def form_d(k):
        R.decode_batch(streams[k], f.s_off, f.clen, slots_d[k], f.x_off, f.ulen, None, sts["d"])

    def form_c(k):
        u = f.ulen.cpu().numpy()                      # the lengths through the host
        ends = np.cumsum(u + gap_h)
        assert ends[-1] <= cap and np.array_equal(ends - u, want_place)
        R.decode_batch(streams[k], f.s_off, f.clen, slots_c[k], f.x_off, f.ulen, None, sts["c"])
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
    assert torch.equal(slots_d[0].view(n, slot)[:, :U], f.x.view(n, slot)[:, :U]), "d is not the content"

    times = S.time_forms((("p", form_p), ("d", form_d), ("c", form_c)), reps, rounds)
    row_ = {"n": n, "U": U, "kind": kind, "gap": GAP, "stream_bytes": int(f.clen.sum().item()), "reply_bytes": cap,
            "reps": reps, "rounds": rounds, "outputs_equal": True}
    row_.update((name, S.stats(v)) for name, v in times.items())
    for other in "dc":
        S.verdict(row_, "p", other)
    return row_


def table(rows):
    return S.table(["files x U", "kind", "p", "d", "c", "p / d", "p / c"], rows,
                   lambda r: [f"{r['n']} x {S.size_name(r['U'])}", r["kind"], *(S.cell(r, k) for k in "pdc"),
                              S.ratio_cell(r, "p", "d"), S.ratio_cell(r, "p", "c")])


if __name__ == "__main__":
    S.main(__file__, shape, SHAPES, {"forms": FORMS, "timing": TIMING}, "readn_pack.json", table=table)
