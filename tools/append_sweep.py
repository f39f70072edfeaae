#!/usr/bin/env python3
"""Appending to streams that stay compressed in device memory: the three ways a caller can do it
(DESIGN.md §4b quotes the table; the method is tools/sweeplib.py's).

  a  scan + append      rle_tail_batch_device, then rle_append_batch_device
  b  append             rle_append_batch_device alone, tail words carried from the previous append
  c  decode, copy, encode   what the batched API offered before: rle_decode_batch_device of every
                        file, a device copy of the new bytes behind the decoded content,
                        rle_encode_batch_device of the whole

Per shape (n files, old content of U bytes each, A new bytes each, one synthetic kind; the shapes are
the product of --old and --new): the files are generated and encoded on the device, and the replicas
of the stream arena are restored (untimed) before every timing, because an append changes its file.
Before any timing the three forms' streams and lengths are compared with each other.  The
algorithmic bytes of each form (what it must read and write, from the lengths) stand beside the
times.

usage: python tools/append_sweep.py [--n 4096] [--reps 16] [--rounds 5] [--shapes 0] [--out profiles/append_batch.json]"""
import sweeplib as S
import torch
from sweeplib import R

FORMS = {"a": "rle_tail_batch_device + rle_append_batch_device",
         "b": "rle_append_batch_device, tail words carried",
         "c": "rle_decode_batch_device + strided device copy of the new bytes + rle_encode_batch_device"}
TIMING = S.timing_text("launch", "the stream arena", "files", cells=False)


def shape(a, s, kind, dev):
    (U, A), n, reps, rounds = s, a.n, a.reps, a.rounds
    # the stored streams: slots of the capacity an append may need; the content arena is form c's, too
    cap = R.append_slot_bytes(R.max_compressed_size(U), A)
    assert cap and cap >= R.max_compressed_size(U + A)
    us, as_ = S.r16(U + A), S.r16(A)
    f = S.stored_files(n, U, kind, cap, dev, slot=us)
    d_new, new_off, len_a = S.gen_files(n, A, kind, dev, index_base=n)
    d_dec, dec_off, s_off = f.x, f.x_off, f.s_off
    caps, len_ua = torch.full_like(len_a, cap), torch.full_like(len_a, U + A)
    rep, lens, tails, ulens, restore = S.replicas(reps, f.streams, f.clen, f.tail, f.ulen)
    out_c = torch.zeros(n * cap, dtype=torch.uint8, device=dev)   # form c's new streams
    len_c = torch.zeros(n, dtype=torch.int64, device=dev)
    st_a, st_b, st_c = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))

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
    assert S.same_streams(rep[0], rep[1], lens[0], cap) and S.same_streams(rep[0], out_c, lens[0], cap), \
        "the forms' streams differ"
    c_old, c_new = int(f.clen.sum().item()), int(len_c.sum().item())
    kept = int((f.tail & 0xFFFFFFFF).sum().item())   # the bytes below every old final token
    written = c_new - kept   # bytes from each old final token's offset to the new end
    nbytes = {
        "a": {"read_bytes": c_old + n * A, "write_bytes": written},
        "b": {"read_bytes": n * A, "write_bytes": written},
        "c": {"read_bytes": c_old + n * A + n * (U + A), "write_bytes": n * U + n * A + c_new},
    }

    times = S.time_forms((("a", form_a), ("b", form_b), ("c", form_c)), reps, rounds, before=restore)
    row = {"n": n, "U": U, "A": A, "kind": kind, "old_stream_bytes": c_old, "new_stream_bytes": c_new,
           "reps": reps, "rounds": rounds, "outputs_equal": True}
    row.update((name, {**S.stats(v), **nbytes[name]}) for name, v in times.items())
    S.over(row, "c", "b")
    S.over(row, "c", "a")
    return row


def shapes(a):
    return [(int(U), int(A)) for U in a.old.split(",") for A in a.new.split(",")]


if __name__ == "__main__":
    S.main(__file__, shape, shapes, {"forms": FORMS, "timing": TIMING}, "append_batch.json", rounds=5,
           options=[("--n", dict(type=int, default=4096)), ("--reps", dict(type=int, default=16)),
                    ("--old", dict(default="4096,65536")), ("--new", dict(default="64,4096"))])
