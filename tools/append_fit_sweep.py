#!/usr/bin/env python3
"""Sizing an append before it is written: the size and fit entries against the plain append
(DESIGN.md §4b quotes the table; the method is tools/sweeplib.py's).

  p  plain append   rle_append_batch_device[_seg]: worst-case slots, C' known only afterwards
  z  size only      rle_append_size_batch_device[_seg]: d_need, nothing else written
  f  fit, cap = C'  rle_append_fit_batch_device[_seg] with exact capacities (one-wave: the size
                    walk and then the write walk)
  g  fit, worst     the same entry with cap = rle_append_slot_bytes (one-wave: the size walk skipped)

Per shape (n files of U old bytes each, A new bytes each, one synthetic kind; the one-wave forms for
small A, the segmented forms for 1 MiB): as tools/append_sweep.py and tools/append_seg_sweep.py --
files generated and encoded on the device, the replicas of the stream arena restored untimed before
every timing.  Before any timing the outputs are compared: z's d_need with p's new lengths, f's and
g's streams, lengths, decoded lengths and tail words with p's.  The baseline is p in the same
process.

usage: python tools/append_fit_sweep.py [--rounds 7] [--n 4096] [--shapes 1] [--out profiles/append_fit.json]"""
import sweeplib as S
import torch
from sweeplib import R

SHAPES = ((4096, 4096, 8, False), (4096, 64, 8, False), (1, 1 << 20, 8, True), (64, 1 << 20, 4, True))   # (n, A, reps, seg)
OLD = 4096
FORMS = {"p": "rle_append_batch_device[_seg], worst-case slots, tail words carried",
         "z": "rle_append_size_batch_device[_seg]",
         "f": "rle_append_fit_batch_device[_seg], cap = C' (from z)",
         "g": "rle_append_fit_batch_device[_seg], cap = rle_append_slot_bytes"}
TIMING = S.timing_text("launch", "the stream arena", "files")


def shape(a, s, kind, dev):
    (n, A, reps, seg), U, rounds = s, OLD, a.rounds
    cap = R.append_slot_bytes(R.max_compressed_size(U), A)
    assert cap
    b = S.stored_files(n, U, kind, cap, dev)
    d_new, new_off, len_a = S.gen_files(n, A, kind, dev, index_base=n)
    s_off, caps = b.s_off, torch.full_like(len_a, cap)
    rep, lens, tails, ulens, restore = S.replicas(reps, b.streams, b.clen, b.tail, b.ulen)
    need = torch.zeros(n, dtype=torch.int64, device=dev)       # z's result: f's capacities
    need_f = torch.zeros(n, dtype=torch.int64, device=dev)
    sts = {name: torch.zeros(n, dtype=torch.int32, device=dev) for name in "pzfg"}
    total = n * A
    ws = R.append_seg_workspace(n, total, dev) if seg else None
    kw = dict(total_new_bytes=total, workspace=ws) if seg else {}
    plain, size, fit = ((R.append_batch_seg, R.append_size_seg, R.append_fit_seg) if seg else
                        (R.append_batch, R.append_size, R.append_fit))

    def form_p(k):
        plain(rep[k], s_off, lens[k], caps, ulens[k], d_new, new_off, len_a, sts["p"], tail=tails[k], **kw)

    def form_z(k):
        size(rep[k], s_off, lens[k], tails[k], d_new, new_off, len_a, need, sts["z"], **kw)

    def form_f(k):
        fit(rep[k], s_off, lens[k], need, ulens[k], d_new, new_off, len_a, need_f, sts["f"], tail=tails[k], **kw)

    def form_g(k):
        fit(rep[k], s_off, lens[k], caps, ulens[k], d_new, new_off, len_a, need_f, sts["g"], tail=tails[k], **kw)

    def same_as_p():   # replica 1 holds what replica 0, p's, holds
        return (torch.equal(lens[0], lens[1]) and torch.equal(tails[0], tails[1]) and torch.equal(ulens[0], ulens[1])
                and S.same_streams(rep[0], rep[1], lens[0], cap))

    # the outputs first: z's need is p's new length and z wrote nothing; f and g leave what p leaves
    restore()
    form_z(1)
    torch.cuda.synchronize()
    assert torch.equal(rep[1], b.streams) and torch.equal(lens[1], b.clen) and torch.equal(tails[1], b.tail)
    form_p(0)
    form_f(1)
    torch.cuda.synchronize()
    assert all(int(sts[k].abs().sum().item()) == 0 for k in "pzf")
    assert torch.equal(need, lens[0]) and torch.equal(need_f, lens[0])
    assert same_as_p(), "f's streams differ from p's"
    restore()
    form_p(0)
    form_g(1)
    torch.cuda.synchronize()
    assert int(sts["g"].abs().sum().item()) == 0 and torch.equal(need_f, lens[0])
    assert same_as_p(), "g's streams differ from p's"
    c_new = int(lens[0].sum().item())

    times = S.time_forms((("p", form_p), ("z", form_z), ("f", form_f), ("g", form_g)), reps, rounds, before=restore)
    row = {"n": n, "U": U, "A": A, "kind": kind, "form": "segmented" if seg else "one-wave",
           "old_stream_bytes": int(b.clen.sum().item()), "new_stream_bytes": c_new,
           "worst_case_slot_bytes": n * cap, "reps": reps, "rounds": rounds, "outputs_equal": True}
    if seg:
        row["segment_bytes"] = R.seg_segment_bytes(total)
    row.update((name, S.stats(v)) for name, v in times.items())
    for name in "zfg":
        S.verdict(row, name, "p")
    return row


def table(rows):
    return S.table(["files x A", "kind", "form", "p", "z", "f", "g", "z / p", "f / p", "g / p"], rows,
                   lambda r: [f"{r['n']} x {S.size_name(r['A'])}", r["kind"], r["form"], *(S.cell(r, k) for k in "pzfg"),
                              *(S.ratio_cell(r, k, "p") for k in "zfg")])


if __name__ == "__main__":
    S.main(__file__, shape, SHAPES, {"forms": FORMS, "timing": TIMING}, "append_fit.json", table=table,
           keep=lambda a, s: not a.n or s[0] == a.n,
           options=[("--n", dict(type=int, default=0, help="only the shapes of this many files (under a kernel trace)"))])
