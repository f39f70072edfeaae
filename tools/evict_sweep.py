#!/usr/bin/env python3
"""Choosing eviction victims: rle_evict_select_device and rle_evict_gather_device against what a
caller had to do before (DESIGN.md §4e quotes the table; the method is tools/sweeplib.py's).

  s  selection       rle_evict_select_device alone: one launch of one workgroup; keys, sizes and masks
                     never leave the device
  g  select+gather   s, then rle_evict_gather_device of five tables in reply order: the arguments of
                     the eviction reply, on the device
  h  host route      what a caller had to do before: d_key, d_len, d_want and both masks copied to the
                     host with a synchronise, a numpy lexsort by (key, index) and a cumsum of the sizes
                     there, and the keep mask and the five gathered tables uploaded (the tables' host
                     copies are the host's own, at no cost)

Per shape (n files): sizes of 1..5000 bytes with wants, one file in 16 not live, one in 32 spared,
timestamp-like keys (most of them distinct); four limits: a store that fits (the one-pass exit), and
max_bytes under which 1 %, 10 % and all of the eligible files go.  Replicas of every input and output
array; h's copies to the host make each of its calls wait for the one before.  Before any timing the
outputs are compared: s's keep mask, victim list and summary with h's, and g's rows with h's.

usage: python tools/evict_sweep.py [--rounds 7] [--shapes 0,2] [--out profiles/evict.json]"""
import numpy as np
import sweeplib as S
import torch
from sweeplib import R

SHAPES = ((64, 16), (4096, 8), (65536, 4))   # (n, reps)
NTABLES = 5
FORMS = {"s": "rle_evict_select_device (one launch, one workgroup)",
         "g": "s, then rle_evict_gather_device of five tables in reply order (one more launch)",
         "h": "d_key, d_len, d_want, d_live and d_spare copied to the host with a synchronise, numpy lexsort and "
              "cumsum there, the keep mask and the five gathered tables uploaded"}
LIMITS = {"fits": "max_bytes = the store's bytes: nothing goes (the one-pass exit)",
          "1 %": "max_bytes under which 1 % of the eligible files go (one at least)",
          "10 %": "max_bytes under which 10 % of the eligible files go",
          "all": "max_bytes = the spared files' bytes: every eligible file goes"}
TIMING = S.timing_text("call", "every input and output array", "files")


def host_select(k, ln, wn, lv, sp, max_bytes):
    """(keep, victims in eviction order, bytes before, bytes after) by sorting on the host."""
    size = np.where(lv != 0, np.maximum(ln, wn), 0)
    idx = np.flatnonzero((lv != 0) & (sp == 0))
    order = idx[np.lexsort((idx, k[idx]))]
    before = int(size.sum())
    m = 0
    if before > max_bytes:
        m = int(np.searchsorted(np.cumsum(size[order]), before - max_bytes)) + 1
    victims = order[:m]
    keep = (lv != 0).astype(np.int32)
    keep[victims] = 0
    return keep, victims, before, before - int(size[victims].sum())


def shape(a, s, limit, dev):
    (n, reps), rounds = s, a.rounds
    rng = np.random.default_rng(n)
    key_h = (0x6530000000 + rng.integers(0, 1 << 24, n)).astype(np.uint64)
    len_h = rng.integers(1, 5001, n).astype(np.uint64)
    want_h = len_h + rng.integers(0, 1000, n).astype(np.uint64)
    live_h = (np.arange(n) % 16 != 5).astype(np.int32)
    spare_h = (np.arange(n) % 32 == 9).astype(np.int32)
    tables_h = [rng.integers(0, 1 << 40, n).astype(np.int64) for _ in range(NTABLES)]
    # the limit
    elig = (live_h != 0) & (spare_h == 0)
    total = int(want_h[live_h != 0].sum())
    count = {"fits": 0, "1 %": max(1, int(elig.sum()) // 100), "10 %": int(elig.sum()) // 10, "all": int(elig.sum())}[limit]
    idx = np.flatnonzero(elig)
    order = idx[np.lexsort((idx, key_h[idx]))]
    max_bytes = total - int(want_h[order[:count]].sum())

    up = lambda v: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev)   # noqa: E731
    key, length, want, live, spare = (up(v).expand(reps, n).contiguous() for v in (key_h, len_h, want_h, live_h, spare_h))
    tables = [up(t) for t in tables_h]
    z = lambda dt, k: torch.zeros(reps, k, dtype=dt, device=dev)   # noqa: E731
    keep = {f: z(torch.int32, n) for f in "sh"}
    victims, summary = z(torch.int32, n), z(torch.int64, R.RLE_EVICT_SUMMARY_WORDS)
    rows = {f: [z(torch.int64, max(count, 1)) for _ in range(NTABLES)] for f in "gh"}

    def form_s(k):
        R.evict_select(key[k], length[k], keep["s"][k], victims[k], summary[k], want=want[k], live=live[k], spare=spare[k],
                       max_bytes=max_bytes)

    def form_g(k):
        form_s(k)
        R.evict_gather(victims[k], summary[k], tables, [r[k] for r in rows["g"]], order=R.RLE_EVICT_ORDER_REPLY)

    def form_h(k):
        kk, ln, wn = (t[k].cpu().numpy().view(np.uint64) for t in (key, length, want))   # through the host
        lv, sp = live[k].cpu().numpy(), spare[k].cpu().numpy()
        kp, vic, before, after = host_select(kk, ln, wn, lv, sp, max_bytes)
        keep["h"][k].copy_(torch.from_numpy(kp), non_blocking=True)
        sent = vic[::-1]
        for t, r in zip(tables_h, rows["h"]):
            r[k][:len(sent)].copy_(torch.from_numpy(t[sent]), non_blocking=True)
        return vic, before, after

    # the outputs first
    form_g(0)
    vic, before, after = form_h(0)
    torch.cuda.synchronize()
    assert summary[0].tolist() == [0, count, before, after, int((live_h != 0).sum()), int((live_h != 0).sum()) - count]
    assert victims[0][:count].tolist() == vic.tolist() and after <= max_bytes
    assert torch.equal(keep["s"][0], keep["h"][0])
    assert all(torch.equal(g[0][:count], h[0][:count]) for g, h in zip(rows["g"], rows["h"]))

    times = S.time_forms((("s", form_s), ("g", form_g), ("h", form_h)), reps, rounds)
    row = {"n": n, "limit": limit, "m": count, "tables": NTABLES, "reps": reps, "rounds": rounds, "outputs_equal": True}
    row.update((name, S.stats(v)) for name, v in times.items())
    for f in "sg":
        S.verdict(row, f, "h")
    return row


def table(rows):
    return S.table(["files", "evicted", "s", "g", "h", "s / h", "g / h"], rows,
                   lambda r: [str(r["n"]), f"{r['limit']} ({r['m']})", *(S.cell(r, k) for k in "sgh"),
                              S.ratio_cell(r, "s", "h"), S.ratio_cell(r, "g", "h")])


if __name__ == "__main__":
    S.main(__file__, shape, SHAPES, {"forms": FORMS, "limits": LIMITS, "timing": TIMING}, "evict.json", kinds=False,
           variants=tuple(LIMITS), table=table)
