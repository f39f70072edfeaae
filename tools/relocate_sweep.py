#!/usr/bin/env python3
"""Relocating stored streams: rle_relocate_batch_device against the streaming copy of the same bytes
and against what a caller had to do before (DESIGN.md §4d quotes the table; the method is
tools/sweeplib.py's).

  r  relocation      rle_relocate_batch_device: the layout launch and the copy launch that follows the
                     per-file map on the device; sizes never leave the device
  m  plain copy      rle_copy_device of the same number of copied bytes, one contiguous range: the
                     ceiling of any relocation (no map, no gaps); the ratio r / m goes in the table
  h  host route      what a caller had to do before: d_len and d_want copied to the host with a
                     synchronise, the slots laid out there, d_new_off and d_new_cap uploaded, and one
                     hipMemcpyAsync device-to-device per file (the source offsets are the host's own
                     copy, at no cost)

Per shape (n streams of C bytes each, random bytes: a copy does not care): the streams packed in the
source arena; twice, with want = C (slots as tight as the streams) and with want = the worst-case slot
of an append of as many bytes again (rle_append_slot_bytes(C, C): gaps larger than the streams).
dst_cap is the layout's total: the room this relocation takes.  Replicas of the source and of every
destination arena; h's copy to the host makes each of its calls wait for the one before.  Before any
timing the outputs are compared: r's destination with h's, byte for byte over the poison, and r's
with m's where the slots are tight.

usage: python tools/relocate_sweep.py [--rounds 7] [--sizes 4096,65536] [--shapes 0,3] [--out profiles/relocate.json]"""
import ctypes
import functools

import numpy as np
import sweeplib as S
import torch
from sweeplib import R

SHAPES = ((1, 4096, 8), (64, 4096, 8), (4096, 4096, 8), (1, 65536, 8), (64, 65536, 8), (4096, 65536, 3),
          (1, 1 << 20, 8), (64, 1 << 20, 4))   # (n, C, reps)
POISON = 0xA5
D2D = 3   # hipMemcpyDeviceToDevice
FORMS = {"r": "rle_relocate_batch_device (layout launch + one copy launch)",
         "m": "rle_copy_device of the same number of copied bytes, one contiguous range (the ceiling)",
         "h": "d_len and d_want copied to the host with a synchronise, the slots laid out there, the "
              "offsets and capacities uploaded, one hipMemcpyAsync device-to-device per file"}
SLOTS = {"tight": "want = C", "worst-case": "want = rle_append_slot_bytes(C, C)"}
TIMING = S.timing_text("call", "the arenas", "streams")


@functools.lru_cache(None)
def hip_runtime():
    """The HIP runtime this process already uses (torch's), for the host route's hipMemcpyAsync."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "no HIP runtime is loaded"
    hip = ctypes.CDLL(paths[0])
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    return hip


def shape(a, s, slots, dev):
    (n, C, reps), rounds, hip = s, a.rounds, hip_runtime()
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)   # noqa: E731
    assert C % 16 == 0
    want_h = [C if slots == "tight" else R.append_slot_bytes(C, C)] * n
    cap = S.r16(max(want_h[0], C))
    total = n * cap
    src = torch.randint(0, 256, (reps, n * C), dtype=torch.uint8, device=dev)
    soff_h = [i * C for i in range(n)]
    off, length, want = i64(soff_h), i64([C] * n), i64(want_h)
    dst = {k: torch.full((reps, total), POISON, dtype=torch.uint8, device=dev) for k in "rh"}
    dst["m"] = torch.full((reps, n * C), POISON, dtype=torch.uint8, device=dev)
    new_off = {k: torch.zeros(n, dtype=torch.int64, device=dev) for k in "rh"}
    new_cap = {k: torch.zeros(n, dtype=torch.int64, device=dev) for k in "rh"}
    d_total = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def form_r(k):
        R.relocate_batch(src[k], off, length, dst["r"][k], new_off["r"], new_cap["r"], d_total, want=want,
                         status=status, dst_cap=total)

    def form_m(k):
        R.copy_device(dst["m"][k], src[k], n * C)

    def form_h(k):
        ln, wn = length.cpu().numpy(), want.cpu().numpy()            # the sizes through the host
        caps = (np.maximum(ln, wn) + 15) & ~15
        offs = np.cumsum(caps) - caps
        assert offs[-1] + caps[-1] <= total
        new_off["h"].copy_(torch.from_numpy(offs), non_blocking=True)
        new_cap["h"].copy_(torch.from_numpy(caps), non_blocking=True)
        d, sbase = dst["h"][k].data_ptr(), src[k].data_ptr()
        for i in range(n):
            rc = hip.hipMemcpyAsync(d + int(offs[i]), sbase + soff_h[i], int(ln[i]), D2D, sp)
            assert rc == 0, rc

    # the outputs first
    for fn in (form_r, form_m, form_h):
        fn(0)
    torch.cuda.synchronize()
    assert int(status.abs().sum().item()) == 0 and int(d_total.item()) == total
    assert torch.equal(new_off["r"], new_off["h"]) and torch.equal(new_cap["r"], new_cap["h"])
    assert torch.equal(dst["r"][0], dst["h"][0]), "r's destination differs from h's"
    assert torch.equal(dst["r"][0].view(n, cap)[:, :C], src[0].view(n, C)), "r is not the streams"
    assert bool((dst["r"][0].view(n, cap)[:, C:] == POISON).all()), "r wrote into a gap"
    assert torch.equal(dst["m"][0], src[0])

    times = S.time_forms((("r", form_r), ("m", form_m), ("h", form_h)), reps, rounds)
    row = {"n": n, "C": C, "slots": slots, "want": want_h[0], "copied_bytes": n * C, "room_bytes": total,
           "span_bytes": R.relocate_span_bytes(total), "reps": reps, "rounds": rounds, "outputs_equal": True}
    row.update((name, S.stats(v)) for name, v in times.items())
    row["r_copy_GBps"] = round(2 * n * C / row["r"]["median_us"] / 1e3, 1)   # bytes read + bytes written
    for other in "mh":
        S.verdict(row, "r", other)
    return row


def table(rows):
    return S.table(["streams x C", "slots", "r", "m", "h", "r / m", "r / h"], rows,
                   lambda r: [f"{r['n']} x {S.size_name(r['C'])}", r["slots"], *(S.cell(r, k) for k in "rmh"),
                              S.ratio_cell(r, "r", "m"), S.ratio_cell(r, "r", "h")])


def keep(a, s):
    sizes = {int(c) for c in a.sizes.split(",") if c}
    return not sizes or s[1] in sizes


if __name__ == "__main__":
    S.main(__file__, shape, SHAPES, {"forms": FORMS, "slots": SLOTS, "timing": TIMING}, "relocate.json", kinds=False,
           variants=tuple(SLOTS), keep=keep, table=table,
           options=[("--sizes", dict(default="", help="comma-separated stream sizes C to run (default: all)"))])
