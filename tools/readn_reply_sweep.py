#!/usr/bin/env python3
"""The whole read-N reply from device state: rle_readn_reply_device (and its _seg form) against the
packed read-N alone and against what a caller had to do for its headers before (DESIGN.md §4c
"Headers and terminator" quotes the table; the method is tools/sweeplib.py's).

  r  whole reply     rle_readn_reply_device(_seg): the layout with derived gaps, the packed decode, the
                     headers and the terminator; nothing visits the host
  p  contents alone  rle_readn_batch_device(_seg) with the same gaps in a device array, headers left
                     unwritten: r - p is the price of the headers and their launch
  h  host headers    what a caller does today: d_ulen copied to the host (which synchronises), the
                     headers formatted there, one copy of them to the device and one strided device
                     copy into the gaps, then p

Per shape (n files of U decoded bytes each, one synthetic kind): files generated and encoded on the
device, decoded lengths from rle_tail_batch_device; every name is 29 bytes, so every header is 49 and a
file's row in the reply is 49 + U bytes, an odd number: headers and contents take every phase mod 16.
Equal lengths keep h as cheap as a caller could make it: the names and their length fields stand in a
prepared template, only the ten digits of each content length are formatted per call (vectorised),
and the headers reach the gaps by one host-to-device copy and one strided device copy.  Replicas of
the stream arena and of every reply; h's copy to the host makes each of its calls wait for the one
before.  Before any timing the outputs are compared: r's reply with h's, byte for byte, its first and
last header with Python's own formatting, and p's contents with r's.

usage: python tools/readn_reply_sweep.py [--rounds 7] [--shapes 0,6] [--out profiles/readn_reply.json]"""
import numpy as np
import sweeplib as S
import torch
from sweeplib import R

# (n, U, reps, segmented)
SHAPES = ((1, 4096, 8, False), (64, 4096, 8, False), (4096, 4096, 8, False), (1, 65536, 8, False),
          (64, 65536, 8, False), (4096, 65536, 4, False), (1, 1 << 20, 8, True), (64, 1 << 20, 4, True))
PLEN, GAP = 29, 49
FORM = R.RLE_REPLY_READN | R.RLE_REPLY_END
POISON = 0xA5
POW10 = 10 ** np.arange(9, -1, -1, dtype=np.int64)
FORMS = {"r": "rle_readn_reply_device(_seg): layout with derived gaps, packed decode, headers and terminator",
         "p": "rle_readn_batch_device(_seg) alone, the 49-byte gaps left unwritten",
         "h": "d_ulen copied to the host, headers formatted there into a prepared template, copied back "
              "and into the gaps by one strided device copy, then p"}
TIMING = S.timing_text("call", "the arenas", "files")


def shape(a, s, kind, dev):
    (n, U, reps, seg), rounds = s, a.rounds
    i64 = lambda v: torch.full((n,), v, dtype=torch.int64, device=dev)   # noqa: E731
    slot, row = S.r16(U), GAP + U
    f = S.stored_files(n, U, kind, S.r16(R.max_compressed_size(U)), dev)
    tin = int(f.clen.sum().item())
    ws = R.decode_packed_seg_workspace(n, tin, dev) if seg else None
    streams = f.streams.expand(reps, -1).contiguous()                    # replicas of the stream arena
    # the path table on the device, and the host's header template (names and their length fields)
    names = [b"/srv/store/file_%013d" % i for i in range(n)]
    assert all(len(p) == PLEN for p in names)
    d_paths = torch.from_numpy(np.frombuffer(b"".join(names), np.uint8).copy()).to(dev)
    path_off, path_len, gap = torch.arange(n, dtype=torch.int64, device=dev) * PLEN, i64(PLEN), i64(GAP)
    templ = np.frombuffer(b"".join(b"%010d%s0000000000" % (PLEN, p) for p in names), np.uint8).reshape(n, GAP).copy()
    hdr_host = torch.from_numpy(templ.copy()).pin_memory()
    hdr_dev = torch.zeros((n, GAP), dtype=torch.uint8, device=dev)
    cap = n * row + 10
    reply = {k: torch.full((reps, cap), POISON, dtype=torch.uint8, device=dev) for k in "rph"}
    place = torch.zeros(n, dtype=torch.int64, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    sts = {name: torch.zeros(n, dtype=torch.int32, device=dev) for name in "rph"}
    want_place = np.arange(n, dtype=np.int64) * row + GAP
    end_dev = torch.full((10,), 0x30, dtype=torch.uint8, device=dev)

    def contents(k, out, status):
        if seg:
            R.readn_batch_seg(streams[k], f.s_off, f.clen, f.ulen, gap, out, place, total, status, out_cap=cap,
                              total_in_bytes=tin, ws=ws)
        else:
            R.readn_batch(streams[k], f.s_off, f.clen, f.ulen, gap, out, place, total, status, out_cap=cap)

    def form_r(k):
        if seg:
            R.readn_reply_seg(streams[k], f.s_off, f.clen, f.ulen, d_paths, path_off, path_len, reply["r"][k], place, total,
                              sts["r"], form=FORM, out_cap=cap, total_in_bytes=tin, ws=ws)
        else:
            R.readn_reply(streams[k], f.s_off, f.clen, f.ulen, d_paths, path_off, path_len, reply["r"][k], place, total,
                          sts["r"], form=FORM, out_cap=cap)

    def form_p(k):
        contents(k, reply["p"][k], sts["p"])

    def form_h(k):
        u = f.ulen.cpu().numpy()                      # the lengths through the host
        hdr_host.numpy()[:, GAP - 10:] = (u[:, None] // POW10) % 10 + 0x30
        hdr_dev.copy_(hdr_host, non_blocking=True)
        out = reply["h"][k]
        out[:n * row].view(n, row)[:, :GAP] = hdr_dev   # the headers into their gaps
        out[n * row:] = end_dev
        contents(k, out, sts["h"])

    # the outputs first
    form_r(0)
    form_p(0)
    form_h(0)
    torch.cuda.synchronize()
    assert all(int(sts[k].abs().sum().item()) == 0 for k in "rph")
    assert np.array_equal(place.cpu().numpy(), want_place)
    assert torch.equal(reply["r"][0], reply["h"][0]), "r's reply differs from h's"
    got = reply["r"][0].cpu().numpy()
    for i in (0, n - 1):
        assert got[i * row:i * row + GAP].tobytes() == b"%010d%s%010d" % (PLEN, names[i], U), "r's header"
    assert got[n * row:].tobytes() == b"0000000000"
    body = lambda t: t[0][:n * row].view(n, row)[:, GAP:]   # noqa: E731
    assert torch.equal(body(reply["p"]), body(reply["r"])), "p's contents differ from r's"
    assert torch.equal(body(reply["r"]), f.x.view(n, slot)[:, :U]), "r is not the content"
    assert bool((reply["p"][0][:n * row].view(n, row)[:, :GAP] == POISON).all())

    times = S.time_forms((("r", form_r), ("p", form_p), ("h", form_h)), reps, rounds)
    row_ = {"n": n, "U": U, "kind": kind, "entry": "rle_readn_reply_device" + ("_seg" if seg else ""), "gap": GAP,
            "stream_bytes": tin, "reply_bytes": cap, "reps": reps, "rounds": rounds, "outputs_equal": True}
    row_.update((name, S.stats(v)) for name, v in times.items())
    for other in "ph":
        S.verdict(row_, "r", other)
    return row_


def table(rows):
    return S.table(["files x U", "kind", "entry", "r", "p", "h", "r - p", "r / h"], rows,
                   lambda r: [f"{r['n']} x {r['U'] >> 10} KiB", r["kind"], "seg" if r["entry"].endswith("_seg") else "one-wave",
                              *(S.cell(r, k) for k in "rph"), f"{r['r_minus_p_us']:+.1f} us {r['r_vs_p']}",
                              S.ratio_cell(r, "r", "h")])


if __name__ == "__main__":
    S.main(__file__, shape, SHAPES, {"forms": FORMS, "timing": TIMING}, "readn_reply.json", table=table)
