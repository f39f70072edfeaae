#!/usr/bin/env python3
"""The whole read-N reply from device state: rle_readn_reply_device (and its _seg form) against the
packed read-N alone and against what a caller had to do for its headers before, timed in one process
on the same files (not bench.py; DESIGN.md §4c "Headers and terminator" quotes the table).

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
and the headers reach the gaps by one host-to-device copy and one strided device copy.  `reps`
replicas of the stream arena and of every reply, device events around `reps` back-to-back calls (one
per replica; h's copy to the host makes each of its calls wait for the one before), a warm-up round,
the forms alternating over `rounds` rounds, median / min / max in us per call.  Before any timing the
outputs are compared: r's reply with h's, byte for byte, its first and last header with Python's own
formatting, and p's contents with r's.  A form counts as faster or slower than another only when the
medians differ by more than the two forms' min-max spreads together.

usage: python tools/readn_reply_sweep.py [--rounds 7] [--out profiles/readn_reply.json]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "c-filestorage-server-and-client_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rle_mi355x as R  # noqa: E402

KINDS = {"random": 1, "runs50": 2}
# (n, U, reps, segmented)
SHAPES = ((1, 4096, 8, False), (64, 4096, 8, False), (4096, 4096, 8, False), (1, 65536, 8, False),
          (64, 65536, 8, False), (4096, 65536, 4, False), (1, 1 << 20, 8, True), (64, 1 << 20, 4, True))
PLEN, GAP = 29, 49
FORM = R.RLE_REPLY_READN | R.RLE_REPLY_END
POISON = 0xA5
POW10 = 10 ** np.arange(9, -1, -1, dtype=np.int64)


def r16(x):
    return (x + 15) & ~15


def shape(n, U, kind, reps, seg, rounds, dev):
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)   # noqa: E731
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    kind_t = torch.full((n,), KINDS[kind], dtype=torch.int32, device=dev)
    slot, cslot, row = r16(U), r16(R.max_compressed_size(U)), GAP + U
    d_x = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    x_off, c_off, len_u = ar * slot, ar * cslot, i64([U] * n)
    R.gen_synthetic(d_x, x_off, len_u, kind_t, ar)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    base = torch.zeros(n * cslot, dtype=torch.uint8, device=dev)
    clen = torch.zeros(n, dtype=torch.int64, device=dev)
    R.encode_batch(d_x, x_off, len_u, base, c_off, clen, st)
    tail = torch.zeros(n, dtype=torch.int64, device=dev)
    ulen = torch.zeros(n, dtype=torch.int64, device=dev)
    R.tail_batch(base, c_off, clen, tail, ulen, st)
    torch.cuda.synchronize()
    assert int(st.abs().sum().item()) == 0 and bool((ulen == U).all())
    tin = int(clen.sum().item())
    ws = R.decode_packed_seg_workspace(n, tin, dev) if seg else None
    streams = base.expand(reps, -1).contiguous()                    # replicas of the stream arena
    # the path table on the device, and the host's header template (names and their length fields)
    names = [b"/srv/store/file_%013d" % i for i in range(n)]
    assert all(len(p) == PLEN for p in names)
    d_paths = torch.from_numpy(np.frombuffer(b"".join(names), np.uint8).copy()).to(dev)
    path_off, path_len, gap = ar * PLEN, i64([PLEN] * n), i64([GAP] * n)
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
            R.readn_batch_seg(streams[k], c_off, clen, ulen, gap, out, place, total, status, out_cap=cap,
                              total_in_bytes=tin, ws=ws)
        else:
            R.readn_batch(streams[k], c_off, clen, ulen, gap, out, place, total, status, out_cap=cap)

    def form_r(k):
        if seg:
            R.readn_reply_seg(streams[k], c_off, clen, ulen, d_paths, path_off, path_len, reply["r"][k], place, total,
                              sts["r"], form=FORM, out_cap=cap, total_in_bytes=tin, ws=ws)
        else:
            R.readn_reply(streams[k], c_off, clen, ulen, d_paths, path_off, path_len, reply["r"][k], place, total,
                          sts["r"], form=FORM, out_cap=cap)

    def form_p(k):
        contents(k, reply["p"][k], sts["p"])

    def form_h(k):
        u = ulen.cpu().numpy()                      # the lengths through the host
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
    assert torch.equal(body(reply["r"]), d_x.view(n, slot)[:, :U]), "r is not the content"
    assert bool((reply["p"][0][:n * row].view(n, row)[:, :GAP] == POISON).all())

    forms = (("r", form_r), ("p", form_p), ("h", form_h))
    times = {name: [] for name, _ in forms}
    s = torch.cuda.current_stream()
    for rnd in range(rounds + 1):   # round 0 warms every form at this shape
        for name, fn in forms:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for k in range(reps):
                fn(k)
            e1.record(s)
            torch.cuda.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1) / reps * 1e3)
    row_ = {"n": n, "U": U, "kind": kind, "entry": "rle_readn_reply_device" + ("_seg" if seg else ""), "gap": GAP,
            "stream_bytes": tin, "reply_bytes": cap, "reps": reps, "rounds": rounds, "outputs_equal": True}
    for name in times:
        v = sorted(times[name])
        row_[name] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2)}
    spread = lambda f: row_[f]["max_us"] - row_[f]["min_us"]   # noqa: E731
    for other in "ph":
        d = row_["r"]["median_us"] - row_[other]["median_us"]
        sp = spread("r") + spread(other)
        row_["r_over_" + other] = round(row_["r"]["median_us"] / row_[other]["median_us"], 3)
        row_["r_minus_" + other + "_us"] = round(d, 2)
        row_["r_spread_with_" + other + "_us"] = round(sp, 2)
        row_["r_vs_" + other] = "slower" if d > sp else ("faster" if -d > sp else "within the spread")
    return row_


def table(rows):
    out = ["| files x U | kind | entry | r | p | h | r - p | r / h |", "|---|---|---|---|---|---|---|---|"]
    cell = lambda r, k: f"{r[k]['median_us']:.1f} ({r[k]['min_us']:.1f}-{r[k]['max_us']:.1f})"   # noqa: E731
    for r in rows:
        out.append(f"| {r['n']} x {r['U'] >> 10} KiB | {r['kind']} | {'seg' if r['entry'].endswith('_seg') else 'one-wave'} | "
                   f"{cell(r, 'r')} | {cell(r, 'p')} | {cell(r, 'h')} | {r['r_minus_p_us']:+.1f} us {r['r_vs_p']} | "
                   f"{r['r_over_h']:.2f} {r['r_vs_h']} |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kinds", default="random,runs50")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "readn_reply.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "readn_reply_sweep.py measures on an MI355X"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    rows = []
    for n, U, reps, seg in SHAPES:
        for kind in a.kinds.split(","):
            rows.append(shape(n, U, kind, reps, seg, a.rounds, dev))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    res = {"tool": "tools/readn_reply_sweep.py", "device": torch.cuda.get_device_name(0), "library": R.version(),
           "forms": {"r": "rle_readn_reply_device(_seg): layout with derived gaps, packed decode, headers and terminator",
                     "p": "rle_readn_batch_device(_seg) alone, the 49-byte gaps left unwritten",
                     "h": "d_ulen copied to the host, headers formatted there into a prepared template, copied back "
                          "and into the gaps by one strided device copy, then p"},
           "timing": "device events around `reps` back-to-back calls (one per replica of the arenas), forms "
                     "alternating over `rounds` rounds after a warm-up round; us per call of n files; median (min-max)",
           "rows": rows, "table": table(rows).split("\n")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(table(rows))


if __name__ == "__main__":
    main()
