#!/usr/bin/env python3
"""Sizing an append before it is written: the size and fit entries against the plain append, timed
in one process on the same files (not bench.py; DESIGN.md §4b quotes the table).

  p  plain append   rle_append_batch_device[_seg]: worst-case slots, C' known only afterwards
  z  size only      rle_append_size_batch_device[_seg]: d_need, nothing else written
  f  fit, cap = C'  rle_append_fit_batch_device[_seg] with exact capacities (one-wave: the size
                    walk and then the write walk)
  g  fit, worst     the same entry with cap = rle_append_slot_bytes (one-wave: the size walk skipped)

Per shape (n files of U old bytes each, A new bytes each, one synthetic kind; the one-wave forms for
small A, the segmented forms for 1 MiB): as tools/append_sweep.py and tools/append_seg_sweep.py --
files generated and encoded on the device, `reps` replicas of the stream arena because an append
changes its file, device events around `reps` back-to-back launches (one per replica), replicas
restored untimed before every timing, a warm-up round, the forms alternating over `rounds` rounds,
median / min / max.  Before any timing the outputs are compared: z's d_need with p's new lengths, f's
and g's streams, lengths, decoded lengths and tail words with p's.  The baseline is p in the same
process; a form counts as slower or faster than p only when the medians differ by more than the two
forms' min-max spreads together.

usage: python tools/append_fit_sweep.py [--rounds 7] [--n 4096] [--out profiles/append_fit.json]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "c-filestorage-server-and-client_amd")]
import torch  # noqa: E402

import rle_mi355x as R  # noqa: E402

KINDS = {"random": 1, "runs50": 2}
SHAPES = ((4096, 4096, 8, False), (4096, 64, 8, False), (1, 1 << 20, 8, True), (64, 1 << 20, 4, True))   # (n, A, reps, seg)
OLD = 4096


def r16(x):
    return (x + 15) & ~15


def shape(n, U, A, kind, reps, seg, rounds, dev):
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)   # noqa: E731
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    kind_t = torch.full((n,), KINDS[kind], dtype=torch.int32, device=dev)
    us, as_ = r16(U), r16(A)
    d_old = torch.zeros(n * us, dtype=torch.uint8, device=dev)
    d_new = torch.zeros(n * as_, dtype=torch.uint8, device=dev)
    old_off, new_off = ar * us, ar * as_
    len_u, len_a = i64([U] * n), i64([A] * n)
    R.gen_synthetic(d_old, old_off, len_u, kind_t, ar)
    R.gen_synthetic(d_new, new_off, len_a, kind_t, ar + n)
    cap = R.append_slot_bytes(R.max_compressed_size(U), A)
    assert cap
    s_off, caps = ar * cap, i64([cap] * n)
    base = torch.zeros(n * cap, dtype=torch.uint8, device=dev)
    base_len = torch.zeros(n, dtype=torch.int64, device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    R.encode_batch(d_old, old_off, len_u, base, s_off, base_len, st)
    base_tail = torch.zeros(n, dtype=torch.int64, device=dev)
    base_ulen = torch.zeros(n, dtype=torch.int64, device=dev)
    R.tail_batch(base, s_off, base_len, base_tail, base_ulen, st)
    torch.cuda.synchronize()
    assert int(st.abs().sum().item()) == 0 and bool((base_ulen == U).all())
    rep = torch.empty(reps, n * cap, dtype=torch.uint8, device=dev)
    lens = torch.empty(reps, n, dtype=torch.int64, device=dev)
    tails = torch.empty(reps, n, dtype=torch.int64, device=dev)
    ulens = torch.empty(reps, n, dtype=torch.int64, device=dev)
    need = torch.zeros(n, dtype=torch.int64, device=dev)       # z's result: f's capacities
    need_f = torch.zeros(n, dtype=torch.int64, device=dev)
    sts = {name: torch.zeros(n, dtype=torch.int32, device=dev) for name in "pzfg"}
    total = n * A
    ws = R.append_seg_workspace(n, total, dev) if seg else None
    kw = dict(total_new_bytes=total, workspace=ws) if seg else {}
    plain, size, fit = ((R.append_batch_seg, R.append_size_seg, R.append_fit_seg) if seg else
                        (R.append_batch, R.append_size, R.append_fit))

    def restore():
        rep.copy_(base.expand(reps, -1))
        lens.copy_(base_len.expand(reps, -1))
        tails.copy_(base_tail.expand(reps, -1))
        ulens.copy_(base_ulen.expand(reps, -1))

    def form_p(k):
        plain(rep[k], s_off, lens[k], caps, ulens[k], d_new, new_off, len_a, sts["p"], tail=tails[k], **kw)

    def form_z(k):
        size(rep[k], s_off, lens[k], tails[k], d_new, new_off, len_a, need, sts["z"], **kw)

    def form_f(k):
        fit(rep[k], s_off, lens[k], need, ulens[k], d_new, new_off, len_a, need_f, sts["f"], tail=tails[k], **kw)

    def form_g(k):
        fit(rep[k], s_off, lens[k], caps, ulens[k], d_new, new_off, len_a, need_f, sts["g"], tail=tails[k], **kw)

    def same_streams(a, b):
        ok = True
        step = max(1, (64 << 20) // cap)   # (in pieces: the masks are n x cap)
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            live = torch.arange(cap, device=dev)[None, :] < lens[a][lo:hi, None]
            va, vb = (t.view(n, cap)[lo:hi] for t in (rep[a], rep[b]))
            ok = ok and bool(((va == vb) | ~live).all())
        return ok

    # the outputs first: z's need is p's new length and z wrote nothing; f and g leave what p leaves
    restore()
    form_z(1)
    torch.cuda.synchronize()
    assert torch.equal(rep[1], base) and torch.equal(lens[1], base_len) and torch.equal(tails[1], base_tail)
    form_p(0)
    form_f(1)
    torch.cuda.synchronize()
    assert all(int(sts[k].abs().sum().item()) == 0 for k in "pzf")
    assert torch.equal(need, lens[0]) and torch.equal(need_f, lens[0])
    assert torch.equal(lens[0], lens[1]) and torch.equal(tails[0], tails[1]) and torch.equal(ulens[0], ulens[1])
    assert same_streams(0, 1), "f's streams differ from p's"
    restore()
    form_p(0)
    form_g(1)
    torch.cuda.synchronize()
    assert int(sts["g"].abs().sum().item()) == 0 and torch.equal(need_f, lens[0])
    assert torch.equal(lens[0], lens[1]) and torch.equal(tails[0], tails[1]) and torch.equal(ulens[0], ulens[1])
    assert same_streams(0, 1), "g's streams differ from p's"
    c_new = int(lens[0].sum().item())

    forms = (("p", form_p), ("z", form_z), ("f", form_f), ("g", form_g))
    times = {name: [] for name, _ in forms}
    s = torch.cuda.current_stream()
    for rnd in range(rounds + 1):   # round 0 warms every form at this shape
        for name, fn in forms:
            restore()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for k in range(reps):
                fn(k)
            e1.record(s)
            torch.cuda.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1) / reps * 1e3)
    row = {"n": n, "U": U, "A": A, "kind": kind, "form": "segmented" if seg else "one-wave",
           "old_stream_bytes": int(base_len.sum().item()), "new_stream_bytes": c_new,
           "worst_case_slot_bytes": n * cap, "reps": reps, "rounds": rounds, "outputs_equal": True}
    if seg:
        row["segment_bytes"] = R.seg_segment_bytes(total)
    for name in times:
        v = sorted(times[name])
        row[name] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2)}
    spread = lambda f: row[f]["max_us"] - row[f]["min_us"]   # noqa: E731
    for name in "zfg":
        d = row[name]["median_us"] - row["p"]["median_us"]
        sp = spread(name) + spread("p")
        row[name + "_over_p"] = round(row[name]["median_us"] / row["p"]["median_us"], 3)
        row[name + "_minus_p_us"] = round(d, 2)
        row[name + "_spread_with_p_us"] = round(sp, 2)
        row[name + "_vs_p"] = "slower" if d > sp else ("faster" if -d > sp else "within the spread")
    return row


def table(rows):
    out = ["| files x A | kind | form | p | z | f | g | z / p | f / p | g / p |", "|---|---|---|---|---|---|---|---|---|---|"]
    cell = lambda r, k: f"{r[k]['median_us']:.1f} ({r[k]['min_us']:.1f}-{r[k]['max_us']:.1f})"   # noqa: E731
    for r in rows:
        a = f"{r['A'] >> 20} MiB" if r["A"] >= 1 << 20 else (f"{r['A'] >> 10} KiB" if r["A"] >= 1024 else f"{r['A']} B")
        out.append(f"| {r['n']} x {a} | {r['kind']} | {r['form']} | {cell(r, 'p')} | {cell(r, 'z')} | {cell(r, 'f')} | "
                   f"{cell(r, 'g')} | {r['z_over_p']:.2f} {r['z_vs_p']} | {r['f_over_p']:.2f} {r['f_vs_p']} | "
                   f"{r['g_over_p']:.2f} {r['g_vs_p']} |")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kinds", default="random,runs50")
    ap.add_argument("--n", type=int, default=0, help="only the shapes of this many files (under a kernel trace)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "append_fit.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "append_fit_sweep.py measures on an MI355X"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    rows = []
    for n, A, reps, seg in SHAPES:
        if a.n and n != a.n:
            continue
        for kind in a.kinds.split(","):
            rows.append(shape(n, OLD, A, kind, reps, seg, a.rounds, dev))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    res = {"tool": "tools/append_fit_sweep.py", "device": torch.cuda.get_device_name(0), "library": R.version(),
           "forms": {"p": "rle_append_batch_device[_seg], worst-case slots, tail words carried",
                     "z": "rle_append_size_batch_device[_seg]",
                     "f": "rle_append_fit_batch_device[_seg], cap = C' (from z)",
                     "g": "rle_append_fit_batch_device[_seg], cap = rle_append_slot_bytes"},
           "timing": "device events around `reps` back-to-back launches (one per replica of the stream arena), "
                     "forms alternating over `rounds` rounds after a warm-up round; us per launch of n files; "
                     "median (min-max)",
           "rows": rows, "table": table(rows).split("\n")}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(table(rows))


if __name__ == "__main__":
    main()
