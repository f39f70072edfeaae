"""What the same-process sweep tools share: the setup of stored files on the device, the timing
loop, the statistics, the verdict rule, the table writer and the main.  (append_sweep,
append_seg_sweep, append_fit_sweep, tail_seg_sweep, readn_pack_sweep, readn_pack_seg_sweep,
readn_reply_sweep, relocate_sweep and evict_sweep import it; not bench.py, and no tool of its own.)

The method, once for all of them.  A tool times a few forms of the same work in one process on the
same files.  Per shape it makes `reps` replicas of every arena a call reads or writes, so that
back-to-back calls do not find what the call before left in the caches (and, for an append, because
the call changes its file).  A timing is device events on the current stream around `reps`
back-to-back calls, one per replica, with a synchronise before the first event and after the
second; what has to be put back between timings (the append tools' replicas) is restored before that
synchronise, outside the events.  Round 0 warms every form at the shape and is dropped; then the
forms alternate, in the given order, over `rounds` rounds.  A form's figure is the median of its
rounds (the upper middle value of an even count) with the min and the max, in us per call, each
rounded to 2 decimals.  The verdict is taken from those rounded figures: a form counts as slower or
faster than another only when the medians differ by more than the two forms' min-max spreads
together, and is "within the spread" otherwise.  A table cell is `median (min-max)`.  Every tool
compares its forms' outputs before any timing; a tool that exits 0 has passed them.

A tool supplies: its shapes, its forms (`form_*`) and their texts, its output checks, its row's own
fields, its table's columns, and one call of main()."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "c-filestorage-server-and-client_amd")]
import torch  # noqa: E402

import rle_mi355x as R  # noqa: E402

KINDS = {"random": 1, "runs50": 2}


def r16(x):
    return (x + 15) & ~15


def size_name(b):
    return f"{b >> 20} MiB" if b >= 1 << 20 else (f"{b >> 10} KiB" if b >= 1024 else f"{b} B")


def device(tool):
    assert torch.cuda.is_available(), f"{tool} measures on an MI355X"
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def gen_files(n, U, kind, dev, slot=None, index_base=0):
    """n files of U bytes of one synthetic kind in slots of `slot` bytes (16-byte aligned by default),
    file i from generator index index_base + i: the arena, the offsets, the lengths."""
    slot = r16(U) if slot is None else slot
    ar = torch.arange(n, dtype=torch.int64, device=dev)
    d_x = torch.zeros(n * slot, dtype=torch.uint8, device=dev)
    x_off, len_u = ar * slot, torch.full((n,), U, dtype=torch.int64, device=dev)
    R.gen_synthetic(d_x, x_off, len_u, torch.full((n,), KINDS[kind], dtype=torch.int32, device=dev), ar + index_base)
    return d_x, x_off, len_u


def stored_files(n, U, kind, cslot, dev, slot=None, index_base=0, tail=True):
    """gen_files, encoded on the device into slots of `cslot` bytes and (tail=True) tail-scanned, every
    status checked.  x / x_off / len_u: the content; streams / s_off / clen: the stored streams;
    tail / ulen: the scan's tail words and decoded lengths (None without the scan)."""
    z = lambda dt: torch.zeros(n, dtype=dt, device=dev)   # noqa: E731
    x, x_off, len_u = gen_files(n, U, kind, dev, slot, index_base)
    f = SimpleNamespace(x=x, x_off=x_off, len_u=len_u, clen=z(torch.int64), tail=None, ulen=None,
                        streams=torch.zeros(n * cslot, dtype=torch.uint8, device=dev),
                        s_off=torch.arange(n, dtype=torch.int64, device=dev) * cslot)
    st = z(torch.int32)
    R.encode_batch(x, x_off, len_u, f.streams, f.s_off, f.clen, st)
    if tail:
        f.tail, f.ulen = z(torch.int64), z(torch.int64)
        R.tail_batch(f.streams, f.s_off, f.clen, f.tail, f.ulen, st)
    torch.cuda.synchronize()
    assert int(st.abs().sum().item()) == 0 and (not tail or bool((f.ulen == U).all()))
    return f


def replicas(reps, *base):
    """`reps` copies of every base tensor, and the function that puts the bases back into them."""
    rep = [torch.empty(reps, *b.shape, dtype=b.dtype, device=b.device) for b in base]

    def restore():
        for r, b in zip(rep, base):
            r.copy_(b.expand(reps, *b.shape))
    return (*rep, restore)


def same_streams(a, b, lens, cap):
    """Two arenas of len(lens) slots of cap bytes hold the same bytes below every stream's length."""
    n, ok = lens.numel(), True
    step = max(1, (64 << 20) // cap)   # (in pieces: the masks are n x cap)
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        live = torch.arange(cap, device=lens.device)[None, :] < lens[lo:hi, None]
        ok = ok and bool(((a.view(n, cap)[lo:hi] == b.view(n, cap)[lo:hi]) | ~live).all())
    return ok


def time_forms(forms, reps, rounds, before=None, cuda=None):
    """{name: [us per call, one per timed round]} of the (name, fn) pairs in `forms`; fn(k) is one call
    on replica k, before() what has to be put back ahead of every timing."""
    cuda = cuda or torch.cuda
    times = {name: [] for name, _ in forms}
    s = cuda.current_stream()
    for rnd in range(rounds + 1):   # round 0 warms every form at this shape
        for name, fn in forms:
            if before:
                before()
            cuda.synchronize()
            e0, e1 = cuda.Event(enable_timing=True), cuda.Event(enable_timing=True)
            e0.record(s)
            for k in range(reps):
                fn(k)
            e1.record(s)
            cuda.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1) / reps * 1e3)
    return times


def timing_text(call, arenas, files, cells=True):
    """The result file's `timing` entry: what one timed call is, what is replicated, what n counts."""
    calls = {"call": "calls", "launch": "launches"}[call]
    return (f"device events around `reps` back-to-back {calls} (one per replica of {arenas}), forms alternating over "
            f"`rounds` rounds after a warm-up round; us per {call} of n {files}" + ("; median (min-max)" if cells else ""))


def stats(v):
    v = sorted(v)
    return {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2)}


def over(row, a, b, digits=2):
    row[f"{a}_over_{b}"] = round(row[a]["median_us"] / row[b]["median_us"], digits)


def verdict(row, a, b, digits=3):
    """Form a against form b, from the row's rounded figures: the ratio, the difference of the medians,
    the two spreads together, and which side of them the difference falls."""
    d = row[a]["median_us"] - row[b]["median_us"]
    sp = (row[a]["max_us"] - row[a]["min_us"]) + (row[b]["max_us"] - row[b]["min_us"])
    over(row, a, b, digits)
    row[f"{a}_minus_{b}_us"] = round(d, 2)
    row[f"{a}_spread_with_{b}_us"] = round(sp, 2)
    row[f"{a}_vs_{b}"] = "slower" if d > sp else ("faster" if -d > sp else "within the spread")


def cell(r, k):
    return f"{r[k]['median_us']:.1f} ({r[k]['min_us']:.1f}-{r[k]['max_us']:.1f})"


def ratio_cell(r, a, b):
    return f"{r[f'{a}_over_{b}']:.2f} {r[f'{a}_vs_{b}']}"


def table(header, rows, cells):
    """A markdown table: the column titles, then cells(r), a row's texts, for every row."""
    line = lambda c: "| " + " | ".join(c) + " |"   # noqa: E731
    return "\n".join([line(header), "|" + "---|" * len(header)] + [line(cells(r)) for r in rows])


def main(tool, shape, shapes, about, out, rounds=7, min_rounds=1, kinds=True, variants=(None,), options=(), keep=None,
         extra=None, table=None):
    """A tool's command line and result file.  shape(a, s, v, dev) measures one row: s an entry of
    `shapes` (a list, or a function of the parsed arguments), v a kind of --kinds or, without kinds, one
    of `variants`.  `about` opens the result (forms, timing and what else describes the run),
    extra(rows) follows it; keep(a, s) is the tool's own filter beside --shapes."""
    name = os.path.basename(tool)
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=rounds)
    if kinds:
        ap.add_argument("--kinds", default="random,runs50")
    for flag, kw in options:
        ap.add_argument(flag, **kw)
    ap.add_argument("--shapes", default="", help="comma-separated indices into the tool's shape list (default: all)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", out))
    a = ap.parse_args()
    assert a.rounds >= min_rounds, f"at least {min_rounds} rounds"
    dev = device(name)
    pick = {int(i) for i in a.shapes.split(",") if i}
    rows = []
    for i, s in enumerate(shapes(a) if callable(shapes) else shapes):
        if (pick and i not in pick) or (keep and not keep(a, s)):
            continue
        for v in (a.kinds.split(",") if kinds else variants):
            rows.append(shape(a, s, v, dev))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    res = {"tool": "tools/" + name, "device": torch.cuda.get_device_name(0), "library": R.version(), **about,
           **(extra(rows) if extra else {}), "rows": rows}
    if table:
        res["table"] = table(rows).split("\n")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if table:
        print(table(rows))
    return res
