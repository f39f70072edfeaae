#!/usr/bin/env python3
"""Markdown table of a tools/ab_events.py run (its stdout): per workload, each build's median
encode / decode µs and the change against the base build (the product, or --base NAME), plus the
round-trip check.  With --twin NAME[,NAME] (further copies of the base build loaded beside it) the
A/A spread, the largest |twin / base - 1|, is printed per workload and kind, and each change is
marked against it: `+` a gain of more than twice the spread, `-` a loss of more than the spread.
usage: python tools/ab_events_table.py <run dir>/ab.json [title] [--base parent --twin parent2,parent3]"""
import json
import sys


def opt(name):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None


def main():
    base_name, twin = opt("--base") or "product", opt("--twin")
    args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in ("--base", "--twin")]
    path = args[0]
    title = args[1] if len(args) > 1 else path
    rows = []
    for line in open(path):
        line = line.strip()
        if not line or line.startswith("{"):
            continue
        wl, js = line.split(" ", 1)
        rows.append((wl, json.loads(js)))
    builds = list(rows[0][1]) if rows else []
    print(f"# {title}\n")
    print("Same-process A/B (tools/ab_events.py): median of the rounds, each round the mean of back-to-back "
          "launches timed by HIP events.  ok = the build's round trip reproduced the input exactly "
          "(ablation builds are timing-only and may fail it).\n")
    if twin:
        print(f"| workload | build | encode µs | vs {base_name} | decode µs | vs {base_name} | ok |")
        print("|---|---|---|---|---|---|---|")
    else:
        print(f"| workload | build | encode µs | decode µs | decode vs {base_name} | ok |")
        print("|---|---|---|---|---|---|")
    for wl, d in rows:
        base = d[base_name]
        twins = twin.split(",") if twin else []
        spread = {k: max(abs(d[t][k]["median_us"] / base[k]["median_us"] - 1) for t in twins) for k in ("enc", "dec")} if twin else None
        for b in builds:
            v = d[b]
            enc, dec = v["enc"]["median_us"], v["dec"]["median_us"]
            ok = "yes" if v["ok"] else "no"
            if not twin:
                print(f"| {wl} | {b} | {enc:.2f} | {dec:.2f} | {100 * (dec / base['dec']['median_us'] - 1):+.1f} % | {ok} |")
                continue
            cells = []
            for k, t in (("enc", enc), ("dec", dec)):
                r = t / base[k]["median_us"] - 1
                mark = "" if b == base_name or b in twins else " `+`" if -r > 2 * spread[k] else " `-`" if r > spread[k] else ""
                cells += [f"{t:.2f}", f"{100 * r:+.1f} %{mark}"]
            print(f"| {wl} | {b} | {cells[0]} | {cells[1]} | {cells[2]} | {cells[3]} | {ok} |")
        if twin:
            print(f"| {wl} | *A/A spread* | | {100 * spread['enc']:.1f} % | | {100 * spread['dec']:.1f} % | |")


if __name__ == "__main__":
    main()
