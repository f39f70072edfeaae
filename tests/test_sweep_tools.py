"""The sweep tools' shared module (tools/sweeplib.py) on the CPU: its verdict rule, statistics and
table writer reproduce every committed result file of the eight tools field for field, the rule's
edges fall where the method says, the timing loop makes its calls in the stated order, and no tool
keeps a copy of the rule or the loop.  Nothing here opens a device."""
import importlib
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import sweeplib as S  # noqa: E402

PROFILES = ("append_batch", "append_seg", "append_fit", "tail_seg", "readn_pack", "readn_pack_seg", "readn_reply",
            "readn_reply_run2", "relocate", "relocate_run2")
TABLES = ("append_fit", "readn_pack", "readn_pack_seg", "readn_reply", "readn_reply_run2", "relocate", "relocate_run2")
EIGHT = ("append_sweep", "append_seg_sweep", "append_fit_sweep", "tail_seg_sweep", "readn_pack_sweep",
         "readn_pack_seg_sweep", "readn_reply_sweep", "relocate_sweep")


def committed(name):
    with open(os.path.join(ROOT, "profiles", name + ".json")) as f:
        res = json.load(f)
    return res, importlib.import_module(os.path.basename(res["tool"])[:-3])


def figures(row):
    """The row's per-form figures alone: what the shared functions may look at."""
    return {k: dict(v) for k, v in row.items() if isinstance(v, dict)}


def reproduce(name):
    """Every derived field and the table of one committed file, from the shared functions; how many of each."""
    res, tool = committed(name)
    count = dict.fromkeys(("vs", "minus", "spread_with", "over", "table"), 0)
    assert res["tool"] == "tools/" + tool.__name__ + ".py" and tool.__name__ in EIGHT
    assert res["forms"] == tool.FORMS and res["timing"] == tool.TIMING
    for row in res["rows"]:
        judged = {m.group(1, 2) for k in row for m in [re.fullmatch(r"(\w)_vs_(\w)", k)] if m}
        assert all(f"{a}_over_{b}" in row for a, b in judged)
        for k in row:
            m = re.fullmatch(r"(\w)_over_(\w)", k)
            if not m:
                continue
            a, b = m.groups()
            got = figures(row)
            if (a, b) in judged:
                S.verdict(got, a, b)
                for field, kind in ((f"{a}_vs_{b}", "vs"), (f"{a}_minus_{b}_us", "minus"),
                                    (f"{a}_spread_with_{b}_us", "spread_with")):
                    assert got[field] == row[field] and type(got[field]) is type(row[field]), (name, field, row)
                    count[kind] += 1
            else:
                S.over(got, a, b)
            assert got[k] == row[k], (name, k, row)
            count["over"] += 1
        if name == "append_seg":   # its older fields come from the shared verdicts, too
            got = tool.judged(figures(row))
            assert len(got) == 3 + 5 and all(row[k] == v for k, v in got.items()), row
    assert ("table" in res) is (name in TABLES)
    if "table" in res:
        assert tool.table(res["rows"]).split("\n") == res["table"]
        count["table"] = 1
    return count


@pytest.mark.parametrize("name", PROFILES)
def test_committed_results_are_reproduced(name):
    reproduce(name)


def test_no_file_row_or_field_is_left_out():
    """The counts of the tools before the fold over the same ten files."""
    counts = [reproduce(name) for name in PROFILES]
    assert {k: sum(c[k] for c in counts) for k in counts[0]} == {"vs": 192, "minus": 192, "spread_with": 192,
                                                                 "over": 234, "table": 7}


def row_of(**forms):
    return {k: dict(zip(("median_us", "min_us", "max_us"), v)) for k, v in forms.items()}


def test_a_difference_equal_to_the_spreads_is_within_the_spread():
    for a, b in (((12.0, 11.0, 13.0), (9.0, 8.5, 9.5)), ((9.0, 8.5, 9.5), (12.0, 11.0, 13.0))):
        row = row_of(a=a, b=b)
        S.verdict(row, "a", "b")
        assert row["a_spread_with_b_us"] == 3.0 and abs(row["a_minus_b_us"]) == 3.0
        assert row["a_vs_b"] == "within the spread"
    for a, b, want in (((12.25, 11.0, 13.0), (9.0, 8.5, 9.5), "slower"), ((9.0, 8.5, 9.5), (12.25, 11.0, 13.0), "faster")):
        row = row_of(a=a, b=b)
        S.verdict(row, "a", "b")
        assert row["a_vs_b"] == want
    assert row["a_over_b"] == round(9.0 / 12.25, 3)
    S.over(row, "a", "b")
    assert row["a_over_b"] == 0.73


def test_the_verdict_is_taken_from_the_rounded_figures():
    b = [10.0, 10.0, 10.0]
    # unrounded, a's median is 2.004 above b's and the spreads make 2.0: slower; rounded, 2.0 against 2.0
    a = [11.0, 13.0, 12.004]
    assert sorted(a)[1] - sorted(b)[1] > (max(a) - min(a)) + (max(b) - min(b))
    row = {"a": S.stats(a), "b": S.stats(b)}
    assert row["a"] == {"median_us": 12.0, "min_us": 11.0, "max_us": 13.0}
    S.verdict(row, "a", "b")
    assert row["a_vs_b"] == "within the spread" and row["a_minus_b_us"] == 2.0 and row["a_spread_with_b_us"] == 2.0
    # and the other way: unrounded 2.006 against 2.008, rounded 2.01 against 2.0
    a = [13.004, 10.996, 12.006]
    assert not sorted(a)[1] - sorted(b)[1] > (max(a) - min(a)) + (max(b) - min(b))
    row = {"a": S.stats(a), "b": S.stats(b)}
    assert row["a"] == {"median_us": 12.01, "min_us": 11.0, "max_us": 13.0}
    S.verdict(row, "a", "b")
    assert row["a_vs_b"] == "slower" and row["a_minus_b_us"] == 2.01 and row["a_spread_with_b_us"] == 2.0
    S.verdict(row, "b", "a")
    assert row["b_vs_a"] == "faster" and row["b_minus_a_us"] == -2.01 and row["b_over_a"] == round(10.0 / 12.01, 3)


def test_statistics():
    assert S.stats([4.0, 1.0, 3.0, 2.0]) == {"median_us": 3.0, "min_us": 1.0, "max_us": 4.0}   # the upper middle value
    assert S.stats([5.0, 1.0, 3.0]) == {"median_us": 3.0, "min_us": 1.0, "max_us": 5.0}
    assert S.stats([7.126]) == {"median_us": 7.13, "min_us": 7.13, "max_us": 7.13}
    assert S.cell({"p": S.stats([7.126])}, "p") == "7.1 (7.1-7.1)"
    assert [S.size_name(b) for b in (64, 4096, 65536, 1 << 20)] == ["64 B", "4 KiB", "64 KiB", "1 MiB"]
    assert S.r16(0) == 0 and S.r16(1) == 16 and S.r16(16) == 16 and S.r16(49 + 4096) == 4160


class FakeCuda:
    """torch.cuda's part in the loop, recording every call; an event pair measures 8 ms."""

    def __init__(self):
        self.log = []

    def current_stream(self):
        self.log.append("current_stream")
        return "the stream"

    def synchronize(self):
        self.log.append("sync")

    def Event(self, enable_timing=False):
        assert enable_timing
        fake = self

        class Event:
            def record(self, stream):
                fake.log.append(("record", stream))

            def elapsed_time(self, other):
                fake.log.append("elapsed")
                return 8.0
        return Event()


@pytest.mark.parametrize("with_before", [False, True])
def test_the_timing_loop_calls_in_order(with_before):
    cuda = FakeCuda()
    forms = [(name, lambda k, name=name: cuda.log.append((name, k))) for name in ("x", "y")]
    before = (lambda: cuda.log.append("before")) if with_before else None
    reps, rounds = 4, 3
    times = S.time_forms(forms, reps, rounds, before=before, cuda=cuda)
    assert times == {"x": [2000.0] * rounds, "y": [2000.0] * rounds}   # 8 ms / 4 calls, in us; round 0 gives no sample
    want = ["current_stream"]
    for rnd in range(rounds + 1):
        for name in ("x", "y"):
            want += ["before"] * with_before + ["sync", ("record", "the stream")]
            want += [(name, k) for k in range(reps)]
            want += [("record", "the stream"), "sync"] + ["elapsed"] * bool(rnd)
    assert cuda.log == want
    assert cuda.log.count("before") == (2 * (rounds + 1) if with_before else 0)


def test_no_copy_of_the_rule_or_the_loop_is_left():
    files = [os.path.join(TOOLS, t + ".py") for t in EIGHT + ("sweeplib",)]
    assert all(os.path.exists(f) for f in files)
    for text in ("elapsed_time", "within the spread"):
        holders = [os.path.basename(f) for f in files if text in open(f).read()]
        assert holders == ["sweeplib.py"], (text, holders)
