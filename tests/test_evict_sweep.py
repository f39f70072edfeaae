"""tools/evict_sweep.py on the CPU: its committed result files (profiles/evict.json and _run2.json) are
reproduced field for field by the shared verdict rule and table writer of tools/sweeplib.py, as
tests/test_sweep_tools.py does for the other tools, and its host route's selection is the reference's
loop (tests/evict_model.py).  Nothing here opens a device."""
import json
import os
import sys

import numpy as np
import pytest

import evict_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import evict_sweep as T  # noqa: E402
import sweeplib as S  # noqa: E402


@pytest.mark.parametrize("name", ["evict", "evict_run2"])
def test_committed_results_are_reproduced(name):
    with open(os.path.join(ROOT, "profiles", name + ".json")) as f:
        res = json.load(f)
    assert res["tool"] == "tools/evict_sweep.py" and res["forms"] == T.FORMS and res["timing"] == T.TIMING
    assert res["limits"] == T.LIMITS
    assert [(r["n"], r["limit"]) for r in res["rows"]] == [(n, v) for n, _ in T.SHAPES for v in T.LIMITS]
    for row in res["rows"]:
        got = {k: dict(v) for k, v in row.items() if isinstance(v, dict)}
        for f in "sg":
            S.verdict(got, f, "h")
        assert row["outputs_equal"] is True and all(row[k] == v for k, v in got.items()), row
    assert T.table(res["rows"]).split("\n") == res["table"]


def test_host_route_selects_what_the_loop_selects():
    rng = np.random.default_rng(3)
    for _ in range(30):
        n = int(rng.integers(1, 200))
        k = rng.integers(0, 40, n).astype(np.uint64) << np.uint64(rng.integers(0, 57))
        ln, wn = rng.integers(0, 500, n).astype(np.uint64), rng.integers(0, 600, n).astype(np.uint64)
        lv, sp = (rng.integers(0, 6, n) != 0).astype(np.int32), (rng.integers(0, 6, n) == 0).astype(np.int32)
        args = [[int(x) for x in v] for v in (k, ln, wn, lv, sp)]
        eligible = M.totals(M.store(*args))[2]
        total = M.totals(M.store(*args))[0]
        max_bytes = int(rng.integers(total - eligible, total + 2))     # (a limit the eligible files can meet)
        want = M.loop_model(*args, max_bytes=max_bytes)
        keep, victims, before, after = T.host_select(k, ln, wn, lv, sp, max_bytes)
        assert want.status == M.OK and want.victims == victims.tolist() and want.keep == keep.tolist()
        assert want.summary[2:4] == [before, after]
