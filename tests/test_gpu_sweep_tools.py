"""The eight sweep tools on the GPU, each at its smallest shape in a process of its own: the tool's
own output comparisons pass (it exits 0), and the file it writes has the committed result's
top-level keys and row keys, in order, with the rounds and reps that were asked for.  No time is
asserted.  Run with -x: a tool that exits non-zero or on a signal is a finding, not a retry."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = {"append_sweep": "append_batch", "append_seg_sweep": "append_seg", "append_fit_sweep": "append_fit",
         "tail_seg_sweep": "tail_seg", "readn_pack_sweep": "readn_pack", "readn_pack_seg_sweep": "readn_pack_seg",
         "readn_reply_sweep": "readn_reply", "relocate_sweep": "relocate"}


@pytest.mark.parametrize("tool", TOOLS)
def test_tool_runs_its_smallest_shape(tool, tmp_path):
    with open(os.path.join(ROOT, "profiles", TOOLS[tool] + ".json")) as f:
        want = json.load(f)
    rounds = 7 if tool == "tail_seg_sweep" else 1   # (tail_seg refuses fewer)
    out = tmp_path / "out.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool + ".py"), "--shapes", "0", "--rounds", str(rounds),
                        "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    with open(out) as f:
        got = json.load(f)
    assert list(got) == list(want) and got["tool"] == want["tool"] == f"tools/{tool}.py"
    assert got["forms"] == want["forms"] and got["timing"] == want["timing"]
    first = want["rows"][0]   # the committed files begin with shape 0
    shape = lambda r: [r[k] for k in ("n", "U", "A", "C") if k in r]   # noqa: E731
    assert got["rows"] and all(shape(r) == shape(first) for r in got["rows"])
    for r in got["rows"]:
        assert list(r) == list(first), (list(r), list(first))
        assert r["rounds"] == rounds and r["reps"] == first["reps"]
        assert all(list(r[k]) == list(first[k]) for k in r if isinstance(r[k], dict))
    if "table" in want:
        assert got["table"][:2] == want["table"][:2] and len(got["table"]) == 2 + len(got["rows"])
