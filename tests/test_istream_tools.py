"""The listing and A/B summaries behind profiles/istream_*.md (CPU): tools/asm_classes.py counts a
kernel's instructions per class and names the kernels that differ between two listing directories;
tools/ab_events_table.py marks a build's change against the A/A spread of the base build's copies."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")

LISTING = """\t.text
_ZN3rle1aEv:                            ; @_ZN3rle1aEv
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_waitcnt lgkmcnt(0)
\tv_mov_b32_e32 v0, 0
\ts_cmp_eq_u32 s0, 0
\ts_cbranch_scc1 .LBB0_2
\tds_read_b128 v[0:3], v0
\t;;#ASMSTART
\ts_nop 1
\t;;#ASMEND
.LBB0_2:
\tbuffer_store_dwordx4 v[0:3], v4, s[0:3], 0 offen
\ts_endpgm
.Lfunc_end0:
_ZN3rle1bEv:
\tv_add_u32_e32 v0, v0, v1
@EXTRA@\ts_endpgm
.Lfunc_end1:
"""


def _run(tool, *args):
    r = subprocess.run([sys.executable, os.path.join(TOOLS, tool), *args], capture_output=True, text=True, check=True)
    return r.stdout


def test_asm_classes_counts_and_diff(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    (a / "k.s").write_text(LISTING.replace("@EXTRA@", ""))
    (b / "k.s").write_text(LISTING.replace("@EXTRA@", "\ts_mov_b32 s0, 1\n"))
    out = _run("asm_classes.py", str(a))
    row = [l for l in out.splitlines() if "_ZN3rle1aEv" in l][0]
    assert "valu 1 salu 1 smem 1 lds 1 vmem 1 branch 2 nop 1 wait 1 total 9" in row
    same = _run("asm_classes.py", str(a), str(a))
    assert same.strip().endswith("2 kernels, 0 changed")
    diff = _run("asm_classes.py", str(b), str(a))
    assert "_ZN3rle1bEv" in diff and "_ZN3rle1aEv" not in diff
    assert diff.strip().endswith("2 kernels, 1 changed")


def test_ab_table_marks_against_the_spread(tmp_path):
    def b(enc, dec):
        return {"enc": {"median_us": enc, "min_us": enc}, "dec": {"median_us": dec, "min_us": dec}, "ok": True}

    res = {"parent": b(10.0, 10.0), "parent2": b(10.05, 9.9), "parent3": b(9.98, 10.0),
           "gain": b(9.8, 9.85), "loss": b(10.1, 10.05), "product": b(10.0, 10.0)}
    p = tmp_path / "ab.txt"
    p.write_text("cfg1 " + json.dumps(res) + "\n" + json.dumps({"cfg1": res}) + "\n")
    out = _run("ab_events_table.py", str(p), "t", "--base", "parent", "--twin", "parent2,parent3")
    rows = {l.split("|")[2].strip(): l for l in out.splitlines() if l.startswith("| cfg1")}
    assert "0.5 %" in rows["*A/A spread*"] and "1.0 %" in rows["*A/A spread*"]
    # encode: -2.0 % against a spread of 0.5 % is a gain; decode: -1.5 % against 1.0 % is not
    assert rows["gain"].count("`+`") == 1 and "-2.0 % `+`" in rows["gain"]
    # encode: +1.0 % is a loss beyond 0.5 %; decode: +0.5 % is inside 1.0 %
    assert rows["loss"].count("`-`") == 1 and "+1.0 % `-`" in rows["loss"]
    assert "`" not in rows["parent2"] and "`" not in rows["parent3"]
    # without --twin: the earlier form, against the product
    old = _run("ab_events_table.py", str(p))
    assert "decode vs product" in old
