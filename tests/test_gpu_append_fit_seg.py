"""rle_append_size_batch_device_seg and rle_append_fit_batch_device_seg on the GPU: the contract of
the one-wave size and fit entries at the segment edges.  Expected streams come from
oracle.encode(x + new); arenas and comparison: tests/append_fit_gpu.py.  Every test names, through
rle_seg_segment_bytes, the segment length it ran at (hint_for(m) as total_new_bytes)."""
import pytest

import append_fit_gpu as FG
import append_fit_model as F
import append_tail_model as M
import rle_mi355x as R
import rle_oracle as O
from test_gpu_append_fit import refusal_cases
from test_gpu_seg_lengths import TILE, hint_for

pytestmark = pytest.mark.gpu
SB = 4 * TILE   # 4032


def hint4():
    h = hint_for(4)
    assert R.seg_segment_bytes(h) == SB
    return h


def edge_files(form, cap, sb=SB, lengths=None, counts=(1, 5, 9, 0), hint=None):
    f = FG.FitFiles(form, hint if hint is not None else hint4())
    for An in lengths or F.seg_edge_lengths(sb):
        for kind in F.KINDS:
            for r in counts:
                x = F.stored_token(r, 32 + (7 * r) % 16)[0] if r else b""
                f.add(x, F.new_of(kind, An, 0x61, 13 * An + r), cap=cap)
    return f


def test_size_at_the_segment_edges():
    f = edge_files("size_seg", "exact")
    _, _, _, _, need, st = f.check("size_seg, edges")
    assert not st.any()
    assert [int(v) for v in need] == [len(O.encode(x + a)) for x, a in zip(f.x, f.new)]


@pytest.mark.parametrize("cap", ["exact", "short"])
def test_fit_at_the_segment_edges(cap):
    f = edge_files("fit_seg", cap)
    _, _, _, _, need, st = f.check(f"fit_seg, edges, cap {cap}")
    assert (st == (0 if cap == "exact" else F.NOFIT)).all()
    assert [int(v) for v in need] == [len(O.encode(x + a)) for x, a in zip(f.x, f.new)]


def test_one_run_through_three_segments_in_an_exact_slot():
    """The uniform writer (no run boundary in a segment) under an exact capacity, and one byte short."""
    for cap in ("exact", "short"):
        f = FG.FitFiles("fit_seg", hint4())
        for r in (1, 5, 9):
            x = F.stored_token(r, 32 + r)[0]
            f.add(x, b"a" * (3 * SB + 2), cap=cap)
            f.add(x, b"a" * (3 * SB + 2) + b"b", cap=cap)
            f.add(x, b"b" * (3 * SB), cap=cap)
        f.check(f"one run, cap {cap}")


@pytest.mark.parametrize("tiles", [4, 9, 16])
def test_one_segment_length_each(tiles):
    s = tiles * TILE
    hint = hint_for(tiles)
    for form in ("size_seg", "fit_seg"):
        f = edge_files(form, "exact", s, (s - 1, s + 1, 2 * s + 3), (5, 0), hint)
        _, _, _, _, need, st = f.check(f"{form}, {tiles} tiles")
        assert not st.any()
        assert [int(v) for v in need] == [len(O.encode(x + a)) for x, a in zip(f.x, f.new)]


def test_nofit_among_good_files_keeps_the_final_token():
    """Files with e > 0 one byte short between files that fit exactly: the final token and every word
    of the refused files are untouched, the neighbours exact."""
    f = FG.FitFiles("fit_seg", hint4())
    for i, r in enumerate(range(1, 9)):
        x = F.stored_token(r, 40 + i)[0]
        lead = b"a" * (1 + i % (9 - r))
        f.add(x, lead + O.gen(1, i, SB + 5), cap="exact")
        f.add(x, lead + O.gen(2, i, 2 * SB + 3), cap="short")
        f.add(x, b"a" * (SB + 40), cap="short")
        f.add(x, lead + O.gen(2, 50 + i, SB - 1), cap="round16")
    _, _, _, _, _, st = f.check("NOFIT among good files")
    assert [int(v) for v in st] == [0, F.NOFIT, F.NOFIT, 0] * 8


def mixed_files(form, hint):
    f = FG.FitFiles(form, hint)
    rc = refusal_cases()
    for i in range(12):
        x = O.gen(i % 5, 400 + i, (0, 1, 50, 1008, 2500, 16)[i % 6])
        f.add(x, O.gen((i + 1) % 5, 500 + i, (5, 0, 1008, SB - 1, 17, 3000)[i % 6]), cap=("exact", "round16", "slot")[i % 3])
        if i < len(rc):
            xb, nb, kw = rc[i]
            f.add(xb, nb, **kw)
    f.add(F.stored_token(5)[0], F.new_of("runs50", SB + 3, 0x61, 1))       # two segments
    f.add(F.stored_token(9)[0], F.new_of("run", SB + 3, 0x61, 2), cap="short")
    f.add(F.stored_token(2)[0], F.new_of("random", 2 * SB + 3, 0x61, 3))    # three: past the tables below
    return f


def test_forms_agree():
    """append_size_seg == append_size, and append_fit_seg == append_fit word for word, on one mixed
    set with files refused by each status; with tables sized for two segments more than files, the
    last file (three segments behind two files of two) is past them: TOOLARGE, untouched."""
    hint = 2 * SB
    assert R.seg_segment_bytes(hint) == SB
    got = {}
    for form in ("size", "size_seg", "fit", "fit_seg"):
        f = mixed_files(form, hint)
        last = len(f) - 1
        got[form] = f.check(f"mixed, {form}", status={last: M.TOOLARGE} if form.endswith("_seg") else None)
    st = got["fit_seg"][5]
    assert {M.MISALIGNED, M.NOTCANON, M.TOOLARGE, F.NOFIT, 0} == {int(v) for v in st}
    cut = mixed_files("fit", hint).arena().soffs[last]
    for a, b in (("size", "size_seg"), ("fit", "fit_seg")):
        assert (got[a][0][:cut] == got[b][0][:cut]).all()
        for k in range(1, 6):
            assert (got[a][k][:last] == got[b][k][:last]).all(), (a, b, k)
