"""rle_append_batch_device_seg on the GPU: the contract of rle_append_batch_device, byte for byte,
at the segment edges.  Expected bytes come from oracle.encode(x + new) and the one-wave append's
model (append_tail_model.append_carried); the whole poisoned image is compared (nothing below t,
nothing at or past the new length changes), with lengths, decoded lengths, tail words and statuses.
Every test names, through rle_seg_segment_bytes, the segment length it ran at (hint_for(m) as
total_new_bytes).  A few MB and a few launches per test."""
import numpy as np
import pytest
import torch

import append_seg_gpu as SG
import append_tail_gpu as G
import append_tail_model as M
import rle_mi355x as R
import rle_oracle as O
from test_gpu_append_batch import literals, new_of, refusal_cases
from test_gpu_seg_lengths import TILE, hint_for

pytestmark = pytest.mark.gpu
SB = 4 * TILE   # 4032: the segment length of the edge tests
KINDS = ("random", "runs50", "zero", "run")


def hint4():
    h = hint_for(4)
    assert R.seg_segment_bytes(h) == SB
    return h


def stored(c, r, p):
    """(x, y): p alternating literals then c^r, so the final token of count r starts at t = p."""
    x = literals(p) + bytes([c]) * r
    y = O.encode(x)
    assert M.tail_of(y)[:2] == (p, r)
    return x, y


def test_edge_sweep():
    """A around the edges of the first, second and fifth segment, four kinds of new bytes, stored
    final tokens of count 1, 5 and 9 at t mod 16 in {0, 7, 15}, and the same A on empty streams."""
    f, xs = SG.SegFiles(hint4()), []
    sweep = (1, 2, 3, SB - 1, SB, SB + 1, SB + 2, SB + 3, 2 * SB - 1, 2 * SB, 2 * SB + 2, 2 * SB + 3, 5 * SB + 17)
    for A in sweep:
        for k, kind in enumerate(KINDS):
            for r, p in ((1, 32), (5, 39), (9, 47), (1, 47), (5, 32), (9, 39), (1, 39), (5, 47), (9, 32)):
                x, y = stored(0x61, r, p)
                new = new_of(kind, A, 0x61, 13 * A + 7 * p + r)
                f.add(y, new)
                xs.append(x + new)
            new = new_of(kind, A, 0x62, 5 * A + k)
            f.add(b"", new, word=R.RLE_TAIL_EMPTY)
            xs.append(new)
    f.check("edge sweep", want=[O.encode(x) for x in xs])


def test_runs_across_segment_edges():
    """Runs that end one byte before, at and one byte after the first and the second segment edge;
    one run through three segments for every r (the uniform writer on the first and on inner
    segments, entered from the carried state); new bytes equal to c for exactly 9 - r and 9 - r + 1
    bytes; a first new byte other than c; c = '9' (the digit equals the value) and c = 0x00."""
    f, xs = SG.SegFiles(hint4()), []
    n3 = 3 * SB + 2
    cuts = [k * SB + d for k in (1, 2) for d in (-1, 0, 1)]
    for r in range(1, 10):
        for c in (0x61, 0x39, 0x00):
            cb, other = bytes([c]), b"b"
            x, y = stored(c, r, 32 + (r * 5 + c) % 16)
            news = [cb * n3,                              # one run through three segments, continuing c
                    other * n3,                           # ... and starting at the first new byte
                    cb * (9 - r) + O.gen(1, r, 2 * SB),     # the final token filled exactly, then literals
                    cb * (9 - r + 1) + O.gen(1, r, 2 * SB),
                    other + cb * (2 * SB)]
            if c == 0x61:
                news += [(cb * cut + other * n3)[:n3] for cut in cuts]
                news += [(other * cut + b"d" * n3)[:n3] for cut in cuts]
            else:
                news += [(cb * cuts[(r + k) % 6] + other * n3)[:n3] for k in (0, 3)]
            for new in news:
                f.add(y, new)
                xs.append(x + new)
    f.check("runs across edges", want=[O.encode(x) for x in xs])


@pytest.mark.parametrize("m", range(4, 17))
def test_every_segment_length(m):
    """Segments of m tiles: A around one and two segments (-1, 0, +1, +3), random and runs50."""
    hint, S = hint_for(m), m * TILE
    assert R.seg_segment_bytes(hint) == S
    f, xs = SG.SegFiles(hint), []
    for i, A in enumerate((S - 1, S, S + 1, S + 3, 2 * S - 1, 2 * S, 2 * S + 1, 2 * S + 3)):
        for kind in ("random", "runs50"):
            x, y = stored(0x61, 1 + (i + m) % 9, 33 + i)
            new = new_of(kind, A, 0x61, 100 * m + i)
            f.add(y, new)
            xs.append(x + new)
    f.add(b"", new_of("runs50", 2 * S + 3, 0, m), word=R.RLE_TAIL_EMPTY)
    xs.append(f.new[-1])
    f.check(f"{m}-tile segments", want=[O.encode(x) for x in xs])


def equivalence_set(form, n=None):
    f = SG.SegFiles(hint4(), form=form)
    rng = np.random.default_rng(300)
    sizes = [0, 1, 2, 3, SB - 1, SB, SB + 1, SB + 3, 2 * SB, 2 * SB + 2, 3 * SB] + [int(v) for v in rng.integers(0, 3 * SB, 64)]
    for i, A in enumerate(sizes):
        for k, kind in enumerate(KINDS):
            r = 1 + (i + 2 * k) % 9
            _, y = stored(0x61, r, 32 + (7 * i + k) % 16) if (i + k) % 7 else (b"", b"")
            f.add(y, new_of(kind, A, 0x61, 31 * i + k), word=None if y else R.RLE_TAIL_EMPTY)
            if n is not None and len(f) == n:
                return f
    return f


def test_same_results_as_the_one_wave_append():
    """One set of 300 files (A from 0 to 3 segments, all kinds) through rle_append_batch_device and
    through the segmented form: image, len, ulen, tail and status identical.  Also n = 1."""
    a, b = equivalence_set("wave"), equivalence_set("seg")
    assert len(a) == len(b) == 300
    ra, rb = a.check("one-wave form"), b.check("segmented form")
    for va, vb in zip(ra, rb):
        assert np.array_equal(np.asarray(va), np.asarray(vb))
    for A in (2 * SB + 2, 5):
        one = SG.SegFiles(hint4())
        one.add(stored(0x61, 4, 40)[1], new_of("runs50", A, 0x61, A))
        one.check(f"n = 1, A = {A}")


def test_chain_of_appends_alternating_forms():
    """8 files, 6 rounds, the forms alternating per round, tail words carried on the device: at the
    end the streams equal encode(total), a tail scan returns the carried tails and decoded lengths,
    and the decode returns the content."""
    n, rounds, cap = 8, 6, 160 * 1024
    hint = hint4()
    rng = np.random.default_rng(86)
    alpha = np.frombuffer(b"ab9\0", np.uint8)
    soffs = [i * (cap + 32) for i in range(n)]
    d_s = torch.full((n * (cap + 32) + 64,), G.POISON, dtype=torch.uint8, device=G.DEV)
    d_len, d_ulen = G.i64([0] * n), G.i64([0] * n)
    d_tail = G.i64([R.RLE_TAIL_EMPTY] * n)
    d_off, d_cap = G.i64(soffs), G.i64([cap] * n)
    status = torch.full((n,), 0x7777, dtype=torch.int32, device=G.DEV)
    ws = R.append_seg_workspace(n, hint, G.DEV)
    totals = [b""] * n
    for k in range(rounds):
        sizes = [(SB + 1, 2 * SB + 2, 0, 37, 3 * SB - 1, 9, SB, 1)[(i + 3 * k) % 8] for i in range(n)]
        news = [np.repeat(rng.choice(alpha, s), rng.integers(1, 12, s)).tobytes()[:s] for s in sizes]
        noffs, ntotal = R.layout(sizes, pad=32)
        nimg = np.zeros(ntotal + 64, np.uint8)
        for a, o in zip(news, noffs):
            nimg[o:o + len(a)] = np.frombuffer(a, np.uint8)
            if a:
                nimg[o + len(a):o + len(a) + 24] = a[-1]
        assert all(R.append_slot_bytes(len(O.encode(t)), s) <= cap for t, s in zip(totals, sizes))
        args = (d_s, d_off, d_len, d_cap, d_ulen, torch.from_numpy(nimg).to(G.DEV), G.i64(noffs), G.i64(sizes), status)
        if k % 2:
            R.append_batch(*args, tail=d_tail)
        else:
            R.append_batch_seg(*args, total_new_bytes=hint, workspace=ws, tail=d_tail)
        assert int(status.abs().sum().item()) == 0, (k, [hex(v) for v in status.cpu().tolist()])
        totals = [t + a for t, a in zip(totals, news)]
    want = [O.encode(t) for t in totals]
    img, ln = d_s.cpu().numpy(), d_len.cpu().numpy()
    exp = np.full(img.shape, G.POISON, np.uint8)
    for i, w in enumerate(want):
        assert int(ln[i]) == len(w), (i, int(ln[i]), len(w))
        exp[soffs[i]:soffs[i] + len(w)] = np.frombuffer(w, np.uint8)
    diff = np.nonzero(img != exp)[0]
    assert diff.size == 0, (int(diff[0]), int(diff[0]) // (cap + 32), int(diff[0]) % (cap + 32), diff.size)
    assert [int(u) for u in d_ulen.cpu()] == [len(t) for t in totals]
    uoffs, utotal = R.layout([len(t) for t in totals], pad=32)
    d_out = torch.zeros(utotal + 64, dtype=torch.uint8, device=G.DEV)
    dst = torch.full((n,), 0x7777, dtype=torch.int32, device=G.DEV)
    R.decode_batch(d_s, d_off, d_len, d_out, G.i64(uoffs), d_ulen, None, dst)
    tail2, ulen2 = G.i64([1] * n), G.i64([1] * n)
    R.tail_batch(d_s, d_off, d_len, tail2, ulen2, status)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert int(dst.abs().sum().item()) == 0 and int(status.abs().sum().item()) == 0
    for i, t in enumerate(totals):
        assert out[uoffs[i]:uoffs[i] + len(t)].tobytes() == t, i
    assert torch.equal(tail2, d_tail) and torch.equal(ulen2, d_ulen)
    assert [int(w) for w in d_tail.cpu()] == [M.word_of(w) for w in want]


def good_files():
    return [(O.encode(O.gen(i % 5, 70 + i, s)), O.gen((i + 2) % 5, 80 + i, a))
            for i, (s, a) in enumerate(((0, 5), (1, 1), (50, 0), (1008, SB), (2500, 17), (1007, 2 * SB + 2), (16, 16),
                                        (1900, 1), (1024, SB + 3), (9, 9), (3000, 3 * SB)))]


def test_refusals_among_good_files():
    """Every refusal of the one-wave append (test_gpu_append_batch.refusal_cases) at the first, a
    middle and the last index among good files of up to three segments: neighbours exact, the refused
    slot, length, decoded length and tail word untouched."""
    cases, goods = refusal_cases(), good_files()
    n = len(goods)
    at = (0, n // 2, n - 1)
    for k in range(0, len(cases), 3):
        group = cases[k:k + 3]
        for rot in range(3):
            f, refused = SG.SegFiles(hint4()), {}
            where = {at[(j + rot) % 3]: c for j, c in enumerate(group)}
            for i, (y, a) in enumerate(goods):
                if i in where:
                    yb, nb, word, cap, shift, status = where[i]
                    f.add(yb, nb, word=word, cap=cap, shift=shift)
                    refused[i] = status
                else:
                    f.add(y, a)
            f.check(f"refusals {k // 3}, rotation {rot}", refused=refused)


def test_total_new_bytes_too_small_refuses_the_trailing_files():
    """6 files of three segments each with tables sized for 6 segments' bytes (12 segments: the
    bytes' 6 and one per file): the first four fit, the last two get RLE_STATUS_TOOLARGE untouched."""
    total = 6 * SB
    assert R.seg_segment_bytes(total) == SB
    f = SG.SegFiles(total)
    for i in range(6):
        f.add(stored(0x61, 1 + i, 32 + i)[1], new_of("runs50" if i & 1 else "random", 3 * SB, 0x61, 40 + i))
    f.check("short segment tables", refused={4: M.TOOLARGE, 5: M.TOOLARGE})


def test_short_workspace_is_refused_on_the_host():
    """workspace_bytes one below rle_append_seg_workspace_bytes: RLE_E_INVAL, nothing launched -- no
    slot, length, tail word or status word changes (the status words keep their fill)."""
    f = SG.SegFiles(hint4(), short_ws=True)
    for y, a in good_files():
        f.add(y, a)
    f.check("short workspace", refused={i: 0x7777 for i in range(len(f))})


def test_hostile_padding_and_head():
    """New content of every length mod 16 around a segment edge whose padding repeats its last byte
    and whose 16 bytes in front hold c (append_seg_gpu.SegFiles.run): neither is content.  The new
    bytes end in the padding's byte and start with c or another byte, after every r."""
    f, xs = SG.SegFiles(hint4()), []
    for r in range(1, 10):
        x, y = stored(0x61, r, 40 + r)
        for A in (1, 15, 16, 17, SB - 15, SB - 1, SB, SB + 1, SB + 16, SB + 17):
            for first in (b"a", b"k"):
                new = (first * 3 + O.gen(2, A + r, A))[:A - 4] + b"zzzz" if A > 7 else first * A
                f.add(y, new)
                xs.append(x + new)
    f.check("hostile padding", want=[O.encode(x) for x in xs])
