"""rle_append_size_batch_device and rle_append_fit_batch_device on the GPU (one wave per file): the
size query gives len(oracle.encode(x + new)) and writes nothing else; the fit append works in a slot
of exactly that many bytes with another file's bytes right behind it, refuses a slot one byte short
before it has touched anything (the final token included), and with worst-case slots is the plain
append word for word.  Arenas: tests/append_fit_gpu.py (packed by the given capacity, poisoned, the
whole image compared after every launch).  A few launches per test."""
import numpy as np
import pytest
import torch

import append_fit_gpu as FG
import append_fit_model as F
import append_tail_model as M
import rle_mi355x as R
import rle_oracle as O

pytestmark = pytest.mark.gpu


def test_size_query_on_the_splice_grid():
    f = FG.FitFiles("size")
    for x, _, new in F.splice_grid():
        f.add(x, new)
    _, _, _, _, need, st = f.check("size, splice grid")
    assert [int(v) for v in need] == [len(O.encode(x + a)) for x, a in zip(f.x, f.new)]
    assert not st.any()


def test_size_query_on_the_a_sweep():
    f = FG.FitFiles("size")
    for x, _, new in F.a_sweep():
        f.add(x, new, cap="round16")
    _, _, _, _, need, st = f.check("size, A sweep")
    assert [int(v) for v in need] == [len(O.encode(x + a)) for x, a in zip(f.x, f.new)]
    assert not st.any()


def exact_fit_files(form="fit", hint=None):
    """Results of every length mod 16 (the literal prefix varies), four capacities, packed slots."""
    f = FG.FitFiles(form, hint)
    shapes = (("random", 17), ("runs50", 1009), ("zero", 2016), ("run", 1025), ("runs50", 3029), ("random", 1))
    for p in range(16):
        for k, cap in enumerate(("exact", "plus1", "round16", "slot")):
            for j, (kind, An) in enumerate(shapes):
                x = F.literals(32 + p) + b"a" * (1 + (k + j) % 9)   # C' = p + a constant of (k, j)
                f.add(x, F.new_of(kind, An, 0x61, 7 * k + j), cap=cap)
    return f


def test_exact_fit():
    """cap in {C', C' + 1, C' rounded up to 16, rle_append_slot_bytes}: the last takes the branch
    that skips the size walk.  A neighbour's bytes or poison start right at cap."""
    f = exact_fit_files()
    _, ln, _, _, need, st = f.check("exact fit")
    assert not st.any() and (ln == need).all()
    for k in range(4):   # every residue of C' mod 16 under every kind of capacity
        assert {int(ln[i]) % 16 for i in range(len(f)) if (i // 6) % 4 == k} == set(range(16)), k
    # empty streams, and the whole A sweep, in exact slots
    f = FG.FitFiles("fit")
    for x, _, new in F.a_sweep():
        f.add(x, new)
    f.check("exact fit, A sweep")


def short_files(form="fit", hint=None):
    f = FG.FitFiles(form, hint)
    for r in range(1, 9):   # e > 0: the new bytes continue c, and a premature rewrite of the token shows
        for lead in (1, 9 - r, 9 - r + 1, 20):
            for tail in (b"", b"k", b"kkk"):
                f.add(F.literals(33 + r) + b"a" * r, b"a" * lead + tail, cap="short")
    for An in (1, 16, 1008, 1009, 3029):
        for kind in F.KINDS:
            f.add(F.literals(47) + b"aaa", F.new_of(kind, An, 0x61, An), cap="short")
            f.add(b"", F.new_of(kind, An, 0x62, An + 1), cap="short")
    return f


def test_one_byte_short():
    """cap = C' - 1: NOFIT, d_need = C', everything untouched; r = 1 files grow the token from one
    byte to three."""
    f = short_files()
    assert any(M.tail_of(y)[1] == 1 and a[:1] == b"a" for y, a in zip(f.y, f.new))
    img, ln, _, _, need, st = f.check("one byte short")
    assert (st == F.NOFIT).all()
    assert [int(v) for v in need] == [len(O.encode(x + a)) for x, a in zip(f.x, f.new)]


def refusal_cases():
    """(x, new, add() arguments): NOFIT, NOTCANON and the two address refusals."""
    x1, x3 = F.literals(40) + b"k", F.literals(1100) + b"ccccc"
    new, cont = O.gen(2, 5, 700), b"ccc" + O.gen(1, 6, 50)
    return [
        (x3, cont, dict(cap="short")),                           # NOFIT with e > 0
        (x1, new, dict(word=M.tail_word(39, 1), cap="slot")),    # NOTCANON: t off by one
        (x1, new, dict(shift=5, cap="slot")),                    # new content misaligned
        (x3, new, dict(cap=0)),                                  # NOFIT, no room at all
        (x3, new, dict(word=M.tail_word(1100, 4))),              # NOTCANON: a wrong r, exact cap
        (x3, new, dict(sshift=8)),                               # the stream misaligned
    ]


def goods():
    return [(O.gen(i % 5, 70 + i, s), O.gen((i + 2) % 5, 80 + i, a))
            for i, (s, a) in enumerate(((0, 5), (1, 1), (50, 0), (1008, 1008), (2500, 17), (1007, 2017), (16, 16),
                                        (1900, 1), (1024, 3000), (9, 9), (3000, 40)))]


@pytest.mark.parametrize("form", ["fit", "size"])
def test_refusals_among_good_files(form):
    """Each refusal at the first, a middle and the last index among files in exact slots."""
    cases, good = refusal_cases(), goods()
    n = len(good)
    at = (0, n // 2, n - 1)
    for k in range(0, len(cases), 3):
        for rot in range(3):
            f = FG.FitFiles(form)
            where = {at[(j + rot) % 3]: c for j, c in enumerate(cases[k:k + 3])}
            for i, (x, a) in enumerate(good):
                if i in where:
                    xb, nb, kw = where[i]
                    f.add(xb, nb, **kw)
                else:
                    f.add(x, a)
            _, _, _, _, need, st = f.check(f"{form}: refusals {k // 3}, rotation {rot}")
            for i in range(n):   # (check has compared every word with the model)
                hard = i in where and bool({"word", "shift", "sshift"} & set(where[i][2]))
                assert (st[i] != 0) == (hard or (i in where and form == "fit")), (form, k, rot, i, hex(st[i]))
                assert (need[i] == 0) == hard, (form, k, rot, i, int(need[i]))


def test_nothing_to_append_needs_no_room():
    f = FG.FitFiles("fit")
    f.add(F.literals(50) + b"aaa", b"", cap=0)
    f.add(b"", b"", cap=0)
    f.add(F.literals(7), b"q")
    _, _, _, _, need, st = f.check("A == 0, cap 0")
    assert not st.any() and [int(v) for v in need] == [len(f.y[0]), 0, 8]


def test_worst_case_caps_equal_the_plain_append():
    f = FG.FitFiles("fit")
    for x, _, new in F.a_sweep((1, 17, 1008, 1025, 3029)):
        f.add(x, new, cap="slot")
    for x, new, kw in refusal_cases()[1:3]:
        f.add(x, new, **kw)
    a, b = f.arena(), f.arena()
    a.launch("fit")
    b.launch("plain")
    ga, gb = a.fetch(), b.fetch()
    f.compare("fit, worst-case caps", a, ga, f.expected(a, "fit"))
    for k in (0, 1, 2, 3, 5):   # image, len, ulen, tail, status
        assert (ga[k] == gb[k]).all(), k


def test_chain_of_sized_appends():
    """64 files, 12 rounds: size, a new arena packed at d_need rounded up to 16 with the streams moved
    on the device, then fit with cap = d_need.  Tails carried on the device throughout."""
    n, rounds = 64, 12
    rng = np.random.default_rng(65)
    alpha = np.frombuffer(b"ab9\0", np.uint8)
    d_s = torch.full((64,), FG.POISON, dtype=torch.uint8, device=FG.DEV)
    d_off, d_len, d_ulen = FG.i64([0] * n), FG.i64([0] * n), FG.i64([0] * n)
    d_tail = FG.i64([R.RLE_TAIL_EMPTY] * n)
    need = torch.zeros(n, dtype=torch.int64, device=FG.DEV)
    need2 = torch.zeros(n, dtype=torch.int64, device=FG.DEV)
    status = torch.full((n,), 0x7777, dtype=torch.int32, device=FG.DEV)
    totals, offs = [b""] * n, [0] * n
    for k in range(rounds):
        sizes = [1100 if k == i % rounds else (i + 7 * k) % 41 for i in range(n)]
        news = [np.repeat(rng.choice(alpha, s), rng.integers(1, 12, s)).tobytes()[:s] for s in sizes]
        noffs, ntotal = R.layout(sizes, pad=32)
        nimg = np.zeros(ntotal + 64, np.uint8)
        for a, o in zip(news, noffs):
            nimg[o:o + len(a)] = np.frombuffer(a, np.uint8)
            if a:
                nimg[o + len(a):o + len(a) + 24] = a[-1]
        d_n, d_noff, d_nlen = torch.from_numpy(nimg).to(FG.DEV), FG.i64(noffs), FG.i64(sizes)
        R.append_size(d_s, d_off, d_len, d_tail, d_n, d_noff, d_nlen, need, status)
        nd, old = [int(v) for v in need.cpu()], [int(v) for v in d_len.cpu()]
        assert int(status.abs().sum().item()) == 0, k
        totals = [t + a for t, a in zip(totals, news)]
        assert nd == [len(O.encode(t)) for t in totals], k
        new_offs, pos = [], 0
        for c in nd:
            new_offs.append(pos)
            pos = FG.r16(pos + c)
        d_s2 = torch.full((pos + 64,), FG.POISON, dtype=torch.uint8, device=FG.DEV)
        for o1, o2, c in zip(offs, new_offs, old):
            if c:
                d_s2[o2:o2 + c] = d_s[o1:o1 + c]   # a device copy
        d_s, offs, d_off = d_s2, new_offs, FG.i64(new_offs)
        got = R.append_fit(d_s, d_off, d_len, need, d_ulen, d_n, d_noff, d_nlen, need2, status, tail=d_tail)
        assert got is d_tail
        assert int(status.abs().sum().item()) == 0, (k, [hex(v) for v in status.cpu().tolist()])
        assert torch.equal(need, need2) and torch.equal(need, d_len)
    want = [O.encode(t) for t in totals]
    img = d_s.cpu().numpy()
    exp = np.full(img.shape, FG.POISON, np.uint8)
    for i, w in enumerate(want):
        exp[offs[i]:offs[i] + len(w)] = np.frombuffer(w, np.uint8)
    assert (img == exp).all()
    assert [int(u) for u in d_ulen.cpu()] == [len(t) for t in totals]
    uoffs, utotal = R.layout([len(t) for t in totals], pad=32)
    d_out = torch.zeros(utotal + 64, dtype=torch.uint8, device=FG.DEV)
    dst = torch.full((n,), 0x7777, dtype=torch.int32, device=FG.DEV)
    R.decode_batch(d_s, d_off, d_len, d_out, FG.i64(uoffs), d_ulen, None, dst)
    tail2, ulen2 = FG.i64([1] * n), FG.i64([1] * n)
    R.tail_batch(d_s, d_off, d_len, tail2, ulen2, status)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert int(dst.abs().sum().item()) == 0 and int(status.abs().sum().item()) == 0
    for i, t in enumerate(totals):
        assert out[uoffs[i]:uoffs[i] + len(t)].tobytes() == t, i
    assert torch.equal(tail2, d_tail) and torch.equal(ulen2, d_ulen)


@pytest.mark.parametrize("form", ["fit", "size"])
def test_batch_sizes(form):
    """n = 1 and n = 4097, exact slots, every third file one byte short."""
    f = FG.FitFiles(form)
    f.add(O.gen(2, 3, 3000), O.gen(2, 4, 1500))
    f.check(f"{form}: n = 1")
    f = FG.FitFiles(form)
    for i in range(4097):
        f.add(O.gen(i % 5, 200 + i, i % 37), O.gen((i + 1) % 5, 300 + i, (i * 7) % 29),
              cap="short" if i % 3 == 2 else "exact")
    _, _, _, _, _, st = f.check(f"{form}: n = 4097")
    if form == "fit":
        assert {int(v) for v in st} == {0, F.NOFIT}
