"""rle_append_batch_device on the GPU: every accepted append equals oracle.encode(x + new) in a
poisoned slot (whole image compared: nothing below t, nothing at or past the new length changes),
lengths, decoded lengths and tail words follow, and refused files come back untouched.  Through the
C ABI, a few launches per test."""
import numpy as np
import pytest
import torch

import append_tail_gpu as G
import append_tail_model as M
import rle_mi355x as R
import rle_oracle as O

pytestmark = pytest.mark.gpu
A_SWEEP = (1, 15, 16, 17, 1007, 1008, 1009, 1023, 1024, 1025, 2016, 3029)


def literals(n, a=b"x", b=b"y"):
    return (a + b) * (n // 2) + (a if n & 1 else b"")


def new_of(kind, A, c, seed):
    if kind == "random":
        return O.gen(1, seed, A)
    if kind == "runs50":
        return O.gen(2, seed, A)
    if kind == "zero":
        return bytes(A)
    return bytes([c]) * A   # "run": continues the old final run across tiles


def test_splice_grid():
    """x = p alternating literals ‖ c^L: every t mod 16 (p in 0..15 and 2000..2015), every final
    count r with and without full 9-chunks before it, bytes 'a', '9' and 0x00, and new bytes that
    leave the run, continue it short of 9, to 9, past 9 and far past it."""
    f, xs = G.Files(), []
    for p in list(range(16)) + list(range(2000, 2016)):
        for r in range(1, 10):
            for L in (r, 9 + r):
                for c in (0x61, 0x39, 0x00):
                    cb = bytes([c])
                    x = literals(p) + cb * L
                    y = O.encode(x)
                    assert M.tail_of(y)[:2] == (len(y) - (1 if r == 1 else 3), r)
                    for new in (b"", cb, cb * (9 - r), cb * (9 - r + 1), cb * 17, b"k", cb * 3 + b"77"):
                        f.add(y, new)
                        xs.append(x + new)
    want = [O.encode(x) for x in xs]
    for i, w in enumerate(want):
        assert M.append_expected(f.y[i], f.new[i]) == w
    f.check("splice grid", want=want)


def test_new_length_sweep():
    """A across the tile sizes, four kinds of new bytes, t mod 16 in {0, 7, 15}, after a final token
    "aa3"; and the same lengths appended to empty streams."""
    f, xs = G.Files(), []
    for A in A_SWEEP:
        for kind in ("random", "runs50", "zero", "run"):
            for p in (32, 39, 47):
                x = literals(p) + b"aaa"
                y = O.encode(x)
                assert M.tail_of(y)[:2] == (p, 3)
                new = new_of(kind, A, 0x61, 11 * A + p)
                f.add(y, new)
                xs.append(x + new)
            # after a final 0x00 literal too, so that "zero" continues the old run
            x = literals(47) + b"\0"
            f.add(O.encode(x), new_of(kind, A, 0, A))
            xs.append(x + f.new[-1])
    for A in A_SWEEP:
        for kind in ("random", "runs50", "zero", "run"):
            new = new_of(kind, A, 0x62, 7 * A)
            f.add(b"", new, word=R.RLE_TAIL_EMPTY)
            xs.append(new)
    f.add(b"", b"", word=R.RLE_TAIL_EMPTY)
    xs.append(b"")
    f.check("A sweep", want=[O.encode(x) for x in xs])


def test_chain_of_appends():
    """64 files, 24 rounds, tails carried on the device from round to round and never re-scanned."""
    n, rounds, cap = 64, 24, 8192
    rng = np.random.default_rng(64)
    alpha = np.frombuffer(b"ab9\0", np.uint8)
    soffs = [i * (cap + 32) for i in range(n)]
    d_s = torch.full((n * (cap + 32) + 64,), G.POISON, dtype=torch.uint8, device=G.DEV)
    d_len, d_ulen = G.i64([0] * n), G.i64([0] * n)
    d_tail = G.i64([R.RLE_TAIL_EMPTY] * n)
    d_off, d_cap = G.i64(soffs), G.i64([cap] * n)
    status = torch.full((n,), 0x7777, dtype=torch.int32, device=G.DEV)
    totals = [b""] * n
    for k in range(rounds):
        sizes = [1100 if k == i % rounds else (i + 7 * k) % 41 for i in range(n)]
        news = [np.repeat(rng.choice(alpha, s), rng.integers(1, 12, s)).tobytes()[:s] for s in sizes]
        assert [len(a) for a in news] == sizes
        noffs, ntotal = R.layout(sizes, pad=32)
        nimg = np.zeros(ntotal + 64, np.uint8)
        for a, o in zip(news, noffs):
            nimg[o:o + len(a)] = np.frombuffer(a, np.uint8)
            if a:
                nimg[o + len(a):o + len(a) + 24] = a[-1]
        assert all(R.append_slot_bytes(len(O.encode(t)), s) <= cap for t, s in zip(totals, sizes))
        got = R.append_batch(d_s, d_off, d_len, d_cap, d_ulen, torch.from_numpy(nimg).to(G.DEV), G.i64(noffs),
                             G.i64(sizes), status, tail=d_tail)
        assert got is d_tail
        assert int(status.abs().sum().item()) == 0, (k, [hex(v) for v in status.cpu().tolist()])
        totals = [t + a for t, a in zip(totals, news)]
    torch.cuda.synchronize()
    assert int(status.abs().sum().item()) == 0
    want = [O.encode(t) for t in totals]
    img, ln = d_s.cpu().numpy(), d_len.cpu().numpy()
    exp = np.full(img.shape, G.POISON, np.uint8)
    for i, w in enumerate(want):
        assert int(ln[i]) == len(w), (i, int(ln[i]), len(w))
        exp[soffs[i]:soffs[i] + len(w)] = np.frombuffer(w, np.uint8)
    diff = np.nonzero(img != exp)[0]
    assert diff.size == 0, (int(diff[0]), int(diff[0]) // (cap + 32), int(diff[0]) % (cap + 32), diff.size)
    assert [int(u) for u in d_ulen.cpu()] == [len(t) for t in totals]
    # the decode gives the content back
    uoffs, utotal = R.layout([len(t) for t in totals], pad=32)
    d_out = torch.zeros(utotal + 64, dtype=torch.uint8, device=G.DEV)
    dst = torch.full((n,), 0x7777, dtype=torch.int32, device=G.DEV)
    R.decode_batch(d_s, d_off, d_len, d_out, G.i64(uoffs), d_ulen, None, dst)
    # ... and a scan of the final streams returns the carried tails and decoded lengths
    tail2, ulen2 = G.i64([1] * n), G.i64([1] * n)
    R.tail_batch(d_s, d_off, d_len, tail2, ulen2, status)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert int(dst.abs().sum().item()) == 0 and int(status.abs().sum().item()) == 0
    for i, t in enumerate(totals):
        assert out[uoffs[i]:uoffs[i] + len(t)].tobytes() == t, i
    assert torch.equal(tail2, d_tail) and torch.equal(ulen2, d_ulen)
    assert [int(w) for w in d_tail.cpu()] == [M.word_of(w) for w in want]


def test_fresh_scan_when_no_tail_is_given():
    """append_batch(tail=None) scans first and returns the new tails."""
    xs = [O.gen(i % 5, 900 + i, s) for i, s in enumerate((0, 1, 9, 10, 1008, 2500, 4096, 33))]
    news = [O.gen((i + 1) % 5, 950 + i, s) for i, s in enumerate((5, 0, 40, 1100, 3, 1008, 17, 2017))]
    ys = [O.encode(x) for x in xs]
    need = [R.append_slot_bytes(len(y), len(a)) for y, a in zip(ys, news)]
    soffs, stotal = R.layout(need, pad=32)
    img = np.full(stotal, G.POISON, np.uint8)
    for y, o in zip(ys, soffs):
        img[o:o + len(y)] = np.frombuffer(y, np.uint8)
    noffs, ntotal = R.layout([len(a) for a in news], pad=32)
    nimg = np.zeros(ntotal, np.uint8)
    for a, o in zip(news, noffs):
        nimg[o:o + len(a)] = np.frombuffer(a, np.uint8)
    d_s, d_len = torch.from_numpy(img.copy()).to(G.DEV), G.i64([len(y) for y in ys])
    status = torch.full((len(xs),), 0x7777, dtype=torch.int32, device=G.DEV)
    tail = R.append_batch(d_s, G.i64(soffs), d_len, G.i64(need), None, torch.from_numpy(nimg).to(G.DEV), G.i64(noffs),
                          G.i64([len(a) for a in news]), status)
    torch.cuda.synchronize()
    assert int(status.abs().sum().item()) == 0
    got = d_s.cpu().numpy()
    for i, (x, a) in enumerate(zip(xs, news)):
        w = O.encode(x + a)
        assert int(d_len[i]) == len(w) and got[soffs[i]:soffs[i] + len(w)].tobytes() == w, i
        assert int(tail[i]) == (M.word_of(w) if w else 0), i
        img[soffs[i]:soffs[i] + len(w)] = np.frombuffer(w, np.uint8)
    assert (got == img).all()


def test_hand_made_stream_keeps_its_prefix():
    """The documented divergence from a whole re-encode (include/rle_mi355x.h): "aa2aa2" passes the
    scan although the encoder would emit "aa4" for its content; appending "a" rewrites only the final
    token, giving "aa2" ‖ encode("aaa") = "aa2aa3", where decode, append, re-encode gives "aa5"."""
    assert G.scan_expected(b"aa2aa2") == (0, M.tail_word(3, 2), 4)
    st, tl, ul = G.scan([b"aa2aa2"])
    assert (int(st[0]), int(tl[0]), int(ul[0])) == (0, M.tail_word(3, 2), 4)
    f = G.Files()
    f.add(b"aa2aa2", b"a", word=int(tl[0]))
    f.check("contract pin", want=[b"aa2" + O.encode(b"aaa")])
    assert b"aa2" + O.encode(b"aaa") == b"aa2aa3" and O.encode(b"aaaaa") == b"aa5"


def refusal_cases():
    """(stream, new, tail word given, capacity given, new-offset shift, status)"""
    y1 = O.encode(literals(40) + b"k")            # final token: one byte at 40
    y3 = O.encode(literals(1100) + b"ccccc")      # final token: "cc5" at 1100
    new = O.gen(2, 5, 700)
    return [
        (y3, new, None, R.append_slot_bytes(len(y3), len(new)) - 1, 0, M.MISALIGNED),     # cap one byte short
        (y1, new, None, None, 5, M.MISALIGNED),                                            # new content misaligned
        (y1, new, M.tail_word(39, 1), None, 0, M.NOTCANON),                                # t off by one
        (y3, new, M.tail_word(1100, 4), None, 0, M.NOTCANON),                              # a wrong r
        (y3, new, R.RLE_TAIL_EMPTY, None, 0, M.NOTCANON),                                  # EMPTY for a non-empty stream
        (y3, new, M.tail_word(1101, 5), None, 0, M.NOTCANON),                              # t off by one, 3-byte token
        (y1, new, M.tail_word(40, 2), None, 0, M.NOTCANON),                                # a wrong r, 1-byte token
        (b"", new, M.tail_word(0, 1), None, 0, M.NOTCANON),                                # a tail for an empty stream
        (y1, b"", M.tail_word(40, 1) | (1 << 36), None, 0, M.NOTCANON),                    # stray bits, A = 0
    ]


def test_refusals_among_good_files():
    """Each refusal at the first, a middle and the last index among good files: neighbours exact, the
    refused slot, length, decoded length and tail word untouched."""
    cases = refusal_cases()
    goods = [(O.encode(O.gen(i % 5, 70 + i, s)), O.gen((i + 2) % 5, 80 + i, a))
             for i, (s, a) in enumerate(((0, 5), (1, 1), (50, 0), (1008, 1008), (2500, 17), (1007, 2017), (16, 16),
                                         (1900, 1), (1024, 3000), (9, 9), (3000, 40)))]
    n = len(goods)
    at = (0, n // 2, n - 1)
    for k in range(0, len(cases), 3):
        group = cases[k:k + 3]
        for rot in range(3):
            f, refused = G.Files(), {}
            where = {at[(j + rot) % 3]: c for j, c in enumerate(group)}
            for i, (y, a) in enumerate(goods):
                if i in where:
                    yb, nb, word, cap, shift, status = where[i]
                    f.add(yb, nb, word=word, cap=cap, shift=shift)
                    refused[i] = status
                else:
                    f.add(y, a)
            f.check(f"refusals {k // 3}, rotation {rot}", refused=refused)


def test_batch_sizes():
    """n = 1 and n = 4097 (more files than one residency round; small files)."""
    f = G.Files()
    f.add(O.encode(O.gen(2, 3, 3000)), O.gen(2, 4, 1500))
    f.check("n = 1")
    f = G.Files()
    for i in range(4097):
        x = O.gen(i % 5, 200 + i, i % 37)
        f.add(O.encode(x), O.gen((i + 1) % 5, 300 + i, (i * 7) % 29))
    f.check("n = 4097")
