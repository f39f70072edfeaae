"""rle_tail_batch_device on the GPU against the documented parse (tests/append_tail_model.py tail_of):
status, tail word and decoded length of every stream, through the C ABI, a few launches per test."""
import numpy as np
import pytest

import append_tail_gpu as G
import append_tail_model as M
import rle_mi355x as R
import rle_oracle as O

pytestmark = pytest.mark.gpu
TILE = 1008
BAD_DIGITS = (b"1", b"0", b":", b"\x00", b"\xb2")


def check(streams, label, **kw):
    st, tl, ul = G.scan(streams, **kw)
    for i, s in enumerate(streams):
        want = G.scan_expected(s)
        got = (int(st[i]), int(tl[i]), int(ul[i]))
        assert got == want, (label, i, len(s), [hex(v) for v in got], [hex(v) for v in want], s[:24], s[-24:])
    return st, tl, ul


def literals(n, a=b"x", b=b"y"):
    return (a + b) * (n // 2) + (a if n & 1 else b"")


def pairs_body(n):
    """n stream bytes: n % 3 literals, then pair tokens "pp2", "qq3" alternating."""
    k = n % 3
    toks = [b"pp2", b"qq3"]
    return literals(k, b"m", b"n") + b"".join(toks[i & 1] for i in range((n - k) // 3))


def test_golden_vectors(vectors):
    streams = [bytes.fromhex(v["out"]) for grp in ("kat", "edge", "ladder", "fuzz") for v in vectors[grp]]
    ins = [bytes.fromhex(v["in"]) for grp in ("kat", "edge", "ladder", "fuzz") for v in vectors[grp]]
    st, tl, ul = check(streams, "golden vectors")
    assert (st == 0).all() and [int(u) for u in ul] == [len(x) for x in ins]


def test_final_token_at_every_offset():
    """The final token at t in 0..48, across the first tile edge (1005..1026) and the second
    (2013..2020), one byte and three bytes long, after alternating literals and after pair tokens
    whose three bytes fall on either side of 1007/1008 and 1023/1024."""
    streams, want_t = [], []
    for t in list(range(0, 49)) + list(range(1005, 1027)) + list(range(2013, 2021)):
        for body in (literals(t), pairs_body(t)):
            for final in (b"Q", b"QQ5"):
                streams.append(body + final)
                want_t.append((t, 1 if len(final) == 1 else 5))
    st, tl, ul = check(streams, "final token offsets")
    assert [(R.tail_offset(w), R.tail_count(w)) for w in tl] == want_t
    assert (st == 0).all()


def test_digit_valued_data():
    rng = np.random.default_rng(5)
    digits = np.frombuffer(b"0123456789", np.uint8)
    xs = []
    for n in (1, 2, 3, 17, 100, 700, 1100, 2500):
        xs.append(rng.choice(digits, n).tobytes())
        xs.append(np.repeat(rng.choice(digits, n), rng.integers(1, 12, n)).tobytes())
    for L in range(1, 31):
        xs += [b"9" * L, b"2" * L, b"k" + b"9" * L, b"2" * L + b"9"]
    xs += [b"1", b"0", b"10", b"01" * 40, b"a1", b"a0", b"110", b"001", b"1" * 11, b"0" * 10 + b"1"]
    streams = [O.encode(x) for x in xs]
    st, tl, ul = check(streams, "digit data")
    assert (st == 0).all() and [int(u) for u in ul] == [len(x) for x in xs]


def test_zero_bytes():
    """A trailing literal 0x00 (it equals the zero the tiles read past C: still a one-byte token) and
    all-zero content."""
    xs = [b"a\0", b"\0", b"abc" * 5 + b"\0", literals(15) + b"\0", literals(1007) + b"\0", literals(1023) + b"\0",
          b"\0a\0", b"zz\0"]
    xs += [bytes(L) for L in (1, 2, 8, 9, 10, 11, 18, 19, 1000, 3024, 3025, 4096, 9000)]
    streams = [O.encode(x) for x in xs]
    assert streams[0] == b"a\0"
    st, tl, ul = check(streams, "zero bytes")
    assert (st == 0).all() and [int(u) for u in ul] == [len(x) for x in xs]
    assert int(tl[0]) == M.tail_word(1, 1)


def test_padding_is_not_part_of_the_stream():
    """Arena bytes behind a stream that would continue its last token (an equal byte and a digit):
    ignored, both where C is a multiple of 16 and where the padding shares the stream's last
    16-byte chunk."""
    streams, padding = [], {}
    for C in (16, 32, 1008, 1024, 2016, 5, 21, 1007, 1009, 1023, 1025):
        for final in (b"Q", b"QQ7"):
            s = literals(C - len(final)) + final
            assert len(s) == C
            padding[len(streams)] = (b"Q7" if len(final) == 1 else b"7Q") + b"QQ9" * 8
            streams.append(s)
    st, tl, ul = check(streams, "hostile padding", padding=padding)
    assert (st == 0).all()


def good_batch():
    return [O.encode(O.gen(i % 5, 40 + i, s)) for i, s in
            enumerate((1, 50, 1008, 2500, 1007, 3024, 16, 1900, 1024, 2017, 0, 3000, 1300, 2048))]


def notcanon_streams():
    """Every NOTCANON class in the first and in the last tile of a three-tile stream (the cut after
    "v v" is the stream's end by definition: once three tiles long, once alone)."""
    out = []
    for d in BAD_DIGITS:
        out.append(literals(100) + b"aa" + d + literals(2400))      # first tile
        out.append(literals(2400) + b"aa" + d + literals(7))        # last tile
        out.append(literals(2500) + b"aa" + d)                      # ... as the final token
    out.append(literals(2500) + b"aa")
    out.append(b"aa")
    out.append(literals(1007) + b"aa")      # the pair straddles the tile edge
    for s in out:
        assert M.tail_of(s) is None
    return out


def test_refusals_among_good_streams():
    """NOTCANON streams, a misaligned offset and an oversized length at the first, a middle and the
    last index of a batch of good streams (the oversized buffer is never read)."""
    good = good_batch()
    n = len(good)
    bad = [("notcanon", s) for s in notcanon_streams()] + [("shift", None), ("huge", None)] * 2
    at = (0, n // 2, n - 1)
    k = 0
    while k < len(bad):
        for rot in range(3):   # every refusal visits all three places
            streams, shift, length, want = list(good), {}, {}, {}
            for j, (kind, s) in enumerate(bad[k:k + 3]):
                i = at[(j + rot) % 3]
                if kind == "notcanon":
                    streams[i] = s
                    want[i] = (M.NOTCANON, 0, 0)
                elif kind == "shift":
                    streams[i] = good[3]
                    shift[i] = 3
                    want[i] = (M.MISALIGNED, 0, 0)
                else:
                    length[i] = M.MAX_BUFFER_BYTES + 1
                    want[i] = (M.TOOLARGE, 0, 0)
            st, tl, ul = G.scan(streams, shift=shift, length=length)
            for i, s in enumerate(streams):
                exp = want.get(i, G.scan_expected(s))
                assert (int(st[i]), int(tl[i]), int(ul[i])) == exp, (k, rot, i, hex(int(st[i])), hex(int(tl[i])))
        k += 3


def test_every_refusal_kind_at_every_place():
    """One launch per place: a NOTCANON stream, a misaligned one and an oversized one rotate through
    the first, the middle and the last index."""
    good = good_batch()
    n = len(good)
    at = (0, n // 2, n - 1)
    nc = literals(1100) + b"aa:" + literals(900)
    for rot in range(3):
        streams, shift, length, want = list(good), {}, {}, {}
        i0, i1, i2 = (at[(j + rot) % 3] for j in range(3))
        streams[i0] = nc
        want[i0] = (M.NOTCANON, 0, 0)
        streams[i1] = good[5]
        shift[i1] = 8
        want[i1] = (M.MISALIGNED, 0, 0)
        length[i2] = 0xFFFFFFFFFF
        want[i2] = (M.TOOLARGE, 0, 0)
        st, tl, ul = G.scan(streams, shift=shift, length=length)
        for i, s in enumerate(streams):
            exp = want.get(i, G.scan_expected(s))
            assert (int(st[i]), int(tl[i]), int(ul[i])) == exp, (rot, i, hex(int(st[i])), hex(int(tl[i])))


def test_batch_sizes():
    one = [O.encode(O.gen(2, 9, 2600))]
    check(one, "n = 1")
    many = [O.encode(O.gen(i % 5, 100 + i, i % 41)) for i in range(4097)]
    many[4096] = O.encode(O.gen(2, 1, 1500))
    many[77] = b"kk"   # one refusal inside the large batch
    st, tl, ul = check(many, "n = 4097")
    assert st[77] == M.NOTCANON and int(st.sum()) == M.NOTCANON
