"""CPU check of the segmented tail scan's algebra (tests/tail_seg_model.py: per-segment summaries for
the three entry phases, phase composition, the 64-bit sum, the last segment's last token start, the
closing rule, the segment-table refusal) against the documented parse (append_tail_model.tail_of),
for segment lengths 3..40 bytes.  No GPU."""
import numpy as np

import append_tail_model as M
import rle_oracle as O
import tail_seg_model as T
from append_seg_model import seg_count, seg_cut

SEG_LENGTHS = range(3, 41)
BAD_DIGITS = (b"1", b"0", b":", b"\x00", b"\xb2")   # test_gpu_tail_scan.BAD_DIGITS


def expected(y):
    tl = M.tail_of(bytes(y))
    if tl is None:
        return M.NOTCANON, 0, 0
    return 0, M.tail_word(tl[0], tl[1]), tl[2]


def check(y, sb, label):
    got = T.tail_seg(y, sb)
    assert got == expected(y), (label, sb, len(y), got, expected(y), y[:48])
    if got[0] == 0 and y:
        # the cut's guarantee: the final token starts in the last segment
        assert (got[1] & 0xFFFFFFFF) >= seg_cut(len(y), sb)[-1][0], (label, sb, len(y))
    return got


def literals(n, a=b"x", b=b"y"):
    return (a + b) * (n // 2) + (a if n & 1 else b"")


def test_last_segment_holds_the_final_token():
    """seg_count lets the last segment absorb a remainder of 1-2 bytes, so with more than one segment
    the last is at least 3 bytes long and a final token of 1 or 3 bytes starts inside it."""
    for sb in SEG_LENGTHS:
        for n in range(1, 5 * sb + 4):
            cut = seg_cut(n, sb)
            assert len(cut) == seg_count(n, sb) and cut[-1][1] == n
            if len(cut) > 1:
                assert cut[-1][1] - cut[-1][0] >= 3
                assert n - 3 >= cut[-1][0]
            assert n - 1 >= cut[-1][0]


def test_golden_vectors(vectors):
    streams = [bytes.fromhex(v["out"]) for grp in ("kat", "edge", "ladder", "fuzz") for v in vectors[grp]]
    for sb in SEG_LENGTHS:
        for y in streams:
            assert check(y, sb, "golden")[0] == 0


def test_every_kind_at_lengths_0_to_200():
    streams = [(O.encode(O.gen(kind, 3 * n + kind, n)), n) for kind in range(5) for n in range(201)]
    for sb in SEG_LENGTHS:
        for y, n in streams:
            st, _, ul = check(y, sb, "kinds")
            assert st == 0 and ul == n


def test_digit_valued_data():
    """test_gpu_tail_scan.test_digit_valued_data's generators: streams whose data bytes are count
    digits, where the entry phases of a segment stay apart longest."""
    rng = np.random.default_rng(5)
    digits = np.frombuffer(b"0123456789", np.uint8)
    xs = []
    for n in (1, 2, 3, 17, 100, 250):
        xs.append(rng.choice(digits, n).tobytes())
        xs.append(np.repeat(rng.choice(digits, n), rng.integers(1, 12, n)).tobytes())
    for L in range(1, 31):
        xs += [b"9" * L, b"2" * L, b"k" + b"9" * L, b"2" * L + b"9"]
    xs += [b"1", b"0", b"10", b"01" * 40, b"a1", b"a0", b"110", b"001", b"1" * 11, b"0" * 10 + b"1"]
    streams = [O.encode(x) for x in xs]
    for sb in SEG_LENGTHS:
        for x, y in zip(xs, streams):
            st, _, ul = check(y, sb, "digits")
            assert st == 0 and ul == len(x)


def notcanon_streams(sb):
    """Every NOTCANON class of test_gpu_tail_scan.notcanon_streams over three segments of sb bytes:
    the bad token in the first, the middle and the last segment, its three bytes split by a segment
    edge both ways ("v | v d" and "v v | d"), as the final token, and the dangling pair."""
    out = []
    n = 3 * sb + 1
    places = [0, 1, sb + 1, 2 * sb + 1, sb - 1, sb - 2, 2 * sb - 1, 2 * sb - 2]
    for d in BAD_DIGITS:
        for p in places:
            out.append(literals(p) + b"aa" + d + literals(n - p - 3))
        out.append(literals(n - 3) + b"aa" + d)
    for C in (2, sb, sb + 1, sb + 2, 2 * sb, 2 * sb + 1, 2 * sb + 2, n):
        out.append(literals(C - 2) + b"aa")
    return out


def test_notcanon_in_every_segment_and_across_the_edges():
    for sb in SEG_LENGTHS:
        for y in notcanon_streams(sb):
            assert M.tail_of(y) is None
            assert check(y, sb, "notcanon") == (M.NOTCANON, 0, 0)


def test_a_bad_pair_on_an_untaken_phase_is_not_a_refusal():
    """"pp99x" parses as "pp9", "9", "x"; entered one byte late it reads the pair "99" with the count
    'x'.  A segment that starts inside it records a stop for that phase, and the scan must not look at
    it: only the taken phase's stop bit refuses."""
    for sb in SEG_LENGTHS:
        untaken_stop = 0
        for k in range(0, 3 * sb + 3):
            y = literals(k) + b"pp99x" + literals(sb + 5, b"m", b"n") + b"zz2"
            assert check(y, sb, "pp99x")[0] == 0
            summ = [T.summarize(y, q0, q1) for q0, q1 in seg_cut(len(y), sb)]
            taken, _, stop = T.compose(summ)
            assert not stop
            untaken_stop += sum(1 for s, e in zip(summ, taken) for f in range(3) if f != e and s[f].stop)
        assert untaken_stop > 0, sb


def test_decoded_length_is_summed_in_64_bits():
    """The sum of the taken counts passes 2^32 (a stream of "aa9" tokens below the 2 GiB limit decodes to
    more than 4 GiB): 90000 segments of 17 tiles of such tokens."""
    per = 9 * (17 * 1008 // 3)
    summ = [[T.Phase(per, 0, False, None)] * 3] * 90000
    taken, U, stop = T.compose(summ)
    assert U == 90000 * per and U > 1 << 32 and not stop and set(taken) == {0}
    y = b"aa9" * 40
    assert T.tail_seg(y, 12) == (0, M.tail_word(len(y) - 3, 9), 9 * 40)


def test_streams_past_the_segment_tables_are_refused():
    """total_in_bytes too small: the bound is total / (sb - 2) + n segments, the leading streams keep
    their results and the ones whose segments reach past the bound get RLE_STATUS_TOOLARGE."""
    sb = 10
    streams = [O.encode(O.gen(i % 5, i, 50)) for i in range(6)]
    full = T.tail_seg_batch(streams, sb, sum(len(y) for y in streams))
    assert full == [expected(y) for y in streams]
    total = 2 * sb
    maxseg = total // (sb - 2) + len(streams)
    got = T.tail_seg_batch(streams, sb, total)
    s0, refused = 0, 0
    for y, g in zip(streams, got):
        s0 += seg_count(len(y), sb)
        if s0 > maxseg:
            assert g == (M.TOOLARGE, 0, 0)
            refused += 1
        else:
            assert g == expected(y)
    assert 0 < refused < len(streams)
    assert T.tail_seg(b"", sb) == (0, 0, 0) and T.tail_seg(b"q", sb) == (0, M.tail_word(0, 1), 1)
