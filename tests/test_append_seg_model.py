"""CPU check of the segmented append's algebra (tests/append_seg_model.py: entering state, seeded
scan, per-segment write with the uniform writer's closed form, new tail word) against the oracle's
encode(x + new) and the one-wave append's model (append_tail_model.append_carried), for segment
lengths 3..40 bytes.  No GPU."""
import append_seg_model as A
import append_tail_model as M
import rle_oracle as O

SEG_LENGTHS = range(3, 41)


def stored(c, r, long_run=False):
    """(x, y) with the final token of count r of byte c (behind full 9-tokens when long_run)."""
    other = b"q" if c != 0x71 else b"w"
    x = b"xy" * 3 + other + bytes([c]) * (r + (9 if long_run else 0))
    y = O.encode(x)
    assert M.tail_of(y)[:2] == (len(y) - (1 if r == 1 else 3), r)
    return x, y


def check(x, y, new, sb, seen=None):
    word = M.word_of(y) if y else 0
    got = A.append_seg(y, word, new, sb)
    want = O.encode(x + new)
    assert got[0] == want, (sb, x[-12:], new[:40], len(new))
    assert got == M.append_carried(y, word, new), (sb, x[-12:], new[:40], len(new))
    if new:
        assert got[1] == M.word_of(want)
    if seen is not None and new:
        c, r, e, vs, _ = A.entry(y, word, new)
        V = A.virtual(c, vs, new)
        segs = A.seg_cut(len(new), sb)
        seen.add((len(segs), e, tuple(A.is_uniform(V, vs + a, vs + b) for a, b in segs)[:1]))


def lengths(sb):
    """0..3 segments of new content: nothing, below a segment, and around every segment edge (a
    remainder of 1-2 bytes stays in the last segment, 3 start a new one)."""
    return sorted({0, 1, 2, sb - 1, sb, sb + 1, sb + 2, sb + 3, 2 * sb - 1, 2 * sb, 2 * sb + 2, 2 * sb + 3,
                   3 * sb - 1, 3 * sb, 3 * sb + 2})


def test_segment_cut_is_the_encodes():
    for sb in SEG_LENGTHS:
        for n in range(0, 4 * sb + 4):
            segs = A.seg_cut(n, sb)
            assert segs[0][0] == 0 and segs[-1][1] == n and len(segs) == max(1, (n + sb - 3) // sb)
            assert all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
            assert all(b - a == sb for a, b in segs[:-1]) and (n < 3 or segs[-1][1] - segs[-1][0] >= 3)


def test_every_r_and_e_over_0_to_3_segments():
    """Every stored count r, new content that leaves the run at once (e = 0), extends the final token
    by e < 9 - r, fills it (e = 9 - r), goes one and many bytes past it, and is the run alone (the
    uniform writer on the first and on inner segments); then literals or another run."""
    seen = set()
    for sb in SEG_LENGTHS:
        for r in range(1, 10):
            for c in (0x61, 0x39):
                x, y = stored(c, r, long_run=(sb + r) % 2 == 0)
                cb = bytes([c])
                for lead in sorted({0, 1, max(9 - r - 1, 0), 9 - r, 9 - r + 1, 9 - r + 9, 4 * sb}):
                    for n in lengths(sb):
                        for rest in (b"kl", b"z"):
                            new = (cb * lead + rest * (n + 1))[:n]
                            check(x, y, new, sb, seen)
    # the sweep reached: 1..3 segments, every e in 0..8, first segments with and without a boundary
    assert {k for k, _, _ in seen} == {1, 2, 3}
    assert {e for _, e, _ in seen} == set(range(9))
    assert {u for _, _, u in seen} == {(True,), (False,)}


def test_runs_ending_around_every_segment_edge():
    """New content of three segments whose runs end one byte before, at and one byte after each
    segment edge, alone and all together, after every r; the byte before the edge run is c or not."""
    for sb in SEG_LENGTHS:
        n = 3 * sb + 2
        cuts = [k * sb + d for k in (1, 2, 3) for d in (-1, 0, 1)]
        for r in (1, 2, 5, 8, 9):
            x, y = stored(0x61, r)
            for first in (b"a", b"b"):
                for cut in cuts:
                    new = (first * cut + b"c" * n)[:n]
                    check(x, y, new, sb)
            for d in (-1, 0, 1):   # a run boundary at every edge + d, and nowhere else
                new = b"".join(bytes([0x62 + k]) * (sb + (d if k == 0 else 0)) for k in range(4))[:n]
                check(x, y, new, sb)


def test_empty_stream_is_a_plain_encode():
    for sb in SEG_LENGTHS:
        for n in lengths(sb):
            for new in ((b"kl" * n)[:n], b"\0" * n, (b"a" * (sb + 1) + b"b" * n)[:n]):
                check(b"", b"", new, sb)


def test_digit_and_zero_bytes():
    """c = '9' with new '9's (the count digit equals the value) and c = 0x00."""
    for sb in (3, 4, 9, 10, 16, 27, 40):
        for c in (0x39, 0x00, 0x32):
            for r in range(1, 10):
                x, y = stored(c, r)
                for n in lengths(sb):
                    check(x, y, bytes([c]) * n, sb)
                    check(x, y, (bytes([c]) * (9 - r) + b"99" + bytes([c]) * n)[:n], sb)
