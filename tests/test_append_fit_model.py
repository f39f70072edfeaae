"""CPU check of the size and fit model (tests/append_fit_model.py) over the shapes the GPU tests run:
the exact new length lies between the old length and rle_append_slot_bytes, equals the oracle's
len(encode(x + new)), and the segmented composition gives the same figure at every segment length
from 4 to 16 tiles.  No GPU."""
import append_fit_model as F
import append_tail_model as M
import rle_mi355x as R
import rle_oracle as O

SEG_TILES = range(4, 17)
SB = 4 * F.TILE


def word(y):
    return M.word_of(y) if y else 0


def check_bounds(x, y, new):
    c = F.need(y, word(y), new)
    assert c == len(O.encode(x + new)), (x[-12:], new[:24], len(new))
    slot = M.slot_bytes(len(y), len(new))
    assert len(y) <= c <= slot, (len(y), c, slot, x[-12:], new[:24], len(new))
    return c


def seg_sweep(sb, lengths, counts, kinds=F.KINDS):
    out = []
    for An in lengths:
        for kind in kinds:
            for r in counts:
                x, y = F.stored_token(r) if r else (b"", b"")
                out.append((x, y, F.new_of(kind, An, 0x61, 13 * An + r)))
    return out


def test_slot_bytes_is_the_librarys():
    for C, An in ((0, 0), (0, 1), (5, 17), (4096, 1 << 20), (0x7FFFFFF0, 1), (1, 0x7FFFFFF0), (0x7FFFFFF1, 0)):
        assert M.slot_bytes(C, An) == R.append_slot_bytes(C, An), (C, An)


def test_need_is_bounded_on_the_splice_grid_and_composes():
    for x, y, new in F.splice_grid():
        c = check_bounds(x, y, new)
        for tiles in (4, 16):   # one segment at every length: the entering state alone
            assert F.need_seg(y, word(y), new, tiles * F.TILE) == c, (tiles, x[-12:], new)


def test_need_is_bounded_on_the_a_sweep_and_composes():
    for x, y, new in F.a_sweep():
        c = check_bounds(x, y, new)
        for tiles in SEG_TILES:
            assert F.need_seg(y, word(y), new, tiles * F.TILE) == c, (tiles, x[-12:], len(new))


def test_need_at_the_segment_edges_of_four_tiles():
    for x, y, new in seg_sweep(SB, F.seg_edge_lengths(SB), (1, 5, 9, 0)):
        c = check_bounds(x, y, new)
        assert F.need_seg(y, word(y), new, SB) == c, (x[-12:], len(new))


def test_need_composes_at_every_segment_length():
    for tiles in SEG_TILES:
        s = tiles * F.TILE
        cases = seg_sweep(s, (s - 1, s + 1, 2 * s + 3), (5,)) + seg_sweep(s, (2 * s + 3,), (0,), ("runs50",))
        for x, y, new in cases:
            c = check_bounds(x, y, new)
            assert F.need_seg(y, word(y), new, s) == c, (tiles, x[-12:], len(new))


def test_fit_decision():
    x, y = F.stored_token(3)
    w = word(y)
    new = b"aaaaaaaab"   # e = 6 fills the token, then "aa2" and "b"
    c = F.need(y, w, new)
    assert c == len(y) + 4
    assert F.decide(y, w, new) == (0, c)
    assert F.decide(y, w, new, cap=c) == (0, c) and F.decide(y, w, new, cap=c - 1) == (F.NOFIT, c)
    assert F.fit(y, w, new, c - 1) == (F.NOFIT, c, y, w)
    st, nd, out, w2 = F.fit(y, w, new, c)
    assert (st, nd, out, w2) == (0, c, O.encode(x + new), M.word_of(O.encode(x + new)))
    # nothing to append: OK with the old length, the capacity not consulted
    assert F.decide(y, w, b"", cap=0) == (0, len(y))
    # the order of the checks: address before tail word, tail word before the capacity
    assert F.decide(y, w, new, cap=0, addr_ok=False) == (M.MISALIGNED, 0)
    assert F.decide(y, w + 1, new, cap=0) == (M.NOTCANON, 0)
    assert F.decide(y, w | (1 << 36), b"", cap=0) == (M.NOTCANON, 0)
    assert F.decide(b"", 0, b"k", cap=0) == (F.NOFIT, 1) and F.decide(b"", 0, b"k", cap=1) == (0, 1)
    # r = 1: the token grows from one byte to three
    x1, y1 = F.stored_token(1)
    assert F.need(y1, word(y1), b"a") == len(y1) + 2
