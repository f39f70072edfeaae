"""CPU tests of the relocation's host model (tests/relocate_model.py): the layout against a brute-force
sum, the span rule and its partition of the destination, the ownership of every 16-byte chunk, and the
64-way search against bisect.  No GPU."""
import bisect
import random

import pytest

import relocate_model as M
import rle_mi355x as R


def brute(length, want, sel, base):
    off, caps, pos = [], [], base
    for c, w, s in zip(length, want, sel):
        m = max(c, w)
        k = ((m + 15) // 16) * 16 if s and m <= R.RLE_MAX_BUFFER_BYTES else 0
        off.append(pos)
        caps.append(k)
        pos += k
    return off, caps, pos


def test_constants_match_the_library():
    assert M.MAXB == R.RLE_MAX_BUFFER_BYTES
    assert (M.OK, M.MISALIGNED, M.TOOLARGE, M.NOFIT) == (R.RLE_STATUS_OK, R.RLE_STATUS_MISALIGNED,
                                                        R.RLE_STATUS_TOOLARGE, R.RLE_STATUS_NOFIT)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2500])
def test_layout_against_brute_force(n):
    rng = random.Random(n)
    length = [rng.choice([0, 1, 15, 16, 17, 4095, 4096, 4097, rng.randrange(1 << 20)]) for _ in range(n)]
    want = [rng.choice([0, c, max(c - 1, 0), c + 1, c + 15, c + 16, c + 100, 3 * c]) for c in length]
    sel = [rng.choice([0, 1, 1, 7]) for _ in range(n)]
    for base in (0, 16, 1 << 33):
        assert M.layout(length, want, sel, base) == brute(length, want, sel, base)
    assert M.layout(length) == brute(length, [0] * n, [1] * n, 0)


def test_layout_sums_pass_2_to_32():
    n = 1500
    length = [R.RLE_MAX_BUFFER_BYTES - 16 * (i % 5) for i in range(n)]   # ~2 GiB each: 3 TB in all
    want = [0] * n
    off, caps, total = M.layout(length, want, None, 1 << 20)
    assert (off, caps, total) == brute(length, want, [1] * n, 1 << 20)
    assert total > 1 << 41 and off[3] > 1 << 32


def test_layout_empty_unselected_and_toolarge():
    big = R.RLE_MAX_BUFFER_BYTES + 1
    # empty files take no bytes but have a place; wants below, at and above C
    assert M.layout([0, 5, 0], [0, 0, 0], None, 32) == ([32, 32, 48], [0, 16, 0], 48)
    assert M.layout([100, 100, 100], [50, 100, 101], None, 0) == ([0, 112, 224], [112, 112, 112], 336)
    # all unselected: nothing has a place, the total is the base
    assert M.layout([7, 4096], None, [0, 0], 64) == ([64, 64], [0, 0], 64)
    # a length or a want past the limit: no slot, the neighbours close up
    assert M.layout([16, big, 16], None, None, 0) == ([0, 16, 16], [16, 0, 16], 32)
    assert M.layout([16, 16, 16], [0, big, 0], None, 0) == ([0, 16, 16], [16, 0, 16], 32)
    assert M.layout([R.RLE_MAX_BUFFER_BYTES], None, None, 0)[1] == [R.RLE_MAX_BUFFER_BYTES]
    st = M.statuses([16, big, 16, 16], [0, 0, big, 0], [1, 1, 1, 0], [True, True, True, False], True)
    assert st == [M.OK, M.TOOLARGE, M.TOOLARGE, M.OK]
    assert M.statuses([16, big, 16], [0, 0, 0], [1, 1, 0], [True] * 3, False) == [M.NOFIT, M.NOFIT, M.OK]


def test_span_rule():
    rooms = list(range(0, 3 << 20, 4099)) + [16384, 16385, 2048 * 16384, 2048 * 16384 + 1, 1 << 30, (1 << 40) + 12345,
                                             (1 << 63) + 99]
    last = 0
    for room in sorted(rooms):
        span = M.span_bytes(room)
        assert span % 16384 == 0 and span >= 16384
        assert span >= last
        last = span
        g = M.grid(room, span)
        assert 1 <= g <= 2048 and g * span >= room and (g - 1) * span < max(room, 1)
    assert M.span_bytes(0) == 16384 and M.span_bytes(2048 * 16384) == 16384 and M.span_bytes(2048 * 16384 + 1) == 32768
    assert M.span_bytes(1 << 20, cus=4) == 32768


@pytest.mark.parametrize("seed", range(6))
def test_spans_partition_the_destination(seed):
    rng = random.Random(seed)
    base = 16 * rng.randrange(0, 5000)
    room = rng.randrange(0, 4 << 20)
    span = M.span_bytes(room, cus=rng.choice([4, 32, 256]))
    for total in (base, base + 16, base + room // 32 * 16, base + room // 16 * 16):
        pos = base
        for w in range(M.grid(room, span)):
            lo, hi = M.wg_range(w, base, span, total)
            if lo >= hi:
                continue
            assert lo == pos and hi > lo
            pos = hi
        assert pos == total


@pytest.mark.parametrize("seed", range(8))
def test_every_chunk_has_exactly_one_owner(seed):
    rng = random.Random(100 + seed)
    n = rng.choice([1, 5, 70, 300])
    length = [rng.choice([0, 1, 15, 16, 17, 1008, 4095, 4096, 4097, 16383, 16384, 16385, rng.randrange(70000)])
              for _ in range(n)]
    want = [rng.choice([0, c, c + 1, c + 16, c + 100, 2 * c + 40]) for c in length]
    sel = [rng.choice([0, 1, 1, 1]) for _ in range(n)]
    aligned = [rng.random() > 0.1 for _ in range(n)]
    base = 16 * rng.randrange(0, 3000)
    new_off, new_cap, total = M.layout(length, want, sel, base)
    slack = rng.choice([0, 16, 100000])
    span = M.span_bytes(total - base + slack, cus=rng.choice([2, 8]))   # few CUs: spans of several granules too
    got = M.chunks(length, aligned, new_off, new_cap, base, total + slack, total, span)
    seen = {}
    for w, i, k in got:
        assert (i, k) not in seen, (i, k, w, seen[(i, k)])
        seen[(i, k)] = w
        lo, hi = M.wg_range(w, base, span, total)
        assert lo <= new_off[i] + 16 * k and new_off[i] + 16 * k + 16 <= hi
    for i in range(n):
        moved = bool(new_cap[i]) and aligned[i]
        for k in range(new_cap[i] // 16):
            assert ((i, k) in seen) == (moved and 16 * k < M.r16(length[i])), (i, k)
    assert M.chunks(length, aligned, new_off, new_cap, base, total - 1, total, span) == []   # NOFIT: nothing moves


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4095, 4096, 4097, 70000])
def test_search_against_bisect(n):
    rng = random.Random(n)
    off, pos = [], 160
    for _ in range(n):   # runs of equal offsets: the zero-size slots
        off.append(pos)
        pos += rng.choice([0, 0, 0, 16, 16, 4096, 1 << 20])
    probes = {off[0], off[-1], pos + 16, off[n // 2], off[n // 2] + 16} | {rng.randrange(off[0], pos + 17) for _ in range(200)}
    bound = 1 if n <= 64 else 2 if n <= 4096 else 3
    for at in probes:
        i, loads = M.find(off, at)
        assert i == bisect.bisect_right(off, at) - 1, (n, at)
        assert loads <= bound, (n, at, loads)
