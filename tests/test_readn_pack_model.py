"""CPU tests of the packed read-N's host models (tests/readn_pack_model.py): the layout the way the
device computes it against numpy.cumsum, and the byte-ownership rule of the packed decode's stores
over every destination phase and every small length.  No GPU."""
import numpy as np

import readn_pack_model as M


def _cumsum_layout(ulen, gap):
    u = np.asarray(ulen, dtype=np.uint64)
    g = np.zeros(len(u), dtype=np.uint64) if gap is None else np.asarray(gap, dtype=np.uint64)
    ends = np.cumsum(u + g, dtype=np.uint64)
    place = ends - u
    return [int(v) for v in place], int(ends[-1]) if len(u) else 0


def _check(ulen, gap):
    place, total = M.layout(ulen, gap)
    wplace, wtotal = _cumsum_layout(ulen, gap)
    assert place == wplace
    assert total == wtotal


def test_layout_ragged_lengths():
    rng = np.random.default_rng(7)
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 5000):
        ulen = [int(v) for v in rng.integers(0, 70000, n)]
        gap = [int(v) for v in rng.integers(20, 120, n)]
        _check(ulen, gap)


def test_layout_zero_lengths_and_zero_gaps():
    n = 1500
    _check([0] * n, [0] * n)
    _check([0] * n, [21] * n)
    _check([0 if i % 3 else 4097 for i in range(n)], [0] * n)
    _check([0 if i % 5 else 13 for i in range(n)], [0 if i % 2 else 33 for i in range(n)])


def test_layout_null_gaps():
    rng = np.random.default_rng(8)
    ulen = [int(v) for v in rng.integers(0, 5000, 2100)]
    _check(ulen, None)
    assert M.layout(ulen, None) == M.layout(ulen, [0] * len(ulen))
    assert M.layout([], None) == ([], 0)


def test_layout_sum_past_32_bits():
    """Three files of just under 2 GiB each pass 2^32 at the third; 3000 of them pass 2^42."""
    big = 0x7FFFFFF0
    place, total = M.layout([big, big, big], [30, 31, 32])
    assert place[2] == 2 * big + 93 and total == 3 * big + 93 and total > 1 << 32
    _check([big] * 3000, [25] * 3000)
    _check([big - i for i in range(1100)], None)


def test_store_ownership_every_phase_and_small_length():
    """For every destination phase and U in 0..48: head bytes, aligned chunks and tail bytes are
    disjoint, cover exactly [p, p + U), the chunks are aligned, and fewer than 16 bytes go one by one
    at either end."""
    for p in range(32, 48):
        for U in range(49):
            head, chunks, tail = M.stores(p, U)
            wide = [b for c in chunks for b in range(c, c + 16)]
            assert all(c % 16 == 0 for c in chunks)
            assert len(head) < 16 and len(tail) < 16
            every = head + wide + tail
            assert len(every) == len(set(every)), (p, U)
            assert sorted(every) == list(range(p, p + U)), (p, U)


def test_abutting_files_share_no_wide_store():
    """Files packed with no gap: no aligned chunk of one file holds a byte of the file in front of
    it or behind it, whatever the two lengths and the phase."""
    for p in range(16, 32):
        for U in range(49):
            own = set(range(p, p + U))
            _, chunks, _ = M.stores(p, U)
            for U2 in range(49):
                q = p + U
                _, chunks2, _ = M.stores(q, U2)
                own2 = set(range(q, q + U2))
                assert not any(b in own2 for c in chunks for b in range(c, c + 16)), (p, U, U2)
                assert not any(b in own for c in chunks2 for b in range(c, c + 16)), (p, U, U2)
            for U0 in range(1, 49):   # the file in front
                _, chunks0, _ = M.stores(p - U0, U0) if p >= U0 else ([], [], [])
                assert not any(b in own for c in chunks0 for b in range(c, c + 16)), (p, U, U0)


def test_reply_is_the_reference_format():
    r = M.reply([b"/tmp/a", b"bb"], [b"xyz", b""])
    assert r == b"0000000006/tmp/a0000000003xyz" + b"0000000002bb0000000000"
    assert len(M.header(b"/tmp/a", 3)) == 20 + 6
