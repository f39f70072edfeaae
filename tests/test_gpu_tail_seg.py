"""rle_tail_batch_device_seg on the GPU against the documented parse (tests/append_tail_model.py
tail_of, through append_tail_gpu.scan_expected): status, tail word and decoded length of every
stream, through the C ABI, a few launches per test.  The shapes are the smallest at which the
segmented form can go wrong: a handful of 4-tile segments (SB = 4032 bytes under a small
total_in_bytes), every test asserting through rle_seg_segment_bytes the segment length it ran at.
Result arrays are pre-filled with append_tail_gpu's poison values."""
import numpy as np
import pytest
import torch

import append_tail_gpu as G
import append_tail_model as M
import rle_mi355x as R
import rle_oracle as O
import tail_seg_model as T
from test_gpu_graph_replay import stream_of_len
from test_gpu_seg_lengths import hint_for
from test_gpu_tail_scan import BAD_DIGITS, literals, pairs_body

pytestmark = pytest.mark.gpu
DEV = G.DEV
TILE = 1008
SB = 4 * TILE


def arena(streams, padding=None, shift=None, length=None):
    """append_tail_gpu.scan's arena: the streams packed 16-byte aligned with PAD spare bytes each.
    padding: {index: bytes written right behind the stream}; shift: {index: bytes added to the
    offset}; length: {index: the length passed instead of the true one}.  -> (d_in, offs, lens)."""
    lens = [len(s) for s in streams]
    offs, total = R.layout(lens, pad=G.PAD)
    host = np.zeros(total + 64, np.uint8)
    for i, (s, o) in enumerate(zip(streams, offs)):
        host[o:o + len(s)] = np.frombuffer(s, np.uint8)
        fill = (padding or {}).get(i, b"")
        host[o + len(s):o + len(s) + len(fill)] = np.frombuffer(fill, np.uint8)
    offs, lens = list(offs), list(lens)
    for i, d in (shift or {}).items():
        offs[i] += d
    for i, v in (length or {}).items():
        lens[i] = v
    return torch.from_numpy(host).to(DEV), G.i64(offs), G.i64(lens)


def results(n):
    return (torch.full((n,), 0x5555555555, dtype=torch.int64, device=DEV),
            torch.full((n,), 0x6666666666, dtype=torch.int64, device=DEV),
            torch.full((n,), 0x7777, dtype=torch.int32, device=DEV))


def host(tail, ulen, status):
    torch.cuda.synchronize()
    return (status.cpu().numpy().astype(np.uint32), tail.cpu().numpy().astype(np.uint64),
            ulen.cpu().numpy().astype(np.uint64))


def scan_seg(streams, total=None, sb=SB, **kw):
    """One rle_tail_batch_device_seg launch over `streams` with total_in_bytes = total (default: the
    sum of the true lengths), which must make the launcher take segments of sb bytes.  Returns
    (status, tail, ulen) as numpy arrays."""
    total = sum(len(s) for s in streams) if total is None else total
    assert R.seg_segment_bytes(total) == sb, (total, R.seg_segment_bytes(total), sb)
    d_in, offs, lens = arena(streams, **kw)
    tail, ulen, status = results(len(streams))
    R.tail_batch_seg(d_in, offs, lens, tail, ulen, status, total_in_bytes=total)
    return host(tail, ulen, status)


def check(streams, label, want=None, **kw):
    st, tl, ul = scan_seg(streams, **kw)
    for i, s in enumerate(streams):
        exp = (want or {}).get(i, G.scan_expected(s))
        got = (int(st[i]), int(tl[i]), int(ul[i]))
        assert got == exp, (label, i, len(s), [hex(v) for v in got], [hex(v) for v in exp], s[:24], s[-24:])
    return st, tl, ul


def test_final_token_around_the_segment_edges():
    """Streams of k SB + d bytes, d in -4..+5: the cut's own edges (remainder 0, 1 and 2 absorbed by
    the last segment, 3 a new 3-byte segment), after literals and after pair tokens that straddle the
    edges with 0, 1 and 2 bytes spilling, ending in a one-byte and in a three-byte final token."""
    streams, want_t = [], []
    for k in (1, 2, 5):
        for d in range(-4, 6):
            for final in (b"Q", b"QQ5"):
                t = k * SB + d - len(final)
                for body in (literals(t), pairs_body(t)):
                    streams.append(body + final)
                    want_t.append((t, 1 if len(final) == 1 else 5))
    st, tl, ul = check(streams, "final token around segment edges")
    assert [(R.tail_offset(w), R.tail_count(w)) for w in tl] == want_t
    assert (st == 0).all()


@pytest.mark.parametrize("m", range(4, 17))
def test_every_segment_length(m):
    """Segments of m tiles (the hint of test_gpu_seg_lengths): encoder streams of one and two segments
    -1, 0, +1 and +3 bytes, random and runs50 content."""
    sb, hint = m * TILE, hint_for(m)
    streams, xs = [], []
    for k in (1, 2):
        for d in (-1, 0, 1, 3):
            for kind in (1, 2):
                y, x = stream_of_len(k * sb + d, kind, 10 * m + k)
                streams.append(y)
                xs.append(x)
    for d in (0, 1, 2):   # pair tokens that spill d bytes over both edges of this length
        x = literals(d, b"m", b"n") + (b"pp" + b"q" * 3) * (2 * sb // 6) + b"Q"
        streams.append(O.encode(x))
        xs.append(x)
        assert streams[-1] == pairs_body(2 * sb + d) + b"Q"
    st, tl, ul = check(streams, f"{m}-tile segments", total=hint, sb=sb)
    assert (st == 0).all() and [int(u) for u in ul] == [len(x) for x in xs]
    one = [streams[5]]   # n = 1: the segments from the stream's own length
    check(one, f"{m}-tile segments, n = 1", total=hint, sb=sb)


def test_digit_valued_and_phase_hostile_data():
    """test_gpu_tail_scan.test_digit_valued_data's generators at lengths that cross one and two segment
    edges (streams of one digit keep the three entry phases apart over whole segments), and
    hand-made streams where only an untaken phase reads a pair with a bad count, right at an edge."""
    rng = np.random.default_rng(5)
    digits = np.frombuffer(b"0123456789", np.uint8)
    xs = []
    for n in (2000, 4000):
        xs.append(rng.choice(digits, 2 * n + 500).tobytes())
        xs.append(np.repeat(rng.choice(digits, n), rng.integers(1, 12, n)).tobytes())
    for C in (SB - 1, SB, SB + 1, SB + 3, 2 * SB, 2 * SB + 2, 2 * SB + 3):   # encode(v^L) is L / 3 bytes long
        xs += [b"9" * (3 * C), b"2" * (3 * C), b"k" + b"9" * (3 * C), b"2" * (3 * C) + b"9"]
    streams = [O.encode(x) for x in xs]
    assert min(len(y) for y in streams) > SB - 3 and max(len(y) for y in streams) > 2 * SB
    st, tl, ul = check(streams, "digit data")
    assert (st == 0).all() and [int(u) for u in ul] == [len(x) for x in xs]
    # "pp99x" is "pp9", "9", "x"; entered one byte late it is the pair "99" with the count 'x'
    hostile = [literals(e + d) + b"pp99x" + literals(SB, b"m", b"n") + b"zz2" for e in (SB, 2 * SB)
               for d in range(-5, 2)]
    st, tl, ul = check(hostile, "a bad pair on an untaken phase")
    assert (st == 0).all()


def notcanon_streams():
    """Every bad count digit, and the dangling pair, in the first, the middle and the last segment of
    a three-segment stream, and with the token's bytes split by a segment edge both ways
    ("v | v d" and "v v | d")."""
    out, n = [], 3 * SB + 1
    for d in BAD_DIGITS:
        for p in (0, 100, SB + 100, 2 * SB + 100, SB - 1, SB - 2, 2 * SB - 1, 2 * SB - 2):
            out.append(literals(p) + b"aa" + d + literals(n - p - 3))
        out.append(literals(n - 3) + b"aa" + d)
    for C in (2, SB, SB + 1, SB + 2, 2 * SB + 1, 2 * SB + 2, n):
        out.append(literals(C - 2) + b"aa")
    for s in out:
        assert M.tail_of(s) is None
    return out


def test_notcanon_in_every_segment():
    streams = notcanon_streams()
    st, tl, ul = check(streams, "notcanon")
    assert (st == M.NOTCANON).all() and not tl.any() and not ul.any()


def good_batch():
    return [O.encode(O.gen(1 + i % 4, 40 + i, s)) for i, s in
            enumerate((3 * SB, 50, SB + 7, 2 * SB + 1, 5 * SB, SB - 1, 2 * SB, 0, 3 * SB + 2))]


def test_refusals_among_good_streams():
    """A NOTCANON stream, a misaligned offset and an oversized length (never read) rotate through the
    first, the middle and the last index of a batch of good multi-segment streams."""
    good = good_batch()
    n = len(good)
    at = (0, n // 2, n - 1)
    nc = literals(SB + 100) + b"aa:" + literals(SB)
    total = 2 * sum(len(s) for s in good) + len(nc)
    for rot in range(3):
        streams, shift, length, want = list(good), {}, {}, {}
        i0, i1, i2 = (at[(j + rot) % 3] for j in range(3))
        streams[i0] = nc
        want[i0] = (M.NOTCANON, 0, 0)
        streams[i1] = good[3]
        shift[i1] = 8
        want[i1] = (M.MISALIGNED, 0, 0)
        length[i2] = (M.MAX_BUFFER_BYTES + 1, 0xFFFFFFFFFF, 1 << 63)[rot]
        want[i2] = (M.TOOLARGE, 0, 0)
        check(streams, f"refusals, rotation {rot}", want=want, total=total, shift=shift, length=length)


def test_total_in_bytes_too_small_refuses_the_trailing_streams():
    """6 streams of three segments each with tables sized for 6 segments' bytes (12 segments: the
    bytes' 6 and one per stream): the first four fit, the last two get RLE_STATUS_TOOLARGE."""
    streams = [stream_of_len(3 * SB, 1 + i % 2, 70 + i)[0] for i in range(6)]
    total = 6 * SB
    want = {4: (M.TOOLARGE, 0, 0), 5: (M.TOOLARGE, 0, 0)}
    check(streams, "short segment tables", want=want, total=total)
    assert T.tail_seg_batch(streams, SB, total) == [want.get(i, G.scan_expected(s)) for i, s in enumerate(streams)]


def test_batch_shapes():
    one = [O.encode(O.gen(2, 9, 3 * SB))]
    check(one, "n = 1")
    mixed = [b"", b"q", b"qq", b"qr", O.encode(O.gen(1, 3, 700)), O.encode(O.gen(3, 4, 5 * SB)), b"", literals(SB + 3),
             O.encode(O.gen(2, 5, 2 * SB)), b"z"]
    st, tl, ul = check(mixed, "mixed lengths")
    assert int(st[2]) == M.NOTCANON and int(st.sum()) == M.NOTCANON
    assert (int(st[0]), int(tl[0]), int(ul[0])) == (0, 0, 0)
    long = [O.encode(O.gen(2, 11, 300 << 10))]   # more than 64 segments: the scan crosses a window
    assert len(long[0]) > 64 * SB + SB
    check(long, "one stream of more than 64 segments")
    check(long + mixed, "the same among short streams")
    many = [O.encode(O.gen(i % 5, 100 + i, i % 41)) for i in range(1025)]
    many[77] = b"kk"   # one refusal inside
    st, tl, ul = check(many, "n = 1025")
    assert st[77] == M.NOTCANON and int(st.sum()) == M.NOTCANON


def test_padding_is_not_part_of_the_stream():
    """Arena bytes behind a stream that would continue its final token (test_gpu_tail_scan's fills),
    at C a multiple of 16 and not, and at the cut's own lengths k SB and k SB + 1."""
    streams, padding = [], {}
    for C in (SB, SB + 1, 2 * SB, 2 * SB + 1, 3 * SB + 16, SB + 5, SB - 16, 2 * SB - 3, 32, 21):
        for final in (b"Q", b"QQ7"):
            s = literals(C - len(final)) + final
            assert len(s) == C
            padding[len(streams)] = (b"Q7" if len(final) == 1 else b"7Q") + b"QQ9" * 8
            streams.append(s)
    st, tl, ul = check(streams, "hostile padding", padding=padding)
    assert (st == 0).all()


def test_same_results_as_the_one_wave_scan():
    """About 300 streams of 0 to 3 segments, every kind, some NOTCANON, through both entry points on
    one arena: the three result arrays are equal, and equal to the model."""
    rng = np.random.default_rng(11)
    streams = []
    for i in range(300):
        u = int(rng.integers(0, 3 * SB))
        if i % 5 == 4:   # pairs: the stream is 1.5 times its content
            u = 2 * u // 3
        y = O.encode(O.gen(i % 5, 900 + i, u))
        if i % 5 == 0:   # zero content compresses to a third: as long as the others
            y = O.encode(O.gen(0, i, 3 * u))
        if i % 23 == 7 and len(y) > 40:
            p = int(rng.integers(0, len(y) - 3))
            y = y[:p] + b"aa" + BAD_DIGITS[i % 5] + y[p + 3:]
        streams.append(y)
    total = sum(len(s) for s in streams)
    assert R.seg_segment_bytes(total) == SB
    d_in, offs, lens = arena(streams)
    a, b = results(len(streams)), results(len(streams))
    R.tail_batch_seg(d_in, offs, lens, *a, total_in_bytes=total)
    R.tail_batch(d_in, offs, lens, *b)
    seg, one = host(*a), host(*b)
    for x, y in zip(seg, one):
        assert np.array_equal(x, y)
    want = [G.scan_expected(s) for s in streams]
    assert [(int(s), int(t), int(u)) for s, t, u in zip(*seg)] == want
    nbad = sum(1 for w in want if w[0])
    assert 5 <= nbad < 60 and sum(1 for s in streams if len(s) > 2 * SB) > 20


def test_decoded_length_past_4_gib():
    """One stream of "aa9" tokens whose decoded length passes 2^32 (C is about 1.43 GB, below the
    2 GiB limit; the smallest C at which a 32-bit sum goes wrong), built on the device."""
    tokens = (1 << 32) // 9 + 1
    C = 3 * tokens
    assert 9 * tokens > 1 << 32 and C <= M.MAX_BUFFER_BYTES
    free, _ = torch.cuda.mem_get_info()
    if free < 4 << 30:
        pytest.skip(f"needs 4 GiB of free device memory for a {C}-byte stream, {free >> 20} MiB free")
    assert R.seg_segment_bytes(C) == 16 * TILE
    # (six tokens more than the stream: readable past C, and a padding that would continue it)
    d_in = torch.tensor([0x61, 0x61, 0x39], dtype=torch.uint8, device=DEV).repeat(tokens + 6)
    tail, ulen, status = results(1)
    R.tail_batch_seg(d_in, G.i64([0]), G.i64([C]), tail, ulen, status, total_in_bytes=C)
    st, tl, ul = host(tail, ulen, status)
    del d_in
    assert (int(st[0]), int(tl[0]), int(ul[0])) == (0, M.tail_word(C - 3, 9), 9 * tokens)
