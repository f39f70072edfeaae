"""GPU parity of the one-wave kernels at single-value spans and short last tiles against the oracle:
the encode's single-value test ahead of its boundary analysis (csrc/rle_device.h enc_span_test) on
single-value buffers at every tile and pair edge, with one differing byte at those edges, with
runs that enter the last pair from literal tiles and value changes at the last tile's first byte;
and the decode of streams whose last 1008-byte tile holds a few bytes, a few pairs, a pair across
the tile edge, the final unbounded token or a non-encoder anomaly, and of single-value streams
that end in a short tile.  Bit-exact, slots poisoned, through the sized batch entry points with
the cooperative kernels off."""
import numpy as np
import pytest

import rle_mi355x as R
import rle_oracle as O
from test_gpu_parity import gpu_decode, gpu_encode

pytestmark = pytest.mark.gpu
STEP = 1008    # decode tile step (csrc/rle_device.h kTileStep)
BATCH = 48
LENGTHS = (1, 2, 8, 9, 10, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 4095, 4096, 4097, 5120)
# ... and the lengths whose last 1024-byte encode tile stands alone (an odd tile count)
ODD_LENGTHS = (1009, 3025, 3030, 5041)


@pytest.fixture(autouse=True)
def _one_wave_kernels():
    R.set_coop_mode(0)
    yield
    R.set_coop_mode(-1)


def _check_encode(xs):
    for i in range(0, len(xs), BATCH):
        part = xs[i:i + BATCH]
        got, st = gpu_encode(part, max_len=max(len(x) for x in part))
        assert (st == 0).all()
        for j, x in enumerate(part):
            assert got[j] == O.encode(x), (i + j, len(x), x[:4].hex())


def _check_decode(streams, us, extra=0):
    """extra: room past U for what the reference writes there (non-encoder streams)."""
    for i in range(0, len(streams), BATCH):
        part, pu = streams[i:i + BATCH], us[i:i + BATCH]
        caps = [u + extra for u in pu]
        dec, st = gpu_decode(part, pu, caps, poison=extra == 0, max_in_len=max(len(s) for s in part),
                             max_out_len=max(pu))
        for j, s in enumerate(part):
            ref, rst = O.decode(s, pu[j], caps[j])
            assert dec[j] == ref, (i + j, len(s), pu[j])
            assert (int(st[j]) & 0xFF) == rst, (i + j, len(s), pu[j], int(st[j]))


def _literals(rng, n, avoid=-1):
    """n random bytes, no two adjacent ones equal, the last one not `avoid`."""
    x = rng.integers(0, 256, size=n).astype(np.int64)
    for k in range(n):
        while (k and x[k] == x[k - 1]) or (k == n - 1 and x[k] == avoid):
            x[k] = (x[k] + 1 + int(rng.integers(0, 200))) % 256
    return bytes(x.astype(np.uint8))


# ---------------------------------------------------------------- encode
def test_single_value_buffers():
    xs = [bytes([v]) * u for u in LENGTHS + ODD_LENGTHS for v in (0, 0x39, 0x41)]
    _check_encode(xs)


def test_one_differing_byte():
    xs = []
    for u in LENGTHS + ODD_LENGTHS:
        for p in sorted({0, u - 1, 1023, 1024, 2047, 2048}):
            if p < u:
                for v in (0, 0x41):
                    x = bytearray([v]) * u
                    x[p] ^= 0x5A
                    xs.append(bytes(x))
    _check_encode(xs)


def test_run_enters_the_last_pair_from_literal_tiles():
    rng = np.random.default_rng(71)
    xs = []
    for u in (2048, 3030, 3072, 4096, 8192):
        # the run starts in a literal tile, at every phase of the 9-byte token grid against the edges
        for start in list(range(0, 11)) + [1000, 1015, 1023, 1024, 1500, 2039, 2040, 2047, 2048, 2049, u - 1030,
                                          u - 1024, u - 1023, u - 9, u - 2, u - 1]:
            if 0 <= start < u:
                for v in (0, 0x39):
                    xs.append(_literals(rng, start, avoid=v) + bytes([v]) * (u - start))
        # ... and the literal data ends in the run's byte (the run starts one byte early)
        xs.append(_literals(rng, 1023, avoid=0) + b"\0" * (u - 1023))
        xs.append(_literals(rng, 2047, avoid=7)[:-1] + b"\7" * (u - 2046))
    _check_encode(xs)


def test_value_change_at_the_last_tile():
    xs = []
    for u in (1024, 2048, 3030, 3072, 4096, 4097, 5120):
        edge = (u - 1) // 1024 * 1024   # the last 1024-byte tile's first byte
        for at in (edge - 1, edge, edge + 1, edge + 8, edge + 9):
            if 0 < at < u:
                xs.append(b"\0" * at + b"\1" * (u - at))
                xs.append(b"\0" * at + b"\1" + b"\0" * (u - at - 1))
                xs.append(b"9" * at + b"8" * (u - at))
    _check_encode(xs)


# ---------------------------------------------------------------- decode
def _tail_stream(rng, k, r, npairs, skip, count=2, val=None):
    """Data whose stream is C = 1008 k + r bytes: literals, and `npairs` pair tokens in the last tile
    (as many as fit with a literal between them), the first one across the tile edge when `skip` is 1
    or 2 (it starts 2 or 1 bytes before the edge, so the tile's first token starts `skip` bytes in).
    count: the pairs' run length; val: their byte (no literal takes it)."""
    C, edge = STEP * k + r, STEP * k
    starts = [edge - 3 + skip] if skip else []
    room = r - skip
    n2 = min(npairs - len(starts), room // 4 if room >= 4 else room // 3)
    if n2 > 0:
        gap = room // n2
        # k = 1: packed against the stream's end (its last token is a pair); else spread over the tile
        starts += [C - 3 - 4 * j for j in range(n2)] if k == 1 else [edge + skip + j * gap for j in range(n2)]
    data, pos, prev = bytearray(), 0, -1
    while pos < C:
        pair = pos in starts
        v = val if pair and val is not None else int(rng.integers(0, 256))
        while v == prev or (val is not None and not pair and v == val):
            v = (v + 1) % 256
        data += bytes([v]) * (count if pair else 1)
        pos += 3 if pair else 1
        prev = v
    assert pos == C
    return bytes(data), C


def _tail_cases():
    rng = np.random.default_rng(1008)
    xs = []
    for k in (1, 4):
        for r in (1, 2, 3, 15, 16, 17, 63, 64, 127, 128, 129):
            for npairs in (0, 1, 4, 5):
                for skip in (0, 1, 2):
                    if skip > r or (skip and npairs == 0):
                        continue
                    xs.append(_tail_stream(rng, k, r, npairs, skip)[0])
            # a pair whose byte equals its digit ("222"), longer runs, and the final lone 0x00
            xs.append(_tail_stream(rng, k, r, 1, 0, val=0x32)[0])
            xs.append(_tail_stream(rng, k, r, 4, 0, count=9)[0])
            xs.append(_tail_stream(rng, k, r, 1, 0, count=5)[0])
            x = _tail_stream(rng, k, r, 1, 0)[0]
            xs.append(x[:-1] + b"\0" if len(x) > 1 and x[-2] != 0 else x)
    return xs


def test_short_last_tiles_of_encoder_streams():
    xs = _tail_cases()
    assert len(xs) > 200
    streams = [O.encode(x) for x in xs]
    rs = {len(s) % STEP for s in streams}
    assert {1, 2, 3, 15, 16, 17, 63, 64, 127, 128, 129} <= rs
    _check_decode(streams, [len(x) for x in xs])


def test_anomalies_in_the_last_tile():
    rng = np.random.default_rng(5)
    streams, us = [], []
    for k in (1, 4):
        for r in (5, 16, 64, 128):
            body = _literals(rng, STEP * k + r - 4, avoid=0x61)
            n = len(body)
            for tail, dec in ((b"aa1", 1), (b"aax", None), (b"aa:", None), (b"aa0", 1), (b"aa", None), (b"aa9", 9)):
                s = body + tail + (b"z" if len(tail) == 3 else b"")
                streams.append(s)
                us.append(n + (dec if dec is not None else 9) + 1)
            # output passing U: the last tile's tokens decode to more than is left
            for short in (1, 3, 8):
                streams.append(body + b"aa9z")
                us.append(n + 10 - short)
    _check_decode(streams, us, extra=32)


def test_single_value_streams_end_in_a_short_tile():
    xs = []
    for u in (3024, 3025, 4096, 4097, 3023, 3026, 3032, 3033, 6048, 6049, 9071, 9072, 9080, 12000):
        for v in (0, 0x32, 0x39, 0x41):
            xs.append(bytes([v]) * u)
    streams = [O.encode(x) for x in xs]
    us = [len(x) for x in xs]
    _check_decode(streams, us)
    # the same streams with a decoded size too large (SHORT: zero fill) and too small (the serial path)
    _check_decode(streams, [u + 7 for u in us])
    _check_decode(streams, [u - 5 for u in us], extra=32)
    # last tiles that break the "v v 9" form at their end: other digits, a non-digit, a final "v v"
    # whose digit is the padding, another byte
    odd, ou = [], []
    for ntok in (336, 337, 400, 455, 671, 672, 673):
        for v in (0, 0x39):
            base = bytes([v, v, 0x39]) * ntok
            for tail, n in ((bytes([v, v, 0x31]), 1), (bytes([v, v, 0x38]), 8), (bytes([v, v, 0x3A]), 9),
                            (bytes([v, v, 0x2F]), 9), (bytes([v, v]), 9), (bytes([v ^ 1]), 1), (bytes([v]), 1),
                            (bytes([v, v, 0x39, v ^ 1, v ^ 1, 0x33]), 12)):
                odd.append(base + tail)
                ou.append(9 * ntok + n)
    _check_decode(odd, ou, extra=32)
