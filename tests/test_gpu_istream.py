"""GPU parity of the small-batch one-wave kernels (encode_kernel<2, 1>, decode_kernel<192, 0, 1>: the
launchers' choice for n <= 4096) where their per-wave instruction stream was shortened
(csrc/rle_device.h kLean: tile loads that leave M0 set, the walk's wait counts without the
sixteen-way switch): the slot and wait bookkeeping at 1 to 7
tiles with the stream ending in either slot, path changes inside one stream (literal, general and
single-value tiles next to each other, a partial chunk pending before a literal tile, short last
tiles), decode streams that leave the tiled path with tile loads still in flight, and all of it
again in hostile slots with the whole output arena compared.  Bit-exact against the oracle
(O.encode / O.decode), statuses included, through encode_batch / decode_batch with n <= 64 and the
cooperative kernels off."""
import numpy as np
import pytest
import torch

import rle_mi355x as R
import rle_oracle as O
from test_gpu_parity import DEV, POISON, _i64, _input_image

pytestmark = pytest.mark.gpu
STEP = 1008    # decode tile step (csrc/rle_device.h kTileStep)
ENC = 1024     # encode tile of buffers up to 16 KiB (kEncStep)
BATCH = 64
GUARD = 16     # spare bytes after every output slot
KINDS = {"zero": 0, "random": 1, "runs50": 2, "runs90": 3}
ENC_SIZES = (1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 4095, 4096, 4097, 5120, 6144, 7168)
DEC_STREAMS = (1007, 1008, 1009, 2015, 2016, 2017, 3024, 4032, 4033, 5040, 6048)
_cache = {}


@pytest.fixture(autouse=True)
def _one_wave_kernels():
    R.set_coop_mode(0)
    yield
    R.set_coop_mode(-1)


# ---------------------------------------------------------------- launches, whole arena compared
def _encode_arena(xs, pad):
    """One launch; returns (arena, offsets, lengths, status).  The arena is poisoned, with GUARD spare
    bytes after every slot; pad: hostile bytes around the input slots (test_gpu_parity._input_image)."""
    sizes = [len(x) for x in xs]
    in_offs, host = _input_image(xs, pad)
    out_offs, total = R.compressed_slots(sizes, pad=GUARD)
    d_in = torch.from_numpy(host).to(DEV)
    d_out = torch.full((total + 64,), POISON, dtype=torch.uint8, device=DEV)
    out_len = torch.zeros(len(xs), dtype=torch.int64, device=DEV)
    status = torch.full((len(xs),), 0x7777, dtype=torch.int32, device=DEV)
    R.encode_batch(d_in, _i64(in_offs), _i64(sizes), d_out, _i64(out_offs), out_len, status, max_len=max(sizes))
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), out_offs, out_len.cpu().numpy(), status.cpu().numpy()


def _check_encode(xs, pad=None):
    for i in range(0, len(xs), BATCH):
        part = xs[i:i + BATCH]
        arena, offs, lens, st = _encode_arena(part, pad)
        want = np.full(arena.shape, POISON, np.uint8)
        for j, x in enumerate(part):
            y = O.encode(x)
            want[offs[j]:offs[j] + len(y)] = np.frombuffer(y, np.uint8)
            assert int(lens[j]) == len(y), (i + j, len(x), int(lens[j]), len(y))
        assert (st == 0).all(), st
        bad = np.nonzero(arena != want)[0]
        assert bad.size == 0, (i, int(bad[0]), [k for k in range(len(part)) if offs[k] <= bad[0]][-1])


def _check_decode(streams, us, extra=0, pad=None):
    """extra: room past U for what the reference writes there (non-encoder streams); those slots start
    zeroed, as the oracle's buffer does, and everything outside the slots is poisoned."""
    for i in range(0, len(streams), BATCH):
        part, pu = streams[i:i + BATCH], us[i:i + BATCH]
        caps = [u + extra for u in pu]
        in_offs, host = _input_image(part, pad)
        out_offs, total = R.layout(caps, pad=GUARD)
        want = np.full(total + 64, POISON, np.uint8)
        init = want.copy()
        rst = []
        for j, s in enumerate(part):
            ref, r = O.decode(s, pu[j], caps[j])
            want[out_offs[j]:out_offs[j] + caps[j]] = np.frombuffer(ref, np.uint8)[:caps[j]]
            if extra:
                init[out_offs[j]:out_offs[j] + caps[j]] = 0
            rst.append(r)
        d_in = torch.from_numpy(host).to(DEV)
        d_out = torch.from_numpy(init).to(DEV)
        status = torch.full((len(part),), 0x7777, dtype=torch.int32, device=DEV)
        R.decode_batch(d_in, _i64(in_offs), _i64([len(s) for s in part]), d_out, _i64(out_offs), _i64(pu), _i64(caps),
                       status, max_in_len=max(len(s) for s in part), max_out_len=max(pu))
        torch.cuda.synchronize()
        arena, st = d_out.cpu().numpy(), status.cpu().numpy()
        bad = np.nonzero(arena != want)[0]
        assert bad.size == 0, (i, int(bad[0]), [k for k in range(len(part)) if out_offs[k] <= bad[0]][-1])
        got = [int(v) & 0xFF for v in st]
        assert got == rst, (i, got, rst)


# ---------------------------------------------------------------- data
def _literals(rng, n, before=-1, avoid=-1):
    """n random bytes, no two adjacent ones equal, the first not `before`, the last not `avoid`."""
    x = rng.integers(0, 256, size=n).astype(np.int64)
    prev = before
    for k in range(n):
        while x[k] == prev or (k == n - 1 and x[k] == avoid):
            x[k] = (x[k] + 1 + int(rng.integers(0, 200))) % 256
        prev = x[k]
    return bytes(x.astype(np.uint8))


def _input_with_stream_length(kind, index, C):
    """Data of the kind whose encoding is exactly C bytes: the longest prefix of the generator's buffer
    that encodes to at most C, then literals (one stream byte each)."""
    x = O.gen(kind, index, 9 * C)
    lo, hi = 0, len(x)
    while lo < hi:   # (the encoded length never falls as the prefix grows)
        mid = (lo + hi + 1) // 2
        if len(O.encode(x[:mid])) <= C:
            lo = mid
        else:
            hi = mid - 1
    rng = np.random.default_rng(1000 * kind + C)
    head = x[:lo]
    need = C - len(O.encode(head))
    x = head + _literals(rng, need, before=head[-1] if head else -1)
    assert len(O.encode(x)) == C, (kind, C, len(O.encode(x)))
    return x


def _dec_length_cases():
    if "dec" not in _cache:
        xs = [_input_with_stream_length(k, 40 + i, C) for k in KINDS.values() for i, C in enumerate(DEC_STREAMS)]
        _cache["dec"] = (xs, [O.encode(x) for x in xs])
    return _cache["dec"]


def _enc_length_cases():
    if "enc" not in _cache:
        _cache["enc"] = [O.gen(k, 7 + i, u) for k in KINDS.values() for i, u in enumerate(ENC_SIZES)]
    return _cache["enc"]


def _stream_tile(rng, form, before):
    """1008 stream bytes (whole tokens) of one form and the data they decode to: L literals, G runs
    of 5 between literals ("v v 5": the literal path declines at the digit), Z the single-value
    form "v v 9" of a byte no neighbour takes."""
    if form == "L":
        d = _literals(rng, STEP, before=before, avoid=0xEE)
        return d, d
    if form == "Z":
        return bytes([0xEE, 0xEE, 0x39]) * (STEP // 3), bytes([0xEE]) * (9 * (STEP // 3))
    s, d, prev = bytearray(), bytearray(), before
    while len(s) < STEP:
        lit = _literals(rng, 1, before=prev, avoid=0xEE)
        if len(s) + 4 <= STEP and len(s) % 7 == 0:
            s += lit * 2 + b"5"
            d += lit * 5
        else:
            s += lit
            d += lit
        prev = lit[0]
    assert len(s) == STEP
    return bytes(s), bytes(d)


def _stream_of(rng, forms, tail=0, lead=0):
    """A stream of `lead` literal bytes, one 1008-byte stretch per form and `tail` literal bytes, with
    its data.  (lead moves every later tile's output offset: a general tile then leaves a partial
    chunk of another length before the tile after it.)"""
    s, d = bytearray(), bytearray()
    for f in ["l%d" % lead] * (lead > 0) + list(forms) + ["l%d" % tail] * (tail > 0):
        before = d[-1] if d else -1
        if f[0] == "l":
            ts = td = _literals(rng, int(f[1:]), before=before, avoid=0xEE)
        else:
            ts, td = _stream_tile(rng, f, before)
        s += ts
        d += td
    s, d = bytes(s), bytes(d)
    assert O.encode(d) == s, forms   # (an encoder stream: every status is 0)
    return s, d


PATHS = ("LGL", "LZL", "LLGLL", "LLLLGL", "GL", "ZL", "LG", "LZ", "GZL", "LZGL", "ZZL", "LLLLLLL", "GLGLG")


def _path_cases():
    if "paths" not in _cache:
        rng = np.random.default_rng(355)
        out = []
        for forms in PATHS:
            for lead, tail in ((0, 0), (1, 1), (7, 3), (15, 4), (0, 5), (3, 16)):
                out.append(_stream_of(rng, forms, tail=tail, lead=lead))
        _cache["paths"] = out
    return _cache["paths"]


def _enc_block(rng, form, before, n=ENC):
    if form == "L":
        return _literals(rng, n, before=before, avoid=0xEE)
    if form == "Z":
        return bytes([0xEE]) * n
    d, prev = bytearray(), before
    while len(d) < n:   # G: runs of 3 to 11 between literals
        lit = _literals(rng, 1, before=prev, avoid=0xEE)
        d += lit * (1 if len(d) % 5 else 3 + len(d) % 9)
        prev = lit[0]
    return bytes(d[:n - 1]) + _literals(rng, 1, before=d[n - 2], avoid=0xEE)


def _enc_path_cases():
    if "encpaths" not in _cache:
        rng = np.random.default_rng(950)
        xs = []
        for forms in ("LLGGLL", "LGLL", "LLZZLL", "LLLZ", "ZZLL", "GGLL", "LLLLLLL", "LLLG", "LZLLL", "LLGL"):
            for tail in (0, 1, 3, 4, 5, 17):
                d = bytearray()
                for f in forms:
                    d += _enc_block(rng, f, d[-1] if d else -1)
                d += _literals(rng, tail, before=d[-1], avoid=0xEE)
                xs.append(bytes(d))
        # a pair whose second tile is the buffer's last, with 1, 3, 4 and 5 output bytes
        for base in (1024, 3072):
            for k in (1, 3, 4, 5):
                xs.append(_literals(rng, base + k))
                xs.append(_literals(rng, base + k - 2) + b"\x07\x07")   # ... ending in a pair
        # a run crossing a pair's middle or its edge, and starting at a pair's first byte
        for u in (4096, 5120):
            for at in (1024, 2048, 3072):
                for v in (0, 0x39):
                    for start, n in ((at - 20, 40), (at - 1, 2), (at, 2), (at, 40), (at - 2, 3), (at, 1100)):
                        n = min(n, u - start)
                        a = _literals(rng, start, avoid=v)
                        xs.append(a + bytes([v]) * n + _literals(rng, u - start - n, before=v))
        _cache["encpaths"] = xs
    return _cache["encpaths"]


def _leaving_cases():
    """Streams the tiled walk gives up on (the exact serial decoder finishes them): a bad digit, an
    unbounded count and output past U, on the first tile, on the last, and right after a literal
    tile; (streams, U, tiles)."""
    if "leave" not in _cache:
        rng = np.random.default_rng(192)
        streams, us = [], []
        for tiles in (1, 2, 3, 5, 6):
            C = STEP * tiles - 40
            for at in sorted({5, STEP + 2, STEP * (tiles - 1) + 9}):
                if at + 4 >= C:
                    continue
                for tok in (b"aa:", b"aax", b"aa/", b"aa\x7f", b"aa\xff", b"aa0"):
                    body = _literals(rng, at, avoid=0x61)
                    rest = _literals(rng, C - at - 3, before=0x61)
                    s = body + tok + rest
                    big = len(s) + 300   # (what the stream decodes to, capped there)
                    n = len(O.decode(s, big, big)[0].rstrip(b"\0"))
                    for u in (len(s) + 90, n, max(1, at + 1), max(1, len(s) - 7)):
                        streams.append(s)
                        us.append(u)
                # output past U with a well-formed stream: the walk stops at the tile that passes it
                s = _literals(rng, at, avoid=0x61) + b"aa9" + _literals(rng, C - at - 3, before=0x61)
                for short in (1, 8, 700):
                    if len(s) + 8 - short > 0:
                        streams.append(s)
                        us.append(len(s) + 6 - short)
        _cache["leave"] = (streams, us)
    return _cache["leave"]


# ---------------------------------------------------------------- slot and wait bookkeeping
@pytest.mark.parametrize("pad", [None, 16])
def test_encode_one_to_seven_tiles(pad):
    _check_encode(_enc_length_cases(), pad)


@pytest.mark.parametrize("pad", [None, 16])
def test_decode_one_to_seven_tiles(pad):
    xs, streams = _dec_length_cases()
    assert sorted({len(s) for s in streams}) == sorted(DEC_STREAMS)
    _check_decode(streams, [len(x) for x in xs], pad=pad)


# ---------------------------------------------------------------- path changes inside one stream
@pytest.mark.parametrize("pad", [None, 16])
def test_decode_path_changes(pad):
    cases = _path_cases()
    _check_decode([s for s, _ in cases], [len(d) for _, d in cases], pad=pad)


def test_decode_short_last_tile_after_literal_tiles():
    rng = np.random.default_rng(4)
    cases = [_stream_of(rng, "L" * k, tail=r) for k in (1, 2, 4) for r in (1, 3, 4, 5)]
    # ... the last bytes a pair (its digit the stream's last byte, or past the tile edge)
    for k in (1, 3):
        for r in (3, 4, 5):
            s, d = _stream_of(rng, "L" * k, tail=r - 3)
            cases.append((s + bytes([s[-1] ^ 0x55]) * 2 + b"2", None))
    streams = [s for s, _ in cases]
    us = [len(d) if d is not None else len(O.decode(s, 1 << 15, 1 << 15)[0].rstrip(b"\0")) for s, d in cases]
    _check_decode(streams, us)
    _check_decode(streams, [u + 3 for u in us])   # (SHORT: the zero fill after the last tile)


@pytest.mark.parametrize("pad", [None, 16])
def test_encode_path_changes(pad):
    _check_encode(_enc_path_cases(), pad)


# ---------------------------------------------------------------- leaving the tiled path
@pytest.mark.parametrize("pad", [None, 16])
def test_decode_leaves_the_tiled_path(pad):
    streams, us = _leaving_cases()
    assert len(streams) > 150
    _check_decode(streams, us, extra=32, pad=pad)
