"""Bytes past a buffer's length are ignored by every form, encode and decode: they read as 0x00
(include/rleCompression.h:17-18; DESIGN.md, the device API's contract).

Every other device test lays its buffers into a zeroed image, so the bytes between a buffer's end
and the next slot are exactly what the kernels are supposed to pretend they are.  Here the image is
hostile (test_gpu_parity._input_image): after each buffer come the bytes last, last, '9', last, ...
(last: the buffer's final byte), so a decoder that read memory would see a pair token and an
encoder its final run going on; with packed slots and a length that is a multiple of 16 the next
buffer itself begins that way.  Both layouts run: packed, and 16 spare bytes after every slot.
Expected outputs are the oracle's: O.encode(x), O.decode(stream, U, cap)."""
import ctypes

import pytest

import rle_mi355x as R
import rle_oracle as O
import stream_family as F
from test_gpu_parity import gpu_decode, gpu_encode

pytestmark = pytest.mark.gpu
S = F.SEG
SIZES = [1, 2, 15, 16, 17, 1007, 1008, 1009, 1023, 1024, 1025, 2016, 4096, S - 1, S, S + 1]
PADS = [0, 16]
_cache = {}


def enc_inputs():
    """Every size x kind; after a buffer whose length is a multiple of 16 (no slack in a packed slot)
    a short buffer that goes on with the same byte."""
    if "x" not in _cache:
        xs = []
        for kind in range(5):
            for i, n in enumerate(SIZES):
                x = O.gen(kind, 500 + 16 * kind + i, n)
                xs.append(x)
                if n % 16 == 0:
                    xs.append(x[-1:] * 5 + bytes([x[-1] ^ 1]))
        _cache["x"] = (xs, [O.encode(x) for x in xs])
    return _cache["x"]


def dec_inputs():
    """(streams, U, cap, expected, clean): the encodings of enc_inputs(); after a stream whose length
    is a multiple of 16 a stream that begins last, last, '9'; and the stream family's cut probes
    (the stream ends after "v" or "vv") at the start, the lane edge and the first tile edge.  clean:
    encoder output at its own size, whose status is 0 in every form -- a kernel that saw the hostile
    bytes as a token and then declined to the exact serial decoder would still produce the right
    bytes, but not that status."""
    if "y" not in _cache:
        xs, ys = enc_inputs()
        streams, us, caps, clean = [], [], [], []
        for x, y in zip(xs, ys):
            streams.append(y)
            us.append(len(x))
            caps.append(len(x))
            clean.append(True)
            if len(y) % 16 == 0:
                streams.append(y[-1:] * 2 + b"9x")
                us.append(10)
                caps.append(10)
                clean.append(True)
        for c in F.cases(F.WAVE_GROUPS["lane"] + F.WAVE_GROUPS["tile1"]):
            if c.probe >= 14:
                streams.append(c.stream)
                us.append(c.U)
                caps.append(c.cap)
                clean.append(False)
        want = [O.decode(s, u, c)[0] for s, u, c in zip(streams, us, caps)]
        for x, y in zip(xs, ys):
            assert want[streams.index(y)] == x
        _cache["y"] = (streams, us, caps, want, clean)
    return _cache["y"]


def _check_encode(pad, **kw):
    xs, ys = enc_inputs()
    got, st = gpu_encode(xs, pad=pad, **kw)
    assert (st == 0).all(), st
    bad = [i for i in range(len(xs)) if got[i] != ys[i]]
    assert not bad, (len(bad), bad[:5], [len(xs[i]) for i in bad[:5]])


def _check_decode(pad, pick=None, at_least=0, **kw):
    """Decode the inputs that `pick` takes (repeated until the launch has `at_least` buffers)."""
    streams, us, caps, want, clean = dec_inputs()
    idx = [i for i in range(len(streams)) if pick is None or pick(i)]
    idx = idx * max(1, -(-at_least // len(idx)))
    dec, st = gpu_decode([streams[i] for i in idx], [us[i] for i in idx], [caps[i] for i in idx], poison=False,
                         pad=pad, **kw)
    bad = [k for k, i in enumerate(idx) if dec[k] != want[i]]
    assert not bad, (len(bad), bad[:5], [(len(streams[idx[k]]), us[idx[k]]) for k in bad[:5]])
    info = R.RLE_STATUS_OVERFLOW | R.RLE_STATUS_SERIAL | R.RLE_STATUS_SHORT
    bad = [k for k, i in enumerate(idx) if int(st[k]) & ~(0 if clean[i] else info)]
    assert not bad, (len(bad), bad[:5], [(len(streams[idx[k]]), us[idx[k]], hex(int(st[k]))) for k in bad[:5]])
    return len(idx)


@pytest.fixture
def always_coop():
    R.set_coop_mode(1)
    yield
    R.set_coop_mode(-1)


# ------------------------------------------------------------------ encode
@pytest.mark.parametrize("pad", PADS)
def test_encode_one_wave(pad):
    _check_encode(pad)


@pytest.mark.parametrize("pad", PADS)
def test_encode_cooperative(pad, always_coop):
    xs, _ = enc_inputs()
    _check_encode(pad, max_len=max(len(x) for x in xs))


@pytest.mark.parametrize("pad", PADS)
def test_seg_encode(pad):
    _check_encode(pad, seg=True)


# ------------------------------------------------------------------ decode
@pytest.mark.parametrize("pad", PADS)
def test_decode_one_wave_192_chunks(pad):
    assert _check_decode(pad) <= 4096


@pytest.mark.parametrize("pad", PADS)
def test_decode_one_wave_96_chunks(pad):
    streams = dec_inputs()[0]
    assert _check_decode(pad, at_least=4097, pick=lambda i: len(streams[i]) <= 8192) >= 4097


@pytest.mark.parametrize("pad", PADS)
def test_decode_cooperative(pad, always_coop):
    """Small buffers (one round, a few waves), then everything the kernels take (80 tiles, 64 KiB)."""
    streams, us = dec_inputs()[:2]
    for mi, mo in ((4096 + 2048, 4096), (80 * F.TILE, 65536)):
        _check_decode(pad, pick=lambda i: len(streams[i]) <= mi and us[i] <= mo, max_in_len=mi, max_out_len=mo)


@pytest.mark.parametrize("pad", PADS)
def test_seg_decode(pad):
    _check_decode(pad, seg=True)


def test_seg_decode_one_buffer_launches():
    streams, us, caps, want, clean = dec_inputs()
    for i in range(0, len(streams), 5):
        for pad in PADS:
            dec, st = gpu_decode([streams[i]], [us[i]], [caps[i]], poison=False, seg=True, pad=pad)
            assert dec[0] == want[i] and (st[0] == 0 or not clean[i]), (i, pad, len(streams[i]), us[i], st)


@pytest.mark.parametrize("waves", [4, 8, 16])
def test_decode_rounds(waves):
    streams, us = dec_inputs()[:2]
    prev = R.set_dec_round(waves)
    R.set_coop_mode(0)
    try:
        for pad in PADS:
            assert _check_decode(pad, at_least=4097, pick=lambda i: len(streams[i]) <= 66000 and us[i] <= 65536,
                                 max_in_len=66000, max_out_len=65536) >= 4097
    finally:
        R.set_coop_mode(-1)
        R.set_dec_round(prev)


# ------------------------------------------------------------------ drop-in, through the C ABI
@pytest.mark.parametrize("n", [1, 16, 4096, 16384, 65536])
def test_dropin_pointer_inside_hostile_buffer(n):
    """RLEcompress / RLEdecompress on a (misaligned) pointer inside a larger buffer whose other bytes
    go on with the data's last byte.  Calls of these sizes copy the caller's bytes into the thread's
    mapped staging buffer (rle_dropin.cpp compress_small_zc / decompress_small_zc), so what the kernels
    find past the length is what the previous call left there: each call is therefore preceded by
    one on the same pointer that is 48 bytes longer, which leaves the hostile bytes in the staging
    right behind the data of the call under test."""
    L = R.lib()
    libc = ctypes.CDLL("libc.so.6")
    libc.free.argtypes = [ctypes.c_void_p]
    extra = 48

    def inside(data):
        last = data[-1]
        img = bytearray(bytes([data[0]]) * 4099 + data + bytes([last, last, 0x39]) * 2048)
        buf = (ctypes.c_char * len(img)).from_buffer(img)
        return buf, ctypes.cast(ctypes.addressof(buf) + 4099, ctypes.c_char_p)

    def compress(px, n):
        c = ctypes.c_size_t(0)
        p = L.RLEcompress(px, n, ctypes.byref(c))
        assert p
        got = ctypes.string_at(p, c.value)
        libc.free(p)
        return got

    def decompress(py, C, U, E):
        p = L.RLEdecompress(py, C, U, E)
        assert p
        got = ctypes.string_at(p, U + E)
        libc.free(p)
        return got

    for kind in range(5):
        x = O.gen(kind, 900 + kind, n)
        y = O.encode(x)
        keep, px = inside(x)
        primed = compress(px, len(x) + extra)
        assert primed == O.encode(x + (x[-1:] * 2 + b"9") * (extra // 3)), (kind, n)
        assert compress(px, len(x)) == y, (kind, n)
        keep, py = inside(y)
        tail = (y[-1:] * 2 + b"9") * (extra // 3)
        assert decompress(py, len(y) + extra, len(x) + 200, 0) == O.decode(y + tail, len(x) + 200, len(x) + 200)[0]
        assert decompress(py, len(y), len(x), 7) == x + bytes(7), (kind, n)
