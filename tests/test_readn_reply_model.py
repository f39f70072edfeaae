"""CPU tests of the reply model (tests/readn_reply_model.py): its fields against libc's own
snprintf("%010ld"), its headers and layout against the packed read-N's model (readn_pack_model), and
the low-ten-digits rule.  No GPU."""
import ctypes

import pytest

import readn_pack_model as M
import readn_reply_model as RM

VALUES = (0, 9, 10, 99, 100, 2 ** 31 - 16, 10 ** 10 - 1)


def c_field(v):
    libc = ctypes.CDLL(None)
    libc.snprintf.restype = ctypes.c_int
    libc.snprintf.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_long]
    buf = ctypes.create_string_buffer(32)
    k = libc.snprintf(buf, 32, b"%010ld", v)
    return buf.raw[:k]


@pytest.mark.parametrize("v", VALUES)
def test_field_is_libc_snprintf(v):
    assert RM.field(v) == c_field(v) and len(RM.field(v)) == 10


def test_low_ten_digits_rule():
    """10^10 and more does not fit: snprintf writes eleven characters and more, the model (and the
    kernel) the low ten digits."""
    for v in (10 ** 10, 10 ** 10 + 7, 2 ** 40 + 123, 2 ** 64 - 1):
        assert len(c_field(v if v < 2 ** 63 else 2 ** 63 - 1)) > 10
        assert RM.field(v) == (b"%d" % v)[-10:] and len(RM.field(v)) == 10
    assert RM.field(10 ** 10 + 7) == b"0000000007"
    assert RM.header(RM.READ, None, 10 ** 10 + 7) == b"0000000007"


def files():
    paths = [b"/a", b"x", b"/srv/store/some/longer/name.bin", b"\x00\xff name", b"/e"]
    contents = [b"hello", b"", b"z" * 1000, b"\x00" * 17, b"q"]
    return paths, contents


def test_headers_per_form():
    assert RM.header(RM.READN, b"/tmp/f", 1234) == b"0000000006/tmp/f0000001234"
    assert RM.header(RM.READN | RM.END, b"/tmp/f", 1234) == RM.header(RM.READN, b"/tmp/f", 1234)
    assert RM.header(RM.READ, b"/tmp/f", 1234) == b"0000001234"
    assert RM.TERMINATOR == b"0" * 10 == RM.field(0)
    for form in RM.FORMS:
        for p in (b"", b"a", b"b" * 255):
            assert len(RM.header(form, p, 77)) == RM.header_bytes(form, len(p))
    for bad in (2, 3, 0x101, 0x200, 0x80000000):
        assert RM.header_bytes(bad, 5) == 0


def test_model_is_the_packed_models_reply():
    paths, contents = files()
    want = M.reply(paths, contents)
    assert RM.reply(paths, contents, RM.READN) == want
    assert RM.reply(paths, contents, RM.READN | RM.END) == want + b"0000000000"
    assert RM.reply(paths[:1], contents[:1], RM.READ) == b"0000000005hello"
    assert RM.reply([], [], RM.READN | RM.END) == b"0000000000" and RM.reply([], [], RM.READN) == b""


@pytest.mark.parametrize("form", RM.FORMS)
def test_layout_with_derived_gaps(form):
    paths, contents = files()
    ulen, pl = [len(c) for c in contents], [len(p) for p in paths]
    place, total = RM.layout(ulen, pl, form)
    want = RM.reply(paths, contents, form)
    assert total == len(want)
    for p, c, at in zip(paths, contents, place):
        h = RM.header(form, p, len(c))
        assert want[at - len(h):at + len(c)] == h + c
    gaps = [RM.header_bytes(form, n) for n in pl]
    assert (place, total - (10 if form & RM.END else 0)) == M.layout(ulen, gaps)
    assert RM.layout([], [], form) == ([], 10 if form & RM.END else 0)


def test_layout_past_one_stride_wraps_in_64_bits():
    n = 1025
    ulen = [(1 << 63) + i for i in range(n)]
    pl = [i % 300 for i in range(n)]
    place, total = RM.layout(ulen, pl, RM.READN | RM.END)
    assert total == (sum(ulen) + sum(pl) + 20 * n + 10) % (1 << 64)
    assert place[1024] == (sum(ulen[:1024]) + sum(pl[:1025]) + 20 * 1025) % (1 << 64)
