"""CPU tests of the host side of the reply entries (include/rle_mi355x.h: rle_reply_header_bytes,
rle_readn_headers_device, rle_readn_reply_device, rle_readn_reply_device_seg): the exports, the C99
declarations, the header lengths, and the returns that are decided before anything is launched, so
that fake pointers are enough.  No GPU."""
import ctypes
import os
import subprocess
import tempfile

import readn_reply_model as RM
import rle_mi355x as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(REPO, "include")
SYMS = ("rle_reply_header_bytes", "rle_readn_headers_device", "rle_readn_reply_device", "rle_readn_reply_device_seg")
BAD_FORMS = (2, 3, 0x101, 0x200, 0x102, 0x10000, 0x80000000)
WS, TOTAL, N = ctypes.c_void_p(0x100000), 1 << 20, 4


def test_symbols_exported_and_wrapped():
    L = R.lib()
    for sym in SYMS:
        assert hasattr(L, sym), sym
    for name in ("reply_header_bytes", "readn_headers", "readn_reply", "readn_reply_seg"):
        assert callable(getattr(R, name)), name
    assert (R.RLE_REPLY_READN, R.RLE_REPLY_READ, R.RLE_REPLY_END) == (RM.READN, RM.READ, RM.END) == (0, 1, 0x100)
    with open(os.path.join(INC, "rle_mi355x.h")) as f:
        text = f.read()
    for sym in SYMS:
        assert text.count(sym) >= 2, sym
    for sym in SYMS[1:]:   # the device entries are named in the capture paragraph ahead of the declarations
        assert text.index(sym) < text.index("#ifndef RLE_MI355X_H"), sym
    for name in ("RLE_REPLY_READN", "RLE_REPLY_READ", "RLE_REPLY_END"):   # (values: the C99 test below)
        assert f"#define {name} " in text, name


def test_declarations_are_c99():
    """A C99 translation unit that includes the header and takes the four addresses with the
    documented types links against the library (compiled and linked, not run)."""
    code = r'''
#include "rle_mi355x.h"
typedef size_t (*bytes_fn)(uint32_t, uint64_t);
typedef int (*headers_fn)(const void*, const uint64_t*, const uint64_t*, const uint64_t*, void*, const uint64_t*,
                          uint32_t, uint32_t, void*);
typedef int (*reply_fn)(const void*, const uint64_t*, const uint64_t*, const uint64_t*, const void*, const uint64_t*,
                        const uint64_t*, void*, uint64_t, uint64_t*, uint64_t*, uint32_t*, uint32_t, uint32_t, void*);
typedef int (*reply_seg_fn)(const void*, const uint64_t*, const uint64_t*, const uint64_t*, const void*,
                            const uint64_t*, const uint64_t*, void*, uint64_t, uint64_t*, uint64_t*, uint32_t*,
                            uint32_t, uint32_t, uint64_t, void*, size_t, void*);
bytes_fn take_bytes(void) { return rle_reply_header_bytes; }
headers_fn take_headers(void) { return rle_readn_headers_device; }
reply_fn take_reply(void) { return rle_readn_reply_device; }
reply_seg_fn take_reply_seg(void) { return rle_readn_reply_device_seg; }
int forms[(RLE_REPLY_READN == 0 && RLE_REPLY_READ == 1 && RLE_REPLY_END == 0x100) ? 1 : -1];
int main(void) {
    return take_bytes() != 0 && take_headers() != 0 && take_reply() != 0 && take_reply_seg() != 0 ? 0 : 1;
}
'''
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.c")
        with open(p, "w") as f:
            f.write(code)
        lib = R.LIB_PATH
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INC, p, "-o", os.path.join(d, "t"),
                            "-L" + os.path.dirname(lib), "-l:" + os.path.basename(lib),
                            "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--allow-shlib-undefined"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_header_bytes():
    f = R.lib().rle_reply_header_bytes
    for pl in (0, 1, 15, 255, 4096, 1 << 33):
        assert int(f(R.RLE_REPLY_READN, pl)) == 20 + pl == RM.header_bytes(RM.READN, pl)
        assert int(f(R.RLE_REPLY_READN | R.RLE_REPLY_END, pl)) == 20 + pl
        assert int(f(R.RLE_REPLY_READ, pl)) == 10 == RM.header_bytes(RM.READ, pl)
        for bad in BAD_FORMS:
            assert int(f(bad, pl)) == 0 == RM.header_bytes(bad, pl), bad
    assert R.reply_header_bytes(R.RLE_REPLY_READN, 7) == 27 and R.reply_header_bytes(R.RLE_REPLY_READ) == 10


def _fake(k):
    return [ctypes.c_void_p(0x1000 * (j + 1)) for j in range(k)]


def test_headers_host_side_returns_with_fake_pointers():
    """paths path_off path_len ulen out place | form n: a bad form is RLE_E_INVAL whatever n; n == 0
    without the terminator is RLE_OK whatever the pointers; with n > 0 a NULL d_ulen, d_out or d_place,
    and in the READN form a NULL path array, is RLE_E_INVAL; with the terminator and n == 0 a NULL
    d_out is."""
    f = R.lib().rle_readn_headers_device
    for bad in BAD_FORMS:
        assert f(*_fake(6), bad, N, None) == R.RLE_E_INVAL, bad
        assert f(*_fake(6), bad, 0, None) == R.RLE_E_INVAL, bad
    for form in (R.RLE_REPLY_READN, R.RLE_REPLY_READ):
        assert f(*([None] * 6), form, 0, None) == R.RLE_OK
        assert f(*_fake(6), form, 0, None) == R.RLE_OK
    for form in (R.RLE_REPLY_READN, R.RLE_REPLY_READN | R.RLE_REPLY_END):
        for k in range(6):
            args = _fake(6)
            args[k] = None
            assert f(*args, form, N, None) == R.RLE_E_INVAL, (form, k)
    for k in (3, 4, 5):
        args = [None] * 3 + _fake(3)   # (the READ form reads no path array)
        args[k] = None
        assert f(*args, R.RLE_REPLY_READ, N, None) == R.RLE_E_INVAL, k
    args = _fake(6)
    args[4] = None
    assert f(*args, R.RLE_REPLY_READN | R.RLE_REPLY_END, 0, None) == R.RLE_E_INVAL


def _reply_call(f, ptrs, form, n, seg, ws=WS, nbytes=None):
    """streams off len ulen paths path_off path_len out | out_cap | place total status | form n"""
    tail = ()
    if seg:
        need = int(R.lib().rle_decode_packed_seg_workspace_bytes(max(n, 1), TOTAL))
        tail = (TOTAL, ws, need if nbytes is None else nbytes)
    return f(*ptrs[:8], 1 << 20, *ptrs[8:], form, n, *tail, None)


def _reply_entries():
    L = R.lib()
    return ((L.rle_readn_reply_device, False), (L.rle_readn_reply_device_seg, True))


def test_reply_bad_forms_are_inval():
    for f, seg in _reply_entries():
        for bad in BAD_FORMS:
            for n in (0, N):
                assert _reply_call(f, _fake(11), bad, n, seg) == R.RLE_E_INVAL, (seg, bad, n)
        assert _reply_call(f, _fake(11), R.RLE_REPLY_READ | R.RLE_REPLY_END, N, seg) == R.RLE_E_INVAL   # (END with READ)


def test_reply_required_pointers():
    """A NULL d_streams, d_off, d_len, d_ulen, d_out, d_place or d_total is RLE_E_INVAL in every form;
    a NULL d_paths, d_path_off or d_path_len in the READN form (with and without the terminator), not
    in the READ form, which with all three NULL gets as far as its next refusal (a NULL d_total)."""
    for f, seg in _reply_entries():
        for form in (R.RLE_REPLY_READN, R.RLE_REPLY_READN | R.RLE_REPLY_END, R.RLE_REPLY_READ):
            for k in (0, 1, 2, 3, 7, 8, 9):
                args = _fake(11)
                args[k] = None
                assert _reply_call(f, args, form, N, seg) == R.RLE_E_INVAL, (seg, form, k)
        for form in (R.RLE_REPLY_READN, R.RLE_REPLY_READN | R.RLE_REPLY_END):
            for k in (4, 5, 6):
                for status in (True, False):
                    args = _fake(11)
                    args[k] = None
                    if not status:
                        args[10] = None
                    assert _reply_call(f, args, form, N, seg) == R.RLE_E_INVAL, (seg, form, k)


def test_reply_n0_returns():
    """n == 0 without the terminator is RLE_OK whatever the pointers (with a d_total it is a launch
    that writes 0 there: tests/test_gpu_readn_reply.py); with the terminator d_out and d_total are
    required."""
    for f, seg in _reply_entries():
        for form in (R.RLE_REPLY_READN, R.RLE_REPLY_READ):
            assert _reply_call(f, [None] * 11, form, 0, seg, ws=None, nbytes=0) == R.RLE_OK, (seg, form)
        for k in (7, 9):
            args = _fake(11)
            args[k] = None
            assert _reply_call(f, args, R.RLE_REPLY_READN | R.RLE_REPLY_END, 0, seg) == R.RLE_E_INVAL, (seg, k)


def test_reply_seg_workspace():
    """A NULL workspace and a short one are RLE_E_INVAL, in every form, with and without status words."""
    L = R.lib()
    f = L.rle_readn_reply_device_seg
    need = int(L.rle_decode_packed_seg_workspace_bytes(N, TOTAL))
    assert need > 1
    for form in (R.RLE_REPLY_READN, R.RLE_REPLY_READN | R.RLE_REPLY_END, R.RLE_REPLY_READ):
        for args in (_fake(11), _fake(10) + [None]):
            assert _reply_call(f, args, form, N, True, ws=None) == R.RLE_E_INVAL
            assert _reply_call(f, args, form, N, True, nbytes=0) == R.RLE_E_INVAL
            assert _reply_call(f, args, form, N, True, nbytes=need - 1) == R.RLE_E_INVAL
