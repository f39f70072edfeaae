"""CPU tests of the host side of the packed read-N entries (include/rle_mi355x.h:
rle_decode_packed_batch_device, rle_readn_layout_device, rle_readn_batch_device): the exports, the
C99 declarations, and the returns that are decided before anything is launched, so that fake pointers
are enough.  No GPU."""
import ctypes
import os
import subprocess
import tempfile

import rle_mi355x as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(REPO, "include")
SYMS = ("rle_decode_packed_batch_device", "rle_readn_layout_device", "rle_readn_batch_device")


def test_symbols_exported_and_wrapped():
    L = R.lib()
    for sym in SYMS:
        assert hasattr(L, sym), sym
    for name in ("decode_packed", "readn_layout", "readn_batch"):
        assert callable(getattr(R, name)), name
    with open(os.path.join(INC, "rle_mi355x.h")) as f:
        text = f.read()
    for sym in SYMS:   # declared, and named in the capture paragraph ahead of the declarations
        assert text.count(sym) >= 2, sym
        assert text.index(sym) < text.index("#ifndef RLE_MI355X_H"), sym


def test_declarations_are_c99():
    """A C99 translation unit that includes the header and takes the three addresses with the
    documented types links against the library (compiled and linked, not run)."""
    code = r'''
#include "rle_mi355x.h"
typedef int (*packed_fn)(const void*, const uint64_t*, const uint64_t*, void*, const uint64_t*, const uint64_t*,
                         uint32_t*, uint32_t, void*);
typedef int (*layout_fn)(const uint64_t*, const uint64_t*, uint64_t*, uint64_t*, uint32_t, void*);
typedef int (*readn_fn)(const void*, const uint64_t*, const uint64_t*, const uint64_t*, const uint64_t*, void*,
                        uint64_t, uint64_t*, uint64_t*, uint32_t*, uint32_t, void*);
packed_fn take_packed(void) { return rle_decode_packed_batch_device; }
layout_fn take_layout(void) { return rle_readn_layout_device; }
readn_fn take_readn(void) { return rle_readn_batch_device; }
int main(void) { return take_packed() != 0 && take_layout() != 0 && take_readn() != 0 ? 0 : 1; }
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


def _fake(k):
    return [ctypes.c_void_p(0x1000 * (j + 1)) for j in range(k)]


def test_decode_packed_host_side_returns_with_fake_pointers():
    """in in_off in_len out out_off out_len status: n == 0 is RLE_OK whatever the pointers; a NULL
    required pointer is RLE_E_INVAL before any launch; d_status may be NULL."""
    f = R.lib().rle_decode_packed_batch_device
    assert f(*([None] * 7), 0, None) == R.RLE_OK
    assert f(*_fake(7), 0, None) == R.RLE_OK
    for k in range(6):
        args = _fake(7)
        args[k] = None
        assert f(*args, 4, None) == R.RLE_E_INVAL, k


def test_layout_host_side_returns_with_fake_pointers():
    """ulen gap place total: a NULL d_ulen, d_place or d_total is RLE_E_INVAL, a NULL d_gap is not
    among them; d_total is needed even for n == 0, which writes it (that write is a launch: its
    RLE_OK is checked on the device, tests/test_gpu_readn_pack.py::test_edge_layouts)."""
    f = R.lib().rle_readn_layout_device
    for k in (0, 2, 3):
        args = _fake(4)
        args[k] = None
        assert f(*args, 4, None) == R.RLE_E_INVAL, k
    args = _fake(4)
    args[1] = None
    args[3] = None   # (NULL gaps do not excuse a NULL total)
    assert f(*args, 4, None) == R.RLE_E_INVAL
    assert f(None, None, None, None, 0, None) == R.RLE_E_INVAL


def test_readn_host_side_returns_with_fake_pointers():
    """streams off len ulen gap out | out_cap | place total status: n == 0 is RLE_OK; a NULL
    d_streams, d_off, d_len, d_ulen, d_out, d_place or d_total is RLE_E_INVAL; d_gap and d_status may
    be NULL."""
    f = R.lib().rle_readn_batch_device

    def call(ptrs, n):
        return f(*ptrs[:6], 1 << 20, *ptrs[6:], n, None)

    assert call([None] * 9, 0) == R.RLE_OK
    for k in (0, 1, 2, 3, 5, 6, 7):
        args = _fake(9)
        args[k] = None
        assert call(args, 4) == R.RLE_E_INVAL, k
