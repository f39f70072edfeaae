"""CPU tests of the segmented packed read-N's host side (include/rle_mi355x.h:
rle_decode_packed_seg_workspace_bytes, rle_decode_packed_batch_device_seg,
rle_readn_batch_device_seg): the exports, the C99 declarations, the workspace size in closed form,
and the returns that are decided before anything is launched, so that fake pointers are enough.
No GPU."""
import ctypes
import os
import subprocess
import tempfile

import pytest

import rle_mi355x as R
from test_seg_abi import NS, TOTALS, seg_bytes_closed_form

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(REPO, "include")
SYMS = ("rle_decode_packed_seg_workspace_bytes", "rle_decode_packed_batch_device_seg", "rle_readn_batch_device_seg")


def test_symbols_exported_and_wrapped():
    L = R.lib()
    for sym in SYMS:
        assert hasattr(L, sym), sym
    assert callable(R.decode_packed_seg_workspace) and callable(R.decode_packed_seg) and callable(R.readn_batch_seg)


def test_declarations_are_c99():
    """A C99 translation unit that includes the header and takes the three addresses with the
    documented types links against the library (compiled and linked, not run)."""
    code = r'''
#include "rle_mi355x.h"
typedef size_t (*ws_fn)(uint32_t, uint64_t);
typedef int (*packed_fn)(const void*, const uint64_t*, const uint64_t*, void*, const uint64_t*, const uint64_t*,
                         uint32_t*, uint32_t, uint64_t, void*, size_t, void*);
typedef int (*readn_fn)(const void*, const uint64_t*, const uint64_t*, const uint64_t*, const uint64_t*, void*,
                        uint64_t, uint64_t*, uint64_t*, uint32_t*, uint32_t, uint64_t, void*, size_t, void*);
ws_fn take_ws(void) { return rle_decode_packed_seg_workspace_bytes; }
packed_fn take_packed(void) { return rle_decode_packed_batch_device_seg; }
readn_fn take_readn(void) { return rle_readn_batch_device_seg; }
int main(void) { return take_ws() != 0 && take_packed() != 0 && take_readn() != 0 ? 0 : 1; }
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


@pytest.mark.parametrize("n", NS)
def test_workspace_size_closed_form(n):
    """The form keeps no record of its own behind the shared tables: the workspace is the segmented
    decode's, rle_seg_workspace_bytes(n, total_in_bytes)."""
    L = R.lib()
    for total in TOTALS:
        want = seg_bytes_closed_form(n, total)
        assert int(L.rle_decode_packed_seg_workspace_bytes(n, total)) == want, (n, total)
        assert want == int(L.rle_seg_workspace_bytes(n, total)) and want % 256 == 0


def _fake(k):
    return [ctypes.c_void_p(0x1000 * (j + 1)) for j in range(k)]


WS, TOTAL, N = ctypes.c_void_p(0x100000), 1 << 20, 4


def test_decode_packed_seg_host_side_returns_with_fake_pointers():
    """in in_off in_len out out_off out_len status: n == 0 is RLE_OK whatever the pointers; a NULL
    required pointer, a NULL workspace and a short workspace are RLE_E_INVAL -- all before any
    launch: the pointers below point nowhere.  d_status may be NULL."""
    L = R.lib()
    f = L.rle_decode_packed_batch_device_seg
    need = int(L.rle_decode_packed_seg_workspace_bytes(N, TOTAL))
    assert need > 1
    assert f(*([None] * 7), 0, 0, None, 0, None) == R.RLE_OK
    assert f(*_fake(7), 0, TOTAL, WS, 0, None) == R.RLE_OK
    for k in range(6):
        args = _fake(7)
        args[k] = None
        assert f(*args, N, TOTAL, WS, need, None) == R.RLE_E_INVAL, k
    for args in (_fake(7), _fake(6) + [None]):   # (with and without status words)
        assert f(*args, N, TOTAL, None, need, None) == R.RLE_E_INVAL
        assert f(*args, N, TOTAL, WS, 0, None) == R.RLE_E_INVAL
        assert f(*args, N, TOTAL, WS, need - 1, None) == R.RLE_E_INVAL


def test_readn_seg_host_side_returns_with_fake_pointers():
    """streams off len ulen gap out | out_cap | place total status: n == 0 is RLE_OK (with a d_total
    it is a launch that writes 0 there: tests/test_gpu_readn_pack_seg.py); a NULL d_streams, d_off,
    d_len, d_ulen, d_out, d_place or d_total, a NULL workspace and a short workspace are
    RLE_E_INVAL; d_gap and d_status may be NULL."""
    L = R.lib()
    f = L.rle_readn_batch_device_seg
    need = int(L.rle_decode_packed_seg_workspace_bytes(N, TOTAL))

    def call(ptrs, n, ws, nbytes):
        return f(*ptrs[:6], 1 << 20, *ptrs[6:], n, TOTAL, ws, nbytes, None)

    assert call([None] * 9, 0, None, 0) == R.RLE_OK
    for k in (0, 1, 2, 3, 5, 6, 7):
        args = _fake(9)
        args[k] = None
        assert call(args, N, WS, need) == R.RLE_E_INVAL, k
    args = _fake(9)
    for a in (args, args[:4] + [None] + args[5:8] + [None]):   # (with and without gaps and status words)
        assert call(a, N, None, need) == R.RLE_E_INVAL
        assert call(a, N, WS, 0) == R.RLE_E_INVAL
        assert call(a, N, WS, need - 1) == R.RLE_E_INVAL
