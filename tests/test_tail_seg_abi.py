"""CPU tests of the segmented tail scan's host side (include/rle_mi355x.h:
rle_tail_seg_workspace_bytes, rle_tail_batch_device_seg): the exports, the C99 declarations, the
workspace size in closed form, and the returns that are decided before anything is launched, so that
fake pointers are enough.  No GPU."""
import ctypes
import os
import subprocess
import tempfile

import pytest

import rle_mi355x as R
from test_seg_abi import NS, TOTALS, seg_bytes_closed_form

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(REPO, "include")


def test_symbols_exported_and_wrapped():
    L = R.lib()
    for sym in ("rle_tail_seg_workspace_bytes", "rle_tail_batch_device_seg"):
        assert hasattr(L, sym), sym
    assert callable(R.tail_seg_workspace) and callable(R.tail_batch_seg)


def test_declarations_are_c99():
    """A C99 translation unit that includes the header and takes both addresses with the documented
    types links against the library (compiled and linked, not run)."""
    code = r'''
#include "rle_mi355x.h"
typedef size_t (*ws_fn)(uint32_t, uint64_t);
typedef int (*tail_fn)(const void*, const uint64_t*, const uint64_t*, uint64_t*, uint64_t*, uint32_t*, uint32_t,
                       uint64_t, void*, size_t, void*);
ws_fn take_ws(void) { return rle_tail_seg_workspace_bytes; }
tail_fn take_tail(void) { return rle_tail_batch_device_seg; }
int main(void) { return take_ws() != 0 && take_tail() != 0 ? 0 : 1; }
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
    """The scan keeps no record of its own behind the shared tables: the workspace is the segmented
    decode's, rle_seg_workspace_bytes(n, total_in_bytes)."""
    L = R.lib()
    for total in TOTALS:
        want = seg_bytes_closed_form(n, total)
        assert int(L.rle_tail_seg_workspace_bytes(n, total)) == want, (n, total)
        assert want == int(L.rle_seg_workspace_bytes(n, total)) and want % 256 == 0


def test_host_side_returns_with_fake_pointers():
    """n == 0 is RLE_OK whatever the pointers; a NULL required pointer, a NULL workspace and a short
    workspace are RLE_E_INVAL -- all before any launch: the pointers below point nowhere."""
    L = R.lib()
    f = L.rle_tail_batch_device_seg
    fake = [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(6)]   # in off len tail ulen status
    ws, total, n = ctypes.c_void_p(0x100000), 1 << 20, 4
    need = int(L.rle_tail_seg_workspace_bytes(n, total))
    assert need > 1
    assert f(*([None] * 6), 0, 0, None, 0, None) == R.RLE_OK
    assert f(*fake, 0, total, ws, 0, None) == R.RLE_OK
    for k in (0, 1, 2, 3):   # every required pointer (d_ulen = 4 and d_status = 5 may be NULL)
        args = list(fake)
        args[k] = None
        assert f(*args, n, total, ws, need, None) == R.RLE_E_INVAL, k
    assert f(*fake, n, total, None, need, None) == R.RLE_E_INVAL
    assert f(*fake, n, total, ws, 0, None) == R.RLE_E_INVAL
    assert f(*fake, n, total, ws, need - 1, None) == R.RLE_E_INVAL
