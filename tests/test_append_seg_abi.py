"""CPU tests of the segmented append's host side (include/rle_mi355x.h:
rle_append_seg_workspace_bytes, rle_append_batch_device_seg): the exports, the C99 declarations, the
workspace size, and the returns that are decided before anything is launched, so that fake pointers
are enough.  No GPU."""
import ctypes
import os
import subprocess
import tempfile

import rle_mi355x as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(REPO, "include")
TILE = 1008


def test_symbols_exported_and_wrapped():
    L = R.lib()
    for sym in ("rle_append_seg_workspace_bytes", "rle_append_batch_device_seg"):
        assert hasattr(L, sym), sym
    assert callable(R.append_seg_workspace) and callable(R.append_batch_seg)


def test_declarations_are_c99():
    """A C99 translation unit that includes the header and takes both addresses with the documented
    types links against the library (compiled and linked, not run)."""
    code = r'''
#include "rle_mi355x.h"
typedef size_t (*ws_fn)(uint32_t, uint64_t);
typedef int (*app_fn)(void*, const uint64_t*, uint64_t*, const uint64_t*, uint64_t*, uint64_t*, const void*,
                      const uint64_t*, const uint64_t*, uint32_t*, uint32_t, uint64_t, void*, size_t, void*);
ws_fn take_ws(void) { return rle_append_seg_workspace_bytes; }
app_fn take_app(void) { return rle_append_batch_device_seg; }
int main(void) { return take_ws() != 0 && take_app() != 0 ? 0 : 1; }
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


def test_workspace_holds_the_encodes_and_grows():
    L = R.lib()
    ws, enc = L.rle_append_seg_workspace_bytes, L.rle_seg_workspace_bytes
    # (totals that take 4-tile segments, and 1 GiB at 16 tiles: more segments at every step.  Not every
    # pair of totals is ordered, tests/test_seg_lengths.py: where the segment length steps up, the
    # segment count steps down)
    assert [R.seg_segment_bytes(t) for t in (1, 16 << 20, 1 << 30)] == [4 * TILE, 4 * TILE, 16 * TILE]
    points = [1, 1 << 16, 1 << 20, 16 << 20, 1 << 30]
    for n in (1, 8, 1100):
        sizes = [int(ws(n, t)) for t in points]
        assert all(int(ws(n, t)) >= int(enc(n, t)) + 16 * n for t in points), n
        assert all(s % 256 == 0 for s in sizes)
        assert all(a < b for a, b in zip(sizes, sizes[1:])), (n, sizes)
    for t in points:
        sizes = [int(ws(n, t)) for n in (1, 8, 1100, 70000)]
        assert all(a < b for a, b in zip(sizes[1:], sizes[2:])) and sizes[0] <= sizes[1], (t, sizes)


def test_host_side_returns_with_fake_pointers():
    """n == 0 is RLE_OK whatever the pointers; a NULL required pointer, a NULL workspace and a short
    workspace are RLE_E_INVAL -- all before any launch: the pointers below point nowhere."""
    L = R.lib()
    f = L.rle_append_batch_device_seg
    fake = [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(10)]   # streams off len cap ulen tail new new_off new_len status
    ws, total, n = ctypes.c_void_p(0x100000), 1 << 20, 4
    need = int(L.rle_append_seg_workspace_bytes(n, total))
    assert f(*([None] * 10), 0, 0, None, 0, None) == R.RLE_OK
    assert f(*fake, 0, total, ws, 0, None) == R.RLE_OK
    for k in (0, 1, 2, 3, 5, 6, 7, 8):   # every required pointer (d_ulen = 4 and d_status = 9 may be NULL)
        args = list(fake)
        args[k] = None
        assert f(*args, n, total, ws, need, None) == R.RLE_E_INVAL, k
    assert f(*fake, n, total, None, need, None) == R.RLE_E_INVAL
    assert f(*fake, n, total, ws, 0, None) == R.RLE_E_INVAL
    assert f(*fake, n, total, ws, need - 1, None) == R.RLE_E_INVAL
    # the size asked for is the one of this n and this total: the encode's size is not enough
    assert f(*fake, n, total, ws, int(L.rle_seg_workspace_bytes(n, total)), None) == R.RLE_E_INVAL
