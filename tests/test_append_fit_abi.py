"""CPU tests of the host side of the append's size and fit entries (include/rle_mi355x.h:
rle_append_size_batch_device, rle_append_fit_batch_device and their _seg forms): the exports, the
C99 declarations, the status constant, and the returns that are decided before anything is launched,
so that fake pointers are enough.  No GPU."""
import ctypes
import os
import subprocess
import tempfile

import rle_mi355x as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(REPO, "include")
SYMS = ("rle_append_size_batch_device", "rle_append_size_batch_device_seg", "rle_append_fit_batch_device",
        "rle_append_fit_batch_device_seg")


def test_symbols_exported_and_wrapped():
    L = R.lib()
    for sym in SYMS:
        assert hasattr(L, sym), sym
    for name in ("append_size", "append_size_seg", "append_fit", "append_fit_seg"):
        assert callable(getattr(R, name)), name
    assert R.RLE_STATUS_NOFIT == 0x2000
    with open(os.path.join(INC, "rle_mi355x.h")) as f:
        assert "#define RLE_STATUS_NOFIT       0x2000u" in f.read()


def test_declarations_are_c99():
    """A C99 translation unit that includes the header and takes the four addresses with the
    documented types links against the library (compiled and linked, not run)."""
    code = r'''
#include "rle_mi355x.h"
typedef int (*size_fn)(const void*, const uint64_t*, const uint64_t*, const uint64_t*, const void*, const uint64_t*,
                       const uint64_t*, uint64_t*, uint32_t*, uint32_t, void*);
typedef int (*size_seg_fn)(const void*, const uint64_t*, const uint64_t*, const uint64_t*, const void*,
                           const uint64_t*, const uint64_t*, uint64_t*, uint32_t*, uint32_t, uint64_t, void*, size_t,
                           void*);
typedef int (*fit_fn)(void*, const uint64_t*, uint64_t*, const uint64_t*, uint64_t*, uint64_t*, const void*,
                      const uint64_t*, const uint64_t*, uint64_t*, uint32_t*, uint32_t, void*);
typedef int (*fit_seg_fn)(void*, const uint64_t*, uint64_t*, const uint64_t*, uint64_t*, uint64_t*, const void*,
                          const uint64_t*, const uint64_t*, uint64_t*, uint32_t*, uint32_t, uint64_t, void*, size_t,
                          void*);
size_fn take_size(void) { return rle_append_size_batch_device; }
size_seg_fn take_size_seg(void) { return rle_append_size_batch_device_seg; }
fit_fn take_fit(void) { return rle_append_fit_batch_device; }
fit_seg_fn take_fit_seg(void) { return rle_append_fit_batch_device_seg; }
int main(void) {
    return take_size() != 0 && take_size_seg() != 0 && take_fit() != 0 && take_fit_seg() != 0 &&
                   RLE_STATUS_NOFIT == 0x2000u
               ? 0
               : 1;
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


def _host_returns(f, nptr, optional):
    """Every host-side return of a _seg form whose first nptr arguments are pointers, those at the
    indices `optional` allowed to be NULL."""
    L = R.lib()
    fake = [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(nptr)]
    ws, total, n = ctypes.c_void_p(0x100000), 1 << 20, 4
    need = int(L.rle_append_seg_workspace_bytes(n, total))
    assert f(*([None] * nptr), 0, 0, None, 0, None) == R.RLE_OK
    assert f(*fake, 0, total, ws, 0, None) == R.RLE_OK
    for k in range(nptr):
        if k in optional:
            continue
        args = list(fake)
        args[k] = None
        assert f(*args, n, total, ws, need, None) == R.RLE_E_INVAL, k
    assert f(*fake, n, total, None, need, None) == R.RLE_E_INVAL
    assert f(*fake, n, total, ws, 0, None) == R.RLE_E_INVAL
    assert f(*fake, n, total, ws, need - 1, None) == R.RLE_E_INVAL
    # the size asked for is the append's of this n and this total: the encode's is not enough
    assert f(*fake, n, total, ws, int(L.rle_seg_workspace_bytes(n, total)), None) == R.RLE_E_INVAL


def test_size_seg_host_side_returns_with_fake_pointers():
    """streams off len tail new new_off new_len need status: all required but the status."""
    _host_returns(R.lib().rle_append_size_batch_device_seg, 9, {8})


def test_fit_seg_host_side_returns_with_fake_pointers():
    """streams off len cap ulen tail new new_off new_len need status: d_ulen and d_status may be NULL."""
    _host_returns(R.lib().rle_append_fit_batch_device_seg, 11, {4, 10})


def test_one_wave_host_side_returns_with_fake_pointers():
    """n == 0 is RLE_OK whatever the pointers; a NULL required pointer, d_need among them, is
    RLE_E_INVAL before any launch."""
    L = R.lib()
    for f, nptr, optional in ((L.rle_append_size_batch_device, 9, {8}), (L.rle_append_fit_batch_device, 11, {4, 10})):
        fake = [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(nptr)]
        assert f(*([None] * nptr), 0, None) == R.RLE_OK
        assert f(*fake, 0, None) == R.RLE_OK
        for k in range(nptr):
            if k in optional:
                continue
            args = list(fake)
            args[k] = None
            assert f(*args, 4, None) == R.RLE_E_INVAL, k
