"""CPU tests of the host side of the relocation entries (include/rle_mi355x.h: rle_relocate_span_bytes,
rle_relocate_layout_device, rle_relocate_batch_device): the exports, the C99 declarations, and the
returns that are decided before anything is launched, so that fake pointers are enough.  No GPU."""
import ctypes
import os
import subprocess
import tempfile

import relocate_model as M
import rle_mi355x as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(REPO, "include")
SYMS = ("rle_relocate_span_bytes", "rle_relocate_layout_device", "rle_relocate_batch_device")


def test_symbols_exported_and_wrapped():
    L = R.lib()
    for sym in SYMS:
        assert hasattr(L, sym), sym
    for name in ("relocate_span_bytes", "relocate_layout", "relocate_batch"):
        assert callable(getattr(R, name)), name
    with open(os.path.join(INC, "rle_mi355x.h")) as f:
        text = f.read()
    for sym in SYMS:
        assert text.count(sym) >= 2, sym
    for sym in SYMS[1:]:   # the two that launch: named in the capture paragraph ahead of the declarations
        assert text.index(sym) < text.index("#ifndef RLE_MI355X_H"), sym


def test_declarations_are_c99():
    """A C99 translation unit that includes the header and takes the three addresses with the
    documented types links against the library (compiled and linked, not run)."""
    code = r'''
#include "rle_mi355x.h"
typedef uint64_t (*span_fn)(uint64_t);
typedef int (*layout_fn)(const uint64_t*, const uint64_t*, const uint32_t*, uint64_t, uint64_t*, uint64_t*, uint64_t*,
                         uint32_t, void*);
typedef int (*batch_fn)(const void*, const uint64_t*, const uint64_t*, const uint64_t*, const uint32_t*, void*, uint64_t,
                        uint64_t, uint64_t*, uint64_t*, uint64_t*, uint32_t*, uint32_t, void*);
span_fn take_span(void) { return rle_relocate_span_bytes; }
layout_fn take_layout(void) { return rle_relocate_layout_device; }
batch_fn take_batch(void) { return rle_relocate_batch_device; }
int main(void) { return take_span() != 0 && take_layout() != 0 && take_batch() != 0 ? 0 : 1; }
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


def test_layout_host_side_returns_with_fake_pointers():
    """len want sel | dst_base | new_off new_cap total: a NULL d_total, or with n > 0 a NULL d_len,
    d_new_off or d_new_cap, a dst_base that is not a multiple of 16 and n past the launch bound are
    RLE_E_INVAL; d_total is needed for n == 0 too, which writes it (that write is a launch: its RLE_OK
    is checked on the device, tests/test_gpu_relocate.py)."""
    f = R.lib().rle_relocate_layout_device

    def call(ptrs, n, base=0):
        return f(*ptrs[:3], base, *ptrs[3:], n, None)

    for k in (0, 3, 4, 5):
        args = _fake(6)
        args[k] = None
        assert call(args, 4) == R.RLE_E_INVAL, k
    args = _fake(6)
    args[1] = args[2] = args[5] = None   # (NULL wants and masks do not excuse a NULL total)
    assert call(args, 4) == R.RLE_E_INVAL
    assert call([None] * 6, 0) == R.RLE_E_INVAL
    for base in (1, 8, 15, 17, (1 << 40) + 4):
        assert call(_fake(6), 4, base) == R.RLE_E_INVAL, base
        assert call(_fake(6), 0, base) == R.RLE_E_INVAL, base
    assert call(_fake(6), (1 << 30) + 1) == R.RLE_E_INVAL


def test_batch_host_side_returns_with_fake_pointers():
    """src off len want sel dst | dst_base dst_cap | new_off new_cap total status: n == 0 without a
    d_total is RLE_OK and launches nothing; a NULL d_src, d_off, d_len, d_dst, d_new_off, d_new_cap or
    d_total, a misaligned d_dst, dst_base & 15 and dst_base > dst_cap are RLE_E_INVAL whatever d_want,
    d_sel and d_status are."""
    f = R.lib().rle_relocate_batch_device

    def call(ptrs, n, base=0, cap=1 << 20):
        return f(*ptrs[:6], base, cap, *ptrs[6:], n, None)

    assert call([None] * 10, 0) == R.RLE_OK
    none_total = _fake(10)
    none_total[8] = None
    assert call(none_total, 0) == R.RLE_OK
    for k in (0, 1, 2, 5, 6, 7, 8):
        for optional in (False, True):
            args = _fake(10)
            args[k] = None
            if optional:
                args[3] = args[4] = args[9] = None
            assert call(args, 4) == R.RLE_E_INVAL, (k, optional)
    for low in (1, 4, 8, 15):
        args = _fake(10)
        args[5] = ctypes.c_void_p(0x6000 + low)
        assert call(args, 4) == R.RLE_E_INVAL, low
    for base in (1, 8, 15, 4097):
        assert call(_fake(10), 4, base) == R.RLE_E_INVAL, base
    assert call(_fake(10), 4, 32, 16) == R.RLE_E_INVAL
    assert call(_fake(10), 4, 1 << 21, 1 << 20) == R.RLE_E_INVAL
    assert call(_fake(10), (1 << 30) + 1) == R.RLE_E_INVAL


def test_span_bytes():
    """A multiple of 16 KiB, at least 16 KiB, monotone in the room; the model's rule for the device's
    CU count (256 assumed without a device)."""
    f = R.relocate_span_bytes
    rooms = sorted(set(list(range(0, 4 << 20, 65521)) + [1, 16384, 16385, 1 << 25, (1 << 25) + 1, 1 << 30, 1 << 34,
                                                         (1 << 40) + 7, (1 << 64) - 1]))
    spans = [f(r) for r in rooms]
    for r, s in zip(rooms, spans):
        assert s % 16384 == 0 and s >= 16384, (r, s)
        assert s * 8 * 1024 >= r, (r, s)   # (no device has more CUs: the grid covers the room)
    assert spans == sorted(spans)
    assert f(0) == 16384 and f(16384) == 16384
    if R.device_count() == 0:
        assert spans == [M.span_bytes(r) for r in rooms]
