"""CPU tests of the host side of the eviction entries (include/rle_mi355x.h: rle_evict_select_device,
rle_evict_gather_device): the exports and their wrappers, the C99 declarations, and the returns that
are decided before anything is launched, so that fake pointers are enough.  No GPU."""
import ctypes
import os
import subprocess
import tempfile

import rle_mi355x as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(REPO, "include")
SYMS = ("rle_evict_select_device", "rle_evict_gather_device")
U64MAX = (1 << 64) - 1


def test_symbols_exported_and_wrapped():
    L = R.lib()
    for sym in SYMS:
        assert hasattr(L, sym), sym
    for name in ("evict_select", "evict_gather"):
        assert callable(getattr(R, name)), name
    assert (R.RLE_EVICT_SLOTS, R.RLE_EVICT_SUMMARY_WORDS, R.RLE_EVICT_ORDER_EVICTION, R.RLE_EVICT_ORDER_REPLY) == (1, 6, 0, 1)
    with open(os.path.join(INC, "rle_mi355x.h")) as f:
        text = f.read()
    for sym in SYMS:   # named in the capture paragraph ahead of the declarations, and declared
        assert text.count(sym) >= 2, sym
        assert text.index(sym) < text.index("#ifndef RLE_MI355X_H"), sym


def test_declarations_are_c99():
    """A C99 translation unit that includes the header, takes the two addresses with the documented
    types and uses the four constants links against the library (compiled and linked, not run)."""
    code = r'''
#include "rle_mi355x.h"
typedef int (*select_fn)(const uint64_t*, const uint64_t*, const uint64_t*, const uint32_t*, const uint32_t*, uint64_t,
                         uint32_t, uint32_t, uint32_t*, uint32_t*, uint64_t*, uint32_t, void*);
typedef int (*gather_fn)(const uint32_t*, const uint64_t*, uint32_t, const uint64_t* const*, uint64_t* const*, uint32_t,
                         uint32_t, void*);
select_fn take_select(void) { return rle_evict_select_device; }
gather_fn take_gather(void) { return rle_evict_gather_device; }
uint64_t summary[RLE_EVICT_SUMMARY_WORDS];
int main(void) {
    return take_select() != 0 && take_gather() != 0 && RLE_EVICT_SLOTS == 1u && RLE_EVICT_ORDER_EVICTION == 0u &&
                   RLE_EVICT_ORDER_REPLY == 1u && sizeof summary == 48 ? 0 : 1;
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


def _fake(k):
    return [ctypes.c_void_p(0x1000 * (j + 1)) for j in range(k)]


def test_select_host_side_returns_with_fake_pointers():
    """key len want live spare | max_bytes max_files flags | keep victims summary: a NULL d_summary
    (for n == 0 too: that call writes it, and its RLE_OK is checked on the device,
    tests/test_gpu_evict.py), with n > 0 a NULL d_key, d_len, d_keep or d_victims, an unknown flag bit
    and n past the launch bound are RLE_E_INVAL, whatever d_want, d_live and d_spare are."""
    f = R.lib().rle_evict_select_device

    def call(ptrs, n, flags=0, max_bytes=U64MAX, max_files=0):
        return f(*ptrs[:5], max_bytes, max_files, flags, *ptrs[5:], n, None)

    for k in (0, 1, 5, 6, 7):
        for optional in (False, True):
            args = _fake(8)
            args[k] = None
            if optional:
                args[2] = args[3] = args[4] = None
            assert call(args, 4) == R.RLE_E_INVAL, (k, optional)
    assert call([None] * 8, 0) == R.RLE_E_INVAL
    no_summary = _fake(8)
    no_summary[7] = None
    assert call(no_summary, 0) == R.RLE_E_INVAL
    for flags in (2, 4, 3, 0x100, 1 << 31, 0xFFFFFFFE):
        assert call(_fake(8), 4, flags) == R.RLE_E_INVAL, flags
        assert call(_fake(8), 0, flags) == R.RLE_E_INVAL, flags
    for flags in (0, R.RLE_EVICT_SLOTS):
        assert call(_fake(8), (1 << 30) + 1, flags) == R.RLE_E_INVAL
        assert call(_fake(8), 0xFFFFFFFF, flags, 0, 1) == R.RLE_E_INVAL


def _tables(k, null_at=None):
    a = (ctypes.c_void_p * 8)(*[0x100000 * (j + 1) for j in range(8)])
    if null_at is not None:
        a[null_at] = None
    return a


def test_gather_host_side_returns_with_fake_pointers():
    """victims summary | order | tables_in tables_out | ntables cap: a NULL argument, a NULL table
    pointer among the first ntables, ntables of 0 or above 8 and an unknown order are RLE_E_INVAL, for
    cap == 0 too; with good arguments cap == 0 is RLE_OK and launches nothing."""
    f = R.lib().rle_evict_gather_device
    v, s = _fake(2)
    tin, tout = _tables(8), _tables(8)
    for nt in range(1, 9):
        for order in (R.RLE_EVICT_ORDER_EVICTION, R.RLE_EVICT_ORDER_REPLY):
            assert f(v, s, order, tin, tout, nt, 0, None) == R.RLE_OK, (nt, order)
    for cap in (0, 5):
        assert f(None, s, 0, tin, tout, 1, cap, None) == R.RLE_E_INVAL
        assert f(v, None, 0, tin, tout, 1, cap, None) == R.RLE_E_INVAL
        assert f(v, s, 0, None, tout, 1, cap, None) == R.RLE_E_INVAL
        assert f(v, s, 0, tin, None, 1, cap, None) == R.RLE_E_INVAL
        for nt in (0, 9, 64, 0xFFFFFFFF):
            assert f(v, s, 0, tin, tout, nt, cap, None) == R.RLE_E_INVAL, nt
        for order in (2, 3, 0x100, 0xFFFFFFFF):
            assert f(v, s, order, tin, tout, 1, cap, None) == R.RLE_E_INVAL, order
        for nt in (1, 5, 8):
            for k in range(nt):
                assert f(v, s, 0, _tables(8, k), tout, nt, cap, None) == R.RLE_E_INVAL, (nt, k)
                assert f(v, s, 1, tin, _tables(8, k), nt, cap, None) == R.RLE_E_INVAL, (nt, k)
    # a NULL past the first ntables is not looked at
    assert f(v, s, 0, _tables(8, 5), _tables(8, 7), 5, 0, None) == R.RLE_OK
