"""CPU tests of the tail scan / in-place append model (tests/append_tail_model.py) against the
oracle, and of the host side of the new entry points (include/rle_mi355x.h): rle_append_slot_bytes,
the exports and the C99 declarations.  No GPU."""
import os
import subprocess
import tempfile

import numpy as np

import append_tail_model as M
import rle_mi355x as R
import rle_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(REPO, "include")
ALPHABETS = (b"ab", b"9", b"123456789", bytes(range(256)), b"\0a", b"\0", b"2", b"23")


def runs(rng, alpha, n, lo=1, hi=25):
    a = np.frombuffer(alpha, np.uint8)
    return np.repeat(rng.choice(a, n), rng.integers(lo, hi, n)).tobytes() if n else b""


def test_model_on_encoder_output():
    """6000 seeded cases over small alphabets (digits and 0x00 among them): the scan of encode(x)
    decodes to len(x), the append composition equals a whole re-encode, and it fits the slot."""
    rng = np.random.default_rng(20)
    for i in range(6000):
        alpha = ALPHABETS[i % len(ALPHABETS)]
        x = runs(rng, alpha, int(rng.integers(0, 60)))
        new = runs(rng, alpha, int(rng.integers(0, 30)))
        y = O.encode(x)
        tl = M.tail_of(y)
        assert tl is not None and tl[2] == len(x), (x, y, tl)
        got = M.append_expected(y, new)
        assert got == O.encode(x + new), (x, new)
        assert len(got) <= M.slot_bytes(len(y), len(new)), (x, new)
        # the carried form (nothing read but the tail word and y[t]) gives the same stream and tail
        assert M.append_carried(y, M.word_of(y), new) == (got, M.word_of(got)), (x, new)
        if y:
            t, r, _ = tl
            assert (t + 1 == len(y)) if r == 1 else (t + 3 == len(y) and y[t] == y[t + 1] and y[t + 2] == 0x30 + r)


def test_chain_carried_through_tails():
    """200 appends, each seeing only the carried tail word: the stream stays encode(total) and the
    carried word stays the scan's."""
    rng = np.random.default_rng(21)
    y, w, total = b"", 0, b""
    for i in range(200):
        alpha = ALPHABETS[(i // 7) % len(ALPHABETS)]
        new = runs(rng, alpha, int(rng.integers(0, 12)), 1, 14)
        y, w = M.append_carried(y, w, new)
        total += new
        assert y == O.encode(total), i
        assert w == (M.word_of(y) if y else 0), i
    assert M.tail_of(y)[2] == len(total)


def test_trailing_zero_literal():
    assert O.encode(b"a\0") == b"a\0"
    assert M.tail_of(O.encode(b"a\0")) == (1, 1, 2)
    assert M.tail_of(b"") == (0, 0, 0)


def test_model_refuses_bad_digits_and_cut_streams():
    for d in (b"1", b"0", b":", b"\x00", b"\xb2"):
        assert M.tail_of(b"xaa" + d) is None, d
        assert M.tail_of(b"xaa" + d + b"qq2") is None, d
    assert M.tail_of(b"xaa") is None          # cut after "v v"
    assert M.tail_of(b"aa") is None
    assert M.tail_of(b"xaa2") == (1, 2, 3)
    assert M.tail_of(b"aa2aa2") == (3, 2, 4)   # hand-made, accepted: not what the encoder emits for aaaa


def test_append_slot_bytes():
    f = R.append_slot_bytes
    assert f(0, 0) == 16 and f(1, 0) == 16
    assert [f(100, a) for a in (0, 1, 7, 8, 4096)] == [128, 128, 128, 128, 6272]
    for C in (0, 1, 15, 16, 17, 4095, 4096, 1 << 20):
        prev = 0
        for A in (0, 1, 2, 7, 8, 9, 15, 16, 17, 1007, 1008, 4096, 65536):
            v = f(C, A)
            assert v == M.slot_bytes(C, A) == ((C + R.max_compressed_size(A + 9) + 15) & ~15)
            assert v % 16 == 0 and v >= prev and v >= C + A
            prev = v
    for A in (0, 5, 4096):
        vals = [f(C, A) for C in range(0, 200)]
        assert vals == sorted(vals)
    big = R.RLE_MAX_BUFFER_BYTES
    assert f(big + 1, 0) == 0 and f(0, big + 1) == 0 and f(big, 0) == 0 and f(big // 2, big // 2) == 0
    assert f(1 << 40, 1) == 0 and f(1, 1 << 40) == 0
    assert f(big - 13, 0) == big          # C + 13 = the limit: the largest slot that is still allowed
    assert f(big - 12, 0) == 0


def test_new_symbols_exported_with_constants():
    L = R.lib()
    for sym in ("rle_append_slot_bytes", "rle_tail_batch_device", "rle_append_batch_device"):
        assert hasattr(L, sym), sym
    assert R.RLE_STATUS_NOTCANON == 0x1000 and R.RLE_TAIL_EMPTY == 0
    # n == 0 launches nothing whatever the pointers; null arrays are refused on the host
    assert L.rle_tail_batch_device(None, None, None, None, None, None, 0, None) == R.RLE_OK
    assert L.rle_append_batch_device(None, None, None, None, None, None, None, None, None, None, 0, None) == R.RLE_OK
    assert L.rle_tail_batch_device(None, None, None, None, None, None, 1, None) == R.RLE_E_INVAL
    assert L.rle_append_batch_device(None, None, None, None, None, None, None, None, None, None, 1,
                                     None) == R.RLE_E_INVAL
    assert R.tail_word(5, 3) == 5 | (3 << 32) and R.tail_offset(R.tail_word(5, 3)) == 5
    assert R.tail_count(R.tail_word(5, 3)) == 3


def test_new_declarations_are_c99():
    """The prototypes and the tail-word macros, checked by a C99 compiler (constant expressions: the
    program is compiled, not run)."""
    code = r'''
#include "rle_mi355x.h"
#define W (((uint64_t)7 << 32) | 1234u)
typedef char check_offset[RLE_TAIL_OFFSET(W) == 1234u ? 1 : -1];
typedef char check_count[RLE_TAIL_COUNT(W) == 7u ? 1 : -1];
typedef char check_empty[RLE_TAIL_EMPTY == 0 ? 1 : -1];
typedef char check_status[RLE_STATUS_NOTCANON == 0x1000u ? 1 : -1];
int main(void) {
    size_t (*a)(uint64_t, uint64_t) = rle_append_slot_bytes;
    int (*b)(const void*, const uint64_t*, const uint64_t*, uint64_t*, uint64_t*, uint32_t*, uint32_t, void*) =
        rle_tail_batch_device;
    int (*c)(void*, const uint64_t*, uint64_t*, const uint64_t*, uint64_t*, uint64_t*, const void*, const uint64_t*,
             const uint64_t*, uint32_t*, uint32_t, void*) = rle_append_batch_device;
    (void)a; (void)b; (void)c;
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "t.c")
        with open(p, "w") as f:
            f.write(code)
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INC, "-c", p, "-o",
                            os.path.join(d, "t.o")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
