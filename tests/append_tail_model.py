"""CPU model of the tail scan and the in-place append (include/rle_mi355x.h:
rle_tail_batch_device, rle_append_batch_device), for the tests.

tail_of(stream) is the documented parse, byte for byte.  append_expected(stream, new) is the
documented result y[0, t) ‖ encode(c^r ‖ new), built on the oracle's encode."""
import functools

import rle_oracle as O

NOTCANON = 0x1000
MISALIGNED = 2
TOOLARGE = 4
MAX_BUFFER_BYTES = 0x7FFFFFF0


@functools.lru_cache(maxsize=4096)
def tail_of(stream):
    """(t, r, U) of a stream the scan accepts -- offset and count of its final token, decoded length
    -- (0, 0, 0) for the empty stream, None where the scan answers NOTCANON."""
    y, C = bytes(stream), len(stream)
    j = t = r = U = 0
    while j < C:
        if j + 1 < C and y[j] == y[j + 1]:
            if j + 2 >= C or not (0x32 <= y[j + 2] <= 0x39):
                return None
            t, r = j, y[j + 2] - 0x30
            U += r
            j += 3
        else:
            t, r = j, 1
            U += 1
            j += 1
    return t, r, U


def tail_word(t, r):
    return t | (r << 32)


def word_of(stream):
    """The tail word of an accepted stream (0 for the empty one)."""
    t, r, _ = tail_of(stream)
    return tail_word(t, r)


def append_expected(stream, new):
    """The slot's content after an accepted append of `new`."""
    y = bytes(stream)
    if not y:
        return O.encode(bytes(new))
    t, r, _ = tail_of(y)
    return y[:t] + O.encode(bytes([y[t]]) * r + bytes(new))


def append_carried(stream, word, new):
    """An accepted append that looks at nothing but the tail word and y[t]: (new stream, new tail
    word).  The new tail comes from the final run of c^r ‖ new alone (a run of L bytes ends in a
    token of (L - 1) % 9 + 1), the way the kernel derives it."""
    y, new = bytes(stream), bytes(new)
    if not new:
        return y, word
    t, r = word & 0xFFFFFFFF, (word >> 32) & 0xF
    v = (bytes([y[t]]) * r if y else b"") + new
    out = (y[:t] if y else b"") + O.encode(v)
    L = 1
    while L < len(v) and v[-1 - L] == v[-1]:
        L += 1
    rn = (L - 1) % 9 + 1
    return out, tail_word(len(out) - (1 if rn == 1 else 3), rn)


def slot_bytes(C, A):
    """rle_append_slot_bytes restated: C + max_compressed_size(A + 9), rounded up to 16; 0 past the limit."""
    if C > MAX_BUFFER_BYTES or A > MAX_BUFFER_BYTES:
        return 0
    s = (C + (A + 9) + (A + 9) // 2 + 15) & ~15
    return 0 if s > MAX_BUFFER_BYTES else s
