"""CPU model of the append's size and fit entries (include/rle_mi355x.h:
rle_append_size_batch_device, rle_append_fit_batch_device and their _seg forms), on top of
append_tail_model.py and append_seg_model.py: the exact new length, the fit decision, and the new
length as the segmented forms compose it from their per-segment summaries.  The case generators at
the end are shared by the CPU and the GPU tests."""
import append_seg_model as A
import append_tail_model as M
import rle_oracle as O

NOFIT = 0x2000
TILE = 1008


def need(y, word, new):
    """d_need of an accepted file: the length the append would leave (C when there is nothing to
    append)."""
    return len(M.append_carried(y, word, new)[0])


def word_ok(y, word):
    """The tail word describes the stream's last bytes (the check of app_accept)."""
    y, C = bytes(y), len(y)
    if word == 0:
        return C == 0
    t, r = word & 0xFFFFFFFF, (word >> 32) & 0xFFFFFFFF
    if (word >> 36) or not 1 <= r <= 9 or C != t + (1 if r == 1 else 3):
        return False
    return r == 1 or (y[t + 1] == y[t] and y[t + 2] == 0x30 + r)


def decide(y, word, new, cap=None, addr_ok=True):
    """(status, d_need) of one file, the checks in the documented order.  cap None: a size entry."""
    C, An = len(y), len(new)
    bad = 0 if M.slot_bytes(C, An) else M.TOOLARGE
    if not addr_ok:
        bad |= M.MISALIGNED
    if not bad and not word_ok(y, word):
        bad = M.NOTCANON
    if bad:
        return bad, 0
    if An == 0:
        return 0, C
    c = need(y, word, new)
    return (NOFIT if cap is not None and cap < c else 0), c


def fit(y, word, new, cap):
    """(status, d_need, stream afterwards, tail word afterwards) of a fit entry on a file whose
    addresses are aligned."""
    st, c = decide(y, word, new, cap)
    if st or not new:
        return st, c, bytes(y), word
    out, w = M.append_carried(y, word, new)
    return 0, c, out, w


def need_seg(y, word, new, sb):
    """C' as the segmented forms compose it: the scan of append_seg_model over segments of sb bytes,
    entered with the append's state, summing each segment's entering piece and rest."""
    y, new = bytes(y), bytes(new)
    if not new:
        return len(y)
    c, r, e, vs, t = A.entry(y, word, new)
    V = A.virtual(c, vs, new)
    segs = [(vs + a, vs + b) for a, b in A.seg_cut(len(new), sb)]
    plan, Cn, _ = A.scan(V, vs, r, e, t, segs)
    assert plan[0][1] == (t + (1 if r + e == 1 else 3) if vs else 0)
    assert Cn == plan[-1][1] + plan[-1][2]
    return Cn


# ---------------------------------------------------------------- shared cases
A_SWEEP = (1, 15, 16, 17, 1007, 1008, 1009, 1023, 1024, 1025, 2016, 3029)
KINDS = ("random", "runs50", "zero", "run")


def literals(n, a=b"x", b=b"y"):
    return (a + b) * (n // 2) + (a if n & 1 else b"")


def new_of(kind, An, c, seed):
    if kind == "random":
        return O.gen(1, seed, An)
    if kind == "runs50":
        return O.gen(2, seed, An)
    if kind == "zero":
        return bytes(An)
    return bytes([c]) * An   # "run": continues the old final run


def splice_grid():
    """(x, y, new) of tests/test_gpu_append_batch.py's splice grid: x = p literals ‖ c^L, every t mod
    16, every final count r with and without full 9-chunks before it, three bytes, and new bytes that
    leave the run, continue it short of 9, to 9, past 9 and far past it."""
    out = []
    for p in list(range(16)) + list(range(2000, 2016)):
        for r in range(1, 10):
            for L in (r, 9 + r):
                for c in (0x61, 0x39, 0x00):
                    cb = bytes([c])
                    x = literals(p) + cb * L
                    y = O.encode(x)
                    for new in (b"", cb, cb * (9 - r), cb * (9 - r + 1), cb * 17, b"k", cb * 3 + b"77"):
                        out.append((x, y, new))
    return out


def a_sweep(lengths=A_SWEEP):
    """(x, y, new) of its A sweep: four kinds after "aa3" at t mod 16 in {0, 7, 15}, after a final
    0x00 literal, and appended to empty streams; and one empty append to an empty stream."""
    out = []
    for An in lengths:
        for kind in KINDS:
            for p in (32, 39, 47):
                x = literals(p) + b"aaa"
                out.append((x, O.encode(x), new_of(kind, An, 0x61, 11 * An + p)))
            x = literals(47) + b"\0"
            out.append((x, O.encode(x), new_of(kind, An, 0, An)))
    for An in lengths:
        for kind in KINDS:
            out.append((b"", b"", new_of(kind, An, 0x62, 7 * An)))
    out.append((b"", b"", b""))
    return out


def seg_edge_lengths(sb):
    """The segmented tests' A sweep around the edges of segments of sb bytes."""
    return (1, 2, 3, sb - 1, sb, sb + 1, sb + 3, 2 * sb - 1, 2 * sb, 2 * sb + 3, 5 * sb + 17)


def stored_token(count, p=40):
    """(x, y): p literals and a final token of `count` bytes 'a'."""
    x = literals(p) + b"a" * count
    return x, O.encode(x)
