"""Host models of the eviction selection (include/rle_mi355x.h: rle_evict_select_device,
rle_evict_gather_device; csrc/rle_evict.h).  No GPU.

loop_model(): the reference restated literally: while over a limit, getVictim's scan of the list for
the smallest key with a strict `<`, skipping the spare; the victim removed, its size subtracted, its
index appended to the eviction order.  (fast=True replaces only the scan, by ArgminScan.)

select_model(): the kernel's own route to the same answer: totals, the byte-wise weighted radix select
of the threshold key with both needs, the index-order scan over the ties, compaction in index order,
then the sort.

bitonic_model(): the sort's network on a list of m (key, index) pairs, padded to the next power of two
by virtual +inf entries.

Both selections return a Result: status, victims (eviction order), keep, summary (the six words)."""
from collections import namedtuple

import numpy as np

M64 = (1 << 64) - 1
MAXB = 0x7FFFFFF0   # RLE_MAX_BUFFER_BYTES
OK, TOOLARGE, NOFIT = 0, 4, 0x2000
SLOTS = 1           # RLE_EVICT_SLOTS
BLOCK = 1024        # the workgroup: the stride of the kernel's scans
ORDER_EVICTION, ORDER_REPLY = 0, 1

Result = namedtuple("Result", "status victims keep summary")


def files(keys, lens, wants=None, live=None, spare=None, flags=0):
    """Per file (key, size, live, eligible, too large), by the header's definitions; the sizes in
    64-bit wrapping arithmetic (they wrap only where TOOLARGE refuses the call)."""
    out = []
    for i, (k, c) in enumerate(zip(keys, lens)):
        m = max(wants[i] if wants is not None else 0, c)
        lv = live is None or live[i] != 0
        el = lv and not (spare is not None and spare[i] != 0)
        size = 0 if not lv else ((m + 15) & ~15 & M64) if flags & SLOTS else m
        out.append((k, size, lv, el, lv and m > MAXB))
    return out


def refusal(status, fs):
    b = sum(f[1] for f in fs) & M64
    c = sum(1 for f in fs if f[2])
    return Result(status, [], [int(f[2]) for f in fs], [status, 0, b, b, c, c])


def over(b, c, max_bytes, max_files):
    return b > max_bytes or (max_files != 0 and c > max_files)


def get_victim(fs, stored):
    """getVictim (src/filesystemApi.c:51-60): the scan of the list for the smallest key."""
    victim = None
    for i in stored:
        if fs[i][3] and (victim is None or fs[i][0] < fs[victim][0]):   # (strict: the first in list order wins)
            victim = i
    return victim


class ArgminScan:
    """get_victim for the stores of thousands of files that the GPU tests compare with: the eligible
    files' keys in list order in a numpy array, of which argmin returns the first of equal minima (the
    strict `<`).  tests/test_evict_model.py holds it to get_victim."""

    def __init__(self, fs, stored):
        self.idx = np.array([i for i in stored if fs[i][3]], dtype=np.int64)
        self.key = np.array([fs[i][0] for i in self.idx], dtype=np.uint64)

    def victim(self):
        if self.idx.size == 0:
            return None
        j = int(np.argmin(self.key))
        v = int(self.idx[j])
        self.idx, self.key = np.delete(self.idx, j), np.delete(self.key, j)
        return v


def loop_model(keys, lens, wants=None, live=None, spare=None, max_bytes=M64, max_files=0, flags=0, fast=False):
    fs = files(keys, lens, wants, live, spare, flags)
    if any(f[4] for f in fs):
        return refusal(TOOLARGE, fs)
    stored = [i for i, f in enumerate(fs) if f[2]]                  # the list, in list order
    b0 = b = sum(fs[i][1] for i in stored)                          # currStorageSize
    c0 = len(stored)
    victims = []
    scan = ArgminScan(fs, stored) if fast else None
    while over(b, len(stored), max_bytes, max_files):               # src/filesystemApi.c:784, :477
        victim = scan.victim() if fast else get_victim(fs, stored)
        if victim is None:                                          # :787 assert(victim); :777-782 E2BIG
            return refusal(NOFIT, fs)
        stored.remove(victim)                                       # :789 destroyFile
        b -= fs[victim][1]
        victims.append(victim)                                      # :792-793 (the list itself is built reversed)
    gone = set(victims)
    keep = [int(f[2] and i not in gone) for i, f in enumerate(fs)]
    return Result(OK, victims, keep, [OK, len(victims), b0, b, c0, c0 - len(victims)])


def covers(b, c, need_b, need_c):
    return b >= need_b and c >= need_c


def bitonic_model(pairs):
    """The network of csrc/rle_evict.h's evict_bitonic on a copy of `pairs`: ascending comparators only,
    each merge opening with the flip i <-> i ^ (k - 1); a pair whose upper partner is at or past m (a
    virtual +inf) is skipped."""
    a, m = list(pairs), len(pairs)
    pow2 = 1
    while pow2 < m:
        pow2 <<= 1
    k = 2
    while k <= pow2:
        j = k >> 1
        while j:
            for i in range(m):
                l = i ^ (k - 1) if j == k >> 1 else i ^ j
                if i < l < m and a[l] < a[i]:
                    a[i], a[l] = a[l], a[i]
            j >>= 1
        k <<= 1
    return a


def select_model(keys, lens, wants=None, live=None, spare=None, max_bytes=M64, max_files=0, flags=0):
    fs = files(keys, lens, wants, live, spare, flags)
    n = len(fs)
    # 1. the totals
    lb, lc = sum(f[1] for f in fs) & M64, sum(1 for f in fs if f[2])
    eb, ec = sum(f[1] for f in fs if f[3]) & M64, sum(1 for f in fs if f[3])
    need_b = lb - max_bytes if lb > max_bytes else 0
    need_c = lc - max_files if max_files != 0 and lc > max_files else 0
    if any(f[4] for f in fs):
        return refusal(TOOLARGE, fs)
    if not covers(eb, ec, need_b, need_c):
        return refusal(NOFIT, fs)
    if need_b == 0 and need_c == 0:
        return Result(OK, [], [int(f[2]) for f in fs], [OK, 0, lb, lb, lc, lc])
    # 2. the threshold key: from the first byte the eligible keys do not share
    k_or, k_and = 0, M64
    for f in fs:
        if f[3]:
            k_or, k_and = k_or | f[0], k_and & f[0]
    differ = k_or ^ k_and
    p = (differ.bit_length() - 1) >> 3 if differ else -1
    prefix = k_and >> (8 * (p + 1)) << (8 * (p + 1))
    while p >= 0:
        sh = 8 * p
        hb, hc = [0] * 256, [0] * 256
        for f in fs:
            if f[3] and f[0] >> (sh + 8) == prefix >> (sh + 8):
                hb[(f[0] >> sh) & 255] += f[1]
                hc[(f[0] >> sh) & 255] += 1
        sb = sc = 0
        picked = []
        for t in range(256):
            if covers(sb + hb[t], sc + hc[t], need_b, need_c) and not covers(sb, sc, need_b, need_c):
                picked.append((t, max(need_b - sb, 0), max(need_c - sc, 0)))
            sb, sc = sb + hb[t], sc + hc[t]
        assert len(picked) == 1, picked    # (one thread writes the pick)
        t, need_b, need_c = picked[0]
        prefix |= t << sh
        p -= 1
    assert need_b > 0 or need_c > 0
    # 3. the last file taken among the ties, in strides of the workgroup with the early exit
    cb = cc = 0
    last = []
    for i0 in range(0, n, BLOCK):
        for i in range(i0, min(n, i0 + BLOCK)):
            if fs[i][3] and fs[i][0] == prefix:
                if covers(cb + fs[i][1], cc + 1, need_b, need_c) and not covers(cb, cc, need_b, need_c):
                    last.append(i)
                cb, cc = cb + fs[i][1], cc + 1
        if covers(cb, cc, need_b, need_c):
            break
    assert len(last) == 1, last
    # 4. compaction in index order
    victims = [i for i, f in enumerate(fs) if f[3] and (f[0] < prefix or (f[0] == prefix and i <= last[0]))]
    gone = sum(fs[i][1] for i in victims)
    keep = [int(f[2]) for f in fs]
    for i in victims:
        keep[i] = 0
    # 5. eviction order
    victims = [i for _, i in bitonic_model([(fs[i][0], i) for i in victims])]
    m = len(victims)
    return Result(OK, victims, keep, [OK, m, lb, lb - gone, lc, lc - m])


def gather(victims, m, order, tables, outs, cap):
    """rle_evict_gather_device on lists: outs (as they are before the call) with rows [0, min(m, cap))
    of every table replaced."""
    res = [list(o) for o in outs]
    for j in range(min(m, cap)):
        v = victims[m - 1 - j] if order == ORDER_REPLY else victims[j]
        for t, o in zip(tables, res):
            o[j] = t[v]
    return res


# ---------------------------------------------------------------- the stores the tests share
def store(keys, lens, wants=None, live=None, spare=None, max_bytes=M64, max_files=0, flags=0):
    return dict(keys=list(keys), lens=list(lens), wants=None if wants is None else list(wants),
                live=None if live is None else list(live), spare=None if spare is None else list(spare),
                max_bytes=max_bytes, max_files=max_files, flags=flags)


def totals(s):
    """(bytes, live files, eligible bytes, eligible files) of a store."""
    fs = files(s["keys"], s["lens"], s["wants"], s["live"], s["spare"], s["flags"])
    return (sum(f[1] for f in fs), sum(1 for f in fs if f[2]), sum(f[1] for f in fs if f[3]),
            sum(1 for f in fs if f[3]))


def prefix_bytes(s, count):
    """The bytes of the first `count` files of the eviction order."""
    fs = files(s["keys"], s["lens"], s["wants"], s["live"], s["spare"], s["flags"])
    order = sorted((f[0], i) for i, f in enumerate(fs) if f[3])
    return sum(fs[i][1] for _, i in order[:count])


def edges(n=130):
    """The named edges: {name: store}.  n >= 64."""
    lens = [100 + (i * 7919) % 2900 for i in range(n)]
    wants = [c + (i % 3) * 50 for i, c in enumerate(lens)]
    live = [int(i % 11 != 3) for i in range(n)]
    spare = [int(i % 13 == 5) for i in range(n)]
    mixed = [0x5F00000000 + (i * 37) % 101 * 1000 for i in range(n)]          # timestamps: ties, shared top bytes
    distinct = [0x5F00000000 + (i * 37) % n for i in range(n)]                # a permutation: no ties
    e = {}

    def add(name, keys, count=None, **kw):
        """A store with max_bytes set so that exactly the first `count` files of the order go."""
        s = store(keys, kw.pop("lens", lens), kw.pop("wants", wants), kw.pop("live", live), kw.pop("spare", spare), **kw)
        if count is not None:
            s["max_bytes"] = totals(s)[0] - prefix_bytes(s, count)
        e[name] = s
        return s

    add("all keys equal", [5] * n, n // 3)
    add("top byte only", [((i * 37) % 251) << 56 for i in range(n)], n // 3)
    add("bottom byte only", [0x1122334455667700 + (i * 37) % 256 for i in range(n)], n // 3)
    add("keys 0 and 2^64-1", [0 if i % 3 else M64 for i in range(n)], 2 * n // 3)
    # the files of the lowest bins of the one differing byte, whole: the excess ends at a bin edge
    s = add("exact at a bin edge", [0x7700 + (i % 8) for i in range(n)])
    fs = files(s["keys"], s["lens"], s["wants"], s["live"], s["spare"])
    s["max_bytes"] = totals(s)[0] - sum(f[1] for f in fs if f[3] and f[0] < 0x7703)
    s = add("exact at a file edge", mixed, 17)
    add("one byte more", mixed, max_bytes=s["max_bytes"] - 1)
    add("ties straddle the cut", [9 if i % 2 else 3 + i % 4 for i in range(n)], n // 2 + 9)
    sp = list(spare)
    sp[distinct.index(min(distinct))] = 1
    lv = list(live)
    lv[distinct.index(min(distinct))] = 1
    add("smallest key spared", distinct, 5, live=lv, spare=sp)
    s = add("files limit decides", mixed)
    s["max_files"] = totals(s)[1] - 7
    s = add("bytes limit decides", mixed, 20)
    s["max_files"] = totals(s)[1] - 2
    big_first = [50000 if distinct[i] - 0x5F00000000 < 3 else 10 for i in range(n)]
    s = add("both bind, files later", distinct, 2, lens=big_first, wants=None, live=None, spare=None)
    s["max_files"] = n - 12
    small_first = [1 if distinct[i] - 0x5F00000000 < 12 else 4000 for i in range(n)]
    s = add("both bind, bytes later", distinct, 20, lens=small_first, wants=None, live=None, spare=None)
    s["max_files"] = n - 5
    add("fits", mixed, 0)
    add("fits with a files limit", mixed, 0, max_files=n)
    s = add("all eligible evicted", mixed)
    s["max_bytes"] = totals(s)[0] - totals(s)[2]
    s = add("NOFIT by bytes", mixed)
    s["max_bytes"] = totals(s)[0] - totals(s)[2] - 1
    s = add("NOFIT by count", mixed)
    s["max_files"] = totals(s)[1] - totals(s)[3] - 1
    w = list(wants)
    w[n // 2 + (0 if live[n // 2] else 1)] = MAXB + 1
    add("TOOLARGE", mixed, max_bytes=1000, wants=w)
    dead_low = [i if not live[i] else 1000 + (i * 37) % 50 for i in range(n)]
    add("dead files hold the smallest keys", dead_low, 9)
    s = add("exact bytes", distinct, lens=[17] * n, wants=None)
    s["max_bytes"] = totals(s)[0] - 40
    add("RLE_EVICT_SLOTS changes the last file", distinct, lens=[17] * n, wants=None, max_bytes=s["max_bytes"], flags=SLOTS)
    return e


def random_store(rng, n):
    """A seeded random store of n files (rng: numpy Generator): mixed masks, wants, limits and flags."""
    kind = int(rng.integers(0, 5))
    if kind == 0:
        keys = rng.integers(0, 4, n)                                        # heavy ties
    elif kind == 1:
        keys = 0x60000000 + rng.integers(0, 1 << 20, n)                     # timestamps
    elif kind == 2:
        keys = rng.integers(0, 1 << 63, n) * 2 + rng.integers(0, 2, n)      # all 64 bits
    elif kind == 3:
        keys = rng.integers(0, 3, n) << 56 | rng.integers(0, 3, n)          # top and bottom bytes
    else:
        keys = rng.integers(0, max(2, n // 4), n) << 8 * int(rng.integers(0, 8))
    keys = [int(k) & M64 for k in keys]
    lens = [int(c) for c in rng.integers(0, 5000, n)]
    wants = [int(c) for c in rng.integers(0, 6000, n)] if rng.integers(0, 2) else None
    live = [int(x) for x in rng.integers(0, 5, n) != 0] if rng.integers(0, 2) else None
    spare = [int(x) for x in rng.integers(0, 8, n) == 0] if rng.integers(0, 2) else None
    s = store(keys, lens, wants, live, spare, flags=int(rng.integers(0, 2)))
    b, c, _, ec = totals(s)
    mode = int(rng.integers(0, 4))
    if mode != 1:
        s["max_bytes"] = int(rng.integers(0, b + b // 8 + 2))
    if mode != 0:
        s["max_files"] = int(rng.integers(max(1, c - ec - 1), c + 3))
    return s
