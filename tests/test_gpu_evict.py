"""GPU tests: rle_evict_select_device and rle_evict_gather_device against the reference's loop
(tests/evict_model.py: loop_model), word for word.  Every output buffer is allocated with guard words
on both sides and pre-filled with a pattern, and the whole buffer is compared: d_victims[m, n) and the
guards stay as they were, and d_victims is wholly untouched after a refusal."""
import numpy as np
import pytest
import torch

import evict_model as M
import rle_mi355x as R
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu
GUARD = 8
PAT32 = 0x5A5A5A5A
PAT64 = 0x5A5A5A5A5A5A5A5A
EDGES = M.edges(130)


def u64(vals):
    """Unsigned 64-bit words as the int64 device tensor the wrappers take."""
    return torch.from_numpy(np.asarray(vals, dtype=np.uint64).view(np.int64)).to(DEV)


def i32(vals):
    return torch.tensor(np.asarray(vals, dtype=np.int64).astype(np.int32), device=DEV)


class Guarded:
    """`count` words between two guards, the whole buffer filled with a pattern; .t is what a call gets."""

    def __init__(self, count, dtype):
        self.pat = PAT32 if dtype == torch.int32 else PAT64
        self.count = count
        self.buf = torch.full((count + 2 * GUARD,), self.pat, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + count]

    def fill(self):
        self.buf.fill_(self.pat)

    def expect(self, head):
        """The whole buffer holds `head` in its first words behind the guard and the pattern elsewhere."""
        want = [self.pat] * GUARD + [int(x) for x in head] + [self.pat] * (self.count - len(head) + GUARD)
        got = self.buf.cpu().numpy()
        got = got.view(np.uint32 if got.dtype == np.int32 else np.uint64).tolist()
        assert got == want


class Store:
    """A store's arrays on the device with guarded outputs; select() runs one call and compares every
    output with loop_model's."""

    def __init__(self, n):
        self.n = n
        self.key, self.len, self.want = (torch.zeros(n, dtype=torch.int64, device=DEV) for _ in range(3))
        self.live, self.spare = (torch.zeros(n, dtype=torch.int32, device=DEV) for _ in range(2))
        self.keep, self.victims = Guarded(n, torch.int32), Guarded(n, torch.int32)
        self.summary = Guarded(R.RLE_EVICT_SUMMARY_WORDS, torch.int64)

    def load(self, s):
        self.s = s
        self.key.copy_(u64(s["keys"]))
        self.len.copy_(u64(s["lens"]))
        for name, t, conv in (("wants", self.want, u64), ("live", self.live, i32), ("spare", self.spare, i32)):
            if s[name] is not None:
                t.copy_(conv(s[name]))
        for g in (self.keep, self.victims, self.summary):
            g.fill()

    def launch(self, stream=None):
        s = self.s
        opt = lambda t, vals: t if vals is not None else None   # noqa: E731
        R.evict_select(self.key, self.len, self.keep.t, self.victims.t, self.summary.t, want=opt(self.want, s["wants"]),
                       live=opt(self.live, s["live"]), spare=opt(self.spare, s["spare"]), max_bytes=s["max_bytes"],
                       max_files=s["max_files"], flags=s["flags"], stream=stream)

    def check(self):
        r = M.loop_model(**self.s, fast=self.n > 300)
        self.summary.expect(r.summary)
        self.keep.expect(r.keep)
        self.victims.expect(r.victims)
        return r

    def select(self, s):
        self.load(s)
        self.launch()
        torch.cuda.synchronize()
        return self.check()


def shape_store(n, seed):
    """n files with timestamp keys (ties among them), wants, and from 63 files on dead and spared ones."""
    rng = np.random.default_rng(seed)
    keys = [int(k) for k in 0x6530000000 + rng.integers(0, max(2, n // 2), n) * 977]
    lens = [int(c) for c in rng.integers(0, 5000, n)]
    wants = [int(c) for c in rng.integers(0, 6000, n)]
    masks = n >= 63
    live = [int(i % 11 != 3) for i in range(n)] if masks else None
    spare = [int(i % 13 == 5) for i in range(n)] if masks else None
    return M.store(keys, lens, wants, live, spare, flags=seed & 1)


def with_count(s, count, by_files=False):
    """The store with limits under which exactly the first `count` files of the order go."""
    s = dict(s)
    b, c, _, _ = M.totals(s)
    if by_files:
        s["max_files"], s["max_bytes"] = c - count, M.M64
        assert count < c     # (max_files == 0 would be no limit)
    else:
        s["max_bytes"], s["max_files"] = b - M.prefix_bytes(s, count), 0
    return s


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4096, 4097, 5000])
def test_shapes(n):
    """For each n, limits that give m = 0, 1, about n / 3 and every eligible file; the bytes limit
    decides, and where the store keeps a file, the files limit once more."""
    base = shape_store(n, 100 + n)
    eligible = M.totals(base)[3]
    st = Store(n)
    for count in sorted({0, 1, max(1, n // 3), eligible}):
        for by_files in (False, True):
            if by_files and count >= M.totals(base)[1]:
                continue
            s = with_count(base, count, by_files)
            r = st.select(s)
            assert r.status == M.OK and r.summary[3] <= s["max_bytes"]
            # (by bytes, files of no bytes at the cut stay: the shortest prefix)
            assert len(r.victims) == count if by_files else len(r.victims) <= count, (n, count)


@pytest.mark.parametrize("m", [4096, 4097])
def test_sort_edge(m):
    """n = 5000 with m at the edge between the sort in LDS and the sort over d_victims."""
    base = shape_store(5000, 77)
    r = Store(5000).select(with_count(base, m, by_files=True))
    assert len(r.victims) == m and r.status == M.OK


@pytest.mark.parametrize("name", sorted(EDGES))
def test_named_edge(name):
    """The model test's named edges at n = 130, as they are and without each optional array."""
    st = Store(130)
    full = EDGES[name]
    st.select(full)
    for drop in ("wants", "live", "spare"):
        if full[drop] is not None:
            st.select(dict(full, **{drop: None}))


def test_refusals_leave_victims_untouched():
    st = Store(130)
    for name, status in (("NOFIT by bytes", M.NOFIT), ("NOFIT by count", M.NOFIT), ("TOOLARGE", M.TOOLARGE)):
        r = st.select(EDGES[name])     # (check() compared the whole d_victims buffer with the pattern)
        assert r.status == status and r.victims == [] and r.summary[1] == 0


def test_empty_store():
    """n == 0: RLE_OK, the summary all zero, nothing else written."""
    st = Store(0)
    r = st.select(M.store([], [], [], [], [], max_bytes=0, max_files=3))
    assert r.summary == [0] * 6


def test_keys_compare_unsigned():
    keys = [1 << 63, 5, (1 << 64) - 1, 0, (1 << 63) - 1]
    r = Store(5).select(M.store(keys, [10] * 5, max_bytes=10))
    assert r.victims == [3, 1, 4, 0]


# ---------------------------------------------------------------- wide keys, several files per thread
# evict_model.random_store's five key kinds (heavy ties, timestamps, all 64 bits, top and bottom bytes,
# shifted) at sizes where each of the 1024 threads holds two or five files, so the radix select runs
# up to eight passes over keys that differ in their top bytes.  The seeds were picked on the CPU; the
# first draw of random_store is the key kind.
WIDE_SEEDS = {1500: (0, 1, 2, 3, 4, 5, 6, 7, 8, 9), 5000: (0, 1, 3, 4, 5, 12, 13, 17, 19, 20)}


def wide_kind(n, seed):
    return int(np.random.default_rng([n, seed]).integers(0, 5))


def test_wide_key_seeds_draw_every_kind():
    for n, seeds in WIDE_SEEDS.items():
        assert {wide_kind(n, seed) for seed in seeds} == {0, 1, 2, 3, 4}, n


@pytest.mark.parametrize("n,seed", [(n, seed) for n, seeds in WIDE_SEEDS.items() for seed in seeds])
def test_wide_keys(n, seed):
    s = M.random_store(np.random.default_rng([n, seed]), n)
    kind = wide_kind(n, seed)
    if kind == 2:
        assert max(s["keys"]) >> 56 and len({k >> 56 for k in s["keys"]}) > 100    # the top byte differs
    if kind == 3:
        assert {k >> 56 for k in s["keys"]} == {0, 1, 2} == {k & 255 for k in s["keys"]}
    Store(n).select(s)


def test_global_sort_of_64_bit_keys():
    """m > 4096 victims (the sort over d_victims in global memory) whose keys use all 64 bits and
    differ in the top byte."""
    n, m = 5000, 4500
    rng = np.random.default_rng(64)
    keys = [int(k) & M.M64 for k in rng.integers(0, 1 << 63, n) * 2 + rng.integers(0, 2, n)]
    s = M.store(keys, [int(c) for c in rng.integers(0, 5000, n)], [int(c) for c in rng.integers(0, 6000, n)])
    r = Store(n).select(with_count(s, m, by_files=True))
    assert r.status == M.OK and len(r.victims) == m
    assert len({keys[v] >> 56 for v in r.victims}) > 200
    assert [keys[v] for v in r.victims] == sorted(keys[v] for v in r.victims)


# ---------------------------------------------------------------- gather
@pytest.fixture(scope="module")
def selected():
    """Two selections at n = 130 left on the device: one with victims, one that fits (m = 0)."""
    out = []
    for name in ("exact at a file edge", "fits"):
        st = Store(130)
        r = st.select(EDGES[name])
        out.append((st, r))
    assert len(out[0][1].victims) == 17 and out[1][1].victims == []
    rng = np.random.default_rng(5)
    tables = [[int(x) for x in rng.integers(0, 1 << 63, 130)] for _ in range(8)]
    return out, tables, [u64(t) for t in tables]


@pytest.mark.parametrize("ntables", [1, 5, 8])
@pytest.mark.parametrize("order", [M.ORDER_EVICTION, M.ORDER_REPLY])
def test_gather(selected, order, ntables):
    """Both orders, cap below, at and above m, cap == 0, and m == 0: rows [0, min(m, cap)) of every
    output table, nothing else."""
    sels, tables, d_tables = selected
    rows = 40
    outs = [Guarded(rows, torch.int64) for _ in range(ntables)]
    for st, r in sels:
        m = len(r.victims)
        for cap in (0, 1, m - 3, m, m + 5, rows):
            if cap < 0:
                continue
            for g in outs:
                g.fill()
            R.evict_gather(st.victims.t, st.summary.t, d_tables[:ntables], [g.t for g in outs], order=order, cap=cap)
            torch.cuda.synchronize()
            want = M.gather(r.victims, m, order, tables[:ntables], [[PAT64] * rows] * ntables, cap)
            for g, w in zip(outs, want):
                g.expect(w)
                assert w[min(m, cap):] == [PAT64] * (rows - min(m, cap))
    # the selections themselves are as they were
    for st, r in sels:
        st.check()
