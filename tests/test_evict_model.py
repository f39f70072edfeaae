"""CPU tests of the eviction selection's models (tests/evict_model.py): the kernel's route
(select_model: totals, weighted radix select, tie scan, compaction, sort) gives what the reference's
loop gives (loop_model) -- victims, their order, the keep mask and all six summary words -- on seeded
random stores and on the named edges, and the sort's network with virtual padding sorts.  No GPU."""
import numpy as np
import pytest

import evict_model as M

EDGES = M.edges(130)


def both(s):
    a, b = M.loop_model(**s), M.select_model(**s)
    assert a == M.loop_model(**s, fast=True)   # (the scan the GPU tests' large stores use)
    assert a.status == b.status
    assert a.victims == b.victims
    assert a.keep == b.keep
    assert a.summary == b.summary
    return a


def test_random_stores():
    """320 seeded stores, n <= 300: mixed masks, wants, both limits and both flags; among them stores
    that fit, stores that evict and stores that cannot be made to fit."""
    rng = np.random.default_rng(7000)
    seen = set()
    for _ in range(320):
        n = int(rng.integers(1, 301))
        r = both(M.random_store(rng, n))
        seen.add((r.status, min(len(r.victims), 2)))
    assert seen >= {(M.OK, 0), (M.OK, 1), (M.OK, 2), (M.NOFIT, 0)}, seen


@pytest.mark.parametrize("name", sorted(EDGES))
def test_named_edge(name):
    both(EDGES[name])


def test_named_edges_are_what_their_names_say():
    r = {k: M.loop_model(**s) for k, s in EDGES.items()}
    n = 130
    for k in ("all keys equal", "top byte only", "bottom byte only"):
        assert len(r[k].victims) == n // 3, k
    assert r["all keys equal"].victims == sorted(r["all keys equal"].victims)   # FIFO over the list
    s = EDGES["keys 0 and 2^64-1"]
    assert {s["keys"][i] for i in r["keys 0 and 2^64-1"].victims} == {0, M.M64}
    for k in ("exact at a bin edge", "exact at a file edge"):   # an exact fit stops
        assert r[k].summary[3] == EDGES[k]["max_bytes"] and r[k].victims, k
    assert {EDGES["exact at a bin edge"]["keys"][i] for i in r["exact at a bin edge"].victims} == {0x7700, 0x7701, 0x7702}
    assert len(r["exact at a file edge"].victims) == 17 and len(r["one byte more"].victims) == 18
    assert r["one byte more"].victims[:17] == r["exact at a file edge"].victims
    s = EDGES["ties straddle the cut"]
    cut = s["keys"][r["ties straddle the cut"].victims[-1]]
    kept_ties = [i for i, k in enumerate(s["keys"]) if k == cut and r["ties straddle the cut"].keep[i] and not s["spare"][i]]
    assert cut == 9 and kept_ties and min(kept_ties) > r["ties straddle the cut"].victims[-1]
    s = EDGES["smallest key spared"]
    low = s["keys"].index(min(s["keys"]))
    assert s["spare"][low] and r["smallest key spared"].keep[low] == 1 and len(r["smallest key spared"].victims) == 5
    assert len(r["files limit decides"].victims) == 7 and EDGES["files limit decides"]["max_bytes"] == M.M64
    assert len(r["bytes limit decides"].victims) == 20
    assert len(r["both bind, files later"].victims) == 12 and len(r["both bind, bytes later"].victims) == 20
    for k in ("fits", "fits with a files limit"):
        assert r[k].status == M.OK and r[k].victims == [] and r[k].summary[2] == r[k].summary[3], k
    t = M.totals(EDGES["all eligible evicted"])
    assert len(r["all eligible evicted"].victims) == t[3] and r["all eligible evicted"].summary[5] == t[1] - t[3]
    for k in ("NOFIT by bytes", "NOFIT by count"):
        assert r[k].status == M.NOFIT and r[k].victims == [] and r[k].summary[1] == 0, k
        assert r[k].keep == [int(x) for x in EDGES[k]["live"]], k
    assert r["TOOLARGE"].status == M.TOOLARGE and r["TOOLARGE"].summary[2] == r["TOOLARGE"].summary[3]
    s = EDGES["dead files hold the smallest keys"]
    assert all(s["live"][i] for i in r["dead files hold the smallest keys"].victims)
    assert len(r["dead files hold the smallest keys"].victims) == 9
    a, b = r["exact bytes"], r["RLE_EVICT_SLOTS changes the last file"]
    assert len(a.victims) == 3 and len(b.victims) > 3 and b.victims[:3] == a.victims


def test_all_eligible_evicted_without_masks():
    n = 70
    s = M.store([n - i for i in range(n)], [10] * n, max_bytes=0)
    r = both(s)
    assert r.victims == list(range(n - 1, -1, -1)) and r.keep == [0] * n and r.summary == [0, n, 10 * n, 0, n, 0]


def test_open_file_handler_single_victim():
    """openFileHandler's eviction: max_files = maxFileNum - 1 with max_bytes = UINT64_MAX takes one."""
    s = M.store([7, 3, 9, 3, 8], [1, 2, 3, 4, 5], max_files=4)
    assert both(s).victims == [1]


def test_empty_store():
    assert both(M.store([], [], max_bytes=0, max_files=1)).summary == [0] * 6


@pytest.mark.parametrize("m", list(range(131)) + [4095, 4096, 4097])
def test_bitonic_model_sorts(m):
    rng = np.random.default_rng(m)
    keys = rng.integers(0, max(2, m // 3), m) if m % 2 else rng.integers(0, 1 << 62, m)
    pairs = [(int(k), i) for i, k in enumerate(keys)]
    pairs = [pairs[i] for i in rng.permutation(m)]
    assert M.bitonic_model(pairs) == sorted(pairs)
