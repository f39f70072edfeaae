"""GPU test: rle_evict_select_device and rle_evict_gather_device replayed from a captured graph, by the
protocol of tests/test_gpu_relocate_replay.py: both captured once on a side stream in the default
capture mode, replayed over data sets rewritten in the same device tensors (keys, sizes, wants and both
masks change within the captured n, limits, flags, order, cap and tables: two sets that evict
different numbers of files, a set that fits and a set refused with NOFIT), every output filled with the
pattern before every run; then eagerly, and once more after the graph is gone.  After every run every
output buffer, guards included, equals the model's (tests/evict_model.py)."""
import numpy as np
import pytest
import torch

import evict_model as M
import rle_mi355x as R
from test_gpu_evict import PAT64, Guarded, Store, u64
from test_gpu_graph_replay import side   # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu
N = 200
MAX_BYTES, MAX_FILES, FLAGS = 300000, 150, R.RLE_EVICT_SLOTS
CAP, NTABLES = 24, 5


def data_sets():
    """(store, m) per set, all under the captured limits."""
    sets = []
    for k, (scale, dead, spared) in enumerate(((4000, 11, 13), (1500, 7, 1000), (1100, 3, 9), (6000, 5, 2))):
        rng = np.random.default_rng(40 + k)
        keys = [int(x) for x in (0x6600000000 << k) + rng.integers(0, 50 + 40 * k, N) * (k + 1)]
        lens = [int(c) for c in rng.integers(0, scale, N)]
        wants = [int(c) for c in rng.integers(0, scale, N)]
        live = [int(i % dead != 1) for i in range(N)]
        spare = [int(i % spared == 0) for i in range(N)]
        s = M.store(keys, lens, wants, live, spare, MAX_BYTES, MAX_FILES, FLAGS)
        sets.append((s, M.loop_model(**s)))
    got = [(r.status, len(r.victims)) for _, r in sets]
    assert got[0][0] == M.OK and got[0][1] > CAP                       # the bytes decide, m above cap
    assert got[1][0] == M.OK and 0 < got[1][1] < CAP                   # the files limit decides, m below cap
    assert got[2] == (M.OK, 0) and got[3] == (M.NOFIT, 0), got         # fits; cannot fit
    return sets


def test_graph_replay(side):
    sets = data_sets()
    rng = np.random.default_rng(9)
    tables = [[int(x) for x in rng.integers(0, 1 << 63, N)] for _ in range(NTABLES)]
    with torch.cuda.stream(side):
        st = Store(N)
        d_tables = [u64(t) for t in tables]
        outs = [Guarded(CAP, torch.int64) for _ in range(NTABLES)]

        def launch():
            st.launch(stream=side)
            R.evict_gather(st.victims.t, st.summary.t, d_tables, [g.t for g in outs], order=R.RLE_EVICT_ORDER_REPLY,
                           cap=CAP, stream=side)

        def run(k, go):
            s, r = sets[k]
            st.load(s)
            for g in outs:
                g.fill()
            go()
            side.synchronize()
            assert st.check() == r
            want = M.gather(r.victims, len(r.victims), M.ORDER_REPLY, tables, [[PAT64] * CAP] * NTABLES, CAP)
            for g, w in zip(outs, want):
                g.expect(w)

        run(0, launch)   # warm-up
        st.load(sets[0][0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch()
    with torch.cuda.stream(side):
        for k in (1, 2, 3, 0, 1, 3, 2):
            run(k, g.replay)
        run(3, launch)   # eager after the replays
        g.reset()
        del g
        run(0, launch)   # eager after the graph
