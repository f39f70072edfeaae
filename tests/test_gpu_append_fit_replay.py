"""GPU tests: rle_append_size_batch_device, rle_append_fit_batch_device and
rle_append_fit_batch_device_seg replayed from a captured graph, by the protocol of
tests/test_gpu_graph_replay.py: captured once on a side stream in the default capture mode, replayed
over data sets rewritten in the same device tensors (streams, offsets, lengths, capacities, tail
words and new content all change; one file goes fit -> NOFIT -> fit, another changes A across a tile
or segment edge), result words poisoned before every run; then eagerly, and once more after the graph
is gone.  After every run each result word and slot equals an eager call's on fresh tensors, and the
model's."""
import pytest
import torch

import append_fit_gpu as FG
import append_fit_model as F
import rle_mi355x as R
import rle_oracle as O
from test_gpu_graph_replay import side   # noqa: F401 (a fixture)
from test_gpu_seg_lengths import TILE

pytestmark = pytest.mark.gpu
SB = 4 * TILE


class Fixed(FG.Arena):
    """Device tensors allocated once for the largest data set; load() rewrites all of them."""

    def __init__(self, arenas):
        self.n = arenas[0].n
        assert all(a.n == self.n for a in arenas)
        self.d_s = torch.full((max(len(a.img) for a in arenas),), FG.POISON, dtype=torch.uint8, device=FG.DEV)
        self.d_n = torch.zeros(max(len(a.nimg) for a in arenas), dtype=torch.uint8, device=FG.DEV)
        i64 = lambda: torch.zeros(self.n, dtype=torch.int64, device=FG.DEV)
        self.d_off, self.d_noff, self.d_nlen, self.d_cap = i64(), i64(), i64(), i64()
        self.d_len, self.d_ulen, self.d_tail, self.d_need = i64(), i64(), i64(), i64()
        self.d_status = torch.zeros(self.n, dtype=torch.int32, device=FG.DEV)
        self.size = 0

    def load(self, a):
        a.upload()
        self.d_s.fill_(FG.POISON)
        self.d_s[:len(a.img)].copy_(a.d_s)
        self.d_n.zero_()
        self.d_n[:len(a.nimg)].copy_(a.d_n)
        for name in ("d_off", "d_noff", "d_nlen", "d_cap", "d_len", "d_ulen", "d_tail", "d_need", "d_status"):
            getattr(self, name).copy_(getattr(a, name))   # d_need, d_status: the poison fills
        self.size = len(a.img)

    def fetch(self):
        got = super().fetch()
        assert bool((self.d_s[self.size:] == FG.POISON).all().item()), "a store past the image"
        return (got[0][:self.size],) + got[1:]


def data_sets(form):
    """Three sets of six files.  File 0: fit -> NOFIT -> fit; file 1: A across a tile edge (the
    segmented form: a segment edge too); the others change streams, lengths and capacities."""
    sets = []
    edge = (1007, 1009, 2017) if form != "fit_seg" else (SB - 1, SB + 1, 2 * SB + 3)
    for k in range(3):
        f = FG.FitFiles(form, 8 * SB)
        f.add(F.literals(40 + 5 * k) + b"a" * (2 + k), b"aaa" + O.gen(2, 10 + k, 900 + 300 * k),
              cap="short" if k == 1 else "exact")
        f.add(F.literals(33 + k) + b"bbb", O.gen(1 + k, 20 + k, edge[k]), cap=("exact", "round16", "exact")[k])
        f.add(O.gen(2, 30 + k, (0, 2500, 17)[k]), O.gen(3, 40 + k, (1500, 0, 3029)[k]), cap=("slot", 0, "exact")[k])
        f.add(O.gen(1, 50 + k, (1008, 1, 300)[k]), O.gen(2, 60 + k, (16, 1024, 1)[k]), cap=("exact", "plus1", "short")[k])
        f.add(F.literals(100 + k) + b"c" * (9 - k), b"c" * (1 + 8 * k) + b"d", cap=("round16", "exact", "slot")[k])
        f.add(O.gen(4, 70 + k, 777 * k), bytes(2000 - 900 * k), cap="exact")
        sets.append(f)
    return sets


@pytest.mark.parametrize("form", ["size", "fit", "fit_seg"])
def test_graph_replay(side, form):
    hint = 8 * SB
    assert R.seg_segment_bytes(hint) == SB
    sets = data_sets(form)
    assert all(sum(len(a) for a in f.new) <= hint for f in sets)
    with torch.cuda.stream(side):
        arenas = [f.arena() for f in sets]
        want = [f.expected(a) for f, a in zip(sets, arenas)]
        if form != "size":
            assert [w[5][0] for w in want] == [0, F.NOFIT, 0]
        for k in range(3):   # a need left over from the previous data set cannot pass for this one
            assert all(a != b for a, b in zip(want[k - 1][4], want[k][4])), k
        fx = Fixed(arenas)
        ws = R.append_seg_workspace(fx.n, hint, FG.DEV) if form == "fit_seg" else None
        launch = lambda: fx.launch(form, hint, ws)

        def run(k, label, go):
            fx.load(arenas[k])
            go()
            side.synchronize()
            got = fx.fetch()
            sets[k].compare(f"{form}: {label}", arenas[k], got, want[k])
            arenas[k].upload()   # an eager call on fresh tensors
            arenas[k].launch(form, hint)
            eager = arenas[k].fetch()
            for a, b in zip(got, eager):
                assert (a == b).all(), (form, label)

        run(0, "warm-up", launch)
        fx.load(arenas[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch()
    with torch.cuda.stream(side):
        for k in (1, 2, 0):
            run(k, f"replay of set {k}", g.replay)
        run(1, "eager after the replays", launch)
        g.reset()
        del g
        run(2, "eager after the graph", launch)
