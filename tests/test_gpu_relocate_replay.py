"""GPU tests: rle_relocate_layout_device and rle_relocate_batch_device replayed from a captured graph,
by the protocol of tests/test_gpu_readn_pack_replay.py: captured once on a side stream in the default
capture mode, replayed over three data sets rewritten in the same device tensors (streams, their
offsets and lengths, wants and selection masks all change within the captured n, dst_base and dst_cap,
and so within the captured span and grid; the second set's slots do not fit, and NOFIT is then
replaced by a set that fits), result words and the destination poisoned before every run; then
eagerly, and once more after the graph is gone.  After every run the destination, d_new_off,
d_new_cap, d_total and the status words equal the model's (tests/relocate_model.py)."""
import numpy as np
import pytest
import torch

import relocate_model as M
import rle_mi355x as R
from test_gpu_graph_replay import side   # noqa: F401 (a fixture)
from test_gpu_parity import DEV, POISON, _i64

pytestmark = pytest.mark.gpu
N = 7
BASE = 48
DST_CAP = BASE + 5 * 16384 - 32   # the captured room: five spans, the last one short
SLOT = 40000 + 32


def data_sets():
    """Three sets of N files: (lengths, wants, masks).  Set 1 needs more than DST_CAP."""
    sets = [([16384, 0, 17, 30000, 1, 4097, 9000], [0, 0, 100, 30001, 0, 0, 9000], [1, 1, 1, 1, 1, 1, 1]),
            ([30000, 20000, 1500, 20160, 900, 33, 16385], [0, 21000, 0, 0, 0, 4096, 0], [1, 1, 0, 1, 1, 1, 1]),
            ([5, 40000, 1008, 0, 2017, 40, 20000], [0, 0, 16384, 0, 0, 0, 33000], [1, 1, 1, 0, 1, 1, 0])]
    totals = [M.layout(*s, BASE)[2] for s in sets]
    assert totals[0] <= DST_CAP and totals[1] > DST_CAP and totals[2] <= DST_CAP and totals[0] != totals[2]
    assert R.relocate_span_bytes(DST_CAP - BASE) == 16384
    return sets


class Fixed:
    """Device tensors allocated once; load() rewrites all of them and poisons every result."""

    def __init__(self):
        self.d_src = torch.zeros(N * SLOT + 64, dtype=torch.uint8, device=DEV)
        self.d_dst = torch.full((DST_CAP + 4096,), POISON, dtype=torch.uint8, device=DEV)
        i64 = lambda: torch.zeros(N, dtype=torch.int64, device=DEV)
        self.off, self.len, self.want, self.new_off, self.new_cap = i64(), i64(), i64(), i64(), i64()
        self.sel = torch.zeros(N, dtype=torch.int32, device=DEV)
        self.total = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.status = torch.zeros(N, dtype=torch.int32, device=DEV)

    def load(self, k, lens, wants, sels):
        """Set k: the streams at offsets that differ from set to set."""
        rng = np.random.default_rng(100 + k)
        self.offs = [((i + k) % N) * SLOT + 16 * (k % 2) for i in range(N)]
        self.img = np.full(self.d_src.numel(), 0x39, np.uint8)
        for c, o in zip(lens, self.offs):
            self.img[o:o + c] = rng.integers(0, 256, c, dtype=np.uint8)
        self.d_src.copy_(torch.from_numpy(self.img).to(DEV))
        self.off.copy_(_i64(self.offs))
        self.len.copy_(_i64(lens))
        self.want.copy_(_i64(wants))
        self.sel.copy_(torch.tensor(sels, dtype=torch.int32, device=DEV))
        self.d_dst.fill_(POISON)
        self.status.fill_(0x7777)
        self.total.fill_(-7)
        self.new_off.fill_(-7)
        self.new_cap.fill_(-7)


@pytest.mark.parametrize("entry", ["relocate_layout", "relocate_batch"])
def test_graph_replay(side, entry):
    sets = data_sets()
    with torch.cuda.stream(side):
        fx = Fixed()
        if entry == "relocate_layout":
            launch = lambda: R.relocate_layout(fx.len, fx.want, fx.sel, fx.new_off, fx.new_cap, fx.total, dst_base=BASE,
                                               stream=side)
        else:
            launch = lambda: R.relocate_batch(fx.d_src, fx.off, fx.len, fx.d_dst, fx.new_off, fx.new_cap, fx.total,
                                              want=fx.want, sel=fx.sel, status=fx.status, dst_base=BASE,
                                              dst_cap=DST_CAP, stream=side)

        def run(k, label, go):
            lens, wants, sels = sets[k]
            fx.load(k, lens, wants, sels)
            go()
            side.synchronize()
            what = (entry, label)
            before = np.full(fx.d_dst.numel(), POISON, np.uint8)
            img, off, cap, total, st = M.expected(fx.img, fx.offs, lens, wants, sels, before, BASE, DST_CAP)
            assert fx.new_off.cpu().tolist() == off and fx.new_cap.cpu().tolist() == cap, what
            assert int(fx.total.item()) == total, what
            if entry == "relocate_batch":
                assert (fx.d_dst.cpu().numpy() == img).all(), what
                assert fx.status.cpu().tolist() == st, what
                assert (R.RLE_STATUS_NOFIT in st) == (k == 1), what
            else:
                assert bool((fx.d_dst == POISON).all().item()), what
                assert fx.status.cpu().tolist() == [0x7777] * N, what
            assert (fx.d_src.cpu().numpy() == fx.img).all(), what

        run(0, "warm-up", launch)
        fx.load(0, *sets[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch()
    with torch.cuda.stream(side):
        for k in (1, 2, 0, 1, 2):
            run(k, f"replay of set {k}", g.replay)
        run(1, "eager after the replays", launch)
        g.reset()
        del g
        run(2, "eager after the graph", launch)
