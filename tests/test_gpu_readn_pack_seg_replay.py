"""GPU tests: rle_decode_packed_batch_device_seg and rle_readn_batch_device_seg replayed from a captured
graph, by the protocol of tests/test_gpu_readn_pack_replay.py: captured once on a side stream in the
default capture mode, replayed over three data sets rewritten in the same device tensors (streams of
one to four 4-tile segments, their offsets and lengths, decoded lengths, gaps and destinations all
change within the captured n, out_cap and total_in_bytes; the second set's reply does not fit, and
NOFIT is then replaced by a set that fits), result words, the reply and the workspace poisoned before
every run; then eagerly, and once more after the graph is gone.  After every run the reply, d_place,
d_total and the status words equal the oracle's and the numpy layout."""
import numpy as np
import pytest
import torch

import readn_pack_seg_gpu as G
import rle_mi355x as R
import rle_oracle as O
from test_gpu_graph_replay import side   # noqa: F401 (a fixture)
from test_gpu_parity import DEV, POISON, _i64
from test_gpu_readn_pack_replay import layout_of

pytestmark = pytest.mark.gpu
N = 6
OUT_CAP = 30000   # the captured capacity of the reply
HINT = G.HINT     # the captured total_in_bytes: 4-tile segments, tables for every set


def data_sets():
    """Three sets of N files: (contents, gaps).  Set 1 is longer than OUT_CAP."""
    sets = []
    for k, sizes in enumerate([(4100, 0, 17, 9000, 1, 12100), (11000, 8100, 4032, 8070, 900, 33),
                               (5, 12090, 4031, 0, 8064, 4040)]):
        contents = [O.gen((i + k) % 5 or 1, 10 * k + i, s) for i, s in enumerate(sizes)]
        gaps = [21 + (7 * i + 11 * k) % 40 for i in range(N)]
        sets.append((contents, gaps))
    totals = [sum(len(x) for x in c) + sum(g) for c, g in sets]
    assert totals[0] <= OUT_CAP and totals[1] > OUT_CAP and totals[2] <= OUT_CAP
    segs = [{G.segments(len(O.encode(x))) for x in c} for c, _ in sets]
    assert all(1 in s and len(s) >= 3 and 3 <= max(s) <= 4 for s in segs), segs
    assert all(sum(len(O.encode(x)) for x in c) <= HINT for c, _ in sets)
    return sets


class Fixed:
    """Device tensors allocated once; load() rewrites all of them and poisons every result."""

    def __init__(self, sets):
        slot = max(R.round16(R.max_compressed_size(len(x))) for c, _ in sets for x in c) + 16
        self.slot = slot
        self.d_in = torch.zeros(N * slot + 64, dtype=torch.uint8, device=DEV)
        self.d_out = torch.full((max(layout_of(c, g)[1] for c, g in sets) + 64,), POISON, dtype=torch.uint8, device=DEV)
        i64 = lambda: torch.zeros(N, dtype=torch.int64, device=DEV)
        self.off, self.clen, self.ulen, self.gap, self.place = i64(), i64(), i64(), i64(), i64()
        self.total = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.status = torch.zeros(N, dtype=torch.int32, device=DEV)
        self.ws = R.decode_packed_seg_workspace(N, HINT, DEV)

    def load(self, k, contents, gaps, places=None):
        """Set k: the streams at offsets that differ from set to set; places: written too (the
        packed decode reads them), else poisoned (the layout writes them)."""
        ys = [O.encode(x) for x in contents]
        offs = [((i + k) % N) * self.slot + 16 * (k % 2) for i in range(N)]
        host = np.full(self.d_in.numel(), 0x39, np.uint8)
        for y, o in zip(ys, offs):
            host[o:o + len(y)] = np.frombuffer(y, np.uint8)   # (the bytes around the streams stay '9')
        self.d_in.copy_(torch.from_numpy(host).to(DEV))
        self.off.copy_(_i64(offs))
        self.clen.copy_(_i64([len(y) for y in ys]))
        self.ulen.copy_(_i64([len(x) for x in contents]))
        self.gap.copy_(_i64(gaps))
        self.d_out.fill_(POISON)
        self.status.fill_(0x7777)
        self.total.fill_(-7)
        self.ws.fill_(0xFF)
        if places is None:
            self.place.fill_(-7)
        else:
            self.place.copy_(_i64(places))

    def image(self, contents, places, written=True):
        img = np.full(self.d_out.numel(), POISON, np.uint8)
        if written:
            for x, p in zip(contents, places):
                img[p:p + len(x)] = np.frombuffer(x, np.uint8)
        return img


@pytest.mark.parametrize("entry", ["decode_packed_seg", "readn_batch_seg"])
def test_graph_replay(side, entry):
    assert R.seg_segment_bytes(HINT) == G.SB
    sets = data_sets()
    with torch.cuda.stream(side):
        fx = Fixed(sets)
        if entry == "decode_packed_seg":
            launch = lambda: R.decode_packed_seg(fx.d_in, fx.off, fx.clen, fx.d_out, fx.place, fx.ulen, fx.status,
                                                 total_in_bytes=HINT, ws=fx.ws, stream=side)
        else:
            launch = lambda: R.readn_batch_seg(fx.d_in, fx.off, fx.clen, fx.ulen, fx.gap, fx.d_out, fx.place, fx.total,
                                               fx.status, out_cap=OUT_CAP, total_in_bytes=HINT, ws=fx.ws, stream=side)

        def run(k, label, go):
            contents, gaps = sets[k]
            places, total = layout_of(contents, gaps)
            fx.load(k, contents, gaps, places if entry == "decode_packed_seg" else None)
            go()
            side.synchronize()
            what = (entry, label)
            fits = entry == "decode_packed_seg" or total <= OUT_CAP
            if entry != "decode_packed_seg":
                assert fx.place.cpu().tolist() == places, what
                assert int(fx.total.item()) == total, what
            want = fx.image(contents, places, written=fits)
            assert (fx.d_out.cpu().numpy() == want).all(), what
            assert fx.status.cpu().tolist() == [0 if fits else R.RLE_STATUS_NOFIT] * N, what

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
