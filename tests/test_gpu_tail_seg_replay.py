"""GPU tests: the caller-owned workspace of rle_tail_batch_device_seg and its replay from a captured
graph, in the manner of tests/test_gpu_workspace_reuse.py and tests/test_gpu_graph_replay.py.

  exact size   rle_tail_seg_workspace_bytes bytes at a 256-byte aligned address between 4 KiB of
               guard bytes (n = 1: no plan and map launches; n = 3; n = 1025: one past the plan
               kernel's 1024 threads), pre-filled with 0x00, 0xFF, 0x01 or 0xA5: the results are the
               documented parse's and both guards are untouched; one byte less is RLE_E_INVAL and
               launches nothing (the result words keep their fill).
  graph        captured once on a side stream in the default capture mode and replayed over data sets
               that differ in every stream, offsets and lengths rewritten in the same device tensors,
               results poisoned before every run; then eagerly, and once more after the graph is gone.
"""
import functools

import numpy as np
import pytest
import torch

import append_tail_gpu as G
import append_tail_model as M
import rle_mi355x as R
from test_gpu_graph_replay import seg_hint, seg_sizes, side, stream_of_len   # noqa: F401 (side: a fixture)
from test_gpu_workspace_reuse import FILLS, Guarded, seg_len, sizes_for

pytestmark = pytest.mark.gpu
DEV = G.DEV
POISON = (0x5555555555, 0x6666666666, 0x7777)   # tail, ulen, status: append_tail_gpu.scan's fills


class Scan:
    """The device tensors of one scan launch, allocated once for the largest data set and rewritten
    per data set on `stream` (packed 16-byte aligned streams, so the offsets move too)."""

    def __init__(self, sets, stream):
        self.stream, self.n = stream, len(sets[0])
        assert all(len(s) == self.n for s in sets)
        need = max(R.layout([len(y) for y in s], pad=G.PAD)[1] for s in sets) + 64
        with torch.cuda.stream(stream):
            self.d_in = torch.zeros(need, dtype=torch.uint8, device=DEV)
            self.off = torch.zeros(self.n, dtype=torch.int64, device=DEV)
            self.len = torch.zeros(self.n, dtype=torch.int64, device=DEV)
            self.tail = torch.zeros(self.n, dtype=torch.int64, device=DEV)
            self.ulen = torch.zeros(self.n, dtype=torch.int64, device=DEV)
            self.status = torch.zeros(self.n, dtype=torch.int32, device=DEV)
        self.cur = None

    def load(self, streams):
        lens = [len(y) for y in streams]
        offs, total = R.layout(lens, pad=G.PAD)
        host = np.zeros(total, np.uint8)
        for y, o in zip(streams, offs):
            host[o:o + len(y)] = np.frombuffer(y, np.uint8)
        with torch.cuda.stream(self.stream):
            self.d_in[:total].copy_(torch.from_numpy(host))
            self.off.copy_(torch.from_numpy(np.asarray(offs, np.int64)))
            self.len.copy_(torch.from_numpy(np.asarray(lens, np.int64)))
            self.tail.fill_(POISON[0])
            self.ulen.fill_(POISON[1])
            self.status.fill_(POISON[2])
        self.cur = streams

    def outputs(self):
        return [self.tail, self.ulen, self.status]

    def launch(self, total, ws):
        R.tail_batch_seg(self.d_in, self.off, self.len, self.tail, self.ulen, self.status, total_in_bytes=total, ws=ws)

    def check(self, label):
        self.stream.synchronize()
        tl, ul, st = (t.cpu().numpy() for t in self.outputs())
        for i, y in enumerate(self.cur):
            got = (int(st[i]), int(tl[i]), int(ul[i]))
            assert got == G.scan_expected(y), (label, i, len(y), [hex(v) for v in got])


def streams_of(sizes, base, refused=None):
    out = [stream_of_len(C, 1 + (i + base) % 4, base + i)[0] for i, C in enumerate(sizes)]
    if refused is not None:
        y = out[refused]
        out[refused] = y[:len(y) // 2] + b"aa:" + y[len(y) // 2 + 3:]
        assert M.tail_of(out[refused]) is None
    return out


@functools.lru_cache(maxsize=None)
def exact_size_streams(n):
    """test_gpu_workspace_reuse's sizes, one NOTCANON stream inside (n = 1025: the long one)."""
    return streams_of(sizes_for(n), 100 * n, refused=(n // 2 if n > 1 else None))


@pytest.mark.parametrize("n", [1, 3, 1025])
@pytest.mark.parametrize("fill", FILLS)
def test_exact_size_between_guards(fill, n):
    streams = exact_size_streams(n)
    total = sum(len(y) for y in streams)
    assert R.seg_segment_bytes(total) == seg_len()
    sc = Scan([streams], torch.cuda.current_stream())
    sc.load(streams)
    need = int(R.lib().rle_tail_seg_workspace_bytes(n, total))
    g = Guarded(need, fill)
    before = [t.clone() for t in sc.outputs()]
    with pytest.raises(R.RLEError, match=f": {R.RLE_E_INVAL}$"):
        sc.launch(total, g.short())
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, sc.outputs())), "a refused call launched something"
    assert bool((g.ws == fill).all().item()) and g.guards_untouched()
    sc.launch(total, g.ws)
    sc.check(f"n={n}, workspace of {fill:#x}")
    assert g.guards_untouched(), "a kernel wrote outside rle_tail_seg_workspace_bytes"


@pytest.mark.parametrize("n", [3, 1])
def test_graph_replay(side, n):
    S, hint = seg_hint(n)
    sizes = seg_sizes(n, S)
    sets = [streams_of(sizes[k], 7000 * k, refused=(min(1, n - 1) if k == 1 else None)) for k in range(len(sizes))]
    want = [[G.scan_expected(y) for y in s] for s in sets]
    for k in range(len(sets)):   # a result left over from the previous data set cannot pass for this one
        assert all(a != b for a, b in zip(want[k - 1], want[k])), k
    assert max(sum(len(y) for y in s) for s in sets) <= hint
    sc = Scan(sets, side)
    ws = R.tail_seg_workspace(n, hint, DEV)
    launch = lambda: sc.launch(hint, ws)
    with torch.cuda.stream(side):
        sc.load(sets[0])
        launch()
        sc.check("warm-up")
        sc.load(sets[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch()
    with torch.cuda.stream(side):
        for k in range(1, len(sets)):
            sc.load(sets[k])
            g.replay()
            sc.check(f"replay {k}")
        sc.load(sets[0])
        launch()
        sc.check("eager after the replays")
        g.reset()
        del g
        sc.load(sets[1])
        launch()
        sc.check("eager after the graph")
