"""GPU tests: rle_readn_headers_device, rle_readn_reply_device and rle_readn_reply_device_seg replayed
from a captured graph, by the protocol of tests/test_gpu_readn_pack_seg_replay.py: captured once on a
side stream in the default capture mode, replayed over three data sets rewritten in the same device
tensors (names, name lengths and offsets, streams, their offsets and lengths, decoded lengths all
change within the captured n, form, out_cap and total_in_bytes; the second set's reply does not fit,
and NOFIT is then replaced by a set that fits), result words, the reply and the workspace poisoned
before every run; then eagerly, and once more after the graph is gone.  After every run the reply,
d_place, d_total and the status words are the model's (tests/readn_reply_model.py)."""
import numpy as np
import pytest
import torch

import readn_reply_gpu as G
import readn_reply_model as RM
import rle_mi355x as R
import rle_oracle as O
from test_gpu_graph_replay import side   # noqa: F401 (a fixture)
from test_gpu_parity import DEV, POISON, _i64

pytestmark = pytest.mark.gpu
N = 6
FORM = RM.READN | RM.END
OUT_CAP = 30000   # the captured capacity of the reply
HINT = G.HINT     # the captured total_in_bytes: 4-tile segments, tables for every set
PATHS_CAP = 1024  # bytes of the path table's buffer


def data_sets():
    """Three sets of N files: (paths, contents).  Set 1 is longer than OUT_CAP."""
    sets = []
    for k, sizes in enumerate([(4100, 0, 17, 9000, 1, 12100), (11000, 8100, 4032, 8070, 900, 33),
                               (5, 12090, 4031, 0, 8064, 4040)]):
        contents = [O.gen((i + k) % 5 or 1, 10 * k + i, s) for i, s in enumerate(sizes)]
        paths = [bytes(0x61 + (i + k + j) % 26 for j in range(1 + (7 * i + 11 * k) % 40)) for i in range(N)]
        sets.append((paths, contents))
    totals = [len(RM.reply(p, c, FORM)) for p, c in sets]
    assert totals[0] <= OUT_CAP and totals[1] > OUT_CAP and totals[2] <= OUT_CAP
    assert len({tuple(len(p) for p in ps) for ps, _ in sets}) == 3
    assert all(sum(len(O.encode(x)) for x in c) <= HINT for _, c in sets)
    return sets


class Fixed:
    """Device tensors allocated once; load() rewrites all of them and poisons every result."""

    def __init__(self, sets):
        slot = max(R.round16(R.max_compressed_size(len(x))) for _, c in sets for x in c) + 16
        self.slot = slot
        self.d_in = torch.zeros(N * slot + 64, dtype=torch.uint8, device=DEV)
        self.d_out = torch.full((max(len(RM.reply(p, c, FORM)) for p, c in sets) + 64,), POISON, dtype=torch.uint8,
                                device=DEV)
        i64 = lambda: torch.zeros(N, dtype=torch.int64, device=DEV)
        self.off, self.clen, self.ulen, self.poff, self.plen, self.place = i64(), i64(), i64(), i64(), i64(), i64()
        self.d_paths = torch.zeros(PATHS_CAP, dtype=torch.uint8, device=DEV)
        self.total = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.status = torch.zeros(N, dtype=torch.int32, device=DEV)
        self.ws = R.decode_packed_seg_workspace(N, HINT, DEV)

    def load(self, k, paths, contents, places=None):
        """Set k: streams and names at offsets that differ from set to set; places: written too (the
        header writer reads them), else poisoned (the layout writes them)."""
        ys = [O.encode(x) for x in contents]
        offs = [((i + k) % N) * self.slot + 16 * (k % 2) for i in range(N)]
        host = np.full(self.d_in.numel(), 0x39, np.uint8)
        for y, o in zip(ys, offs):
            host[o:o + len(y)] = np.frombuffer(y, np.uint8)   # (the bytes around the streams stay '9')
        self.d_in.copy_(torch.from_numpy(host).to(DEV))
        blob, poffs, pos = np.full(PATHS_CAP, 0x23, np.uint8), [0] * N, 1 + k
        for i in sorted(range(N), key=lambda i: (i + k) % N):   # (the names in another order per set)
            poffs[i] = pos
            blob[pos:pos + len(paths[i])] = np.frombuffer(paths[i], np.uint8)
            pos += len(paths[i]) + (i + k) % 3
        assert pos <= PATHS_CAP
        self.d_paths.copy_(torch.from_numpy(blob).to(DEV))
        self.off.copy_(_i64(offs))
        self.clen.copy_(_i64([len(y) for y in ys]))
        self.ulen.copy_(_i64([len(x) for x in contents]))
        self.poff.copy_(_i64(poffs))
        self.plen.copy_(_i64([len(p) for p in paths]))
        self.d_out.fill_(POISON)
        self.status.fill_(0x7777)
        self.total.fill_(-7)
        self.ws.fill_(0xFF)
        if places is None:
            self.place.fill_(-7)
        else:
            self.place.copy_(_i64(places))


@pytest.mark.parametrize("entry", ["readn_headers", "readn_reply", "readn_reply_seg"])
def test_graph_replay(side, entry):
    assert R.seg_segment_bytes(HINT) == G.SB
    sets = data_sets()
    with torch.cuda.stream(side):
        fx = Fixed(sets)
        common = (fx.d_in, fx.off, fx.clen, fx.ulen, fx.d_paths, fx.poff, fx.plen, fx.d_out, fx.place, fx.total, fx.status)
        if entry == "readn_headers":
            launch = lambda: R.readn_headers(fx.d_paths, fx.poff, fx.plen, fx.ulen, fx.d_out, fx.place, form=FORM,
                                             stream=side)
        elif entry == "readn_reply":
            launch = lambda: R.readn_reply(*common, form=FORM, out_cap=OUT_CAP, stream=side)
        else:
            launch = lambda: R.readn_reply_seg(*common, form=FORM, out_cap=OUT_CAP, total_in_bytes=HINT, ws=fx.ws,
                                               stream=side)

        def run(k, label, go):
            paths, contents = sets[k]
            reply = RM.reply(paths, contents, FORM)
            places, total = RM.layout([len(c) for c in contents], [len(p) for p in paths], FORM)
            alone = entry == "readn_headers"
            fx.load(k, paths, contents, places if alone else None)
            go()
            side.synchronize()
            what = (entry, label)
            got = fx.d_out.cpu().numpy()
            if alone:   # the headers and the terminator alone (no capacity rule), the contents' ranges poison
                want = G.image_of(reply, len(got))
                for c, p in zip(contents, places):
                    want[p:p + len(c)] = POISON
                assert (got == want).all(), what
                return
            fits = total <= OUT_CAP
            assert fx.place.cpu().tolist() == places and int(fx.total.item()) == total, what
            assert (got == G.image_of(reply if fits else b"", len(got))).all(), what
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
