"""GPU tests of rle_readn_batch_device_seg (include/rle_mi355x.h, DESIGN.md §4c "Segmented form"): the
reply readNFilesHandler builds, byte for byte, from streams encoded on the device and lengths that
never leave it, with several waves per stream; the reply's capacity; NULL gaps; n = 0; and agreement
with rle_readn_batch_device.  About 300 files of 0 to 3 four-tile segments, a few launches in all."""
import numpy as np
import pytest
import torch

import readn_pack_seg_gpu as G
import rle_mi355x as R
import rle_oracle as O
from test_gpu_parity import DEV, POISON, _i64
from test_gpu_readn_pack import Store, numpy_layout

pytestmark = pytest.mark.gpu
GAP = 49   # a header of 20 + 29 path bytes in front of every file
N = 300


def contents():
    """N files: random, runs50, runs90, pairs and zero content of 0 .. about 3 SB stream bytes, with
    empty files (C = 0, U = 0) among them."""
    rng = np.random.default_rng(5)
    xs = []
    for i in range(N):
        kind = i % 5
        u = int(rng.integers(1, 3 * G.SB - 200))
        if kind == 0:
            u *= 3    # zero content: three stream bytes per nine
        if kind == 3:
            u *= 2    # runs90 compresses to under a half
        if i % 23 == 7:
            u = 0
        if i % 29 == 3:
            u = int(rng.integers(1, 20))
        x = O.gen(kind, 100 + i, u)
        while len(O.encode(x)) > 3 * G.SB + 2:   # (pairs expand by a half)
            x = x[:len(x) * 3 // 4]
        xs.append(x)
    return xs


@pytest.fixture(scope="module")
def stored():
    xs = contents()
    store = Store(xs)
    clen = store.clen.cpu().tolist()
    assert store.ulen.cpu().tolist() == [len(x) for x in xs]
    segs = {0 if c == 0 else G.segments(c) for c in clen}
    assert segs == {0, 1, 2, 3}, segs
    hint = sum(clen)
    assert R.seg_segment_bytes(hint) == G.SB
    return xs, store, hint


def reply_of(xs, gaps, size):
    """(the device buffer with the headers written and poison elsewhere, the expected image)."""
    start = np.full(size, POISON, np.uint8)
    want = np.full(size, POISON, np.uint8)
    pos = 0
    for i, x in enumerate(xs):
        g = gaps[i] if gaps is not None else 0
        h = (b"%010d" % i + b"/srv/store/some/path/of/a/file" + b"%010d" % len(x))[:g].ljust(g, b"#")
        start[pos:pos + g] = want[pos:pos + g] = np.frombuffer(h, np.uint8)
        pos += g
        want[pos:pos + len(x)] = np.frombuffer(x, np.uint8)
        pos += len(x)
    return torch.from_numpy(start).to(DEV), start, want, pos


def readn_seg(store, d_out, gaps, hint, out_cap=None, seg=True):
    n = store.n
    place = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    total = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    status = torch.full((n,), 0x7777, dtype=torch.int32, device=DEV)
    g = None if gaps is None else _i64(gaps)
    if seg:
        R.readn_batch_seg(store.d_c, store.off, store.clen, store.ulen, g, d_out, place, total, status, out_cap=out_cap,
                          total_in_bytes=hint)
    else:
        R.readn_batch(store.d_c, store.off, store.clen, store.ulen, g, d_out, place, total, status, out_cap=out_cap)
    torch.cuda.synchronize()
    return place.cpu().numpy(), int(total.item()), status.cpu().numpy()


def test_reply_byte_for_byte_and_agreement(stored):
    """The reply with a 49-byte header in front of every file, written before the call and never by
    it; d_place and *d_total against numpy; and the same buffer, words and statuses from
    rle_readn_batch_device."""
    xs, store, hint = stored
    gaps = [GAP] * N
    wplace, wtotal = numpy_layout([len(x) for x in xs], gaps)
    d_out, _, want, end = reply_of(xs, gaps, wtotal + 100)
    assert end == wtotal
    place, total, st = readn_seg(store, d_out, gaps, hint)
    assert total == wtotal and (place == wplace).all()
    assert (st == 0).all(), [(i, hex(int(s))) for i, s in enumerate(st) if s][:5]
    got = d_out.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert not len(bad), (len(bad), int(bad[0]), int(np.searchsorted(wplace, bad[0], side="right")) - 1)
    d_one, _, _, _ = reply_of(xs, gaps, wtotal + 100)
    place1, total1, st1 = readn_seg(store, d_one, gaps, hint, seg=False)
    assert total1 == total and (place1 == place).all() and (st1 == st).all()
    assert torch.equal(d_one, d_out)


def test_capacity(stored):
    """out_cap equal to the total passes; one byte short: every status NOFIT, not a byte of d_out
    changed, d_place and *d_total written all the same."""
    xs, store, hint = stored
    gaps = [GAP] * N
    wplace, wtotal = numpy_layout([len(x) for x in xs], gaps)
    d_out, start, want, _ = reply_of(xs, gaps, wtotal + 64)
    place, total, st = readn_seg(store, d_out, gaps, hint, out_cap=wtotal - 1)
    assert list(st) == [R.RLE_STATUS_NOFIT] * N
    assert (d_out.cpu().numpy() == start).all()
    assert total == wtotal and (place == wplace).all()
    place, total, st = readn_seg(store, d_out, gaps, hint, out_cap=wtotal)
    assert (st == 0).all() and total == wtotal and (place == wplace).all()
    assert (d_out.cpu().numpy() == want).all()


def test_null_gaps_and_no_files(stored):
    """d_gap = NULL: the contents alone, abutting at whatever phase their lengths give; n = 0 writes
    *d_total = 0 and nothing else."""
    xs, store, hint = stored
    wplace, wtotal = numpy_layout([len(x) for x in xs], None)
    assert len({int(p) % 16 for p in wplace}) == 16
    d_out, _, want, _ = reply_of(xs, None, wtotal + 64)
    place, total, st = readn_seg(store, d_out, None, hint)
    assert (st == 0).all() and total == wtotal and (place == wplace).all()
    assert (d_out.cpu().numpy() == want).all()

    tot = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    d_out.fill_(POISON)
    R.readn_batch_seg(store.d_c, empty, empty, empty, None, d_out, empty, tot, None, total_in_bytes=0,
                      ws=torch.zeros(512, dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()
    assert int(tot.item()) == 0 and bool((d_out == POISON).all().item())
