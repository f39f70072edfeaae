"""GPU tests of rle_readn_layout_device and rle_readn_batch_device (include/rle_mi355x.h, DESIGN.md
§4c): the reply readNFilesHandler builds (reference src/filesystemApi.c:663-691), byte for byte, from
streams encoded on the device and lengths that never leave it; the reply's capacity; edge layouts;
and the layout alone past one stride of its workgroup."""
import numpy as np
import pytest
import torch

import readn_pack_model as M
import rle_mi355x as R
import rle_oracle as O
from test_gpu_parity import DEV, POISON, _i64

pytestmark = pytest.mark.gpu
TILE = 1008


class Store:
    """Files encoded on the device: the streams in worst-case slots, their lengths from the encode
    and their decoded lengths from the tail scan, all in device memory."""

    def __init__(self, contents):
        self.contents = contents
        self.n = n = len(contents)
        sizes = [len(x) for x in contents]
        in_offs, in_total = R.layout(sizes)
        host = np.zeros(in_total, np.uint8)
        for x, o in zip(contents, in_offs):
            host[o:o + len(x)] = np.frombuffer(x, np.uint8)
        offs, total = R.compressed_slots(sizes)
        self.d_c = torch.zeros(total, dtype=torch.uint8, device=DEV)
        self.off = _i64(offs)
        self.clen = torch.zeros(n, dtype=torch.int64, device=DEV)
        st = torch.zeros(n, dtype=torch.int32, device=DEV)
        R.encode_batch(torch.from_numpy(host).to(DEV), _i64(in_offs), _i64(sizes), self.d_c, self.off, self.clen, st)
        self.tail = torch.zeros(n, dtype=torch.int64, device=DEV)
        self.ulen = torch.full((n,), -1, dtype=torch.int64, device=DEV)
        st2 = torch.zeros(n, dtype=torch.int32, device=DEV)
        R.tail_batch(self.d_c, self.off, self.clen, self.tail, self.ulen, st2)
        torch.cuda.synchronize()
        assert int(st.abs().sum().item()) == 0 and int(st2.abs().sum().item()) == 0

    def readn(self, d_out, gaps, out_cap=None):
        """One rle_readn_batch_device call: (place, total, status) as numpy."""
        n = self.n
        place = torch.full((n,), -7, dtype=torch.int64, device=DEV)
        total = torch.full((1,), -7, dtype=torch.int64, device=DEV)
        status = torch.full((n,), 0x7777, dtype=torch.int32, device=DEV)
        R.readn_batch(self.d_c, self.off, self.clen, self.ulen, None if gaps is None else _i64(gaps), d_out, place,
                      total, status, out_cap=out_cap)
        torch.cuda.synchronize()
        return place.cpu().numpy(), int(total.item()), status.cpu().numpy()


def numpy_layout(ulen, gaps):
    u = np.asarray(ulen, np.int64)
    g = np.zeros(len(u), np.int64) if gaps is None else np.asarray(gaps, np.int64)
    ends = np.cumsum(u + g)
    return ends - u, int(ends[-1]) if len(u) else 0


def mixed_files():
    """14 files of mixed kinds, 1-3 decode tiles of stream each, with path names of different lengths."""
    sizes = [900, 1500, 2600, 3024, 6049, 1008, 2017, 700, 2500, 1200, 2900, 1999, 333, 1900]
    kinds = [1, 2, 3, 0, 0, 4, 1, 2, 3, 4, 1, 2, 3, 4]
    contents = [O.gen(k, 20 + i, s) for i, (k, s) in enumerate(zip(kinds, sizes))]
    for x in contents:
        assert 1 <= -(-len(O.encode(x)) // TILE) <= 3
    paths = [b"/srv/store/" + b"d%d/" % i * (i % 4) + b"file_%d" % (7 ** i) + b".bin" * (i % 3) for i in range(14)]
    assert len({len(p) for p in paths}) >= 8
    return paths, contents


@pytest.fixture(scope="module")
def stored():
    paths, contents = mixed_files()
    return paths, contents, Store(contents)


def reply_buffer(paths, contents, size):
    """The device buffer with the test's headers written where the reference puts them, poison
    everywhere else; and the header lengths."""
    host = np.full(size, POISON, np.uint8)
    pos, gaps = 0, []
    for p, x in zip(paths, contents):
        h = M.header(p, len(x))
        host[pos:pos + len(h)] = np.frombuffer(h, np.uint8)
        gaps.append(len(h))
        pos += len(h) + len(x)
    return torch.from_numpy(host).to(DEV), gaps


def test_reference_reply_byte_for_byte(stored):
    paths, contents, store = stored
    assert store.ulen.cpu().tolist() == [len(x) for x in contents]
    want = M.reply(paths, contents)
    size = len(want) + 100
    d_out, gaps = reply_buffer(paths, contents, size)
    assert gaps == [20 + len(p) for p in paths]
    place, total, st = store.readn(d_out, gaps)
    wplace, wtotal = numpy_layout([len(x) for x in contents], gaps)
    assert total == wtotal == len(want) and (place == wplace).all()
    assert (st == 0).all(), st
    got = d_out.cpu().numpy()
    assert got[:total].tobytes() == want
    assert (got[total:] == POISON).all()


def test_capacity(stored):
    """out_cap one byte short: every status NOFIT, not a byte written, place and total still right;
    out_cap exact: the reply."""
    paths, contents, store = stored
    want = M.reply(paths, contents)
    gaps = [20 + len(p) for p in paths]
    wplace, wtotal = numpy_layout([len(x) for x in contents], gaps)
    d_out = torch.full((len(want) + 64,), POISON, dtype=torch.uint8, device=DEV)
    place, total, st = store.readn(d_out, gaps, out_cap=wtotal - 1)
    assert list(st) == [R.RLE_STATUS_NOFIT] * store.n
    assert bool((d_out == POISON).all().item())
    assert total == wtotal and (place == wplace).all()
    d_out, _ = reply_buffer(paths, contents, len(want) + 64)
    place, total, st = store.readn(d_out, gaps, out_cap=wtotal)
    assert (st == 0).all() and total == wtotal and (place == wplace).all()
    got = d_out.cpu().numpy()
    assert got[:total].tobytes() == want and (got[total:] == POISON).all()


def test_edge_layouts(stored):
    """n = 1; NULL gaps (the contents alone, abutting); an empty file among the others; n = 0."""
    one = Store([O.gen(2, 5, 1777)])
    d_out = torch.full((1777 + 40 + 64,), POISON, dtype=torch.uint8, device=DEV)
    place, total, st = one.readn(d_out, [37])
    assert list(place) == [37] and total == 37 + 1777 and list(st) == [0]
    got = d_out.cpu().numpy()
    assert (got[:37] == POISON).all() and got[37:total].tobytes() == one.contents[0] and (got[total:] == POISON).all()

    _, contents, store = stored
    body = b"".join(contents)
    d_out = torch.full((len(body) + 64,), POISON, dtype=torch.uint8, device=DEV)
    place, total, st = store.readn(d_out, None)
    assert total == len(body) and (st == 0).all()
    assert (place == numpy_layout([len(x) for x in contents], None)[0]).all()
    got = d_out.cpu().numpy()
    assert got[:total].tobytes() == body and (got[total:] == POISON).all()

    some = [O.gen(1, 1, 1009), b"", O.gen(3, 2, 50), b"", b"", O.gen(4, 3, 2100), b""]
    paths = [b"p%d" % (10 ** i) for i in range(len(some))]
    st3 = Store(some)
    want = M.reply(paths, some)
    d_out, gaps = reply_buffer(paths, some, len(want) + 64)
    place, total, st = st3.readn(d_out, gaps)
    assert (st == 0).all() and total == len(want)
    got = d_out.cpu().numpy()
    assert got[:total].tobytes() == want and (got[total:] == POISON).all()

    tot = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    R.readn_layout(empty, None, empty, tot)
    torch.cuda.synchronize()
    assert int(tot.item()) == 0


@pytest.mark.parametrize("gaps", [True, False])
def test_layout_alone_past_one_stride(gaps):
    """n = 5000: five strides of the workgroup, the last one partial; against numpy."""
    rng = np.random.default_rng(11)
    n = 5000
    ulen = rng.integers(0, 1 << 31, n).astype(np.int64)   # the sum passes 2^32 many times over
    ulen[::17] = 0
    gap = rng.integers(20, 300, n).astype(np.int64) if gaps else None
    place = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    total = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    R.readn_layout(_i64(ulen), None if gap is None else _i64(gap), place, total)
    torch.cuda.synchronize()
    wplace, wtotal = numpy_layout(ulen, gap)
    assert wtotal > 1 << 40
    assert int(total.item()) == wtotal
    assert (place.cpu().numpy() == wplace).all()
    assert M.layout([int(v) for v in ulen], None if gap is None else [int(v) for v in gap])[1] == wtotal
