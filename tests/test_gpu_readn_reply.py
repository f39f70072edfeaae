"""GPU tests of rle_readn_reply_device (include/rle_mi355x.h, DESIGN.md §4c "Headers and terminator"):
the whole wire reply -- headers, contents and terminator -- from streams encoded on the device, decoded
lengths from the tail scan and a path table on the device, against the model's bytes
(tests/readn_reply_model.py); the reply's capacity; refused and flagged files among good ones; the
READ form; n == 0."""
import numpy as np
import pytest
import torch

import readn_reply_gpu as G
import readn_reply_model as RM
import rle_mi355x as R
import rle_oracle as O
from test_gpu_parity import DEV, POISON, _i64, _input_image

pytestmark = pytest.mark.gpu
NS = (1, 2, 65, 1025)   # (1025: past one stride of the layout's workgroup)
_files = {}


def files(n):
    """n small files, every 4th empty (its neighbours' headers abut), every 5th with a one-byte name;
    encoded once per n."""
    if n not in _files:
        _files[n] = G.Files(G.names(n), G.small_contents(n, seed=n))
    return _files[n]


@pytest.mark.parametrize("end", [False, True])
@pytest.mark.parametrize("n", NS)
def test_reply_is_the_models(n, end):
    f = files(n)
    assert f.store.ulen.cpu().tolist() == [len(c) for c in f.contents]
    assert n == 1 or (any(len(c) == 0 for c in f.contents) and any(len(p) == 1 for p in f.paths))
    f.check(RM.READN | (RM.END if end else 0))


@pytest.mark.parametrize("form", [RM.READN, RM.READN | RM.END, RM.READ])
def test_capacity(form):
    """out_cap exact: the reply.  One byte short: every status NOFIT, not a byte written (no header,
    no terminator), place and total still right.  With the terminator also the capacity that holds
    everything but the terminator."""
    f = files(1) if form == RM.READ else files(65)
    reply, place, total = f.want(form)
    f.check(form, size=total + G.SLACK, out_cap=total)
    for cap in [total - 1, 0] + ([total - 10] if form & RM.END else []):
        got, gplace, gtotal, st = f.run(form, size=total + G.SLACK, out_cap=cap)
        assert list(st) == [R.RLE_STATUS_NOFIT] * f.n, (form, cap)
        assert (got == POISON).all(), (form, cap)
        assert gtotal == total and list(gplace) == place, (form, cap)


def test_refused_and_flagged_files_keep_their_headers():
    """A stream that overflows its length, one that is short of it and one at a misaligned address
    among good ones: every header is there, and contents and status words are those of
    rle_readn_batch_device on the same arguments."""
    xs = [O.gen(1 + i % 4, 40 + i, 300 + 171 * i) for i in range(7)]
    ys = [O.encode(x) for x in xs]
    us = [len(x) for x in xs]
    us[1] -= 5    # OVERFLOW through the serial path
    us[4] += 40   # SHORT
    offs, host = _input_image(ys, None)
    offs = list(offs)
    offs[5] += 1  # MISALIGNED (the stream is read nowhere)
    paths = G.names(7, one_byte_every=3)
    table = G.PathTable(paths)
    d_c, off, clen, ulen = torch.from_numpy(host).to(DEV), _i64(offs), _i64([len(y) for y in ys]), _i64(us)
    place, total = RM.layout(us, [len(p) for p in paths], RM.READN | RM.END)
    size = total + G.SLACK

    d_ref = torch.full((size,), POISON, dtype=torch.uint8, device=DEV)
    rplace = torch.zeros(7, dtype=torch.int64, device=DEV)
    rtotal = torch.zeros(1, dtype=torch.int64, device=DEV)
    rst = torch.full((7,), 0x7777, dtype=torch.int32, device=DEV)
    R.readn_batch(d_c, off, clen, ulen, _i64([20 + len(p) for p in paths]), d_ref, rplace, rtotal, rst)
    torch.cuda.synchronize()
    want = d_ref.cpu().numpy()
    assert rplace.cpu().tolist() == place and int(rtotal.item()) == total - 10
    for p, u, at in zip(paths, us, place):
        h = RM.header(RM.READN, p, u)
        assert (want[at - len(h):at] == POISON).all()
        want[at - len(h):at] = np.frombuffer(h, np.uint8)
    want[total - 10:total] = 0x30
    assert (want[place[5]:place[5] + us[5]] == POISON).all()   # (the refused file's range stays as it was)

    got, gplace, gtotal, st = G.call_reply(d_c, off, clen, ulen, table, RM.READN | RM.END, size)
    assert gtotal == total and list(gplace) == place
    bad = np.flatnonzero(got != want)
    assert not len(bad), (len(bad), int(bad[0]))
    assert list(st) == rst.cpu().tolist()
    assert st[1] & R.RLE_STATUS_OVERFLOW and st[4] & R.RLE_STATUS_SHORT and st[5] == R.RLE_STATUS_MISALIGNED
    assert all(st[i] == 0 for i in (0, 2, 3, 6))


def test_read_form_one_file():
    """READ_FILE's reply: "%010ld" and the content; the path arrays are NULL."""
    f = files(1)
    got = f.check(RM.READ)
    assert got[:10].tobytes() == b"%010d" % len(f.contents[0])


def tiny_contents(n):
    """n files of 0..3 bytes, every length among any four neighbours."""
    return [bytes(0x61 + (i + k) % 26 for k in range((i + i // 4) % 4)) for i in range(n)]


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_read_form_past_one_stride(n):
    """The READ form's gaps (ten per file, no path lengths read) at the edges of the layout's stride of
    1024 files and two strides on: reply, place and total are the model's, byte for byte."""
    contents = tiny_contents(n)
    lens = np.array([len(c) for c in contents])
    assert set(lens[:4]) == {0, 1, 2, 3}
    f = G.Files(G.names(n), contents)
    _, place, total = f.want(RM.READ)   # (the model's figures, against the closed form)
    assert total == 10 * n + lens.sum() and place == list(10 * np.arange(1, n + 1) + np.cumsum(lens) - lens)
    f.check(RM.READ)


def test_no_files():
    """n == 0: with the terminator the reply is the ten '0' (or NOFIT's nothing, under 10 bytes of
    capacity); without it *d_total = 0 and nothing is written."""
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    d_c = torch.zeros(16, dtype=torch.uint8, device=DEV)
    for form, cap, reply, total in ((RM.READN | RM.END, 10, b"0" * 10, 10), (RM.READN | RM.END, 9, b"", 10),
                                    (RM.READN, 0, b"", 0), (RM.READ, 0, b"", 0)):
        got, _, gtotal, _ = G.call_reply(d_c, empty, empty, empty, None, form, 10 + G.SLACK, out_cap=cap)
        assert gtotal == total, (form, cap)
        assert (got == G.image_of(reply, len(got))).all(), (form, cap)
