"""GPU tests of rle_readn_reply_device_seg (include/rle_mi355x.h, DESIGN.md §4c "Headers and
terminator"): the replies of tests/test_gpu_readn_reply.py through the segmented entry, at the
shortest segment (4 tiles), equal the one-wave entry's byte for byte and word for word; files of
several segments and a serial-flagged file among them; capacity; n == 0."""
import numpy as np
import pytest
import torch

import readn_pack_gpu as P
import readn_reply_gpu as G
import readn_reply_model as RM
import rle_mi355x as R
import rle_oracle as O
from test_gpu_parity import DEV, POISON, _i64, _input_image
from test_gpu_readn_reply import NS, files

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("end", [False, True])
@pytest.mark.parametrize("n", NS)
def test_seg_reply_is_the_one_wave_entrys(n, end):
    f = files(n)
    form = RM.READN | (RM.END if end else 0)
    one = f.run(form)
    seg = f.run(form, seg=True)
    assert (seg[0] == one[0]).all() and list(seg[1]) == list(one[1]) and seg[2] == one[2]
    assert list(seg[3]) == list(one[3])
    f.check(form, seg=True)


def test_seg_read_form_and_capacity():
    f = files(1)
    f.check(RM.READ, seg=True)
    f = files(65)
    form = RM.READN | RM.END
    reply, place, total = f.want(form)
    f.check(form, size=total + G.SLACK, out_cap=total, seg=True)
    for cap in (total - 1, total - 10):
        got, gplace, gtotal, st = f.run(form, size=total + G.SLACK, out_cap=cap, seg=True)
        assert list(st) == [R.RLE_STATUS_NOFIT] * f.n and (got == POISON).all()
        assert gtotal == total and list(gplace) == place


def test_seg_many_segments_and_a_serial_file():
    """Files of one to four 4-tile segments (literal content: the stream is the content), a file whose
    length is short of its stream (OVERFLOW, decoded by the exact serial path) and a misaligned one:
    the model's headers around the packed decode's bytes, and the one-wave entry's reply and words."""
    xs = [P.literals(G.SB * 3 + 500, 1), O.gen(2, 7, 900), P.literals(G.SB * 2 + 17, 2), b"",
          P.literals(G.SB + 99, 3), O.gen(3, 9, 5000), P.literals(G.SB * 2 + 3000, 4)]
    ys = [O.encode(x) for x in xs]
    segs = [max(1, (len(y) + G.SB - 3) // G.SB) for y in ys]
    assert max(segs) >= 4 and sum(s >= 3 for s in segs) >= 2, segs
    us = [len(x) for x in xs]
    us[2] -= 9    # OVERFLOW, serial
    offs, host = _input_image(ys, None)
    offs = list(offs)
    offs[4] += 3  # MISALIGNED
    paths = G.names(7, one_byte_every=3)
    table = G.PathTable(paths)
    d_c, off, clen, ulen = torch.from_numpy(host).to(DEV), _i64(offs), _i64([len(y) for y in ys]), _i64(us)
    form = RM.READN | RM.END
    place, total = RM.layout(us, [len(p) for p in paths], form)
    size = total + G.SLACK
    one = G.call_reply(d_c, off, clen, ulen, table, form, size)
    seg = G.call_reply(d_c, off, clen, ulen, table, form, size, seg=True)
    assert seg[2] == one[2] == total and list(seg[1]) == list(one[1]) == place
    assert list(seg[3]) == list(one[3])
    st = seg[3]
    assert st[2] & R.RLE_STATUS_SERIAL and st[2] & R.RLE_STATUS_OVERFLOW and st[4] == R.RLE_STATUS_MISALIGNED
    assert all(st[i] == 0 for i in (0, 1, 3, 5, 6))
    bad = np.flatnonzero(seg[0] != one[0])
    assert not len(bad), (len(bad), int(bad[0]))
    want = np.full(size, POISON, np.uint8)
    for i, (p, x, u, at) in enumerate(zip(paths, xs, us, place)):
        h = RM.header(form, p, u)
        want[at - len(h):at] = np.frombuffer(h, np.uint8)
        if i != 4:
            want[at:at + u] = np.frombuffer(x[:u], np.uint8)
    want[total - 10:total] = 0x30
    bad = np.flatnonzero(seg[0] != want)
    assert not len(bad), (len(bad), int(bad[0]))


def test_seg_no_files():
    """n == 0 needs no workspace: the terminator alone, or nothing."""
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    d_c = torch.zeros(16, dtype=torch.uint8, device=DEV)
    for form, cap, reply, total in ((RM.READN | RM.END, 10, b"0" * 10, 10), (RM.READN | RM.END, 9, b"", 10),
                                    (RM.READN, 0, b"", 0)):
        got, _, gtotal, _ = G.call_reply(d_c, empty, empty, empty, None, form, 10 + G.SLACK, out_cap=cap, seg=True)
        assert gtotal == total and (got == G.image_of(reply, len(got))).all(), (form, cap)
