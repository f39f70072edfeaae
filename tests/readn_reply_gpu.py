"""GPU helpers of the reply tests (tests/test_gpu_readn_headers.py, test_gpu_readn_reply.py,
test_gpu_readn_reply_seg.py, test_gpu_readn_reply_replay.py): the path table on the device, batches of
files with names, and one call of a reply entry into a poisoned image.

Every comparison is of the whole image after a poison pre-fill, with SLACK poisoned bytes behind the
reply, so a stray byte shows anywhere."""
import numpy as np
import torch

import readn_reply_model as RM
import rle_mi355x as R
import rle_oracle as O
from test_gpu_parity import DEV, POISON, _i64
from test_gpu_readn_pack import Store

SLACK = 48   # poisoned bytes kept behind the reply
HINT = 1 << 20   # total_in_bytes of the segmented calls: the shortest segment, 4 tiles
SB = 4 * 1008


class PathTable:
    """Names on the device, one behind the other with 0..3 bytes of '#' between them, so that they
    start at every alignment; no NUL anywhere."""

    def __init__(self, paths):
        self.paths = paths
        blob, offs = bytearray(b"#"), []
        for i, p in enumerate(paths):
            offs.append(len(blob))
            blob += p + b"#" * (i % 4)
        self.d_paths = torch.from_numpy(np.frombuffer(bytes(blob) + b"#", np.uint8).copy()).to(DEV)
        self.off = _i64(offs)
        self.len = _i64([len(p) for p in paths])


def names(n, one_byte_every=5):
    """n names of lengths 1..40 or so, every one_byte_every-th a single byte."""
    out = []
    for i in range(n):
        if i % one_byte_every == 0:
            out.append(bytes([0x41 + i % 26]))
        else:
            out.append(b"/srv/" + b"d%d/" % (i % 7) * (i % 4) + b"f%d" % (i * 2654435761 % 10 ** (1 + i % 9)))
    return out


def small_contents(n, seed=0):
    """n files of 0..700 bytes of the synthetic kinds; every 4th is empty, so headers abut."""
    return [b"" if i % 4 == 1 else O.gen(1 + (i + seed) % 4, seed + i, 1 + (i * 37 + seed) % 700) for i in range(n)]


def image_of(reply, size):
    img = np.full(size, POISON, np.uint8)
    img[:len(reply)] = np.frombuffer(reply, np.uint8)
    return img


def call_reply(d_c, off, clen, ulen, table, form, size, out_cap=None, seg=False, hint=HINT, ws=None):
    """One call of rle_readn_reply_device (or its _seg form) into a poisoned image of `size` bytes:
    (image, place, total, status) as numpy / int."""
    n = off.numel()
    d_out = torch.full((size,), POISON, dtype=torch.uint8, device=DEV)
    place = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    total = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    status = torch.full((n,), 0x7777, dtype=torch.int32, device=DEV)
    tb = (None, None, None) if table is None else (table.d_paths, table.off, table.len)
    cap = size - SLACK if out_cap is None else out_cap
    if seg:
        assert R.seg_segment_bytes(hint) == SB and int(clen.sum().item()) <= hint
        R.readn_reply_seg(d_c, off, clen, ulen, *tb, d_out, place, total, status, form=form, out_cap=cap,
                          total_in_bytes=hint, ws=ws)
    else:
        R.readn_reply(d_c, off, clen, ulen, *tb, d_out, place, total, status, form=form, out_cap=cap)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), place.cpu().numpy(), int(total.item()), status.cpu().numpy()


class Files:
    """Files encoded on the device (test_gpu_readn_pack.Store: streams from the encode, d_ulen from the
    tail scan, so no length visits the host) with their names in a PathTable."""

    def __init__(self, paths, contents):
        assert len(paths) == len(contents)
        self.paths, self.contents = paths, contents
        self.store = Store(contents)
        self.table = PathTable(paths)
        self.n = len(paths)

    def want(self, form):
        """(reply bytes, place, total) of the model."""
        reply = RM.reply(self.paths, self.contents, form)
        place, total = RM.layout([len(c) for c in self.contents], [len(p) for p in self.paths], form)
        assert total == len(reply)
        return reply, place, total

    def run(self, form, size=None, **kw):
        s = self.store
        size = len(RM.reply(self.paths, self.contents, form)) + SLACK if size is None else size
        return call_reply(s.d_c, s.off, s.clen, s.ulen, None if form == RM.READ else self.table, form, size, **kw)

    def check(self, form, **kw):
        """The call's image is the model's reply over the poison, place and total the model's, every
        status word 0.  Returns the image."""
        reply, place, total = self.want(form)
        got, gplace, gtotal, st = self.run(form, **kw)
        assert gtotal == total and list(gplace) == place, (form, gtotal, total)
        bad = np.flatnonzero(got != image_of(reply, len(got)))
        assert not len(bad), (form, kw.get("seg"), f"{len(bad)} bytes differ, the first at {int(bad[0])}")
        assert (st == 0).all(), [(i, hex(int(s))) for i, s in enumerate(st) if s][:5]
        return got
