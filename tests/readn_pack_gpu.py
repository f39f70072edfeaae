"""GPU helpers of the packed read-N tests (tests/test_gpu_decode_packed.py, test_gpu_readn_pack.py,
test_gpu_readn_pack_replay.py): batches of stored streams with byte-granular destinations, the
expected reply image from the oracle, and the launch of rle_decode_packed_batch_device on them.

Every comparison is of the whole output image after a poison pre-fill, so a stray byte shows
anywhere: in front of a file, between files, behind the last one."""
import numpy as np
import torch

import rle_mi355x as R
import rle_oracle as O
from test_gpu_parity import DEV, POISON, _i64, _input_image

SLACK = 48   # poisoned bytes kept behind the last file
_ref = {}


def decoded(y, U):
    """(bytes, oracle status) of O.decode(y, U), computed once per (stream, U)."""
    k = (y, U)
    if k not in _ref:
        _ref[k] = O.decode(y, U)
    return _ref[k]


def literals(n, seed=0):
    """n bytes without two equal neighbours: n one-byte tokens, and the stream is the content."""
    return bytes(((i * 7 + seed) % 251 + 1) if i % 2 == 0 else 0xFE - (i % 3) for i in range(n))


def stream_of_length(kind, seed, C):
    """Content of the synthetic kind whose encoded stream is exactly C bytes long: a prefix of
    O.gen(kind, seed, .), found by bisection (the stream length grows with the prefix, by at most 2
    per byte), with one more byte that starts a new token where the prefix lands on C - 1."""
    x = O.gen(kind, seed, 6 * C + 256)   # (runs90 encodes to about 0.4 of its length)
    lo, hi = 0, len(x)   # len(encode(x[:lo])) <= C < len(encode(x[:hi]))
    assert len(O.encode(x)) > C
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if len(O.encode(x[:mid])) <= C:
            lo = mid
        else:
            hi = mid
    x = x[:lo]
    if len(O.encode(x)) == C - 1:
        x += bytes([(x[-1] + 1) & 0xFF])
    assert len(O.encode(x)) == C, (kind, seed, C)
    return x


class Batch:
    """Files (stream, U) with destinations in one reply image."""

    def __init__(self, pad=None):
        self.streams, self.us, self.places = [], [], []
        self.pos, self.pad = 0, pad

    def add(self, y, U, gap=0):
        """The next file, `gap` bytes behind the end of the one before."""
        self.pos += gap
        self.streams.append(y)
        self.us.append(U)
        self.places.append(self.pos)
        self.pos += U
        return len(self.us) - 1

    def add_at_phase(self, phase, y, U, gap=0, seed=0):
        """The next file at destination phase `phase` (mod 16): a filler file of 0..15 bytes in front
        of it takes up the difference, so that every file still abuts its neighbours (or lies `gap`
        bytes behind them)."""
        f = (phase - 2 * gap - self.pos) % 16
        x = O.gen(1 + seed % 4, 900 + seed, f)
        self.add(O.encode(x), f, gap)
        i = self.add(y, U, gap)
        assert self.places[i] % 16 == phase
        return i

    @property
    def n(self):
        return len(self.us)

    @property
    def size(self):
        return self.pos + SLACK

    def want(self, skip=()):
        """(image, oracle status words): every file's O.decode(y, U) at its place over the poison; the
        files in `skip` leave theirs."""
        img = np.full(self.size, POISON, np.uint8)
        ost = []
        for i, (y, U, p) in enumerate(zip(self.streams, self.us, self.places)):
            ref, st = decoded(y, U)
            ost.append(st)
            if i not in skip:
                img[p:p + U] = np.frombuffer(ref, np.uint8)
        return img, ost

    def upload(self):
        self.in_offs, host = _input_image(self.streams, self.pad)
        self.d_in = torch.from_numpy(host).to(DEV)

    def run(self, in_offs=None, us=None):
        """One rle_decode_packed_batch_device launch into a poisoned image: (image, status)."""
        self.upload()
        d_out = torch.full((self.size,), POISON, dtype=torch.uint8, device=DEV)
        status = torch.full((self.n,), 0x7777, dtype=torch.int32, device=DEV)
        R.decode_packed(self.d_in, _i64(self.in_offs if in_offs is None else in_offs),
                        _i64([len(s) for s in self.streams]), d_out, _i64(self.places),
                        _i64(self.us if us is None else us), status)
        torch.cuda.synchronize()
        return d_out.cpu().numpy(), status.cpu().numpy()

    def compare(self, label, got, want):
        bad = np.flatnonzero(got != want)
        if len(bad):
            b = int(bad[0])
            owner = [i for i, (p, U) in enumerate(zip(self.places, self.us)) if p <= b < p + U]
            i = owner[0] if owner else None
            raise AssertionError((label, f"{len(bad)} bytes differ, the first at {b}", "file", i,
                                  None if i is None else (self.places[i], self.us[i], len(self.streams[i])),
                                  hex(int(got[b])), hex(int(want[b]))))

    def check(self, label, clean=True):
        """Run, compare the image; clean: every status word is 0 (encoder output at its own length);
        else the OVERFLOW bit is the oracle's.  Returns the status words."""
        got, st = self.run()
        want, ost = self.want()
        self.compare(label, got, want)
        if clean:
            assert (st == 0).all(), (label, [(i, hex(int(s))) for i, s in enumerate(st) if s][:5])
        else:
            bad = [i for i in range(self.n) if (int(st[i]) & R.RLE_STATUS_OVERFLOW) != (ost[i] & 1)]
            assert not bad, (label, bad[:5])
        return st
