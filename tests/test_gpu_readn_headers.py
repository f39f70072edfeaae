"""GPU tests of rle_readn_headers_device (include/rle_mi355x.h, DESIGN.md §4c "Headers and
terminator"): the header writer alone, at places the test gives.  File i's header goes to exactly
[place[i] - gap_i, place[i]) and the terminator to the ten bytes behind the last file; every other
byte of the image, the contents' ranges included, keeps its poison."""
import numpy as np
import pytest
import torch

import readn_reply_model as RM
import rle_mi355x as R
from readn_reply_gpu import SLACK, PathTable
from test_gpu_parity import DEV, POISON, _i64

pytestmark = pytest.mark.gpu
US = (0, 9, 10, 99, 100, 9999, 10000, 65536, 100000)


def run_headers(paths, ulen, place, form, size):
    """One rle_readn_headers_device call into a poisoned image: the image."""
    table = PathTable(paths)
    d_out = torch.full((size,), POISON, dtype=torch.uint8, device=DEV)
    tb = (None, None, None) if form == RM.READ else (table.d_paths, table.off, table.len)
    R.readn_headers(*tb, _i64(ulen), d_out, _i64(place), form=form)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def want_headers(paths, ulen, place, form, size):
    img = np.full(size, POISON, np.uint8)
    for p, u, at in zip(paths, ulen, place):
        h = RM.header(form, p, u)
        img[at - len(h):at] = np.frombuffer(h, np.uint8)
    if form & RM.END:
        at = place[-1] + ulen[-1] if place else 0
        img[at:at + 10] = 0x30
    return img


def compare(label, got, want):
    bad = np.flatnonzero(got != want)
    assert not len(bad), (label, f"{len(bad)} bytes differ, the first at {int(bad[0])}",
                          got[max(0, int(bad[0]) - 8):int(bad[0]) + 8].tobytes())


def phase_files():
    """Path lengths 1..48 and a 255-byte path, the decoded lengths of US in turn; one name is made of
    the poison value."""
    paths = [bytes((0x61 + (i + k) % 26) for k in range(L)) for i, L in enumerate(range(1, 49))]
    paths.append(bytes(0x30 + k % 75 for k in range(255)))
    paths[20] = bytes([POISON]) * len(paths[20])
    ulen = [US[(2 * i + i // 9) % len(US)] for i in range(len(paths))]
    assert set(ulen) == set(US)
    return paths, ulen


@pytest.mark.parametrize("form", RM.FORMS)
def test_headers_at_every_phase(form):
    paths, ulen = phase_files()
    place, total = RM.layout(ulen, [len(p) for p in paths], form)
    if form != RM.READ:   # headers and contents start at every phase of a 16-byte chunk
        assert {p % 16 for p in place} == set(range(16))
        assert {(p - 20 - len(s)) % 16 for p, s in zip(place, paths)} == set(range(16))
        assert {(p - 10) % 16 for p in place} == set(range(16))   # (the second field)
    size = total + SLACK
    got = run_headers(paths, ulen, place, form, size)
    want = want_headers(paths, ulen, place, form, size)
    assert (want[total:] == POISON).all() and (form & RM.END == 0 or (want[total - 10:total] == 0x30).all())
    compare(form, got, want)


def test_read_form_at_every_phase():
    """The READ form's ten bytes in front of places at every phase; no path array is read (all NULL)."""
    ulen = [US[i % len(US)] for i in range(32)]
    place = [40 * i + 10 + i % 16 for i in range(32)]
    assert {p % 16 for p in place} == set(range(16))
    size = place[-1] + SLACK
    compare("read", run_headers([b""] * 32, ulen, place, RM.READ, size), want_headers([b""] * 32, ulen, place, RM.READ, size))


@pytest.mark.parametrize("form", RM.FORMS)
def test_low_ten_digits_of_a_long_length(form):
    """d_ulen = 10^10 + 7 (and 5 * 10^9, past 2^32 but within ten digits, and 2^64 - 1) at hand-given
    places: the low ten decimal digits; with the terminator, its place is d_place[n-1] + d_ulen[n-1],
    so the last file is a short one."""
    paths = [b"/big/one", b"q", b"/edge", b"/last"]
    ulen = [10 ** 10 + 7, 5 * 10 ** 9, 2 ** 64 - 1, 33]
    place = [61, 130, 199, 270]
    size = 270 + 33 + 10 + SLACK
    d_ulen = np.array(ulen, np.uint64).view(np.int64)
    got = run_headers(paths, d_ulen, place, form, size)
    want = want_headers(paths, ulen, place, form, size)
    assert want[51:61].tobytes() == b"0000000007"
    assert want[120:130].tobytes() == b"5000000000" and want[189:199].tobytes() == b"%010d" % ((2 ** 64 - 1) % 10 ** 10)
    compare(form, got, want)


def test_terminator_alone_and_nothing_at_all():
    """n == 0: with the terminator the ten '0' at the start of d_out, without it no launch at all."""
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    for form, want in ((RM.READN | RM.END, b"0" * 10), (RM.READN, b""), (RM.READ, b"")):
        d_out = torch.full((10 + SLACK,), POISON, dtype=torch.uint8, device=DEV)
        R.readn_headers(None, None, None, empty, d_out, empty, form=form)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert got[:len(want)].tobytes() == want and (got[len(want):] == POISON).all(), form
