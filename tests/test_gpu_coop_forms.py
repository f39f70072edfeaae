"""GPU parity of every form of the cooperative kernels (csrc/rle_coop.hip), batched and by value.

The kernels are a table of template instantiations -- encode (W, R): W waves, R rounds; decode
(W, Umax, R): also the staging size -- chosen from a launch's size hints by csrc/rle_coop_limits.h.
tests/coop_forms.py builds each form's cases (sizes at every tile count, runs at every wave and round
edge, carried run starts, the staging's extremes; streams the encoder never emits at the first, last
wave, round and last tile edges, the form's limits, one-tile streams, buffers past the form); here
each form runs them

  batched   in one launch under the form's largest hint and again under its smallest (the library's
            query rle_mi355x_coop_form says both select the form), cooperative mode 1;
  by value  a rotating sample of about 40 cases, one rle_encode_coop_one / rle_decode_coop_one call
            each (the kernels the drop-in's single calls run), with and without
            RLE_LAUNCH_STATUS_FLAG: the same bytes, length and status as the batched run.

Every comparison is bit-exact against the oracle: encode byte for byte with status 0 and nothing
written past C (slots poisoned); decode over the whole cap, the OVERFLOW bit, and the routing
condition of tests/test_gpu_stream_family.py check() (tiled-class without RLE_STATUS_SERIAL,
serial-class with it).  Each test prints its form and case counts."""
import numpy as np
import pytest
import torch

import coop_forms as CF
import rle_mi355x as R
import rle_oracle as O
from test_gpu_parity import DEV, POISON, gpu_encode
from test_gpu_stream_family import check, decode

pytestmark = pytest.mark.gpu
_id = lambda f: "x".join(str(v) for v in f)
SAMPLE = 40
UNSET = 0x7777


@pytest.fixture(autouse=True, scope="module")
def _always_coop():
    R.set_coop_mode(1)
    yield
    R.set_coop_mode(-1)


def _dev_bytes(b, extra=16):
    """b on the device, zero-padded to a multiple of 16 and `extra` bytes more."""
    host = np.zeros(R.round16(len(b)) + extra, np.uint8)
    host[:len(b)] = np.frombuffer(b, np.uint8)
    return torch.from_numpy(host).to(DEV)


# ------------------------------------------------------------------ encode
def _encode_one(x, flags):
    U = len(x)
    room = R.max_compressed_size(U)
    d_src = _dev_bytes(x)
    d_dst = torch.full((R.round16(room) + 64,), POISON, dtype=torch.uint8, device=DEV)
    out_len = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    status = torch.full((1,), UNSET, dtype=torch.int32, device=DEV)
    rc = R.encode_coop_one(d_src, d_dst, U, out_len, status, flags=flags)
    torch.cuda.synchronize()
    return rc, d_dst.cpu().numpy(), int(out_len.item()), int(status.item())


@pytest.mark.parametrize("form", CF.ENC_FORMS, ids=_id)
def test_encode_form(form):
    cases = CF.enc_cases(form)
    xs = [c.data for c in cases]
    refs = [O.encode(x) for x in xs]
    for hint in CF.enc_hints(form):
        assert R.coop_enc_form(hint) == form, hint
        ys, st = gpu_encode(xs, max_len=hint)   # (asserts that nothing was written past C)
        bad = [cases[i] for i in range(len(xs)) if ys[i] != refs[i] or st[i] != 0]
        assert not bad, (hint, len(bad), bad[:4])
    own = [i for i, x in enumerate(xs) if R.coop_enc_form(len(x)) == form]
    sample = CF.rotating_sample(own, lambda i: cases[i].group, SAMPLE, CF.ENC_FORMS.index(form))
    assert len(sample) == SAMPLE and len({cases[i].group for i in sample}) >= 4, len(sample)
    for flags in (0, R.RLE_LAUNCH_STATUS_FLAG):
        for i in sample:
            rc, out, n, s = _encode_one(xs[i], flags)
            assert rc == 1 and n == len(refs[i]) and s == 0, (cases[i], flags, rc, n, s)
            assert out[:n].tobytes() == refs[i], (cases[i], flags)
            assert (out[n:] == POISON).all(), (cases[i], flags)
    print(f"encode form {form}: {len(cases)} cases batched under hints {CF.enc_hints(form)}, "
          f"{len(sample)} by value x 2 flag settings")


@pytest.mark.parametrize("U", [0, 1, 1023, 1024, 65537, 1 << 20])
def test_encode_by_value_declines_other_sizes(U):
    """Sizes outside the cooperative range: 0, nothing launched, output, length and status untouched."""
    assert R.coop_enc_form(U) is None
    for flags in (0, R.RLE_LAUNCH_STATUS_FLAG):
        rc, out, n, s = _encode_one(bytes(U), flags)
        assert rc == 0 and n == -1 and s == UNSET and (out == POISON).all(), (U, flags, rc, n, s)


# ------------------------------------------------------------------ decode
def _decode_one(c, flags, C=None, U=None):
    C = len(c.stream) if C is None else C
    U = c.U if U is None else U
    cap = max(c.cap, U)
    d_src = _dev_bytes(c.stream)
    d_dst = torch.full((R.round16(cap) + 64,), POISON, dtype=torch.uint8, device=DEV)
    d_dst[:cap] = 0   # (the reference's calloc; past cap: the guard)
    status = torch.full((1,), UNSET, dtype=torch.int32, device=DEV)
    rc = R.decode_coop_one(d_src, d_dst, C, U, cap, status, flags=flags)
    torch.cuda.synchronize()
    return rc, d_dst.cpu().numpy(), int(status.item()), cap


@pytest.mark.parametrize("form", CF.DEC_FORMS, ids=_id)
def test_decode_form(form):
    cases = CF.dec_cases(form)
    hi, lo = CF.dec_hints(form)
    assert R.coop_dec_form(*hi) == form and R.coop_dec_form(*lo) == form
    dec, st = decode(cases, max_in_len=hi[0], max_out_len=hi[1])
    check(cases, dec, st, routing=True, pins=False)
    for c, d, s in zip(cases, dec, st):
        if c.valid:
            assert int(s) == 0, (c, hex(int(s)))
        if c.group == "short":
            assert int(s) == R.RLE_STATUS_SHORT, (c, hex(int(s)))
    # the smallest hints select the same kernel: the same bytes and status words
    dec2, st2 = decode(cases, max_in_len=lo[0], max_out_len=lo[1])
    bad = [cases[i] for i in range(len(cases)) if dec2[i] != dec[i] or st2[i] != st[i]]
    assert not bad, (lo, len(bad), bad[:4])
    own = [i for i, c in enumerate(cases) if R.coop_dec_form(len(c.stream), c.U) == form]
    sample = CF.rotating_sample(own, lambda i: (cases[i].group, cases[i].serial), SAMPLE, CF.DEC_FORMS.index(form))
    assert len(sample) == SAMPLE, len(sample)
    assert any(cases[i].serial for i in sample) and any(not cases[i].serial for i in sample)
    for flags in (0, R.RLE_LAUNCH_STATUS_FLAG):
        for i in sample:
            rc, out, s, cap = _decode_one(cases[i], flags)
            assert rc == 1 and s == int(st[i]), (cases[i], flags, rc, hex(s), hex(int(st[i])))
            assert out[:cap].tobytes() == dec[i], (cases[i], flags)
            assert (out[cap:] == POISON).all(), (cases[i], flags)
    print(f"decode form {form}: {len(cases)} cases batched under hints {hi} and {lo}, "
          f"{len(sample)} by value x 2 flag settings")


@pytest.mark.parametrize("C,U", [(0, 0), (1008, 1008), (1008, 65536), (80641, 60000), (2000, 65537), (80641, 65537)])
def test_decode_by_value_declines_other_sizes(C, U):
    assert R.coop_dec_form(C, U) is None
    c = CF.DecCase("declined", bytes(C), U, U, False, "declined")
    for flags in (0, R.RLE_LAUNCH_STATUS_FLAG):
        rc, out, s, cap = _decode_one(c, flags)
        assert rc == 0 and s == UNSET, (C, U, flags, rc, hex(s))
        assert not out[:cap].any() and (out[cap:] == POISON).all(), (C, U, flags)


# ------------------------------------------------------------------ the write-back store policy
def test_write_back_policy_launches():
    """Past 4096 buffers the cooperative launches store write-back instead of write-through
    (rle_coop.hip coop_store_policy): 4097 buffers through the 4-wave forms."""
    n = 4097
    ec = [c for c in CF.enc_cases((4, 1)) if c.fits]
    xs = [ec[i % len(ec)].data for i in range(n)]
    assert R.coop_enc_form(4096) == (4, 1)
    ys, st = gpu_encode(xs, max_len=4096)
    assert (st == 0).all()
    refs = [O.encode(c.data) for c in ec]
    bad = [i for i in range(n) if ys[i] != refs[i % len(ec)]]
    assert not bad, (len(bad), ec[bad[0] % len(ec)])
    form = (4, 32768, 1)
    dc = CF.dec_cases(form)
    cs = [dc[i % len(dc)] for i in range(n)]
    hi, _ = CF.dec_hints(form)
    assert R.coop_dec_form(*hi) == form
    dec, st = decode(cs, max_in_len=hi[0], max_out_len=hi[1])
    check(cs, dec, st, routing=True, pins=False)
    print(f"write-back: {n} buffers, encode form (4, 1) and decode form {form}")
