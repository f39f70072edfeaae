"""Refused buffers, in every launch form, among good ones.

The device API skips a buffer it cannot process and says so in its status word
(include/rle_mi355x.h): RLE_STATUS_MISALIGNED for an input or output slot that is not 16-byte
aligned and for a decode slot with cap < U, RLE_STATUS_TOOLARGE for a buffer whose segments do not
fit the tables a segmented launch sized from total_in_bytes.  Every kernel repeats the guard
(rle_kernels.hip, rle_coop.hip, rle_round.h, rle_segmented.hip -- where the summary, scan and write
launches must agree, through the per-buffer flag, to skip the buffer).  Here each refusal sits at
the first, a middle and the last index of a batch of valid buffers, in every form, and:

  refused buffer   status exactly the refusal's bit, encode out_len 0, every byte of its output
                   slot still the poison value;
  other buffers    status 0 and bytes equal to the oracle's, nothing written outside [0, C) / [0, U)
                   (the whole output image is compared, so a refusal that spoils a neighbour shows).

Slots have 32 spare bytes, so a buffer shifted off its alignment stays inside its own slot."""
import ctypes

import numpy as np
import pytest
import torch

import rle_mi355x as R
import rle_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0xA5
TILE = 1008
SIZES = [1008, 2500, 1007, 3024, 1900, 1024, 2017, 3000, 1300, 2048, 1009, 2999, 1600, 3023]   # 1-3 tiles
ROUND_MIN_IN = 8064   # the round kernel's threshold on the max_in_len hint (8 decode tiles)


def _i64(v):
    return torch.tensor(np.asarray(v, dtype=np.int64), device=DEV)


def batch(scale=1, seed=0):
    """14 valid buffers of mixed kinds, 1-3 tiles each (scale 4: 1-3 of the shortest segments)."""
    return [O.gen(i % 5, 300 + seed + i, s * scale) for i, s in enumerate(SIZES)]


def rotations(n, kinds):
    """Three launches' refusals {index: kind}: every kind once at the first, a middle and the last
    index."""
    at = (0, n // 2, n - 1)
    return [{at[j]: kinds[(j + r) % 3] for j in range(3)} for r in range(3)]


def _image(bufs, offs, total):
    host = np.zeros(total, np.uint8)
    for b, o in zip(bufs, offs):
        host[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return host


def _compare(got, want, offs, label):
    diff = np.nonzero(got != want)[0]
    if diff.size:
        p = int(diff[0])
        b = max(i for i, o in enumerate(offs) if o <= p) if p >= min(offs) else -1
        raise AssertionError(f"{label}: output byte {p} (slot of buffer {b}, +{p - offs[b]}) is {got[p]:#x}, "
                             f"expected {want[p]:#x}; {diff.size} bytes differ")


def encode_refusals(xs, bad, launch, label, preset=0x7777, want_status=R.RLE_STATUS_MISALIGNED):
    """One encode launch of xs with the buffers of `bad` ({index: "in" | "out" | "both" | "fit"})
    shifted off their alignment ("fit": left alone, refused for another reason)."""
    n, sizes = len(xs), [len(x) for x in xs]
    in_offs, in_total = R.layout(sizes, pad=32)
    out_offs, out_total = R.compressed_slots(sizes, pad=32)
    slots = list(out_offs)
    in_offs, out_offs = list(in_offs), list(out_offs)
    for i, kind in bad.items():
        in_offs[i] += 3 if kind in ("in", "both") else 0
        out_offs[i] += 5 if kind in ("out", "both") else 0
    d_in = torch.from_numpy(_image(xs, in_offs, in_total + 64)).to(DEV)
    d_out = torch.full((out_total + 64,), POISON, dtype=torch.uint8, device=DEV)
    out_len = torch.full((n,), 0x5555, dtype=torch.int64, device=DEV)
    status = torch.full((n,), preset, dtype=torch.int32, device=DEV)
    launch(d_in, _i64(in_offs), _i64(sizes), d_out, _i64(out_offs), out_len, status, max(sizes))
    torch.cuda.synchronize()
    st, ol = status.cpu().numpy().astype(np.uint32), out_len.cpu().numpy()
    want = np.full(out_total + 64, POISON, np.uint8)
    for i, x in enumerate(xs):
        if i in bad:
            assert st[i] == want_status and ol[i] == 0, (label, i, bad[i], hex(st[i]), ol[i])
        else:
            y = O.encode(x)
            assert st[i] == 0 and ol[i] == len(y), (label, i, hex(st[i]), ol[i], len(y))
            want[out_offs[i]:out_offs[i] + len(y)] = np.frombuffer(y, np.uint8)
    _compare(d_out.cpu().numpy(), want, slots, label)


def decode_refusals(xs, bad, launch, label, preset=0x7777, want_status=R.RLE_STATUS_MISALIGNED):
    """One decode launch of the oracle's streams of xs; bad: {index: "in" | "out" | "cap" | "fit"}
    ("cap": cap = U - 1)."""
    n, us = len(xs), [len(x) for x in xs]
    ys = [O.encode(x) for x in xs]
    cs = [len(y) for y in ys]
    in_offs, in_total = R.layout(cs, pad=32)
    out_offs, out_total = R.layout(us, pad=32)
    slots = list(out_offs)
    in_offs, out_offs, caps = list(in_offs), list(out_offs), list(us)
    for i, kind in bad.items():
        in_offs[i] += 3 if kind == "in" else 0
        out_offs[i] += 5 if kind == "out" else 0
        caps[i] -= 1 if kind == "cap" else 0
        assert kind != "cap" or us[i] > 0
    d_in = torch.from_numpy(_image(ys, in_offs, in_total + 64)).to(DEV)
    d_out = torch.full((out_total + 64,), POISON, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), preset, dtype=torch.int32, device=DEV)
    launch(d_in, _i64(in_offs), _i64(cs), d_out, _i64(out_offs), _i64(us), _i64(caps), status, max(cs), max(us))
    torch.cuda.synchronize()
    st = status.cpu().numpy().astype(np.uint32)
    want = np.full(out_total + 64, POISON, np.uint8)
    for i, x in enumerate(xs):
        if i in bad:
            assert st[i] == want_status, (label, i, bad[i], hex(st[i]))
        else:
            assert st[i] == 0, (label, i, hex(st[i]))
            want[out_offs[i]:out_offs[i] + len(x)] = np.frombuffer(x, np.uint8)
    _compare(d_out.cpu().numpy(), want, slots, label)


# ------------------------------------------------------------------ the launch forms
def _enc_wave(d_in, ioff, ilen, d_out, ooff, olen, st, mx):
    R.encode_batch(d_in, ioff, ilen, d_out, ooff, olen, st)


def _enc_sized(d_in, ioff, ilen, d_out, ooff, olen, st, mx):
    R.encode_batch(d_in, ioff, ilen, d_out, ooff, olen, st, max_len=mx)


def _enc_flag(d_in, ioff, ilen, d_out, ooff, olen, st, mx):
    R.encode_batch(d_in, ioff, ilen, d_out, ooff, olen, st, max_len=mx, flags=R.RLE_LAUNCH_STATUS_FLAG)


def _enc_seg(d_in, ioff, ilen, d_out, ooff, olen, st, mx):
    R.encode_batch_seg(d_in, ioff, ilen, d_out, ooff, olen, st)


def _dec_wave(d_in, ioff, ilen, d_out, ooff, ulen, cap, st, mi, mo):
    R.decode_batch(d_in, ioff, ilen, d_out, ooff, ulen, cap, st)


def _dec_sized(d_in, ioff, ilen, d_out, ooff, ulen, cap, st, mi, mo):
    R.decode_batch(d_in, ioff, ilen, d_out, ooff, ulen, cap, st, max_in_len=mi, max_out_len=mo)


def _dec_flag(d_in, ioff, ilen, d_out, ooff, ulen, cap, st, mi, mo):
    R.decode_batch(d_in, ioff, ilen, d_out, ooff, ulen, cap, st, max_in_len=mi, max_out_len=mo,
                   flags=R.RLE_LAUNCH_STATUS_FLAG)


def _dec_round(d_in, ioff, ilen, d_out, ooff, ulen, cap, st, mi, mo):
    R.decode_batch(d_in, ioff, ilen, d_out, ooff, ulen, cap, st, max_in_len=max(mi, ROUND_MIN_IN), max_out_len=mo)


def _dec_seg(d_in, ioff, ilen, d_out, ooff, ulen, cap, st, mi, mo):
    R.decode_batch_seg(d_in, ioff, ilen, d_out, ooff, ulen, cap, st)


@pytest.fixture
def always_coop():
    R.set_coop_mode(1)
    yield
    R.set_coop_mode(-1)


ENC_KINDS = ("in", "out", "both")
DEC_KINDS = ("in", "out", "cap")


def _small_batch_forms(enc, dec, label, preset=0x7777, scale=1):
    xs = batch(scale)
    for r, bad in enumerate(rotations(len(xs), ENC_KINDS)):
        encode_refusals(xs, bad, enc, f"{label} encode, rotation {r}", preset)
    for r, bad in enumerate(rotations(len(xs), DEC_KINDS)):
        decode_refusals(xs, bad, dec, f"{label} decode, rotation {r}", preset)


def test_one_wave():
    _small_batch_forms(_enc_wave, _dec_wave, "one wave")


def test_sized_cooperative(always_coop):
    _small_batch_forms(_enc_sized, _dec_sized, "cooperative")


def test_sized_cooperative_status_flag(always_coop):
    """RLE_LAUNCH_STATUS_FLAG: the status word is stored last, over a preset no status takes."""
    _small_batch_forms(_enc_flag, _dec_flag, "cooperative, status flag", preset=-1)


def test_segmented_many_buffers():
    """Buffers of 1-3 segments: the summary, scan and write launches agree to skip the refused ones."""
    _small_batch_forms(_enc_seg, _dec_seg, "segmented", scale=4)


def test_segmented_one_buffer():
    """n = 1 (no plan and map launches): each refusal alone, and a good buffer."""
    x = O.gen(2, 77, 3 * 4032 + 100)
    for kind in ENC_KINDS:
        encode_refusals([x], {0: kind}, _enc_seg, f"segmented n = 1 encode, {kind}")
    for kind in DEC_KINDS:
        decode_refusals([x], {0: kind}, _dec_seg, f"segmented n = 1 decode, {kind}")
    encode_refusals([x], {}, _enc_seg, "segmented n = 1 encode, good")
    decode_refusals([x], {}, _dec_seg, "segmented n = 1 decode, good")


def _tiny_batch(n):
    """n buffers of 1 .. 400 bytes and a few of 1-3 tiles, mixed kinds (uneven lengths, so the
    issue-order sort of a large decode has something to sort)."""
    rng = np.random.default_rng(n)
    sizes = rng.integers(1, 400, size=n)
    sizes[::97] = rng.integers(TILE, 3 * TILE, size=len(sizes[::97]))
    return [O.gen(i % 5, 7000 + i, int(s)) for i, s in enumerate(sizes)]


def test_decode_in_rounds():
    """set_dec_round(4), more than 4096 tiny buffers through the sized entry point (the hint is the
    round kernel's threshold)."""
    xs = _tiny_batch(4100)
    prev = R.set_dec_round(4)
    R.set_coop_mode(0)
    try:
        for r, bad in enumerate(rotations(len(xs), DEC_KINDS)):
            decode_refusals(xs, bad, _dec_round, f"rounds decode, rotation {r}")
    finally:
        R.set_coop_mode(-1)
        R.set_dec_round(prev)


def test_large_batch_one_wave_decode():
    """n = 4100: past one residency round the launch sorts its buffers into an issue order
    (rle_kernels.hip dec_order_local_kernel), and the sort sees the refused buffers."""
    xs = _tiny_batch(4100)
    for r, bad in enumerate(rotations(len(xs), DEC_KINDS)):
        decode_refusals(xs, bad, _dec_wave, f"large-batch decode, rotation {r}")


# ------------------------------------------------------------------ segments that do not fit
def seg_count(n, sb):
    """rle_segmented.hip seg_count: a remainder of 1-2 bytes joins the last segment."""
    return max(1, (n + sb - 3) // sb)


def refused_by_tables(lens, hint, sb):
    """rle_segmented.hip max_segments and the scans' `s1 > maxseg`: the buffers whose last segment's
    cumulative index exceeds the tables sized from the hint."""
    maxseg = hint // (sb - 2) + len(lens)
    out, cum = set(), 0
    for i, n in enumerate(lens):
        cum += seg_count(n, sb)
        if cum > maxseg:
            out.add(i)
    return out


def _short_hint_launches(xs, hint, label):
    """Encode xs, and decode its streams, with a total_in_bytes that is too small, in a workspace
    sized for the true total (larger than the launch requires: a wrong skip shows as wrong bytes or
    a wrong status, not as a stray write)."""
    n = len(xs)
    ys = [O.encode(x) for x in xs]
    for lens, run, form in (([len(x) for x in xs], encode_refusals, "encode"),
                            ([len(y) for y in ys], decode_refusals, "decode")):
        sb = R.seg_segment_bytes(hint)
        assert sb == R.seg_segment_bytes(sum(lens)) == 4 * TILE   # (the workspace's carve-up is the launch's)
        ws = R.seg_workspace(n, sum(lens), DEV)
        assert int(R.lib().rle_seg_workspace_bytes(n, sum(lens))) >= int(R.lib().rle_seg_workspace_bytes(n, hint))
        bad = {i: "fit" for i in refused_by_tables(lens, hint, sb)}
        assert bad and (len(bad) < n or n == 1), (label, form, sorted(bad))   # some refused, some not
        if form == "encode":
            launch = lambda d_in, ioff, ilen, d_out, ooff, olen, st, mx: R.encode_batch_seg(   # noqa: E731
                d_in, ioff, ilen, d_out, ooff, olen, st, total_in_bytes=hint, workspace=ws)
        else:
            launch = lambda d_in, ioff, ilen, d_out, ooff, ulen, cap, st, mi, mo: R.decode_batch_seg(   # noqa: E731
                d_in, ioff, ilen, d_out, ooff, ulen, cap, st, total_in_bytes=hint, workspace=ws)
        run(xs, bad, launch, f"{label} {form}, hint {hint}", want_status=R.RLE_STATUS_TOOLARGE)


@pytest.mark.parametrize("covered", [3, 4])
def test_total_in_bytes_too_small(covered):
    """8 buffers of about 3 segments each, total_in_bytes covering only the first 3 or 4: the
    buffers past the tables get RLE_STATUS_TOOLARGE (the documented contract), the others are
    exact."""
    xs = [O.gen(1 + i % 4, 900 + i, 3 * 4032 + (-700, 5, 900, -3, 0, 2, 1500, 3)[i]) for i in range(8)]
    _short_hint_launches(xs, sum(len(x) for x in xs[:covered]), f"{covered} of 8 covered")
    _short_hint_launches(xs, sum(len(O.encode(x)) for x in xs[:covered]), f"{covered} of 8 streams covered")


def test_total_in_bytes_too_small_one_buffer():
    """n = 1 with a hint of 1 byte: one segment fits, a second does not."""
    for size, refused in ((4032 + 2, False), (4032 + 3, True), (3 * 4032, True), (100, False)):
        x = O.gen(1, size, size)   # (random: the stream is no shorter, so the decode agrees)
        assert len(O.encode(x)) >= size
        assert (refused_by_tables([size], 1, 4 * TILE) == {0}) == refused
        if refused:
            _short_hint_launches([x], 1, f"one buffer of {size}")
        else:
            ws = R.seg_workspace(1, size, DEV)
            encode_refusals([x], {}, lambda d_in, ioff, ilen, d_out, ooff, olen, st, mx: R.encode_batch_seg(
                d_in, ioff, ilen, d_out, ooff, olen, st, total_in_bytes=1, workspace=ws), f"one buffer of {size} fits")


def test_total_in_bytes_too_small_many_buffers():
    """n = 1100 (past 1024 the plan kernel gives each thread more than one buffer), empty buffers
    among them, the hint covering the first 300."""
    rng = np.random.default_rng(1100)
    sizes = rng.integers(4500, 9000, size=1100)
    sizes[::9] = 0
    sizes[5::50] = rng.integers(1, 30, size=len(sizes[5::50]))
    xs = [O.gen(1 + i % 4, 1100 + i, int(s)) for i, s in enumerate(sizes)]
    _short_hint_launches(xs, sum(len(x) for x in xs[:300]), "300 of 1100 covered")


# ------------------------------------------------------------------ host refusals (nothing launched)
def test_host_refusals_launch_nothing():
    """A workspace one byte short is RLE_E_INVAL, n = 0 is RLE_OK; neither writes anything."""
    xs = batch(4)
    n, sizes = len(xs), [len(x) for x in xs]
    total = sum(sizes)
    in_offs, in_total = R.layout(sizes)
    out_offs, out_total = R.compressed_slots(sizes)
    d_in = torch.from_numpy(_image(xs, in_offs, in_total)).to(DEV)
    d_out = torch.full((out_total,), POISON, dtype=torch.uint8, device=DEV)
    out_len = torch.full((n,), 0x5555, dtype=torch.int64, device=DEV)
    status = torch.full((n,), 0x7777, dtype=torch.int32, device=DEV)
    ioff, ilen, ooff = _i64(in_offs), _i64(sizes), _i64(out_offs)
    need = int(R.lib().rle_seg_workspace_bytes(n, total))
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    wp = ctypes.c_void_p((ws.data_ptr() + 255) & ~255)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    L = R.lib()
    enc = lambda k, nbytes: L.rle_encode_batch_device_seg(p(d_in), p(ioff), p(ilen), p(d_out), p(ooff), p(out_len),   # noqa: E731
                                                          p(status), k, total, wp, nbytes, None)
    dec = lambda k, nbytes: L.rle_decode_batch_device_seg(p(d_in), p(ioff), p(ilen), p(d_out), p(ooff), p(ilen),   # noqa: E731
                                                          None, p(status), k, total, wp, nbytes, None)
    assert enc(n, need - 1) == R.RLE_E_INVAL and dec(n, need - 1) == R.RLE_E_INVAL
    assert enc(0, need) == R.RLE_OK and dec(0, need) == R.RLE_OK
    assert enc(0, 0) == R.RLE_OK
    torch.cuda.synchronize()
    assert (d_out == POISON).all() and (out_len == 0x5555).all() and (status == 0x7777).all()
    assert enc(n, need) == R.RLE_OK   # (the same arguments with the whole workspace do launch)
    torch.cuda.synchronize()
    assert (status == 0).all() and [int(v) for v in out_len.cpu()] == [len(O.encode(x)) for x in xs]
