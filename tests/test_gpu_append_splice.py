"""GPU tests of the fused append's splice routes (csrc/rle_route.h AppendRoute::SmallSplice and
LargeSplice) and of the device kernels behind them (csrc/rle_fileops.hip), which the systematic
append tests of test_gpu_fileops.py no longer reach: their streams of a few dozen bytes run the
Mapped route, where the final run, the splice head and the final-token check are never computed.

  (a) rle_append_prepare_device against numpy, at every small size and run start, around the
      4096-byte block edges of last_run_kernel and past the 4 MiB one pass of its grid covers;
  (b) the final-run battery behind carriers that put the call on either splice route, long final
      runs, whole-file runs and new content past the one-wave and the one-trip encode;
  (c) the tiny streams themselves through SmallSplice (RLE_MI355X_SMALL=copy, a fresh process);
  (d) streams that are not encoder output on both splice routes (the whole re-encode);
  (e) the documented exception: a hand-made stream with a canonical final token keeps its prefix.

Every case asserts the route it aims at from the drop-in's own accounting (routed_append), so a
changed threshold fails these tests instead of moving them off the splice; the shapes are also rows
of tests/test_route.py.  Bit-exact against the oracle everywhere."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import rle_mi355x as R
import rle_oracle as O
import test_gpu_fileops as F
from test_append_model import head_for

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SMALL, LARGE, MAPPED, NONE = "small_splice", "large_splice", "mapped", "none"


def routed_append(content, U, new):
    """One RLEappend through the C ABI.  Returns (stream, route, kept): the route classified from
    what the call added to the drop-in's accounting, kept = whether it returned old[0, C - tok) ‖ tail.
    SmallSplice stages round16(C) + 16 + round16(A) + 128 bytes, the other routes C + A; of those,
    LargeSplice spends time staging its input (or kept the prefix) and Mapped has no staging phase.
    Also checks the block's zero tail: 16 zero bytes past C', which the reference's decoder reads."""
    L = R.lib()
    C, A = len(content), len(new)
    c = ctypes.c_size_t(0)
    s0 = R.dropin_stats()
    p = L.RLEappend(content, C, U, new, A, ctypes.byref(c))
    s1 = R.dropin_stats()
    assert p, "RLEappend returned NULL"
    raw = ctypes.string_at(p, c.value + 16)
    R._libc.free(p)
    d = {k: s1[k] - s0[k] for k in s1}
    if d["calls_append"] != 1:   # U == 0: an RLEcompress of the new bytes
        route = NONE
    elif d["bytes_h2d"] != C + A:
        assert d["bytes_h2d"] == R.round16(C) + 16 + R.round16(A) + 128, d
        route = SMALL
    elif d["calls_append_spliced"] or d["ns_stage_in"]:
        route = LARGE
    else:
        route = MAPPED
    assert raw[c.value:] == bytes(16), (C, U, A, route, raw[c.value:])
    return raw[:c.value], route, d["calls_append_spliced"]


_CARRIER = {}


def carrier(route):
    """66 000 bytes that put an append behind them on `route` under default settings: zeros encode
    to 22 KB (a one-wave decode, below kSegDecodeBytes, of content past the mapped route's 64 KiB),
    random bytes to more than 32 KiB (a segmented decode).  Callers add b"xy"."""
    if route not in _CARRIER:
        _CARRIER[route] = bytes(66000) if route == SMALL else O.gen(1, 4242, 66000)
    return _CARRIER[route]


def check_spliced(old, new, route):
    """Encoder output `old` ‖ new on `route`, the prefix kept."""
    y = O.encode(old)
    got, rt, kept = routed_append(y, len(old), new)
    where = (len(y), len(old), len(new), old[-48:], new[:48])
    assert rt == route, (rt,) + where
    assert got == O.encode(old + new), where
    assert kept == 1, where
    return rt


ROUTES = [SMALL, LARGE]


# ---------------------------------------------------------------- (a) the device kernels
def _prepare_batch(cases):
    """rle_append_prepare_device on every (x, U) of cases, x a uint8 array of round16(U) + 16 bytes:
    all inputs in one device buffer, every call queued on the current stream, one copy back.
    Returns (meta [n, 4] uint64, head [n, 16] uint8)."""
    import torch
    n = len(cases)
    offs, total = R.layout([len(x) for x, _ in cases])
    host = np.zeros(total, np.uint8)
    for (x, _), o in zip(cases, offs):
        host[o:o + len(x)] = x
    d_mid = torch.from_numpy(host).cuda()
    d_head = torch.full((n, 16), 0xA5, dtype=torch.uint8, device="cuda")
    d_meta = torch.full((n, 4), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    for i, ((_, U), o) in enumerate(zip(cases, offs)):
        R.append_prepare(d_mid[o:], U, d_head[i], d_meta[i])
    torch.cuda.synchronize()
    return d_meta.cpu().numpy().view(np.uint64), d_head.cpu().numpy()


def _prepare_case(base, U, start, c):
    """U bytes whose final run c^(U - start) starts at `start`, in round16(U) + 16 bytes: below the
    run bytes of `base` (some equal to c) with a byte other than c just before it; past U, in the
    chunk the kernel loads whole and masks by < U, bytes other than c."""
    x = np.array(base[:R.round16(U) + 16], dtype=np.uint8)
    x[start:U] = c
    x[U:] = c ^ 0x5A
    if start:
        x[start - 1] = c ^ 1
    return x


def _prepare_expected(x, U):
    c = int(x[U - 1])
    ne = np.flatnonzero(x[:U] != c)
    start = int(ne[-1]) + 1 if len(ne) else 0
    r = (U - start - 1) % 9 + 1
    return start, r, head_for(c, r)


def _check_prepare(cases, info):
    meta, head = _prepare_batch(cases)
    for i, (x, U) in enumerate(cases):
        start, r, h = _prepare_expected(x, U)
        assert (int(meta[i, 0]), int(meta[i, 1])) == (start, r), (info[i], meta[i])
        assert head[i].tobytes() == h, (info[i], head[i].tobytes(), h)
        assert meta[i, 2:4].tobytes() == h, (info[i], meta[i, 2:4].tobytes(), h)


PREPARE_C = (0x00, 0xFF, ord("9"), ord("a"))


def test_prepare_every_small_size_and_start():
    """U = 1..48 (up to three 16-byte chunks, the last partly masked) with the final run starting at
    every position."""
    rng = np.random.default_rng(3)
    cases, info = [], []
    for c in PREPARE_C:
        base = rng.choice(np.array([c, c ^ 1, c ^ 0x80, c ^ 0x33], np.uint8), 80)
        for U in range(1, 49):
            for start in range(U):
                x = _prepare_case(base, U, start, c)
                assert _prepare_expected(x, U)[0] == start
                cases.append((x, U))
                info.append((c, U, start))
    assert len(cases) == 4 * 1176
    _check_prepare(cases, info)


def test_prepare_block_edges():
    """One block of last_run_kernel reads 4096 bytes counted down from round16(U), and the early exit
    compares the start found so far with those block tops: run starts around every multiple of 4096
    and around every block top, in one to four blocks."""
    rng = np.random.default_rng(4)
    cases, info = [], []
    for c in PREPARE_C:
        base = rng.choice(np.array([c, c ^ 1, c ^ 0x80, c ^ 0x33], np.uint8), 12288 + 32)
        for U in (4095, 4096, 4097, 8197, 12288):
            starts = {0, 1, 15, 16, 17, U - 1}
            for m in range(4096, U + 4096, 4096):
                starts |= {m - 1, m, m + 1}                                       # multiples of 4096
                starts |= {R.round16(U) - m - 1, R.round16(U) - m, R.round16(U) - m + 1}   # block tops
            for start in sorted(s for s in starts if 0 <= s < U):
                x = _prepare_case(base, U, start, c)
                assert _prepare_expected(x, U)[0] == start
                cases.append((x, U))
                info.append((c, U, start))
    _check_prepare(cases, info)


def test_prepare_past_one_grid_pass():
    """The grid is capped at 1024 blocks of 4096 bytes, so U = 4 MiB + 4096 + 7 is the smallest size
    whose stride loop runs a second time; that pass covers the lowest addresses (below 4112 here)."""
    U = (4 << 20) + 4096 + 7
    low = R.round16(U) - (4 << 20)
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, R.round16(U) + 16, dtype=np.uint8)
    for c in PREPARE_C:
        cases, info = [], []
        for start in (0, 5, 4099, low - 1, low, low + 1, (4 << 20) - 1, 4 << 20, U - 1):
            x = _prepare_case(base, U, start, c)
            assert _prepare_expected(x, U)[0] == start
            cases.append((x, U))
            info.append((c, U, start))
        _check_prepare(cases, info)


def test_prepare_invalid_arguments():
    import torch
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    m = torch.zeros(4, dtype=torch.int64, device="cuda")
    f, p, null = R.lib().rle_append_prepare_device, ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(0)
    mp, s = ctypes.c_void_p(m.data_ptr()), R._stream_ptr(None)
    RLE_E_INVAL = -1
    assert f(p, 0, p, mp, s) == RLE_E_INVAL
    assert f(null, 16, p, mp, s) == RLE_E_INVAL
    assert f(p, 16, null, mp, s) == RLE_E_INVAL
    assert f(p, 16, p, null, s) == RLE_E_INVAL
    with pytest.raises(R.RLEError):
        R.append_prepare(d, 0, d, m)
    torch.cuda.synchronize()
    assert not d.any() and not m.any()


# ---------------------------------------------------------------- (b) the tail battery on both splice routes
@pytest.mark.parametrize("route", ROUTES)
def test_splice_final_run_remainders(route):
    """test_append_final_run_remainders' cases (every r = 1..9, runs up to 40 bytes, which also start
    on and cross every 16-byte chunk offset) behind the carrier; each case already starts with b"xy"."""
    base = carrier(route)
    cases = F.final_run_cases()
    assert len(cases) == 1600
    for old, new in cases:
        check_spliced(base + old, new, route)


@pytest.mark.parametrize("route", ROUTES)
def test_splice_digit_heavy_streams(route):
    """test_append_digit_heavy_streams' generator behind the carrier, which ends in a byte (y) outside
    its alphabets."""
    base = carrier(route) + b"xy"
    for old, new in F.digit_heavy_cases():
        check_spliced(base + old, new, route)


@pytest.mark.parametrize("route", ROUTES)
def test_splice_long_final_runs(route):
    """Final runs around one, two and three blocks of last_run_kernel."""
    base = carrier(route) + b"xy"
    for ch in (b"q", b"9", b"\0"):
        for L in list(range(4090, 4101)) + [8191, 8192, 8193, 12287, 12288, 12289]:
            for new in (b"", ch, ch * 9, b"z", ch * 20 + b"z"):
                check_spliced(base + ch * L, new, route)


def test_splice_whole_file_runs():
    """A file that is one run (the final run starts at 0, the whole buffer is read): every remainder
    on SmallSplice (66 000..66 008 bytes) and on LargeSplice (100 000..100 008: a stream of 33 336
    bytes, past the one-wave decode)."""
    for L0, route in ((66000, SMALL), (100000, LARGE)):
        for ch in (b"q", b"9", b"\0"):
            for L in range(L0, L0 + 9):
                for new in (b"", ch * 3, b"z" + ch):
                    check_spliced(ch * L, new, route)


@pytest.mark.parametrize("route", ROUTES)
def test_splice_long_new_content(route):
    """New content at the last size of the one-wave tail encode (A = 49 135, SmallSplice behind the
    run carrier), the first segmented one (49 136: LargeSplice, a one-wave decode with a segmented
    encode) and past one trip (140 000: the encoded tail is fetched once its size is known, from the
    filler on); r = 1..9, the new bytes continue the run."""
    base = carrier(route) + b"xy"
    for A in (49135, 49136, 140000):
        for ch in (b"q", b"9"):
            for r in range(1, 10):
                new = ch * 7 + O.gen(2, 100 * r + A, A - 7)
                check_spliced(base + ch * r, new, SMALL if route == SMALL and A == 49135 else LARGE)


# ---------------------------------------------------------------- (c) the tiny battery on SmallSplice
_TINY_CODE = r'''
import sys
sys.path[:0] = sys.argv[1:4]
import rle_mi355x as R, rle_oracle as O
import test_gpu_fileops as F
import test_gpu_append_splice as S
n = {S.SMALL: 0, S.LARGE: 0, S.MAPPED: 0, S.NONE: 0, "kept": 0}
def run(content, U, new, want):
    got, rt, kept = S.routed_append(content, U, new)
    assert got == want, (content, U, new, got, want)
    if content and U:
        assert rt == S.SMALL, (content, U, new, rt)
    # encoder output: the stream is what the encoder gives for what it decodes to
    assert kept == int(bool(content) and bool(U) and O.encode(O.decode(content, U)[0]) == content), (content, U, new, kept)
    n[rt] += 1
    n["kept"] += kept
    return kept
for old, new in F.final_run_cases():
    y = O.encode(old)
    assert run(y, len(old), new, F.ref_append(y, len(old), new)) == 1
for old, new in F.digit_heavy_cases():
    assert run(O.encode(old), len(old), new, O.encode(old + new)) == 1
assert run(b"", 0, b"", b"") == 0
assert run(b"", 0, b"aaab", b"aa3b") == 0
assert run(b"", 5, b"ab", F.ref_append(b"", 5, b"ab")) == 0
for content, U, new in F.NOT_ENCODER_CASES:
    # (b"xx5yy7", 12) is what the encoder emits for x^5 y^7: it keeps its prefix; the others are rejects
    assert run(content, U, new, F.ref_append(content, U, new)) == (content == b"xx5yy7")
print("ok", n)
'''


def test_tiny_streams_on_small_splice_subprocess():
    """The three tiny tests' cases of test_gpu_fileops.py with the zero-copy form off
    (RLE_MI355X_SMALL=copy, read at library init: a fresh process), where they run SmallSplice: the
    splice head and the new bytes sit 16 bytes behind a stream of a few bytes, so the decode's chunk
    over-read sees the previous call's head."""
    env = dict(os.environ, RLE_MI355X_SMALL="copy")
    r = subprocess.run([sys.executable, "-c", _TINY_CODE, os.path.join(ROOT, "c-filestorage-server-and-client_amd"),
                        os.path.join(ROOT, "oracle"), HERE], env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.stdout[-1500:], r.stderr[-3000:])
    print(r.stdout.strip())


# ---------------------------------------------------------------- (d) not encoder output, on both splice routes
def _prime_mid():
    """Leaves this thread's decode buffer (d_mid) holding 70 000 bytes of 0xEE, so that a decode that
    does not zero what it leaves unwritten below U shows in the next call's result."""
    ee = b"\xee" * 70000
    got, rt, kept = routed_append(O.encode(ee), 70000, b"")
    assert (got, rt, kept) == (O.encode(ee), SMALL, 1)


def _not_encoder_streams(route):
    """(name, stream, U, expected route) behind the carrier of `route`."""
    plain = carrier(route)[:33000] + b"kkkk" + carrier(route)[33000:] + b"xy" + b"q" * 5
    y = O.encode(plain)
    N = len(plain)
    assert y.endswith(b"yqq5") and O.decode(y, N) == (plain, 0)
    i = y.find(b"kk4", 10000)
    assert i > 0 and y.count(b"kk4") == 1
    digit = y[:i + 2] + b":" + y[i + 3:]
    final = y[:-3] + b"qq3qq2"
    assert O.decode(final, N) == (plain, 0)
    # three whose decoded tail agrees with their final token, so that only the decode's status tells:
    # kk: decodes like kk9k (a count of 10); U past the end of a stream that ends in a zero run
    # (\0\05, then 9 more zeros: r is still 5); U inside a final run q^14 (qq9qq5 cut to q^5)
    ten = carrier(route)[:33000] + b"k" * 10 + carrier(route)[33000:] + b"xy" + b"q" * 5
    y10 = O.encode(ten)
    assert y10.count(b"kk9k") == 1
    same = y10.replace(b"kk9k", b"kk:")
    assert O.decode(same, len(ten)) == (ten, 0)
    zrun = carrier(route) + b"xy" + bytes(5)
    qrun = carrier(route) + b"xy" + b"q" * 14
    assert O.encode(zrun).endswith(b"y\0\0" + b"5") and O.encode(qrun).endswith(b"yqq9qq5")
    return [("bad count digit", digit, N, route),
            ("short", y, N + 37, route),
            ("overflow", y, N - 1, route),
            ("cut final pair", y[:-1], N, route),
            ("final token digit", final, N, route),
            ("bad count digit, the same bytes", same, len(ten), route),
            ("short, the zero tail agrees", O.encode(zrun), len(zrun) + 9, route),
            ("overflow, the cut run agrees", O.encode(qrun), len(qrun) - 9, route),
            ("no stream", b"", 70000, LARGE),
            ("U == 0", y, 0, NONE)]


@pytest.mark.parametrize("route", ROUTES)
def test_splice_rejects_streams_that_are_not_encoder_output(route):
    """The final-token check refuses each of these and the call re-encodes decode(old)[0, U) ‖ new
    whole (reencode_whole), as the reference does."""
    for name, content, U, want_route in _not_encoder_streams(route):
        for new in (b"", b"qqz", bytes(range(40))):
            _prime_mid()
            got, rt, kept = routed_append(content, U, new)
            if name == "no stream" and not new:
                assert rt in (LARGE, MAPPED)   # nothing is staged at all: the accounting cannot tell
            else:
                assert rt == want_route, (name, len(new), rt)
            assert got == F.ref_append(content, U, new), (name, len(content), U, new)
            assert kept == 0, (name, new)


# ---------------------------------------------------------------- (e) the documented exception
@pytest.mark.parametrize("route", ROUTES)
def test_splice_keeps_a_hand_made_prefix(route):
    """include/rle_fileops.h: "other hand-made streams keep their non-canonical prefix".  A stream
    with vv2vv2 (the encoder writes vv4) in the middle and a canonical final token decodes cleanly, so
    the splice may keep it; whatever the route does, the result decodes to the old content ‖ new."""
    a, b = carrier(route)[:33000], carrier(route)[33000:]
    assert a[-1:] != b"v" and b[:1] != b"v"
    for tail in (b"q", b"q" * 5, b"q" * 13):
        content = O.encode(a) + b"vv2vv2" + O.encode(b + b"xy" + tail)
        U = 66000 + 4 + 2 + len(tail)
        plain, st = O.decode(content, U)
        assert st == 0 and plain == a + b"vvvv" + b + b"xy" + tail
        for new in (b"", b"qqz", bytes(range(40))):
            got, rt, _ = routed_append(content, U, new)
            assert rt == route, (rt, len(tail), new)
            assert O.decode(got, U + len(new)) == (plain + new, 0), (len(tail), new)
