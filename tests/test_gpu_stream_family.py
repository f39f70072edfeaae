"""GPU decode parity for streams the encoder never emits, placed at every decode form's own edges.

tests/stream_family.py builds the cases: a valid prefix of exactly p bytes, then a probe (adjacent
pair tokens of one value, "vv2v", mixed counts inside a uniform tile, count digits '0' '1' ':' '/'
0x00 0x7F 0x80 0xB5 0xFF 'a', or the stream cut after "v" / "vv"), then nothing or one more tile
and a half of valid tokens; U at, below and above the decoded length; cap with room for every
write, and once cap = U (exact fit, or the OVERFLOW truncation).  p walks the lane edge (the count
digit comes from the next lane), the tile edges (from the next tile's lookahead lane), the segment,
round and stream ends of each form:

  one wave, 192 chunks   decode_batch, n <= 4096
  one wave, 96 chunks    decode_batch, n >= 4097 (rle_kernels.hip decode_launch `large`)
  cooperative            set_coop_mode(1) + the batch's size hints; a later round past 16 tiles
  segmented              decode_batch_seg, many buffers and one buffer (RLE_SEG_ONE)
  rounds                 set_dec_round(4 / 8 / 16), more than 4096 buffers
  drop-in                RLEdecompress with E = C + 16, RLEdecompressN (cap = U)

Every output is compared byte for byte over the whole cap with the oracle's (outputs pre-filled
with zeros, as the reference's calloc), the OVERFLOW bit with the oracle's status, and -- since the
GPU machine has no reference -- the sha256 of stream | U | device output per position with the pins
tests/golden/make_golden.py took from the compiled reference (tests/golden/stream_family.json).

Routing: in the one-wave and cooperative forms every tiled-class case (stream_family.needs_serial
false) must come back without RLE_STATUS_SERIAL and every serial-class case with it, so a kernel
that declined everything does not pass.  The predicate is the rule documented at
csrc/rle_device.h dec_serial (counts outside '2'..'9' -- '1' is never emitted as a count and the
digit test declines it -- unbounded counts before the last token, or a decoded size past U); the
kernels agreed with it as written, neither side was changed.  The round form decides per buffer in
the same way and holds the same condition; the segmented form asserts serial-class => SERIAL only
(its scan sends a whole buffer to the serial path when a taken phase declines in any segment)."""
import json
import os

import pytest
import torch

import rle_mi355x as R
import rle_oracle as O
import stream_family as F
from conftest import GOLDEN
from test_gpu_parity import gpu_decode

pytestmark = pytest.mark.gpu
INFO = R.RLE_STATUS_OVERFLOW | R.RLE_STATUS_SERIAL | R.RLE_STATUS_SHORT

with open(os.path.join(GOLDEN, "stream_family.json")) as _f:
    PINS = json.load(_f)["positions"]


def check(cases, dec, st, routing, pins=True):
    """Bytes over the whole cap, the OVERFLOW bit, the routing condition and (for whole families in
    position order) the reference's pins."""
    tiled_serial = 0
    for i, c in enumerate(cases):
        ref, ost = O.decode(c.stream, c.U, c.cap)
        assert dec[i] == ref, (i, c)
        s = int(st[i])
        assert s & ~INFO == 0, (i, c, hex(s))
        assert (s & R.RLE_STATUS_OVERFLOW) == (ost & 1), (i, c, hex(s))
        if c.serial:
            assert s & R.RLE_STATUS_SERIAL, (i, c, hex(s))
        elif s & R.RLE_STATUS_SERIAL:
            assert not routing, (i, c, hex(s))
            tiled_serial += 1
    if pins:
        i = 0
        while i < len(cases):
            fam = F.family(cases[i].p)
            assert cases[i] is fam[0] and cases[i + len(fam) - 1] is fam[-1]
            assert F.pin(fam, dec[i:i + len(fam)]) == PINS[str(fam[0].p)], fam[0].p
            i += len(fam)
    nser = sum(c.serial for c in cases)
    print(f"{len(cases)} cases: {len(cases) - nser} tiled-class ({tiled_serial} came back SERIAL), {nser} serial-class")


def decode(cases, **kw):
    return gpu_decode([c.stream for c in cases], [c.U for c in cases], [c.cap for c in cases], poison=False, **kw)


# ------------------------------------------------------------------ one wave per buffer
@pytest.mark.parametrize("group", sorted(F.WAVE_GROUPS))
def test_one_wave_192_chunks(group):
    cases = F.cases(F.WAVE_GROUPS[group])
    assert len(cases) <= 4096
    dec, st = decode(cases)
    check(cases, dec, st, routing=True)


def test_one_wave_96_chunks():
    """Past 4096 buffers the launcher takes the 96-chunk staging: every one-wave position in one
    batch (the all-pairs prefixes decode to 3 x their length: several passes of that staging)."""
    cases = F.cases([p for g in sorted(F.WAVE_GROUPS) for p in F.WAVE_GROUPS[g]])
    assert len(cases) >= 4097
    dec, st = decode(cases)
    check(cases, dec, st, routing=True)


# ------------------------------------------------------------------ cooperative
@pytest.fixture
def always_coop():
    R.set_coop_mode(1)
    yield
    R.set_coop_mode(-1)


@pytest.mark.parametrize("group", sorted(F.COOP_GROUPS))
def test_cooperative(group, always_coop):
    """One workgroup per buffer, a wave per tile: the probe at the edge between wave k - 1 and wave k
    (the phase map, decoded length, serial flag and tail byte cross through LDS, rle_coop.hip
    dec_coop_body), and past 16 tiles at the edge between two rounds.  The hints are the batch's
    own largest sizes, so every buffer stays inside the kernel's tiles and staging."""
    cases = F.cases(F.COOP_GROUPS[group])
    mi, mo = max(len(c.stream) for c in cases), max(c.U for c in cases)
    assert mi > F.TILE and mo <= 65536 and (group != "round2" or mi > 16 * F.TILE)
    dec, st = decode(cases, max_in_len=mi, max_out_len=mo)
    check(cases, dec, st, routing=True)


# ------------------------------------------------------------------ segmented
def _seg_tiles(total):
    """The launcher's segment length in tiles: a mirror of rle_segmented.hip seg_bytes (about 16
    segments per CU over the batch, 4..16 tiles),
    checked against the library's own query (rle_seg_segment_bytes).  The tests below assert this
    mirror's value, so that they fail
    loudly -- rather than quietly test no segment edge -- if seg_bytes changes or the device has
    so few CUs (a partition of the chip) that these launch sizes give another segment length; such
    a failure asks for other launch sizes here, it is no decoder bug."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = min(16, max(4, (total + F.TILE - 1) // F.TILE // (ncu * 16)))
    assert R.seg_segment_bytes(total) == tiles * F.TILE, (total, tiles, R.seg_segment_bytes(total))
    return tiles


def _seg_decode_in_launches(cases, limit, want_tiles):
    """Decode in launches of at most `limit` stream bytes each, so that the launcher picks segments
    of `want_tiles` tiles and the positions under test are segment edges."""
    dec, st, i = [], [], 0
    while i < len(cases):
        j, total = i, 0
        while j < len(cases) and (j == i or total + len(cases[j].stream) <= limit):
            total += len(cases[j].stream)
            j += 1
        assert _seg_tiles(total) == want_tiles, (total, _seg_tiles(total))
        d, s = decode(cases[i:j], seg=True)
        dec += d
        st += list(s)
        i = j
    return dec, st


SEG_S = F.SEG


def test_seg_small_launches():
    """Probes at S - 4 .. S + 2, 2 S - 4 .. 2 S + 2 and one tile past S (S = 64512, a multiple of
    every segment length these launches take), in launches small enough
    for the shortest segments (4 tiles): the summaries' serial bits and the scan across the
    edge a bad or odd token sits on."""
    cases = F.cases(F.seg_positions(SEG_S))
    dec, st = _seg_decode_in_launches(cases, 12 << 20, 4)
    check(cases, dec, st, routing=False)


def test_seg_one_launch():
    """The same cases in one launch, large enough for the longest segments (16 tiles)."""
    cases = F.cases(F.seg_positions(SEG_S))
    reps = 1
    while _seg_tiles(reps * sum(len(c.stream) for c in cases)) < 16:
        reps += 1
    dec, st = decode(cases * reps, seg=True)
    n = len(cases)
    check(cases, dec[:n], st[:n], routing=False)
    for r in range(1, reps):   # (the repeats only make the launch large enough)
        assert dec[r * n:(r + 1) * n] == dec[:n]


def test_seg_first_edges():
    """Probes at the first and second edge of the shortest segments (4 x 1008 and 8 x 1008)."""
    cases = F.cases(F.around(4 * F.TILE) + F.around(8 * F.TILE))
    dec, st = _seg_decode_in_launches(cases, 12 << 20, 4)
    check(cases, dec, st, routing=False)


def test_seg_one_buffer_launches():
    """Launches of one buffer (RLE_SEG_ONE: segments from the length, no plan and map launches): a
    rotating sample of the segment-edge cases, one launch each."""
    cases = F.cases(F.seg_positions(SEG_S))
    sample = cases[::max(1, len(cases) // 24)]
    assert any(c.serial for c in sample) and any(not c.serial for c in sample)
    dec, st = [], []
    for c in sample:
        d, s = decode([c], seg=True)
        dec += d
        st += list(s)
    check(sample, dec, st, routing=False, pins=False)


# ------------------------------------------------------------------ rounds (opt-in)
@pytest.mark.parametrize("waves", [4, 8, 16])
def test_rounds(waves):
    """The large-batch decode in rounds (rle_round.h): the probe at the edge of the first tile, of
    the round's last wave (waves - 1 | waves) and of the next round's first (waves | waves + 1).
    The hint is at least the round kernel's threshold of 8 tiles."""
    cases = F.cases(F.round_positions(waves))
    assert len(cases) >= 4097
    mi = max(8 * F.TILE, max(len(c.stream) for c in cases))
    prev = R.set_dec_round(waves)
    R.set_coop_mode(0)
    try:
        dec, st = decode(cases, max_in_len=mi, max_out_len=max(c.U for c in cases))
    finally:
        R.set_coop_mode(-1)
        R.set_dec_round(prev)
    check(cases, dec, st, routing=True)


# ------------------------------------------------------------------ drop-in
def _dropin_cases(exact):
    ps = [p for g in sorted(F.WAVE_GROUPS) for p in F.WAVE_GROUPS[g]]
    ps += [p for g in sorted(F.COOP_GROUPS) for p in F.COOP_GROUPS[g] if p not in ps]
    cs = [c for c in F.cases(ps) if (c.cap == c.U) == exact and len(c.stream) <= 65536]
    return cs[::max(1, len(cs) // 300)]


def test_dropin_decompress_with_room():
    """RLEdecompress(y, C, U, E = C + 16) on about 300 cases: U + E bytes as the reference's (the
    copies of the E region on the serial exits, rle_dropin.cpp)."""
    cs = _dropin_cases(False)
    assert 250 <= len(cs) <= 400 and any(c.serial for c in cs) and any(not c.serial for c in cs)
    for c in cs:
        assert R.decompress(c.stream, c.U, c.cap - c.U) == O.decode(c.stream, c.U, c.cap)[0], c


def test_dropin_decompress_n_exact_caps():
    """RLEdecompressN in groups of up to 64 streams with cap = U."""
    cs = _dropin_cases(True)
    assert len(cs) >= 250
    for i in range(0, len(cs), 64):
        g = cs[i:i + 64]
        got = R.decompress_n([c.stream for c in g], [c.U for c in g])
        for c, out in zip(g, got):
            assert out == O.decode(c.stream, c.U, c.U)[0], c
