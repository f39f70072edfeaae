"""GPU parity of the SEGMENTED codec at every segment length the launcher can pick: 4 .. 16 tiles
of 1008 bytes (rle_segmented.hip seg_bytes).  In production a length follows from the size of the
launch (one more tile per 1008 x 16 x CUs bytes: on 256 CUs 4 tiles up to about 20 MB, 16 from
about 66 MB), so the lengths between belong to single files and read-N chunks of 20-64 MiB.  Here
total_in_bytes -- which only has to be at least the sum of the lengths -- is passed as the hint
m x 1008 x 16 x CUs, and a launch of a few MB runs with m-tile segments: buffers of a few segments
each, sized and filled so that run ends, tokens, '9' runs and bad counts sit on the edges of THAT
length (tests/test_gpu_segmented.py places its cases at multiples of 64512, which only the 4-, 8-
and 16-tile lengths divide).  What differs between the lengths: an odd tile count puts every inner
segment's last tile in the other slot of the tile walk's double buffer; the in-run fast path, the
uniform-segment writers and the rule that a buffer's last segment absorbs 1-2 bytes test a tile's
position against the segment's last tile; the workspace carve-up follows the segment count; and
from 5 tiles on the decode's write pass is always the 96-chunk kernel.

Every test asserts, through rle_seg_segment_bytes, the length it ran at, so a device with another
CU count fails there and not silently at other edges.  Outputs are compared byte for byte with the
oracle, slots poisoned (seg_encode / seg_decode below: test_gpu_parity's launches with the hint);
encode status 0, decode status without error bits."""
import pytest
import torch

import rle_mi355x as R
import rle_oracle as O
import stream_family as F
from test_gpu_parity import DEV, POISON, _i64, _input_image
from test_gpu_stream_family import check

pytestmark = pytest.mark.gpu
TILE = F.TILE
LENGTHS = list(range(4, 17))


def hint_for(m):
    """A total_in_bytes that makes the launcher take m-tile segments on this device."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    hint = m * TILE * 16 * ncu
    assert R.seg_segment_bytes(hint) == m * TILE, (m, ncu, R.seg_segment_bytes(hint))
    return hint


def seg_encode(bufs, hint):
    """One segmented encode launch with total_in_bytes = hint, which also sizes the workspace
    (otherwise test_gpu_parity.gpu_encode: poisoned slots, nothing written past C); returns
    (outputs, status)."""
    n, sizes = len(bufs), [len(b) for b in bufs]
    in_offs, host = _input_image(bufs, None)
    out_offs, out_total = R.compressed_slots(sizes)
    d_in = torch.from_numpy(host).to(DEV)
    d_out = torch.full((out_total + 16,), POISON, dtype=torch.uint8, device=DEV)
    out_len = torch.zeros(n, dtype=torch.int64, device=DEV)
    status = torch.full((n,), 0x7777, dtype=torch.int32, device=DEV)
    R.encode_batch_seg(d_in, _i64(in_offs), _i64(sizes), d_out, _i64(out_offs), out_len, status, total_in_bytes=hint)
    torch.cuda.synchronize()
    out, lens = d_out.cpu().numpy(), out_len.cpu().numpy()
    res = []
    for i in range(n):
        o, c = out_offs[i], int(lens[i])
        res.append(out[o:o + c].tobytes())
        end = out_offs[i + 1] if i + 1 < n else out_total
        assert (out[o + c:end] == POISON).all(), f"encode wrote past C in buffer {i}"
    return res, status.cpu().numpy()


def seg_decode(streams, usizes, caps, hint, poison=True):
    """One segmented decode launch with total_in_bytes = hint (otherwise test_gpu_parity.gpu_decode);
    returns (the cap bytes of every slot, status)."""
    n = len(streams)
    in_offs, host = _input_image(streams, None)
    out_offs, out_total = R.layout(caps)
    d_in = torch.from_numpy(host).to(DEV)
    d_out = torch.full((out_total + 16,), POISON if poison else 0, dtype=torch.uint8, device=DEV)
    status = torch.full((n,), 0x7777, dtype=torch.int32, device=DEV)
    R.decode_batch_seg(d_in, _i64(in_offs), _i64([len(s) for s in streams]), d_out, _i64(out_offs), _i64(usizes),
                       _i64(caps), status, total_in_bytes=hint)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    return [out[o:o + c].tobytes() for o, c in zip(out_offs, caps)], status.cpu().numpy()


def valid_cases(m):
    """{group: [buffers]} for segments of sb = 1008 m bytes."""
    sb = TILE * m
    g = {}
    # sizes on both sides of every rule of seg_count (a remainder of 1-2 bytes joins the last segment)
    g["sizes"] = [O.gen(kind, 100 * k + d + 7 + m, k * sb + d) for k in (1, 2, 3)
                  for d in (-3, -2, -1, 0, 1, 2, 3, 4, 17) for kind in range(5)]
    g["tiny"] = [b"", b"a", bytes(5)]
    ks = (1, 2, 5, 8, 9, 10, 17, 100)   # a run ending / starting k bytes around a segment edge
    g["cross_ab"] = [b"a" * (sb - k) + b"b" * (2 * k + 9) + b"c" * 1000 for k in ks]
    g["cross_gen"] = [O.gen(1, k, sb - k) + b"z" * (k + 40) + O.gen(3, k, sb) for k in ks]
    # segments without a run boundary, runs ending 0..10 bytes past a segment's end, every run phase
    g["uniform_z"] = [O.gen(1, e, 100 + e) + b"z" * (3 * sb + e) + O.gen(1, 50 + e, 3000) for e in range(11)]
    g["uniform_0"] = [bytes(2 * sb + e) for e in range(11)]
    g["uniform_from_0"] = [bytes(sb + 2000) + O.gen(1, 3, sb), bytes(2 * sb) + b"\x01" + bytes(sb)]
    g["uniform_phase"] = [O.gen(1, 90 + ph, sb - ph) + b"\xee" * (2 * sb + 17) + b"\xef" for ph in range(9)]
    # '9' runs and digit bytes: decode phases that never re-synchronise
    g["nines"] = [b"9" * (2 * sb + 7), b"3" * (sb + 3), b"99" * sb]
    # compressed streams whose segment edges fall inside 3-byte tokens at every offset
    g["tokens"] = [b"x" * k + b"aaab" * (sb // 4 + 10) for k in range(6)]
    return g


def flat(groups):
    return [(name, i, x) for name, xs in groups.items() for i, x in enumerate(xs)]


def one_buffer_sample(m, cases):
    """Indices of about a dozen labelled cases, at least one of every group, rotating with m."""
    by_group = {}
    for k, (name, _, _) in enumerate(cases):
        by_group.setdefault(name, []).append(k)
    out = []
    for name, ks in by_group.items():
        out += sorted({ks[(7 * m + 11 * j) % len(ks)] for j in range(3 if name == "sizes" else 1)})
    assert len(by_group) == 10 and 10 <= len(out) <= 14
    return out


@pytest.fixture(scope="module", params=LENGTHS)
def length(request):
    """(m, hint, labelled cases, the oracle's streams), built once per segment length."""
    m = request.param
    cases = flat(valid_cases(m))
    return m, hint_for(m), cases, [O.encode(x) for _, _, x in cases]


def _encode_check(m, hint, cases, refs):
    xs = [x for _, _, x in cases]
    assert sum(len(x) for x in xs) <= hint
    ys, st = seg_encode(xs, hint)
    assert (st == 0).all(), (m, st)
    for (name, i, x), y, ref in zip(cases, ys, refs):
        assert y == ref, (m, name, i, len(x), len(y), len(ref))


def _decode_check(m, hint, cases, refs):
    assert sum(len(y) for y in refs) <= hint
    us = [len(x) for _, _, x in cases]
    dec, st = seg_decode(refs, us, us, hint)
    for (name, i, x), d in zip(cases, dec):
        assert d == x, (m, name, i, len(x))
    assert ((st & 0xFF) == 0).all(), (m, st)


def test_valid_data_one_launch(length):
    """Every case in one encode launch and one decode launch (of the oracle's streams)."""
    m, hint, cases, refs = length
    _encode_check(m, hint, cases, refs)
    _decode_check(m, hint, cases, refs)


def test_valid_data_one_buffer_launches(length):
    """n = 1: the route without the plan and map launches (segments from the buffer's length)."""
    m, hint, cases, refs = length
    for k in one_buffer_sample(m, cases):
        _encode_check(m, hint, [cases[k]], [refs[k]])
        _decode_check(m, hint, [cases[k]], [refs[k]])


@pytest.mark.parametrize("m", F.SEG_TILES_BETWEEN)
def test_streams_the_encoder_never_emits(m):
    """Decode only: the stream family's probes (adjacent pairs, bad and odd count digits, cut
    streams) at -4 .. +2 around the first edge of m-tile segments, and for 5 and 7 tiles around the
    second edge; bytes over the whole cap, the OVERFLOW bit, serial-class => SERIAL, and the pins
    taken from the compiled reference."""
    hint = hint_for(m)
    positions = F.seg_length_positions(m)
    assert positions[:7] == F.around(m * TILE) and (len(positions) == 14) == (m in (5, 7))
    for lo in range(0, len(positions), 7):   # one launch per edge
        cases = F.cases(positions[lo:lo + 7])
        assert sum(len(c.stream) for c in cases) <= hint
        dec, st = seg_decode([c.stream for c in cases], [c.U for c in cases], [c.cap for c in cases], hint,
                             poison=False)
        check(cases, dec, st, routing=False)


# (m, d, kind, the decode's segment length in tiles on 256 CUs): the launcher sees C on the decode,
# so its length follows from the compressed size (runs50 barely compresses, runs90 to under a half)
DROPIN_FILES = [(5, 1, 2, 4), (11, -1, 3, 5), (15, 3, 2, 15)]


@pytest.mark.parametrize("m,d,kind,dec_tiles", DROPIN_FILES)
def test_dropin_files_between_20_and_64_mib(m, d, kind, dec_tiles):
    """Where these lengths arise in production: RLEcompress / RLEdecompress of one file whose size
    alone makes the launcher take m-tile segments."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    x = O.gen(kind, m, m * TILE * 16 * ncu + d)
    assert R.seg_segment_bytes(len(x)) == m * TILE
    y = R.compress(x)
    assert y == O.encode(x)
    assert R.seg_segment_bytes(len(y)) == dec_tiles * TILE, (len(y), R.seg_segment_bytes(len(y)))
    if m == 11:
        assert R.decompress(y, len(x), 5) == x + bytes(5)
    else:
        assert R.decompress(y, len(x)) == x
