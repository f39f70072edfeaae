"""GPU tests of rle_decode_packed_batch_device_seg (include/rle_mi355x.h, DESIGN.md §4c "Segmented
form"): the packed decode with several waves per stream.  Streams of one to five 4-tile segments
(tests/readn_pack_seg_gpu.py), destinations at every byte phase, files abutting; every comparison is
of the whole reply image after a poison pre-fill against rle_oracle.decode, and of image and status
words against the one-wave form's on the same batch.  A few launches per test."""
import pytest

import readn_pack_gpu as P
import readn_pack_seg_gpu as G
import readn_pack_seg_model as S
import rle_mi355x as R
import rle_oracle as O
from readn_pack_seg_gpu import SB, TILE
from test_gpu_seg_lengths import hint_for, seg_decode
from test_gpu_workspace_reuse import Guarded

pytestmark = pytest.mark.gpu
EDGE_D = (-1, 0, 1, 3)   # a remainder of 1-2 bytes joins the last segment; 3 make one of their own
_cache = {}


def edge_files(sb=SB, ks=(1, 2), kinds=("literal", 1, 2), seed=0):
    """(stream, U) of k sb + d stream bytes for k in ks, d in EDGE_D: literal, random and runs50."""
    key = (sb, ks, kinds, seed)
    if key not in _cache:
        out = []
        for kind in kinds:
            for k in ks:
                for d in EDGE_D:
                    C = k * sb + d
                    x = P.literals(C, seed + k + d) if kind == "literal" else P.stream_of_length(kind, seed + 9 * k + d, C)
                    y = O.encode(x)
                    assert len(y) == C
                    out.append((y, len(x)))
        _cache[key] = out
    return _cache[key]


def test_every_destination_phase_at_the_segment_edges():
    """Every destination phase 0..15 x streams of k SB + d bytes: two launches (k = 1 and k = 2)."""
    for k in (1, 2):
        files = edge_files(ks=(k,))
        b = P.Batch()
        for phase in range(16):
            for j, (y, U) in enumerate(files):
                assert G.segments(len(y)) == k + (EDGE_D[j % 4] == 3)
                b.add_at_phase(phase, y, U, seed=phase + j)
        G.check_seg(b, f"segment edges, k = {k}")


def shifted_file(s, extra):
    """(content, stream, the first inner boundary's output offset): leading run tokens that decode to
    s bytes more than they take, then one-byte tokens across the first segment edge."""
    a, r = divmod(s, 6)
    runs = [9] * a + [3 + r]
    x = b"".join(bytes([0x00 if i % 2 == 0 else 0xFF]) * n for i, n in enumerate(runs))
    nlit = SB + extra - 3 * len(runs)
    x += P.literals(nlit, s)
    y = O.encode(x)
    assert len(y) == SB + extra and len(x) == len(y) + s
    off = SB + s
    assert O.encode(x[:off]) == y[:SB]   # the segment edge is a token edge: segment 1 starts at output off
    return x, y, off


def test_every_inner_boundary_phase():
    """For every head 0..15, files whose first inner segment boundary lands on every output phase:
    the leading run tokens shift the output against the input by s = 0..15 bytes.  One launch."""
    b = P.Batch()
    seen = set()
    for head in range(16):
        for s in range(16):
            x, y, off = shifted_file(s, 40 + 3 * s + head)
            i = b.add_at_phase(head, y, len(x), seed=head + s)
            sh, fl = S.entry(head, off)
            stores = S.segment_stores(b.places[i], [0, off], len(x))
            assert stores[1][0][:1] == ([b.places[i] + off] if sh else []) and fl % 16 == 0
            seen.add((b.places[i] % 16, sh))
    assert seen == {(h, p) for h in range(16) for p in range(16)}
    G.check_seg(b, "inner boundary phases")


def mixed_of_stream_length(C, seed, avoid):
    """runs50 content whose stream is C bytes and whose first and last byte differ from `avoid`."""
    for k in range(20):
        x = P.stream_of_length(2, seed + k, C)
        if x[0] != avoid and x[-1] != avoid and x[-1] != x[-2]:
            return x
    raise AssertionError("no such content")


def test_uniform_segments():
    """dec_seg_fill: zero-filled content of three segments (and three bytes more: a fourth) at every
    destination phase; a single-value segment between two mixed ones; a file whose last segment is
    single-valued, which takes the walk and closes the file."""
    z = 0x5A
    one = bytes([z]) * (9 * SB // 3)   # SB bytes of "z z 9" tokens
    assert O.encode(one) == bytes([z, z, 0x39]) * (SB // 3)
    m1, m3 = mixed_of_stream_length(SB, 3, z), mixed_of_stream_length(SB + 700, 5, z)
    between, last = m1 + one + m3, m1 + one
    assert O.encode(between) == O.encode(m1) + O.encode(one) + O.encode(m3) and len(O.encode(between)) == 3 * SB + 700
    assert O.encode(last) == O.encode(m1) + O.encode(one) and G.segments(len(O.encode(last))) == 2
    b = P.Batch()
    for phase in range(16):
        for U in (9 * SB, 9 * SB + 5):
            y = O.encode(bytes(U))
            assert G.segments(len(y)) == (3 if U == 9 * SB else 4)
            b.add_at_phase(phase, y, U, seed=phase)
        x = (between, last)[phase % 2]
        b.add_at_phase(phase, O.encode(x), len(x), seed=phase + 1)
    for x in (between, last):
        b.add_at_phase(7, O.encode(x), len(x))
    G.check_seg(b, "uniform segments")


def test_tiny_and_empty_files():
    """Last segments of 3..15 stream bytes (and "v v 1", one byte; "v v 2", two), files with C = 0 and
    U > 0 (zero fill), with U = 0, and with C < 3, between large neighbours."""
    big = edge_files(ks=(2,))
    files = []
    for r in range(3, 16):
        y = P.literals(SB + r, r)
        files.append((y, len(y)))
    base = P.literals(SB, 77)
    files += [(base + b"\x07\x071", SB + 1), (base + b"\x07\x072", SB + 2)]
    files += [(b"", 0), (b"", 1), (b"", 15), (b"", 16), (b"", 33), (b"a", 1), (b"ab", 2), (b"a", 0), (b"ab", 1), (b"zz", 2)]
    b = P.Batch()
    for j, (y, U) in enumerate(files):
        nb = big[j % len(big)]
        b.add(nb[0], nb[1])
        b.add_at_phase((5 * j + 3) % 16, y, U, seed=j)
    b.add(*big[0])
    G.check_seg(b, "tiny and empty files", clean=False)


@pytest.mark.parametrize("m", range(4, 17))
def test_every_segment_length(m):
    """m-tile segments (the hint of tests/test_gpu_seg_lengths.py): streams of one and two segments
    -1, 0, +1, +3 bytes at two odd destination phases, and one of them alone (n = 1: no plan and no
    map launch)."""
    hint, sb = hint_for(m), m * TILE
    files = edge_files(sb=sb, kinds=("literal", 2), seed=m)
    b = P.Batch()
    for phase in (5, 11):
        for j, (y, U) in enumerate(files):
            b.add_at_phase(phase, y, U, seed=m + j)
    assert sum(len(y) for y in b.streams) <= hint and R.seg_segment_bytes(hint) == sb
    G.check_seg(b, f"{m}-tile segments", hint=hint, check_sb=False)
    one = P.Batch()
    one.add(*files[(3 * m) % len(files)], gap=3 + m % 13)
    G.check_seg(one, f"{m}-tile segments, n = 1", hint=hint, check_sb=False)


def never_emitted():
    """(stream, U) longer than one segment and shorter than three, that the encoder never emits: a bad
    count digit in the first segment, in the second and at the edge; a pair read only on an untaken
    phase at an edge (valid: it must stay tiled); U one too small and U too large."""
    lit = P.literals(2 * SB + 500, 11)
    out = []
    for pos in (700, SB + 900, SB - 2, SB - 1):   # "v v /": the digit '0' - 1 is an unbounded count
        y = bytearray(lit)
        y[pos:pos + 3] = bytes([0x21, 0x21, 0x2F])
        assert y[pos - 1] != 0x21 and y[pos + 3] != 0x2F
        out.append((bytes(y), len(y) + 50))
    y = bytearray(lit)   # "a a 5" across the edge, then "5 /": phase 0 of segment 1 reads "5 5 /"
    y[SB - 2:SB + 3] = b"\x21\x215" + b"5/"
    assert y[SB - 3] != 0x21 and y[SB + 3] != 0x2F
    y = bytes(y)
    U = len(O.decode(y, 3 * len(y))[0].rstrip(b"\x00"))
    out.append((y, U))
    x = mixed_of_stream_length(2 * SB + 300, 21, 0)   # (ends in a one-byte token: U - 1 cuts a token off)
    out += [(O.encode(x), len(x) - 1), (O.encode(x), len(x) + 40), (y, U - 1), (y, U + 17)]
    return out, 4   # (the index of the stream that stays tiled)


def test_streams_the_encoder_never_emits():
    """Unaligned abutting destinations; the oracle's bytes; status words those of
    rle_decode_batch_device_seg on the same streams in aligned slots."""
    files, tiled = never_emitted()
    assert all(SB < len(y) < 3 * SB for y, _ in files)
    b = P.Batch()
    for j, (y, U) in enumerate(files):
        b.add_at_phase((7 * j + 1) % 16, y, U, seed=j)
        b.add(P.literals(30 + j, j), 30 + j)
    st = G.check_seg(b, "never emitted", clean=False)
    _, ast = seg_decode(b.streams, b.us, b.us, G.hint_of(b.streams), poison=False)
    assert [int(s) for s in st] == [int(s) for s in ast]
    mine = [int(st[3 * j + 1]) for j in range(len(files))]   # (a filler in front of each, a small file behind)
    assert mine[tiled] == 0
    assert all(s & R.RLE_STATUS_SERIAL for s in mine[:4]) and mine[5] & R.RLE_STATUS_OVERFLOW
    assert mine[6] == R.RLE_STATUS_SHORT and mine[8] == R.RLE_STATUS_SHORT and mine[7] & R.RLE_STATUS_OVERFLOW


@pytest.mark.parametrize("pad", [0, 16])
def test_hostile_input_padding(pad):
    """The arena bytes behind each stream continue its last token (tests/test_gpu_hostile_pad.py):
    they read as zero, and encoder output keeps status 0."""
    b = P.Batch(pad=pad)
    files = edge_files() + [(O.encode(bytes(u)), u) for u in (9 * SB, 9 * SB + 5, 9 * SB - 9)]
    files += [(y[-1:] * 2 + b"9x", 10) for y, _ in edge_files()[:6]]
    for j, (y, U) in enumerate(files):
        b.add_at_phase((3 * j + 2) % 16, y, U, seed=j)
    G.check_seg(b, f"hostile pad {pad}")


def test_refusals_leave_their_range_untouched():
    """At the first, a middle and the last index among good files: a misaligned stream address; a
    stream or decoded length past RLE_MAX_BUFFER_BYTES (a length override: the stream is never
    read).  And a stream past the segment tables, from a total_in_bytes too small for it: the tables
    hold the segments in index order, so that refusal takes the file that passes them and every file
    behind it.  The refused ranges keep their poison, the neighbours, abutting them, are exact."""
    files = (edge_files() * 2)[:13]
    b = P.Batch()
    for j, (y, U) in enumerate(files):
        b.add(y, U)
    n, refused = b.n, (0, 6, 12)
    b.upload()
    offs = list(b.in_offs)
    for i in refused:
        offs[i] += 1 + i
    got, st = G.run_seg(b, in_offs=offs)
    b.compare("misaligned", got, b.want(skip=refused)[0])
    assert [int(s) for s in st] == [R.RLE_STATUS_MISALIGNED if i in refused else 0 for i in range(n)]

    us, lens = list(b.us), [len(y) for y in b.streams]
    us[0] = us[12] = R.RLE_MAX_BUFFER_BYTES + 1
    lens[6] = R.RLE_MAX_BUFFER_BYTES + 1
    got, st = G.run_seg(b, us=us, lens=lens, hint=G.hint_of(b.streams))
    b.compare("too large", got, b.want(skip=refused)[0])
    assert [int(s) for s in st] == [R.RLE_STATUS_TOOLARGE if i in refused else 0 for i in range(n)]

    segs = [G.segments(len(y)) for y in b.streams]
    keep = 11   # files 0..10 fit the tables, file 11 (more than one segment) passes them
    assert segs[keep] > 1
    small = (sum(segs[:keep]) + 1 - n) * (SB - 2)   # max_segments = total / (sb - 2) + n
    assert small >= 0 and R.seg_segment_bytes(small) == SB and small < sum(lens)
    got, st = G.run_seg(b, hint=small, check_sb=False)
    late = tuple(range(keep, n))
    b.compare("past the tables", got, b.want(skip=late)[0])
    assert [int(s) for s in st] == [R.RLE_STATUS_TOOLARGE if i in late else 0 for i in range(n)]


def test_workspace_exact_dirty_and_reused():
    """The workspace at exactly rle_decode_packed_seg_workspace_bytes between guard bytes, pre-filled
    with 0xFF, and the same one reused for a second, smaller shape; no status pointer on the way."""
    first, second = P.Batch(), P.Batch()
    for j, (y, U) in enumerate(edge_files()):
        first.add_at_phase((5 * j + 1) % 16, y, U, seed=j)
    for j, (y, U) in enumerate(edge_files()[3:9]):
        second.add_at_phase((3 * j + 9) % 16, y, U, seed=j)
    hint = G.hint_of(first.streams)
    need = int(R.lib().rle_decode_packed_seg_workspace_bytes(first.n, hint))
    assert need >= int(R.lib().rle_decode_packed_seg_workspace_bytes(second.n, hint))
    g = Guarded(need, 0xFF)
    with pytest.raises(R.RLEError, match=f": {R.RLE_E_INVAL}$"):
        G.run_seg(first, hint=hint, ws=g.short())
    assert bool((g.ws == 0xFF).all().item()) and g.guards_untouched()
    for b, label in ((first, "first shape"), (second, "second shape"), (first, "first shape again")):
        got, st = G.run_seg(b, hint=hint, ws=g.ws)
        b.compare(label, got, b.want()[0])
        assert (st == 0).all() and g.guards_untouched(), label
    got, _ = G.run_seg(second, hint=hint, ws=g.ws, status=False)
    second.compare("no status words", got, second.want()[0])
    assert g.guards_untouched()


def test_agrees_with_the_one_wave_form(vectors):
    """A mixed batch -- the golden vectors' invalid streams, segment-edge files at their own and at
    wrong lengths, zero content, tiny files -- byte for byte and status word for status word."""
    cases = vectors["invalid_decode"]
    files = [(bytes.fromhex(v["in"]), v["U"]) for v in cases]
    for y, U in edge_files()[::2]:
        files += [(y, U), (y, U + 7), (y, max(U - 3, 0))]
    files += [(O.encode(bytes(u)), u) for u in (0, 1, 3024, 9 * SB + 1)]
    b = P.Batch()
    for j, (y, U) in enumerate(files):
        b.add_at_phase((11 * j + 4) % 16, y, U, seed=j)
    st = G.check_seg(b, "mixed batch", clean=False, agree=True)
    assert any(int(s) & R.RLE_STATUS_SERIAL for s in st) and any(int(s) == R.RLE_STATUS_SHORT for s in st)
