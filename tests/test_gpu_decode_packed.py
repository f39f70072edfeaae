"""GPU tests of rle_decode_packed_batch_device (include/rle_mi355x.h): the decode with
byte-granular destinations.  Every comparison is against rle_oracle.decode(y, U) and of the whole
output image after a poison pre-fill (tests/readn_pack_gpu.py), so one stray byte shows anywhere,
between abutting files included.  Small batches, many cases per launch."""
import pytest
import torch

import readn_pack_gpu as P
import rle_mi355x as R
import rle_oracle as O
from test_gpu_parity import DEV, POISON, _i64, gpu_decode

pytestmark = pytest.mark.gpu
TILE = 1008          # stream bytes per decode tile
UNIFORM = 3024       # decoded bytes of a tile of "v v 9" tokens
TINY = [0, 1, 2, 3, 14, 15, 16, 17, 31, 32, 33]
_cache = {}


def edge_contents():
    """Contents whose streams end within two bytes of a tile edge, one to three tiles: random,
    runs50, runs90 and pairs."""
    if "edge" not in _cache:
        xs = []
        for kind in (1, 2, 3, 4):
            for k in (1, 2, 3):
                for d in (-2, -1, 0, 1, 2):
                    xs.append(P.stream_of_length(kind, 40 * kind + 5 * k + d, TILE * k + d))
        _cache["edge"] = [(O.encode(x), len(x)) for x in xs]
    return _cache["edge"]


def zero_contents():
    return [(O.encode(bytes(u)), u) for k in (1, 2, 3) for u in (UNIFORM * k - 1, UNIFORM * k, UNIFORM * k + 1)]


def literal_contents():
    xs = [P.literals(TILE * k + d, 3 * k + d) for k in (1, 2, 3) for d in (-1, 0, 1)]
    assert all(O.encode(x) == x for x in xs)
    return [(x, len(x)) for x in xs]


@pytest.mark.parametrize("gap", [0, 1])
def test_every_phase_and_tiny_length(gap):
    """One launch: every destination phase 0..15 with every U of TINY, files abutting (gap 0) or one
    byte apart (gap 1, the byte between keeps its poison); the fillers add lengths 0..15."""
    b = P.Batch()
    for phase in range(16):
        for j, U in enumerate(TINY):
            x = O.gen((phase + j) % 5, 16 * phase + j, U)
            b.add_at_phase(phase, O.encode(x), U, gap, seed=phase + j)
    seen = {(p % 16, U) for p, U in zip(b.places, b.us)}
    assert all((ph, U) in seen for ph in range(16) for U in TINY)
    b.check(f"tiny lengths, gap {gap}")


@pytest.mark.parametrize("what", ["edge", "zero", "literal"])
def test_tile_and_staging_edges_at_every_phase(what):
    """One to three decode tiles at every destination phase: streams ending around a tile edge;
    zero content of 3024 k - 1 .. + 1 bytes (the single-value and uniform tile paths behind a first
    tile that shares its first chunk); literal-only content (the literal fast path)."""
    files = {"edge": edge_contents, "zero": zero_contents, "literal": literal_contents}[what]()
    b = P.Batch()
    for phase in range(16):
        for j, (y, U) in enumerate(files):
            b.add_at_phase(phase, y, U, seed=phase + j)
    b.check(what)


def invalid_cases(vectors):
    cases = vectors["invalid_decode"]
    return [bytes.fromhex(v["in"]) for v in cases], [v["U"] for v in cases]


def aligned_status(streams, us):
    """rle_decode_batch_device's bytes and status words for the same files, cap = U."""
    return gpu_decode(streams, us, list(us), poison=False)


def test_invalid_streams_abutting(vectors):
    """The invalid-stream decodes of the golden vectors in one batch, file i at destination phase
    i mod 16, files abutting: the oracle's bytes, its OVERFLOW bit, and the aligned decode's status
    words, word for word."""
    streams, us = invalid_cases(vectors)
    b = P.Batch()
    for i, (y, U) in enumerate(zip(streams, us)):
        b.add_at_phase(i % 16, y, U, seed=i)
    st = b.check("invalid streams", clean=False)
    _, ast = aligned_status(b.streams, b.us)
    assert [int(s) for s in st] == [int(s) for s in ast]
    assert any(int(s) & R.RLE_STATUS_SERIAL for s in st)


def test_overflow_and_short_at_unaligned_destinations():
    """U smaller than the stream decodes to (OVERFLOW, through the exact serial path: truncated at
    U, nothing behind it) and larger (SHORT: zero fill to U), one to three tiles, every phase."""
    b = P.Batch()
    files = []
    for k, (y, U) in enumerate(edge_contents()[::7] + zero_contents()[::4] + [(b"aa9" * 3, 27), (b"abc", 3)]):
        files += [(y, max(U - 1 - k, 0)), (y, U + 1 + k), (y, U // 2), (y, U + 40)]
    for j, (y, U) in enumerate(files):
        b.add_at_phase((5 * j + 1) % 16, y, U, seed=j)
    st = b.check("overflow and short", clean=False)
    _, ast = aligned_status(b.streams, b.us)
    assert [int(s) for s in st] == [int(s) for s in ast]
    assert any(int(s) & R.RLE_STATUS_OVERFLOW for s in st) and any(int(s) & R.RLE_STATUS_SHORT for s in st)


@pytest.mark.parametrize("pad", [0, 16])
def test_hostile_input_padding(pad):
    """The arena bytes behind each stream continue its last token (test_gpu_parity._input_image, as
    tests/test_gpu_hostile_pad.py): they read as zero, and encoder output keeps status 0."""
    b = P.Batch(pad=pad)
    tiny = [(O.encode(x), len(x)) for x in (O.gen(k % 5, 70 + k, u) for k, u in enumerate([1, 2, 15, 16, 17, 33, 1007, 1024]))]
    tiny += [(y[-1:] * 2 + b"9x", 10) for y, _ in edge_contents() if len(y) % 16 == 0]
    for j, (y, U) in enumerate(edge_contents() + zero_contents() + literal_contents() + tiny):
        b.add_at_phase((3 * j + 2) % 16, y, U, seed=j)
    b.check(f"hostile pad {pad}")


def test_refusals_leave_their_range_untouched():
    """A misaligned stream address at the first, a middle and the last index among good files, and a
    decoded length past RLE_MAX_BUFFER_BYTES: the refused ranges keep their poison, the neighbours,
    abutting them, are exact."""
    b = P.Batch()
    files = edge_contents()[:9]
    for j, (y, U) in enumerate(files):
        b.add(y, U)
    b.upload()
    offs = list(b.in_offs)
    refused = (0, 4, len(files) - 1)
    for i in refused:
        offs[i] += 1 + i
    us = list(b.us)
    us[2] = R.RLE_MAX_BUFFER_BYTES + 1
    got, st = b.run(in_offs=offs, us=us)
    want, _ = b.want(skip=refused + (2,))
    b.compare("refusals", got, want)
    exp = [0] * b.n
    for i in refused:
        exp[i] = R.RLE_STATUS_MISALIGNED
    exp[2] = R.RLE_STATUS_TOOLARGE
    assert [int(s) for s in st] == exp


def test_agrees_with_the_aligned_decode(vectors):
    """With every destination 16-byte aligned, bytes and status words equal
    rle_decode_batch_device's on the same batch (cap = U)."""
    streams, us = invalid_cases(vectors)
    for y, U in edge_contents()[::3] + zero_contents() + literal_contents()[:3]:
        streams += [y, y]
        us += [U, U + 7]
    offs, total = R.layout(us)
    b = P.Batch()
    b.streams, b.us, b.places, b.pos = streams, us, offs, total
    got, st = b.run()
    dec, ast = aligned_status(streams, us)
    for i, (o, U) in enumerate(zip(offs, us)):
        assert got[o:o + U].tobytes() == dec[i], i
    assert [int(s) for s in st] == [int(s) for s in ast]
    want, _ = b.want()
    b.compare("aligned destinations", got, want)


def test_more_files_than_one_residency_round():
    """4100 files (the launch form of more than 4096: smaller staging, plain stores), abutting at
    whatever phase their lengths give, multi-pass tiles among them; a NULL status pointer."""
    files = edge_contents()[::4] + zero_contents()[::2] + literal_contents()[::3]
    files += [(O.encode(x), len(x)) for x in (O.gen(k % 5, 300 + k, 1 + 37 * k) for k in range(24))]
    b = P.Batch()
    for i in range(4100):
        y, U = files[i % len(files)]
        b.add(y, U, gap=1 if i % 97 == 0 else 0)
    assert len({p % 16 for p in b.places}) == 16
    b.check("4100 files")
    d_out = torch.full((b.size,), POISON, dtype=torch.uint8, device=DEV)
    R.decode_packed(b.d_in, _i64(b.in_offs), _i64([len(s) for s in b.streams]), d_out, _i64(b.places), _i64(b.us), None)
    torch.cuda.synchronize()
    b.compare("no status", d_out.cpu().numpy(), b.want()[0])
