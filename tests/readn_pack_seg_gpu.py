"""GPU helpers of the segmented packed read-N tests (tests/test_gpu_decode_packed_seg.py,
test_gpu_readn_pack_seg.py, test_gpu_readn_pack_seg_replay.py): the launch of
rle_decode_packed_batch_device_seg on a readn_pack_gpu.Batch, and the comparison of its reply image
and status words with the oracle's and with the one-wave form's.

The tests run at the shortest segment, SB = 4 tiles of 1008 stream bytes, which a launch takes under
a small total_in_bytes (HINT, or the streams' sum when that is larger): every test asserts it through
rle_seg_segment_bytes, so a device on which the hint gives another length fails there."""
import torch

import readn_pack_gpu as P
import rle_mi355x as R
from test_gpu_parity import DEV, POISON, _i64

TILE = 1008
SB = 4 * TILE
HINT = 1 << 20


def hint_of(streams, hint=None):
    """total_in_bytes of a launch over these streams: at least their sum, and 4-tile segments."""
    hint = max(HINT, sum(len(s) for s in streams)) if hint is None else hint
    assert R.seg_segment_bytes(hint) == SB, (hint, R.seg_segment_bytes(hint))
    return hint


def segments(C, sb=SB):
    """Segments of a C-byte stream (rle_seg_device.h seg_count)."""
    return max(1, (C + sb - 3) // sb)


def run_seg(b, hint=None, in_offs=None, us=None, lens=None, ws=None, status=True, check_sb=True):
    """One rle_decode_packed_batch_device_seg launch of Batch b into a poisoned image: (image, status)."""
    b.upload()
    lens = [len(s) for s in b.streams] if lens is None else lens
    if check_sb:
        hint = hint_of(b.streams, hint)
    d_out = torch.full((b.size,), POISON, dtype=torch.uint8, device=DEV)
    st = torch.full((b.n,), 0x7777, dtype=torch.int32, device=DEV) if status else None
    R.decode_packed_seg(b.d_in, _i64(b.in_offs if in_offs is None else in_offs), _i64(lens), d_out, _i64(b.places),
                        _i64(b.us if us is None else us), st, total_in_bytes=hint, ws=ws)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), st.cpu().numpy() if status else None


def check_seg(b, label, clean=True, agree=True, **kw):
    """Run the segmented form; the image is the oracle's over the poison.  clean: every status word is
    0; else the OVERFLOW bit is the oracle's.  agree: image and status words equal the one-wave
    form's (rle_decode_packed_batch_device) on the same batch.  Returns the status words."""
    got, st = run_seg(b, **kw)
    want, ost = b.want()
    b.compare(label, got, want)
    if clean:
        assert (st == 0).all(), (label, [(i, hex(int(s))) for i, s in enumerate(st) if s][:5])
    else:
        bad = [i for i in range(b.n) if (int(st[i]) & R.RLE_STATUS_OVERFLOW) != (ost[i] & 1)]
        assert not bad, (label, bad[:5])
    if agree:
        one, ost1 = b.run()
        b.compare(label + " (one-wave form)", one, got)
        assert [int(s) for s in st] == [int(s) for s in ost1], label
    return st

