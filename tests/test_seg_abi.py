"""CPU tests of the segmented codec's host side (include/rle_mi355x.h: rle_seg_workspace_bytes,
rle_append_seg_workspace_bytes, rle_encode_batch_device_seg, rle_decode_batch_device_seg): the
workspace sizes in closed form, and the returns that are decided before anything is launched, so
that fake pointers are enough.  No call here passes every host check: it would launch on pointers
that point nowhere.  No GPU."""
import ctypes

import pytest

import rle_mi355x as R

TILE = 1008
NS = (1, 2, 8, 63, 64, 1100, 70000)
TOTALS = (0, 1, 4030, 4031, 64 << 10, 1 << 20, (16 << 20) + 5, 5 * TILE * 4096 - TILE, 5 * TILE * 4096, 1 << 30,
          16 << 30)


def al(x):
    return (x + 255) & ~255


def seg_bytes_closed_form(n, total):
    """The carve-up of the workspace: seg_first, seg_buf, summaries, plans, per-buffer flags, and the
    three tables of the single-pass test variants, each rounded up to 256 bytes, over the segment
    bound m of n buffers holding `total` bytes."""
    sb = R.seg_segment_bytes(total)
    m = min(total // (sb - 2) + n, 0xFFFFFFF0)
    return al(4 * (n + 1)) + al(4 * m) + al(16 * m) + al(8 * m) + al(4 * n) + al(4 * m) + al(16 * m) + al(4)


@pytest.mark.parametrize("n", NS)
def test_workspace_sizes_closed_form(n):
    L = R.lib()
    for total in TOTALS:
        want = seg_bytes_closed_form(n, total)
        assert int(L.rle_seg_workspace_bytes(n, total)) == want, (n, total)
        assert int(L.rle_append_seg_workspace_bytes(n, total)) == al(want) + al(16 * n), (n, total)


def _cases():
    L = R.lib()
    # in in_off in_len out out_off out_len (status) / ... out_len out_cap (status): status and the
    # decode's out_cap may be NULL
    return (("encode", L.rle_encode_batch_device_seg, 7, (0, 1, 2, 3, 4, 5)),
            ("decode", L.rle_decode_batch_device_seg, 8, (0, 1, 2, 3, 4, 5)))


def test_host_side_returns_with_fake_pointers():
    """n == 0 is RLE_OK whatever the pointers; a NULL required pointer, a NULL workspace and a short
    workspace are RLE_E_INVAL, with or without a usable device -- all before any launch."""
    L = R.lib()
    ws, total, n = ctypes.c_void_p(0x100000), 1 << 20, 4
    need = int(L.rle_seg_workspace_bytes(n, total))
    assert need > 1
    for name, f, nptr, required in _cases():
        fake = [ctypes.c_void_p(0x1000 * (k + 1)) for k in range(nptr)]
        assert f(*([None] * nptr), 0, 0, None, 0, None) == R.RLE_OK, name
        assert f(*fake, 0, total, ws, 0, None) == R.RLE_OK, name
        for k in required:
            args = list(fake)
            args[k] = None
            assert f(*args, n, total, ws, need, None) == R.RLE_E_INVAL, (name, k)
        assert f(*fake, n, total, None, need, None) == R.RLE_E_INVAL, name
        assert f(*fake, n, total, ws, 0, None) == R.RLE_E_INVAL, name
        assert f(*fake, n, total, ws, need - 1, None) == R.RLE_E_INVAL, name
