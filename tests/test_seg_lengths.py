"""CPU pin of the segmented launcher's segment length (rle_seg_segment_bytes, host only: the value
rle_segmented.hip seg_bytes hands every kernel of a launch): clamp(ceil(total / 1008) / (16 CUs),
4, 16) tiles of 1008 bytes.  The table is the one of a 256-CU device (an MI355X; also what the
library assumes when no device is usable), where one tile more per segment comes with every
1008 x 4096 bytes of launch: 4 tiles up to about 20 MB, 16 from about 66 MB, every length between.
The GPU tests name their segment edges through the same query (tests/test_gpu_seg_lengths.py)."""
import rle_mi355x as R

TILE = 1008
STEP = TILE * 4096   # bytes of launch per tile of segment length, at 256 CUs (16 segments per CU)


def test_segment_length_table_at_256_cus():
    q = R.seg_segment_bytes
    assert q(1) == 4 * TILE and q(1 << 20) == 4 * TILE and q(0) == 4 * TILE
    assert q(1 << 30) == 16 * TILE and q(17 * STEP) == 16 * TILE
    for m in range(5, 17):
        assert q(m * STEP) == m * TILE, m
        # the tile count is rounded up, so the step to m tiles is at the first byte of the launch's
        # (4096 m)-th tile: 1007 bytes below m * STEP, and every total from there on takes m tiles
        assert q(m * STEP - 1) == m * TILE, m
        assert q(m * STEP - (TILE - 1)) == m * TILE, m
        assert q(m * STEP - TILE) == (m - 1) * TILE, m
        assert q((m + 1) * STEP - TILE) == min(m, 16) * TILE, m
    assert q(5 * STEP - TILE) == 4 * TILE


def test_workspace_is_monotone_across_the_table():
    """Across the table's points (1 byte, 1 MiB, m * STEP - 1 and m * STEP for m = 5..16, 1 GiB) a
    larger total_in_bytes never asks for a smaller workspace.  (Not a property of every pair of
    totals: the last total that still takes (m - 1)-tile segments has more segments, and a larger
    workspace, than the first one that takes m-tile segments; the workspace goes with the
    total_in_bytes of its own launch.)"""
    points = [1, 1 << 20]
    for m in range(5, 17):
        points += [m * STEP - 1, m * STEP]
    points += [1 << 30]
    assert points == sorted(points)
    for n in (1, 8, 1100):
        ws = [int(R.lib().rle_seg_workspace_bytes(n, t)) for t in points]
        assert all(a <= b for a, b in zip(ws, ws[1:])), (n, ws)
        assert ws[0] > 0
