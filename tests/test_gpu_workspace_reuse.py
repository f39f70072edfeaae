"""GPU tests: the caller-owned workspace of the segmented encode, decode and append.

R.seg_workspace / R.append_seg_workspace hand out 256 bytes more than the library asks for, so the
rest of the suite would not see a kernel that wrote a little past rle_seg_workspace_bytes, and it
gives every launch a workspace of its own.  Here:

  exact size   the library's byte count, at a 256-byte aligned address inside a larger tensor with
               4 KiB of guard bytes on both sides: the result is the oracle's and both guards are
               untouched; one byte less is RLE_E_INVAL and launches nothing.  n = 1 (no plan and
               map launches), n = 3, and n = 1025 (one past the plan kernel's 1024 threads).
  dirty        the whole workspace pre-filled with 0x00, 0xFF, 0x01 or 0xA5: no table may be read
               before the launch wrote it.
  reuse        one workspace, never cleared, through batches of other shapes, a batch with a
               refused buffer, an encode, then a decode, then a segmented append.

Outputs are compared with the oracle byte for byte, status words exactly (an encoder stream never
shows SERIAL or INTERNAL), through the launch tensors of tests/test_gpu_graph_replay.py (outputs
and status poisoned before every launch)."""
import pytest
import torch

import rle_mi355x as R
import rle_oracle as O
from test_gpu_graph_replay import Appends, Stage, dec_buf, enc_buf, stored_contents
from test_gpu_parity import DEV

pytestmark = pytest.mark.gpu
GUARD = 4096
GUARD_BYTE = 0x3C
FILLS = [0x00, 0xFF, 0x01, 0xA5]
OPS = ["encode", "decode", "append"]


def seg_len():
    return R.seg_segment_bytes(1)


def sizes_for(n):
    S = seg_len()
    if n == 1:
        return [3 * S + 5]
    if n == 3:
        return [5 * S, S - 1, 3 * S + 5]
    return [(7 * i) % 41 for i in range(512)] + [3 * S + 5] + [(5 * i) % 37 for i in range(n - 513)]


def batch(op, sizes, base, refused=None):
    """The launch's buffers: encode inputs / decode streams of these sizes (test_gpu_graph_replay Buf),
    or the new bytes of an append."""
    kinds = lambda i: 1 + (i + base) % 4
    if op == "encode":
        return [enc_buf(O.gen(kinds(i), base + i, s), refused=(i == refused)) for i, s in enumerate(sizes)]
    if op == "decode":
        return [dec_buf(s, kinds(i), base + i, room=16 * (i % 2), refused=(i == refused)) for i, s in enumerate(sizes)]
    return [O.gen(kinds(i), base + i, s) for i, s in enumerate(sizes)]


class Launch:
    """One segmented launch with its tensors: total = the sum of the lengths it was given."""

    def __init__(self, op, items):
        self.op, self.n = op, len(items)
        s = torch.cuda.current_stream()
        if op == "append":
            self.total = sum(len(a) for a in items)
            self.new = items
            self.t = Appends(stored_contents(self.n), [items], s)
            self.t.load(items)
            self.need = int(R.lib().rle_append_seg_workspace_bytes(self.n, self.total))
        else:
            self.total = sum(len(b.data) for b in items)
            self.t = Stage("enc" if op == "encode" else "dec", [items], s)
            self.t.load(items)
            self.need = int(R.lib().rle_seg_workspace_bytes(self.n, self.total))
        assert R.seg_segment_bytes(self.total) == seg_len()

    def run(self, ws):
        t = self.t
        if self.op == "encode":
            R.encode_batch_seg(t.d_in, t.in_off, t.in_len, t.d_out, t.out_off, t.out_len, t.status,
                               total_in_bytes=self.total, workspace=ws)
        elif self.op == "decode":
            R.decode_batch_seg(t.d_in, t.in_off, t.in_len, t.d_out, t.out_off, t.out_len, t.cap, t.status,
                               total_in_bytes=self.total, workspace=ws)
        else:
            R.append_batch_seg(t.d_s, t.off, t.d_len, t.cap, t.d_ulen, t.d_n, t.new_off, t.new_len, t.status,
                               total_new_bytes=self.total, workspace=ws, tail=t.d_tail)

    def check(self, label):
        if self.op == "append":
            self.t.check(label, self.new)
        else:
            self.t.check(label)

    def outputs(self):
        t = self.t
        return [t.d_s, t.d_len, t.d_ulen, t.d_tail, t.status] if self.op == "append" else [t.d_out, t.out_len, t.status]


class Guarded:
    """`need` workspace bytes at a 256-byte aligned address, 4 KiB of guard bytes before and after."""

    def __init__(self, need, fill):
        self.big = torch.full((need + 2 * GUARD + 256,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        a = self.big.data_ptr()
        self.off, self.need = ((a + GUARD + 255) & ~255) - a, need
        self.ws = self.big[self.off:self.off + need]
        self.ws.fill_(fill)
        wp, wn = R._ws_ptr(self.ws)
        assert wp.value == a + self.off and wp.value % 256 == 0 and wn == need   # the size passed is exact

    def short(self):
        return self.big[self.off:self.off + self.need - 1]

    def guards_untouched(self):
        lo, hi = self.big[self.off - GUARD:self.off], self.big[self.off + self.need:self.off + self.need + GUARD]
        return bool((lo == GUARD_BYTE).all().item()) and bool((hi == GUARD_BYTE).all().item())


@pytest.mark.parametrize("n", [1, 3, 1025])
@pytest.mark.parametrize("op", OPS)
def test_exact_size_between_guards(op, n):
    L = Launch(op, batch(op, sizes_for(n), 100 * n))
    g = Guarded(L.need, 0xA5)
    before = [t.clone() for t in L.outputs()]
    with pytest.raises(R.RLEError, match=f": {R.RLE_E_INVAL}$"):
        L.run(g.short())
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, L.outputs())), "a refused call launched something"
    assert bool((g.ws == 0xA5).all().item()) and g.guards_untouched()
    L.run(g.ws)
    L.check(f"{op} n={n}")
    assert g.guards_untouched(), "a kernel wrote outside rle_seg_workspace_bytes"


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("op", OPS)
def test_dirty_workspace(op, fill):
    for n in (3, 1):
        items = batch(op, sizes_for(n), 300 + n)
        L = Launch(op, items)
        ws = (R.append_seg_workspace if op == "append" else R.seg_workspace)(n, L.total, DEV)
        ws.fill_(fill)
        L.run(ws)
        L.check(f"{op} n={n} workspace of {fill:#x}")
        if op == "append":   # and the same bytes as an eager run on a fresh workspace
            F = Launch(op, items)
            F.run(R.append_seg_workspace(n, F.total, DEV))
            F.check("fresh workspace")
            assert all(torch.equal(a, b) for a, b in zip(L.outputs(), F.outputs()))


def test_reuse_across_shapes():
    """One workspace sized for the largest launch, filled once and never cleared."""
    S = seg_len()
    steps = []
    for op in ("encode", "decode"):
        first = batch(op, [5 * S] * 3, 500)
        steps += [(op, "3 x 5S", first),
                  (op, "1 x S-1", batch(op, [S - 1], 510)),
                  (op, "a refused buffer among good ones", batch(op, [S + 1, 3 * S + 5, 2 * S], 520, refused=1)),
                  (op, "the first batch again", first)]
    steps.append(("append", "after a decode", batch("append", [S + 1, 3 * S + 5, 1], 530)))
    launches = [(op, label, Launch(op, items)) for op, label, items in steps]
    ws = torch.full((max(L.need for _, _, L in launches) + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    for op, label, L in launches:
        L.run(ws)
        L.check(f"{op}: {label}")
