"""GPU tests of rle_relocate_layout_device and rle_relocate_batch_device (include/rle_mi355x.h,
DESIGN.md §4d) against the host model (tests/relocate_model.py) and, for the write path's chain, the
oracle.

Every comparison of a relocation is of the WHOLE destination tensor after a poison pre-fill: stream
bytes, the zero pad up to the next 16, the poison of the gaps, of the bytes below dst_base and of the
bytes past *d_total; with d_new_off, d_new_cap, *d_total, every status word, and the source arena,
which must not change.  The source's bytes around the streams are 0x5C, so a pad copied instead of
zeroed shows."""
import numpy as np
import pytest
import torch

import relocate_model as M
import rle_mi355x as R
import rle_oracle as O
from append_fit_gpu import DEV, POISON, Arena, i64, r16

pytestmark = pytest.mark.gpu
FILL = 0x5C
SPAN = 16384
BIG = R.RLE_MAX_BUFFER_BYTES + 1


def source(lens, shifts=None, seed=0):
    """(image, offsets): streams of random bytes packed 16-byte aligned, one spare chunk between
    them; shifts: {index: bytes added to the offset}."""
    rng = np.random.default_rng(seed)
    offs, pos = [], 32
    for i, c in enumerate(lens):
        offs.append(pos + (shifts or {}).get(i, 0))
        pos = r16(pos + (c if c < BIG else 0)) + 16
    img = np.full(pos + 64, FILL, np.uint8)
    for c, o in zip(lens, offs):
        if c < BIG:
            img[o:o + c] = rng.integers(0, 256, c, dtype=np.uint8)
    return img, offs


def i32(v):
    return torch.tensor(np.asarray(v, dtype=np.int32), device=DEV)


def relocate(label, img, offs, lens, wants=None, sels=None, dst_base=0, slack=0, dst_cap=None, size=None,
             status=True, layout_only=False):
    """One call over fresh tensors, everything compared with the model.  dst_cap: default the
    model's total + slack.  Returns (destination image, new_off, new_cap, total)."""
    n = len(lens)
    total = M.layout(lens, wants, sels, dst_base)[2]
    dst_cap = total + slack if dst_cap is None else dst_cap
    size = max(dst_cap, total if total <= dst_cap else 0, dst_base) + 64 if size is None else size
    d_src = torch.from_numpy(img.copy()).to(DEV)
    d_dst = torch.full((size,), POISON, dtype=torch.uint8, device=DEV)
    d_off, d_len = i64(offs), i64(lens)
    d_want = None if wants is None else i64(wants)
    d_sel = None if sels is None else i32(sels)
    new_off = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    new_cap = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    d_total = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    d_st = torch.full((n,), 0x7777, dtype=torch.int32, device=DEV) if status else None
    if layout_only:
        R.relocate_layout(d_len, d_want, d_sel, new_off, new_cap, d_total, dst_base=dst_base)
    else:
        R.relocate_batch(d_src, d_off, d_len, d_dst, new_off, new_cap, d_total, want=d_want, sel=d_sel, status=d_st,
                         dst_base=dst_base, dst_cap=dst_cap)
    torch.cuda.synchronize()
    before = np.full(size, POISON, np.uint8)
    if layout_only:
        eimg, (eoff, ecap, etotal), est = before, M.layout(lens, wants, sels, dst_base), None
    else:
        eimg, eoff, ecap, etotal, est = M.expected(img, offs, lens, wants, sels, before, dst_base, dst_cap)
    assert etotal == total
    u = lambda t: [int(v) for v in t.cpu().numpy().astype(np.uint64)]
    goff, gcap = u(new_off), u(new_cap)
    assert int(d_total.item()) == total, (label, int(d_total.item()), total)
    assert goff == eoff, (label, "new_off", [(i, a, b) for i, (a, b) in enumerate(zip(goff, eoff)) if a != b][:4])
    assert gcap == ecap, (label, "new_cap", [(i, a, b) for i, (a, b) in enumerate(zip(gcap, ecap)) if a != b][:4])
    got = d_dst.cpu().numpy()
    if status and not layout_only:
        gst = [int(v) for v in d_st.cpu().numpy().astype(np.uint32)]
        assert gst == est, (label, "status", [(i, hex(a), hex(b)) for i, (a, b) in enumerate(zip(gst, est)) if a != b][:4])
    bad = np.flatnonzero(got != eimg)
    if len(bad):
        p = int(bad[0])
        b = max([i for i in range(n) if eoff[i] <= p], default=-1)
        raise AssertionError(f"{label}: destination byte {p} is {got[p]:#x}, expected {eimg[p]:#x} (file {b}: slot at "
                             f"{eoff[b] if b >= 0 else None}, C {lens[b]}, cap {ecap[b]}); {len(bad)} bytes differ")
    assert (d_src.cpu().numpy() == img).all(), (label, "the source arena changed")
    return got, goff, gcap, total


def edge_files():
    """(lens, wants) whose streams' starts, last whole chunks, partial chunks and gaps fall at
    SPAN * k + d of the destination for every d of the issue's list: a stream end at edge + d puts its
    last whole chunk and its partial chunk on either side of the edge, a slot end at edge + d (d a
    multiple of 16) puts the next stream's start there and the gap across the edge."""
    lens, wants, pos = [], [], 0
    deltas = (-17, -16, -15, -1, 0, 1, 15, 16, 17)

    def add(c, w):
        nonlocal pos
        lens.append(c)
        wants.append(w)
        pos += r16(max(c, w))

    def next_edge():
        return (pos // SPAN + 1) * SPAN + (SPAN if pos % SPAN > SPAN - 512 else 0)

    for d in deltas:   # the stream ends at edge + d
        add(next_edge() + d - pos, 0)
    for d in deltas:   # the stream ends 100 bytes in front of edge + d and its slot reaches across
        e = next_edge()
        add(e + d - 100 - pos, e + d - pos + 48)
    for d in (-16, 0, 16):   # the slot ends, and the next stream starts, at edge + d
        e = next_edge()
        add(40, e + d - pos)
        assert pos == e + d
        add(1009, 0)
    for d in deltas:   # the stream ends at edge + d and its gap runs on for 4 KiB behind it
        e = next_edge()
        add(e + d - pos, e + d - pos + 4096)
    return lens, wants


def test_every_edge():
    lens, wants = [], []
    for c in list(range(0, 50)) + [1007, 1008, 1009, 4095, 4096, 4097]:
        for w in (0, c, c + 1, c + 15, c + 16, c + 100):
            lens.append(c)
            wants.append(w)
    el, ew = edge_files()
    lens, wants = el + lens + el[::-1], ew + wants + ew[::-1]
    img, offs = source(lens, seed=1)
    total = M.layout(lens, wants)[2]
    assert total > 20 * SPAN and R.relocate_span_bytes(total + 4096) == SPAN
    relocate("edges, room past the total", img, offs, lens, wants, slack=4096)
    relocate("edges, exact room", img, offs, lens, wants)
    relocate("edges, no wants", img, offs, lens, None, slack=32)
    relocate("edges, layout alone", img, offs, lens, wants, layout_only=True)


def test_empty_batch_and_empty_files():
    total = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    R.relocate_layout(none, None, None, none, none, total, dst_base=4096)
    assert int(total.item()) == 4096
    total.fill_(-7)
    d = torch.full((256,), POISON, dtype=torch.uint8, device=DEV)
    R.relocate_batch(d, none, none, d, none, none, total, dst_base=64)
    assert int(total.item()) == 64 and bool((d == POISON).all().item())
    img, offs = source([0, 0, 0])
    relocate("empty files", img, offs, [0, 0, 0], slack=64)
    relocate("empty files with wants", img, offs, [0, 0, 0], [0, 33, 0])
    relocate("no room at all", img, offs, [0, 0, 0], dst_base=32, dst_cap=32)
    relocate("one byte", *source([1]), [1])


@pytest.mark.parametrize("mask", ["all", "none", "alternating", "first", "last", "null"])
def test_selection_masks(mask):
    lens = [5000, 17, 0, 16384, 33000, 1008, 4097, 15, 16, 70000, 1, 2500]
    wants = [0, 100, 0, 16385, 0, 3000, 0, 0, 64, 70016, 0, 0]
    n = len(lens)
    sels = {"all": [1] * n, "none": [0] * n, "alternating": [i % 2 * 0x101 for i in range(n)],
            "first": [7] + [0] * (n - 1), "last": [0] * (n - 1) + [1], "null": None}[mask]
    img, offs = source(lens, seed=2)
    relocate(mask, img, offs, lens, wants, sels, slack=48)
    relocate(mask + ", no status", img, offs, lens, wants, sels, status=False)


@pytest.mark.parametrize("dst_base", [16, 4096 + 48, 3 * SPAN - 16])
def test_dst_base_leaves_the_bytes_below_untouched(dst_base):
    lens = [20000, 3, 16384 - 48, 40000, 0, 999]
    img, offs = source(lens, seed=3)
    relocate(f"base {dst_base}", img, offs, lens, [0, 0, 0, 40100, 16, 0], None, dst_base=dst_base, slack=16)


def test_capacity():
    lens = [3000, 17000, 5, 0, 40000]
    wants = [3100, 0, 0, 20, 0]
    img, offs = source(lens, seed=4)
    for base in (0, 2048):
        total = M.layout(lens, wants, None, base)[2]
        relocate("exact", img, offs, lens, wants, dst_base=base, dst_cap=total)
        for sels in (None, [1, 0, 1, 1, 1]):
            total = M.layout(lens, wants, sels, base)[2]
            got = relocate("one short", img, offs, lens, wants, sels, dst_base=base, dst_cap=total - 1, size=total + 64)
            assert (got[0] == POISON).all()
        relocate("far short", img, offs, lens, wants, dst_base=base, dst_cap=base, size=total + 64)


def test_refusals_among_good_files():
    lens = [5000, 4096, 33000, BIG, 1008, 2000, 17, 16400]
    wants = [0, 4200, 0, 0, 0, BIG + 5, 0, 0]
    img, offs = source(lens, shifts={1: 8}, seed=5)
    got, off, cap, _ = relocate("refusals", img, offs, lens, wants, slack=64)
    assert cap[1] == r16(4200) and (got[off[1]:off[1] + cap[1]] == POISON).all()   # reserved, untouched
    assert cap[3] == 0 and cap[5] == 0 and off[4] == off[3] and off[6] == off[5]
    relocate("refusals, masked out", img, offs, lens, wants, [1, 0, 1, 0, 1, 0, 1, 1])
    # the largest sizes the library takes still get their slots in the layout
    relocate("largest sizes", img, offs[:3], [R.RLE_MAX_BUFFER_BYTES, 16, BIG], [0, R.RLE_MAX_BUFFER_BYTES - 1, 0],
             layout_only=True, size=64)


# ---------------------------------------------------------------- the write path's chain
def chain_contents(n):
    """Contents whose streams end in tokens of every kind, some empty, some long."""
    xs = []
    for i in range(n):
        size = [0, 1, 17, 300, 1008, 4096, 9000, 20000][i % 8] + i
        x = O.gen(1 + i % 4, 50 + i, size) if i % 8 else b""
        xs.append(x + bytes([0x61 + i % 3]) * (i % 11))
    return xs


def chain_news(n, k):
    sizes = [0, 1, 9, 100, 1500, 4096, 12000]
    return [O.gen(1 + (i + k) % 4, 900 + 31 * k + i, sizes[(i + 2 * k) % len(sizes)]) for i in range(n)]


def test_chain_size_relocate_fit_against_the_oracle():
    """rle_append_size_batch_device, rle_relocate_batch_device with d_want = d_need into the other
    arena, rle_append_fit_batch_device with d_cap = d_new_cap: every file equals the oracle's
    encode(x + new), with no NOFIT; four times, the two arenas taking turns.  Offsets, lengths,
    capacities, tail words and decoded lengths never leave the device."""
    n = 24
    xs = chain_contents(n)
    ys = [O.encode(x) for x in xs]
    a = Arena(ys, [b""] * n, [0] * n, [r16(len(y)) for y in ys], [len(x) for x in xs])
    d_off, d_len, d_cap, d_ulen = a.d_off, a.d_len, a.d_cap, a.d_ulen
    d_tail = torch.zeros(n, dtype=torch.int64, device=DEV)
    R.tail_batch(a.d_s, d_off, d_len, d_tail)
    room = sum(r16(R.max_compressed_size(len(x) + 4 * 12000)) for x in xs)
    arenas = [a.d_s, torch.empty(room, dtype=torch.uint8, device=DEV)]
    for k in range(4):
        news = chain_news(n, k)
        src, dst = arenas[k % 2], arenas[(k + 1) % 2]
        if dst.numel() < room:
            dst = arenas[(k + 1) % 2] = torch.empty(room, dtype=torch.uint8, device=DEV)
        dst.fill_(POISON)
        nw = Arena(ys, news, [0] * n, [0] * n, [0] * n)   # (the new bytes' arena only)
        need = torch.full((n,), -7, dtype=torch.int64, device=DEV)
        st = torch.full((3, n), 0x7777, dtype=torch.int32, device=DEV)
        new_off, new_cap = torch.zeros(n, dtype=torch.int64, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV)
        total = torch.zeros(1, dtype=torch.int64, device=DEV)
        R.append_size(src, d_off, d_len, d_tail, nw.d_n, nw.d_noff, nw.d_nlen, need, st[0])
        R.relocate_batch(src, d_off, d_len, dst, new_off, new_cap, total, want=need, status=st[1])
        d_off, d_cap = new_off, new_cap
        need2 = torch.full((n,), -7, dtype=torch.int64, device=DEV)
        R.append_fit(dst, d_off, d_len, d_cap, d_ulen, nw.d_n, nw.d_noff, nw.d_nlen, need2, st[2], tail=d_tail)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [[0] * n] * 3, (k, st.cpu().tolist())
        xs = [x + a_ for x, a_ in zip(xs, news)]
        ys = [O.encode(x) for x in xs]
        img, off, ln = dst.cpu().numpy(), d_off.cpu().tolist(), d_len.cpu().tolist()
        assert ln == [len(y) for y in ys] and need2.cpu().tolist() == ln and need.cpu().tolist() == ln, k
        assert d_cap.cpu().tolist() == [r16(c) for c in ln] and d_ulen.cpu().tolist() == [len(x) for x in xs], k
        assert int(total.item()) == sum(r16(c) for c in ln), k
        for i, y in enumerate(ys):
            assert img[off[i]:off[i] + ln[i]].tobytes() == y, (k, i)


def test_partial_relocation_inside_one_arena():
    """Only the files the fit append refused move, to dst_base = the arena's used end; the others
    keep their places, and the second fit append finishes the batch."""
    n = 16
    xs = chain_contents(n)
    news = [O.gen(1 + i % 4, 7000 + i, [1, 0, 3000, 2, 40, 9000][i % 6]) for i in range(n)]
    ys = [O.encode(x) for x in xs]
    a = Arena(ys, news, [0] * n, [r16(len(y)) for y in ys], [len(x) for x in xs])
    used = r16(a.soffs[-1] + len(ys[-1]))
    arena = torch.full((used + sum(r16(len(y) + R.max_compressed_size(len(w) + 9)) for y, w in zip(ys, news)) + 64,),
                       POISON, dtype=torch.uint8, device=DEV)
    arena[:a.d_s.numel()] = a.d_s
    d_tail = torch.zeros(n, dtype=torch.int64, device=DEV)
    R.tail_batch(arena, a.d_off, a.d_len, d_tail)
    st = torch.full((3, n), 0x7777, dtype=torch.int32, device=DEV)
    R.append_fit(arena, a.d_off, a.d_len, a.d_cap, a.d_ulen, a.d_n, a.d_noff, a.d_nlen, a.d_need, st[0], tail=d_tail)
    sel = (st[0] == R.RLE_STATUS_NOFIT).to(torch.int32)
    before = arena.clone()
    new_off, new_cap = torch.zeros(n, dtype=torch.int64, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV)
    total = torch.zeros(1, dtype=torch.int64, device=DEV)
    R.relocate_batch(arena, a.d_off, a.d_len, arena, new_off, new_cap, total, want=a.d_need, sel=sel, status=st[1],
                     dst_base=used)
    moved = sel != 0
    assert bool((arena[:used] == before[:used]).all().item())   # nobody's old place changed
    d_off, d_cap = torch.where(moved, new_off, a.d_off), torch.where(moved, new_cap, a.d_cap)
    d_nlen = torch.where(moved, a.d_nlen, torch.zeros_like(a.d_nlen))   # (the others are done: A = 0)
    need2 = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    R.append_fit(arena, d_off, a.d_len, d_cap, a.d_ulen, a.d_n, a.d_noff, d_nlen, need2, st[2], tail=d_tail)
    torch.cuda.synchronize()
    first = st[0].cpu().tolist()
    assert set(first) == {0, R.RLE_STATUS_NOFIT} and 3 <= first.count(0) <= n - 3, first
    assert st[1:].cpu().tolist() == [[0] * n] * 2
    want = [O.encode(x + w) for x, w in zip(xs, news)]
    img, off, ln = arena.cpu().numpy(), d_off.cpu().tolist(), a.d_len.cpu().tolist()
    assert int(total.item()) == used + sum(r16(len(y)) for y, s in zip(want, first) if s)
    for i, y in enumerate(want):
        assert (off[i] >= used) == (first[i] != 0) and (first[i] != 0 or off[i] == a.soffs[i]), i
        assert ln[i] == len(y) and img[off[i]:off[i] + ln[i]].tobytes() == y, i
    assert a.d_ulen.cpu().tolist() == [len(x) + len(w) for x, w in zip(xs, news)]


def test_tail_scan_and_reply_after_a_relocation():
    """The tail words and decoded lengths carried across a relocation are what a fresh scan of the
    new arena gives, and the wire reply read from the new arena is the old one's, byte for byte."""
    import readn_reply_gpu as G
    import readn_reply_model as RM
    n = 40
    files = G.Files(G.names(n), G.small_contents(n, seed=3))
    s = files.store
    dst = torch.full((int(s.d_c.numel()),), POISON, dtype=torch.uint8, device=DEV)
    new_off, new_cap = torch.zeros(n, dtype=torch.int64, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV)
    total = torch.zeros(1, dtype=torch.int64, device=DEV)
    st = torch.full((n,), 0x7777, dtype=torch.int32, device=DEV)
    R.relocate_batch(s.d_c, s.off, s.clen, dst, new_off, new_cap, total, status=st)
    tail = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    ulen = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    st2 = torch.full((n,), 0x7777, dtype=torch.int32, device=DEV)
    R.tail_batch(dst, new_off, s.clen, tail, ulen, st2)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * n and st2.cpu().tolist() == [0] * n
    assert torch.equal(tail, s.tail) and torch.equal(ulen, s.ulen)
    assert int(total.item()) == sum(r16(int(c)) for c in s.clen.cpu().tolist()) < s.d_c.numel()   # packed
    form = RM.READN | RM.END
    size = len(RM.reply(files.paths, files.contents, form)) + G.SLACK
    old = G.call_reply(s.d_c, s.off, s.clen, s.ulen, files.table, form, size)
    new = G.call_reply(dst, new_off, s.clen, s.ulen, files.table, form, size)
    assert (old[0] == new[0]).all() and (old[1] == new[1]).all() and old[2] == new[2]
    assert (old[3] == 0).all() and (new[3] == 0).all()
    assert (new[0] == G.image_of(RM.reply(files.paths, files.contents, form), size)).all()


def test_larger_shapes():
    lens = [(1 << 20) - 3] + [65536 - 7 * (i % 9) for i in range(64)] + [4096 + (i % 7) - 3 for i in range(512)]
    img, offs = source(lens, seed=8)
    relocate("1 MiB + 64 x 64 KiB + 512 x 4 KiB", img, offs, lens, slack=16)
    order = np.random.default_rng(9).permutation(len(lens))
    lens2 = [lens[i] for i in order]
    relocate("the same, shuffled, into gaps", img, [offs[i] for i in order], lens2, [c + c // 2 for c in lens2])


def test_4096_streams_of_4k():
    lens = [4096 - (i % 5) for i in range(4096)]
    img, offs = source(lens, seed=10)
    relocate("4096 x 4 KiB", img, offs, lens)
    wants = [R.append_slot_bytes(c, 4096) for c in lens]
    room = M.layout(lens, wants)[2]
    assert R.relocate_span_bytes(room) == 2 * SPAN   # a span of two passes
    relocate("4096 x 4 KiB into worst-case slots", img, offs, lens, wants)
