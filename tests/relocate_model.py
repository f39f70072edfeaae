"""Host model of the relocation of stored streams (include/rle_mi355x.h: rle_relocate_span_bytes,
rle_relocate_layout_device, rle_relocate_batch_device; csrc/rle_relocate.h).  No GPU.

layout(): the slots the way relocate_layout_kernel computes them: the caps by the one rule, summed by
readn_layout_kernel's scan (readn_pack_model.layout) started at dst_base, in 64-bit wrapping arithmetic.

span_bytes(), grid(), wg_range(): the host's span rule and the destination bytes workgroup w owns.

find(): the 64-way search of relocate_copy_kernel over new_off, with the number of dependent loads.

chunks(): which 16-byte chunks of which slots each workgroup moves, by the kernel's own walk.

expected(): everything one rle_relocate_batch_device call must leave, from numpy images."""
import numpy as np

import readn_pack_model as P

M64 = (1 << 64) - 1
MAXB = 0x7FFFFFF0   # RLE_MAX_BUFFER_BYTES
OK, MISALIGNED, TOOLARGE, NOFIT = 0, 2, 4, 0x2000
GRANULE = 16384
WAVE = 64


def r16(v):
    return (v + 15) & ~15


def cap(length, want, sel):
    m = max(want, length)
    return r16(m) if sel and m <= MAXB else 0


def caps(length, want=None, sel=None):
    n = len(length)
    want = [0] * n if want is None else want
    sel = [1] * n if sel is None else sel
    return [cap(c, w, s != 0) for c, w, s in zip(length, want, sel)]


def layout(length, want=None, sel=None, dst_base=0):
    """(new_off, new_cap, total) as relocate_layout_kernel writes them."""
    cs = caps(length, want, sel)
    place, total = P.layout(cs)
    return [(dst_base + p) & M64 for p in place], cs, (dst_base + total) & M64


def span_bytes(room, cus=256):
    """max(16 KiB, ceil(room / (8 * CUs))) rounded up to 16 KiB."""
    parts = 8 * cus
    per = (room + parts - 1) // parts
    return max(GRANULE, (per + GRANULE - 1) // GRANULE * GRANULE)


def grid(room, span):
    """Workgroups of the copy launch: the spans that cover the room, one at least (the status words)."""
    return max(1, (room + span - 1) // span)


def wg_range(w, dst_base, span, total):
    """[lo, hi) of the destination bytes workgroup w owns; lo >= hi: none."""
    lo = dst_base + w * span
    return lo, min(lo + span, total)


def find(new_off, at):
    """(the last i with new_off[i] <= at, dependent loads): 64 lanes probe evenly spaced entries of
    the candidate range [a, b) per step.  new_off is non-decreasing and new_off[0] <= at."""
    a, b, loads = 0, len(new_off), 0
    while True:
        step = (b - a + WAVE - 1) // WAVE
        c = sum(1 for lane in range(WAVE) if a + lane * step < b and new_off[a + lane * step] <= at)
        loads += 1
        assert c >= 1
        a += (c - 1) * step
        if step == 1:
            return a, loads
        b = min(a + step, b)


def chunks(length, aligned, new_off, new_cap, dst_base, dst_cap, total, span):
    """[(workgroup, file, chunk)] of every 16-byte chunk the copy launch stores, by the kernel's walk:
    the search for the owner of the range's first byte, then forward until a file starts at or past
    the range's end.  Nothing where the slots do not fit."""
    out = []
    if total > dst_cap:
        return out
    n = len(length)
    for w in range(grid(dst_cap - dst_base, span)):
        lo, hi = wg_range(w, dst_base, span, total)
        if lo >= hi:
            continue
        i = find(new_off, lo)[0]
        while i < n and new_off[i] < hi:
            o = new_off[i]
            if new_cap[i] and aligned[i]:
                frm, to = max(o, lo), min(o + r16(length[i]), hi)
                out += [(w, i, k) for k in range((frm - o) // 16, (to - o) // 16)]   # (none where to <= frm)
            i += 1
    return out


def statuses(length, want, sel, aligned, fits):
    st = []
    for c, w, s, a in zip(length, want, sel, aligned):
        if not s:
            st.append(OK)
        elif not fits:
            st.append(NOFIT)
        elif c > MAXB or w > MAXB:
            st.append(TOOLARGE)
        else:
            st.append(OK if a else MISALIGNED)
    return st


def expected(src, offs, length, want, sel, dst, dst_base, dst_cap):
    """(image, new_off, new_cap, total, status) one relocation of these files must leave: src and dst
    are numpy uint8 images (dst as it is before the call: poison), offs the streams' offsets in src
    (an offset that is not a multiple of 16 is a misaligned stream: the arenas are 16-byte aligned)."""
    n = len(length)
    want = [0] * n if want is None else want
    sel = [1] * n if sel is None else sel
    new_off, new_cap, total = layout(length, want, sel, dst_base)
    fits = total <= dst_cap
    aligned = [o % 16 == 0 for o in offs]
    img = dst.copy()
    if fits:
        for i in range(n):
            if new_cap[i] and aligned[i]:
                c, o = length[i], new_off[i]
                img[o:o + c] = src[offs[i]:offs[i] + c]
                img[o + c:o + r16(c)] = 0
    return img, new_off, new_cap, total, statuses(length, want, sel, aligned, fits)
