"""Pure-Python model of the SEGMENTED append (include/rle_mi355x.h rle_append_batch_device_seg;
csrc/rle_fileops.hip append_seg_*), on top of seg_model.py: the entering state, the seeded scan, the
per-segment write and the new tail word, written plainly so tests/test_append_seg_model.py can check
them against the oracle and against append_tail_model.append_carried.

The new bytes are encoded in the virtual coordinates of the one-wave append: 16 head positions,
then the new bytes from position vs = 16 (vs = 0 for an empty stream, a plain encode).  Of the head
the kernels know only what the entry record holds -- the byte c in front of the new content and the
run start 16 - r -- and never read it.  The model's virtual buffer therefore holds c at position 15
alone and another byte below it: a step that looked further back than the record would see a run
start at 15 and fail the comparison for every r > 1."""
import seg_model as S


def seg_count(n, sb):
    """Segments of n bytes (csrc/rle_seg_device.h seg_count): the last absorbs a remainder of 1-2."""
    return (n + sb - 3) // sb or 1


def seg_cut(n, sb):
    k = seg_count(n, sb)
    return [(i * sb, n if i + 1 == k else (i + 1) * sb) for i in range(k)]


def entry(y, word, new):
    """The entry record of one accepted file: (c, r, e, vs, t).  e: the leading new bytes equal to c
    that the rewritten final token takes, at most 9 - r."""
    if not y:
        return 0, 0, 0, 0, 0
    t, r = word & 0xFFFFFFFF, (word >> 32) & 0xF
    c, e = y[t], 0
    while e < min(len(new), 9 - r) and new[e] == c:
        e += 1
    return c, r, e, 16, t


def virtual(c, vs, new):
    return (bytes([c ^ 0xFF]) * 15 + bytes([c]) if vs else b"") + bytes(new)


def scan(V, vs, r, e, t, segs):
    """The encode's scan (seg_model.enc_scan) entered with the append's state: run start 16 - r and
    the output offset behind the final token once it counts r + e.  segs in virtual positions.
    Returns (per segment (rs, off, cnt), C', the final run's start)."""
    rs_run = 16 - r if vs else 0
    off = t + (1 if r + e == 1 else 3) if vs else 0
    plan = []
    for (p0, p1) in segs:
        L0, lb, cont, rest = S.enc_summary(V, p0, p1)
        piece = 0 if p0 == 0 else S.enc_piece_count(L0, (p0 - 1 - rs_run) % 9, cont)
        plan.append((rs_run, off, piece + rest))
        off += piece + rest
        if lb is not None:
            rs_run = lb
    return plan, off, rs_run


def is_uniform(V, p0, p1):
    """No run boundary in [p0, p1): the segment the uniform writer takes (never position 0)."""
    return p0 > 0 and all(V[i] == V[i - 1] for i in range(p0, p1))


def uniform_write(V, p0, p1, rs):
    """enc_seg_uniform: the tokens starting in a boundary-free segment, from its byte, the entering
    run start and the (up to 8) equal bytes behind it."""
    v, U = V[p0], len(V)
    ext = 0
    while ext < 8 and p1 + ext < U and V[p1 + ext] == v:
        ext += 1
    f = p0 + (9 - (p0 - rs) % 9) % 9
    if f >= p1:
        return b""
    ns = (p1 - 1 - f) // 9 + 1
    cl = min(p1 + ext - (f + 9 * (ns - 1)), 9)
    return bytes([v, v, 0x39]) * (ns - 1) + (bytes([v, v, 0x30 + cl]) if cl >= 2 else bytes([v]))


def append_seg(y, word, new, sb):
    """(new stream, new tail word) of an accepted segmented append with segments of sb bytes."""
    y, new = bytes(y), bytes(new)
    if not new:
        return y, word
    c, r, e, vs, t = entry(y, word, new)
    V = virtual(c, vs, new)
    segs = [(vs + a, vs + b) for a, b in seg_cut(len(new), sb)]
    plan, Cn, frs = scan(V, vs, r, e, t, segs)
    out = bytearray(Cn)
    out[:len(y)] = y
    if e:   # the scan rewrites the final token; nothing else below the first segment's offset changes
        out[t:t + 3] = bytes([c, c, 0x30 + r + e])
    for (p0, p1), (rs, off, cnt) in zip(segs, plan):
        piece = uniform_write(V, p0, p1, rs) if is_uniform(V, p0, p1) else S.enc_write(V, p0, p1, rs)
        assert len(piece) == cnt, (p0, p1, rs, len(piece), cnt)
        out[off:off + cnt] = piece
    rn = (len(V) - frs - 1) % 9 + 1
    return bytes(out), (Cn - (1 if rn == 1 else 3)) | (rn << 32)
