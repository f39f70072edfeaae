"""Host model of the segmented packed decode's stores (include/rle_mi355x.h:
rle_decode_packed_batch_device_seg, rle_readn_batch_device_seg; DESIGN.md §4c, "Segmented form").
No GPU.

tests/readn_pack_model.py splits a file at byte p with decoded length U into head bytes, aligned
16-byte chunks and tail bytes.  Here the same split is made per segment of a file.  The write pass
(csrc/rle_segmented.hip, dec_seg_write_packed_kernel) bases a file at base = p - head, head = p % 16,
and a segment whose scanned output offset is off enters at head + off of that base:
DecState.head = (head + off) % 16 and the flushed position is head + off rounded down to 16
(entry()).  Segment k owns the output [off[k], off[k + 1]) of the file, the last one [off[-1], U):
its bytes in front of the first 16-byte boundary and behind the last one share their chunk with the
previous and the next segment (or, at the file's two ends, with other files) and go out one by one
(dec_flush's and dec_finish's st.head branches, dec_seg_fill's two ends); only the aligned chunks
wholly inside the segment's output are stored whole.  A segment may decode to nothing."""
import readn_pack_model as M


def entry(head, off):
    """(DecState.head, flushed) of a segment entering at scanned output offset off of a file whose
    destination has the low four bits head: positions in the base's offsets."""
    a = head + off
    return a & 15, a & ~15


def segment_stores(p, offs, U):
    """Per segment (head bytes, aligned chunk starts, tail bytes), as absolute byte positions, of a
    file at byte p with decoded length U whose segments' file-relative output offsets are offs
    (offs[0] == 0, non-decreasing, at most U)."""
    assert offs and offs[0] == 0 and all(a <= b for a, b in zip(offs, offs[1:])) and offs[-1] <= U
    head, base = p % 16, p - p % 16
    out = []
    for k, off in enumerate(offs):
        end = offs[k + 1] if k + 1 < len(offs) else U
        sh, fl = entry(head, off)
        assert base + fl + sh == p + off and fl % 16 == 0
        out.append(M.stores(p + off, end - off))
    return out
