"""CPU model of the segmented tail scan (include/rle_mi355x.h rle_tail_batch_device_seg;
csrc/rle_fileops.hip tail_seg_scan_kernel over the segmented decode's summaries), for the tests: the
two passes restated plainly over an arbitrary segment length.

summarize(y, q0, q1)   one segment, for each entry phase e = 0, 1, 2 (the first token starts at
                       q0 + e): the decoded bytes of the tokens starting in [q0 + e, q1), the exit
                       phase (how far the last of them reaches past q1), whether the parse stops (a
                       pair whose count digit is not '2'..'9' or lies past C), and the last token start.
compose(summaries)     one stream: the entry phase each segment is actually taken with, the sum of
                       the taken counts in 64 bits, and whether a taken phase stops.
tail_seg(y, sb)        (status, tail word, ulen): the cut (seg_count / seg_range: the last segment
                       absorbs a remainder of 1-2 bytes, so the final token starts in it), the
                       segment-table refusal, compose, the last start of the last segment's taken
                       phase, and the one-wave scan's closing rule.
The device keeps no last start per phase: its scan wave walks the last segment again from the taken
phase, which gives summarize(...)[taken].last."""
from collections import namedtuple

from append_seg_model import seg_count, seg_cut
from append_tail_model import MAX_BUFFER_BYTES, NOTCANON, TOOLARGE, tail_word

Phase = namedtuple("Phase", "count exit stop last")
U64 = (1 << 64) - 1


def summarize(y, q0, q1):
    C = len(y)
    out = []
    for e in range(3):
        j, cnt, stop, last = q0 + e, 0, False, None
        while j < q1:
            last = j
            if j + 1 < C and y[j] == y[j + 1]:
                if j + 2 < C and 0x32 <= y[j + 2] <= 0x39:
                    cnt += y[j + 2] - 0x30
                else:
                    stop = True   # the phases go on as for any pair: three bytes
                j += 3
            else:
                cnt += 1
                j += 1
        out.append(Phase(cnt, j - q1, stop, last))
    return out


def compose(summaries):
    """-> (taken entry phase per segment, U mod 2^64, a taken phase stops)."""
    e, U, stop, taken = 0, 0, False, []
    for s in summaries:
        taken.append(e)
        U = (U + s[e].count) & U64
        stop = stop or s[e].stop
        e = s[e].exit
    return taken, U, stop


def close(y, last):
    """The closing rule: the tail word when the final token, starting at `last`, ends the stream at
    C exactly, else None."""
    C = len(y)
    if last is not None and last + 1 == C:
        return tail_word(last, 1)
    if last is not None and last + 3 == C and 1 <= y[C - 1] - 0x30 <= 9:
        return tail_word(last, y[C - 1] - 0x30)
    return None


def tail_seg(y, sb, s0=0, maxseg=None):
    """(status, tail word, ulen) of one stream whose segments are [s0, s0 + seg_count) of a launch
    whose tables hold maxseg segments (None: enough)."""
    y, C = bytes(y), len(y)
    if C > MAX_BUFFER_BYTES or (maxseg is not None and s0 + seg_count(C, sb) > maxseg):
        return TOOLARGE, 0, 0
    if C == 0:
        return 0, 0, 0
    cut = seg_cut(C, sb)
    summ = [summarize(y, q0, q1) for q0, q1 in cut]
    taken, U, stop = compose(summ)
    word = None if stop else close(y, summ[-1][taken[-1]].last)
    if word is None:
        return NOTCANON, 0, 0
    return 0, word, U


def tail_seg_batch(streams, sb, total):
    """Every stream of one launch with this total_in_bytes: the segment bound is total / (sb - 2) + n,
    and a stream whose segments reach past it is refused."""
    maxseg = min(total // (sb - 2) + len(streams), 0xFFFFFFF0)
    out, s0 = [], 0
    for y in streams:
        out.append(tail_seg(y, sb, s0, maxseg))
        s0 += seg_count(len(y) if len(y) <= MAX_BUFFER_BYTES else 0, sb)
    return out
