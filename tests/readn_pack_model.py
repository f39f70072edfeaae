"""Host models of the packed read-N (include/rle_mi355x.h: rle_decode_packed_batch_device,
rle_readn_layout_device, rle_readn_batch_device).  No GPU.

layout(): the reply's layout the way readn_layout_kernel computes it (csrc/rle_kernels.hip): strides
of one workgroup's 1024 threads, a 64-lane inclusive scan per wave, the 16 wave sums exchanged, the
total so far carried into the next stride, all in 64-bit wrapping arithmetic.

stores(): which bytes of the reply a file at byte p with decoded length U may write, and how wide:
the bytes of its first 16-byte chunk (shared with whatever lies in front of p), the aligned 16-byte
chunks that lie wholly inside [p, p + U), and the bytes of its last chunk (shared with whatever lies
behind p + U).  The kernel's 16-byte stores may only cover bytes of the second kind or, unaligned,
bytes of the file's own range; the first and the third kind are written with byte stores
(dec_flush's and dec_finish's st.head branches, dec_serial_packed).

reply(): the reply readNFilesHandler builds (reference src/filesystemApi.c:663-691): per file
"%010ld%s%010ld" (path length, path, content length) and the content right behind it."""

WAVE, BLOCK = 64, 1024
M64 = (1 << 64) - 1


def layout(ulen, gap=None):
    """(place, total) as readn_layout_kernel writes them; gap None: no gaps."""
    n = len(ulen)
    gap = [0] * n if gap is None else gap
    place, carry = [0] * n, 0
    for i0 in range(0, n, BLOCK):
        x = [(gap[i] + ulen[i]) & M64 if i < n else 0 for i in range(i0, i0 + BLOCK)]
        incl, wsum = [], []
        for w in range(BLOCK // WAVE):
            s = 0
            for lane in range(WAVE):
                s = (s + x[w * WAVE + lane]) & M64
                incl.append(s)
            wsum.append(s)
        for t in range(min(BLOCK, n - i0)):
            before = (carry + sum(wsum[:t // WAVE])) & M64
            place[i0 + t] = (before + incl[t] - x[t] + gap[i0 + t]) & M64
        carry = (carry + sum(wsum)) & M64
    return place, carry


def stores(p, U):
    """(head, chunks, tail): the byte positions of [p, p + U) written one by one in front of the first
    16-byte boundary, the starts of the aligned 16-byte chunks stored whole, and the byte positions
    written one by one behind the last boundary."""
    end = p + U
    a0, a1 = (p + 15) & ~15, end & ~15
    head = list(range(p, min(a0, end)))
    chunks = list(range(a0, a1, 16))
    tail = list(range(max(a1, a0), end))
    return head, chunks, tail


def header(path, ulen):
    return b"%010d%s%010d" % (len(path), path, ulen)


def reply(paths, contents):
    """The reply buffer of readNFilesHandler for these files, in order."""
    return b"".join(header(p, len(c)) + c for p, c in zip(paths, contents))
