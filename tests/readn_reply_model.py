"""Host model of the whole read-N reply (include/rle_mi355x.h: rle_reply_header_bytes,
rle_readn_headers_device, rle_readn_reply_device and its _seg form; DESIGN.md §4c, "Headers and
terminator").  No GPU.

field(): one "%010ld" field as readn_header_kernel writes it (csrc/rle_kernels.hip): the low ten
decimal digits of the value, which is snprintf's output for every value below 10^10.

header(): the bytes in front of a file's content per form: READN "%010ld%s%010ld" (path length, path,
content length; reference src/filesystemApi.c:675-679, src/server.c:53-58), READ "%010ld" (content
length; src/server.c:262-264).  TERMINATOR: the reference's NO_MORE_CONTENT (src/server.c:122).

layout(): readn_pack_model.layout with the gaps derived from the path lengths, and the terminator
counted in the total.  reply(): the wire bytes."""
import readn_pack_model as M

READN, READ, END = 0, 1, 0x100
FORMS = (READN, READ, READN | END)
TERMINATOR = b"0000000000"
M64 = (1 << 64) - 1


def header_bytes(form, path_len):
    """rle_reply_header_bytes."""
    if form not in FORMS:
        return 0
    return 10 if form == READ else 20 + path_len


def field(v):
    return b"%010d" % (v % 10 ** 10)


def header(form, path, ulen):
    assert form in FORMS
    if form == READ:
        return field(ulen)
    return field(len(path)) + path + field(ulen)


def layout(ulen, path_lens, form):
    """(place, total) as readn_reply_layout_kernel writes them."""
    assert form in FORMS
    gaps = [10] * len(ulen) if form == READ else [20 + pl for pl in path_lens]
    place, total = M.layout(ulen, gaps)
    return place, (total + (10 if form & END else 0)) & M64


def reply(paths, contents, form=READN):
    """The wire reply for these files, in order."""
    body = b"".join(header(form, p, len(c)) + c for p, c in zip(paths, contents))
    return body + (TERMINATOR if form & END else b"")
