// Host side of the read-N family (include/rle_mi355x.h: rle_readn_layout_device, rle_readn_batch_device,
// rle_readn_headers_device, rle_readn_reply_device in csrc/rle_kernels.hip; rle_readn_batch_device_seg,
// rle_readn_reply_device_seg in csrc/rle_segmented.hip): the two launches every form shares, and the
// one sequence of checks and launches the four read-N entries run.  No device code.
#pragma once
#include "rle_device.h"   // kMaxGrid

namespace rle {
// The headers of the full reply (rle_readn_reply_device and its _seg form): the path table and the form.
struct ReplyHeaders {
    const void* paths;
    const uint64_t* path_off;
    const uint64_t* path_len;
    uint32_t form;   // RLE_REPLY_READN, RLE_REPLY_READ or RLE_REPLY_READN | RLE_REPLY_END
};
// The layout launch into d_place and *d_total, ahead of the decode.  hdr NULL: the caller's gaps
// (readn_layout_kernel; d_gap NULL: none).  Else the gaps are derived from hdr->path_len (the READ
// form's are 10 and path_len is not read) and the terminator is counted (readn_reply_layout_kernel).
// n is bounded by the caller (kMaxGrid).
int readn_layout_launch(const uint64_t* d_ulen, const uint64_t* d_gap, const ReplyHeaders* hdr, uint64_t* d_place,
                        uint64_t* d_total, uint32_t n, void* stream);
// The headers and the terminator (readn_header_kernel; d_total NULL: rle_readn_headers_device, no
// capacity rule; no launch where there is neither a file nor a terminator).
int readn_header_launch(const void* d_paths, const uint64_t* d_path_off, const uint64_t* d_path_len,
                        const uint64_t* d_ulen, void* d_out, const uint64_t* d_place, uint32_t form, uint32_t n,
                        const uint64_t* d_total, uint64_t out_cap, void* stream);
inline bool reply_form_ok(uint32_t form) {
    return form == RLE_REPLY_READN || form == RLE_REPLY_READ || form == (RLE_REPLY_READN | RLE_REPLY_END);
}

// What the four read-N entries have in common.  hdr NULL: rle_readn_batch_device(_seg), the gaps
// d_gap; else the full reply.
struct ReadN {
    const void* streams;
    const uint64_t *off, *len, *ulen, *gap;
    void* out;
    uint64_t out_cap;
    uint64_t *place, *total;
    uint32_t n;
    const ReplyHeaders* hdr;
    void* stream;
};
// The one sequence: the form, n == 0 (*total = 0 through the layout launch where total is given; with
// RLE_REPLY_END the reply is the terminator alone and goes on), the pointers and the bound on n, then
// prepare() (the _seg forms' workspace check; not for the terminator alone, which decodes nothing),
// the layout launch, decode() (the packed decode's launches, d_place as its offsets) and the headers.
// The first failure returns; everything decidable on the host comes before the first launch.
template <class Prepare, class Decode>
int readn_run(const ReadN& a, Prepare prepare, Decode decode) {
    const ReplyHeaders* h = a.hdr;
    if (h && !reply_form_ok(h->form)) return RLE_E_INVAL;
    if (a.n == 0 && !(h && (h->form & RLE_REPLY_END)))
        return a.total ? readn_layout_launch(a.ulen, a.gap, h, a.place, a.total, 0u, a.stream) : RLE_OK;
    if (!a.out || !a.total || a.n > kMaxGrid) return RLE_E_INVAL;
    if (a.n != 0) {
        if (!a.streams || !a.off || !a.len || !a.ulen || !a.place) return RLE_E_INVAL;
        if (h && h->form != RLE_REPLY_READ && (!h->paths || !h->path_off || !h->path_len)) return RLE_E_INVAL;
        if (const int rc = prepare()) return rc;
    }
    if (const int rc = readn_layout_launch(a.ulen, a.gap, h, a.place, a.total, a.n, a.stream)) return rc;
    if (a.n != 0)
        if (const int rc = decode()) return rc;
    if (!h) return RLE_OK;
    return readn_header_launch(h->paths, h->path_off, h->path_len, a.ulen, a.out, a.place, h->form, a.n, a.total,
                               a.out_cap, a.stream);
}
}  // namespace rle
