// Host side of the full read-N reply (include/rle_mi355x.h: rle_readn_headers_device,
// rle_readn_reply_device in csrc/rle_kernels.hip, rle_readn_reply_device_seg in csrc/rle_segmented.hip):
// the two launches the reply entries share, and their argument checks.  No device code.
#pragma once
#include <stdint.h>

#include "rle_mi355x.h"

namespace rle {
// The full reply's two launches of its own (rle_readn_reply_device and its _seg form, which make them
// around their decode): the layout with the gaps derived from d_path_len (readn_reply_layout_kernel;
// the READ form passes no d_path_len) and the terminator counted, and the headers and the terminator
// (readn_header_kernel; d_total NULL: rle_readn_headers_device, no capacity rule; no launch where
// there is neither a file nor a terminator).
int readn_reply_layout_launch(const uint64_t* d_ulen, const uint64_t* d_path_len, uint64_t* d_place,
                              uint64_t* d_total, uint32_t form, uint32_t n, void* stream);
int readn_header_launch(const void* d_paths, const uint64_t* d_path_off, const uint64_t* d_path_len,
                        const uint64_t* d_ulen, void* d_out, const uint64_t* d_place, uint32_t form, uint32_t n,
                        const uint64_t* d_total, uint64_t out_cap, void* stream);
// RLE_REPLY_READN, RLE_REPLY_READ or RLE_REPLY_READN | RLE_REPLY_END
inline bool reply_form_ok(uint32_t form) {
    return form == RLE_REPLY_READN || form == RLE_REPLY_READ || form == (RLE_REPLY_READN | RLE_REPLY_END);
}
// The host-side argument check of the two reply entries (n > 0 and n == 0 with the terminator)
inline bool reply_args_ok(const void* d_streams, const uint64_t* d_off, const uint64_t* d_len, const uint64_t* d_ulen,
                          const void* d_paths, const uint64_t* d_path_off, const uint64_t* d_path_len,
                          const void* d_out, const uint64_t* d_place, const uint64_t* d_total, uint32_t form,
                          uint32_t n) {
    if (!d_out || !d_total) return false;
    if (n == 0) return true;
    if (!d_streams || !d_off || !d_len || !d_ulen || !d_place) return false;
    return form == RLE_REPLY_READ || (d_paths && d_path_off && d_path_len);
}
}  // namespace rle
