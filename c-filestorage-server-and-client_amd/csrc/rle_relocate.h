// Relocating stored streams (include/rle_mi355x.h: rle_relocate_span_bytes, rle_relocate_layout_device,
// rle_relocate_batch_device): the slots' layout as one more caller of readn_layout_body,
// the copy kernel that follows the per-file map the layout left in device memory, and their entries.
// Included by csrc/rle_kernels.hip behind the read-N family.
#pragma once

namespace rle {

// ================================================================ slot layout (rle_relocate_layout_device)
// File i's slot: round_up_16(max(want, len)) bytes when it is selected and that maximum is a size the
// library handles, else none.  The one rule of both launches.
__device__ __forceinline__ uint64_t relocate_cap(uint64_t len, uint64_t want, bool sel) {
    const uint64_t m = want > len ? want : len;
    return sel && m <= kMaxBufferBytes ? (m + 15u) & ~(uint64_t)15u : 0u;
}
// new_off[i] = base + the caps before file i, new_cap[i] = file i's, *total = base + all of them:
// readn_layout_body with no gaps, the caps as its lengths (it asks for each file's once: the cap is
// stored on the way) and the sums started at base.
__global__ __launch_bounds__(kLayoutBlock) void relocate_layout_kernel(const uint64_t* __restrict__ len,
                                                                       const uint64_t* __restrict__ want,
                                                                       const uint32_t* __restrict__ sel,
                                                                       uint64_t base, uint64_t* __restrict__ new_off,
                                                                       uint64_t* __restrict__ new_cap,
                                                                       uint64_t* __restrict__ total, uint32_t n) {
    readn_layout_body(
        [&](u32 i) -> uint64_t {
            const uint64_t c = relocate_cap(len[i], want ? want[i] : 0u, !sel || sel[i] != 0u);
            new_cap[i] = c;
            return c;
        },
        new_off, total, n, base, 0u, [](u32) -> uint64_t { return 0u; });
}

// ================================================================ the copy (rle_relocate_batch_device)
constexpr u32 kRelBlock = 256u;                 // copy_kernel's
constexpr u32 kRelPass = 4u * kRelBlock;        // 16-byte chunks a workgroup moves per pass: four per lane
constexpr uint64_t kRelSpanMin = 16384u;        // span granule: one pass
__device__ __forceinline__ uint64_t readlane64(uint64_t v, u32 l) {
    return (uint64_t)readlane((u32)v, l) | ((uint64_t)readlane((u32)(v >> 32), l) << 32);
}
// The last file whose new_off is at or below `at` (new_off is non-decreasing, new_off[0] <= at): of a
// run of equal offsets, the zero-size slots and the file behind them, that is the file that owns the
// byte.  All 64 lanes probe evenly spaced entries of the candidate range and the range shrinks 64
// times per step: ceil(log64 n) dependent loads.  Wave-uniform result; all lanes active.
__device__ __forceinline__ u32 relocate_find(const uint64_t* __restrict__ new_off, u32 n, uint64_t at, u32 lane) {
    u32 a = 0u, b = n;   // the answer lies in [a, b), new_off[a] <= at
    for (;;) {
        const u32 span = b - a;
        const u32 step = (span + kWave - 1u) / kWave;   // 1 on the last round
        const u32 p = a + lane * step;
        const bool le = p < b && new_off[p] <= at;
        const u32 c = (u32)__builtin_popcountll(__builtin_amdgcn_ballot_w64(le));   // a prefix of the lanes, >= 1
        a = uniform(a + (c - 1u) * step);
        if (step == 1u) return a;
        b = a + step < b ? a + step : b;
    }
}
// The chunk that holds byte C of the stream: bytes at and past `keep` (1..15) of it are zero.
__device__ __forceinline__ u32x4 relocate_mask(u32x4 v, u32 keep) {
    u32x4 r;
#pragma unroll
    for (u32 m = 0; m < 4u; ++m) {
        const u32 lo = 4u * m;
        r[m] = keep >= lo + 4u ? v[m] : keep <= lo ? 0u : v[m] & ((1u << (8u * (keep - lo))) - 1u);
    }
    return r;
}
// Workgroup w owns the destination bytes [dst_base + w * span, + span) below *total: it finds the
// file that owns its first byte, then walks the files forward (their map words loaded 64 files at a
// time, one per lane) until one starts at or past its range's end, and moves each slot's chunks that
// lie in its range: a slot across a span edge is written by both neighbours, each chunk by the one
// whose range holds it.  Chunks at or past round_up_16(C) are neither loaded nor stored.  The status
// words go by a stride of the whole grid over the files.  No workgroup waits for another.
template <bool kNt>
__global__ __launch_bounds__(kRelBlock) void relocate_copy_kernel(
    const uint8_t* __restrict__ src, const uint64_t* __restrict__ off, const uint64_t* __restrict__ len,
    const uint64_t* __restrict__ want, const uint32_t* __restrict__ sel, uint8_t* __restrict__ dst, uint64_t dst_base,
    uint64_t dst_cap, const uint64_t* __restrict__ new_off, const uint64_t* __restrict__ new_cap,
    const uint64_t* __restrict__ total, uint32_t* __restrict__ status, uint32_t n, uint64_t span) {
    const u32 tid = threadIdx.x, lane = tid & (kWave - 1);
    const uint64_t tot = *total;
    const bool nofit = tot > dst_cap;
    if (status) {
        const uint64_t stride = (uint64_t)gridDim.x * kRelBlock;
        for (uint64_t i = (uint64_t)blockIdx.x * kRelBlock + tid; i < n; i += stride) {
            u32 st = RLE_STATUS_OK;
            if (!sel || sel[i] != 0u) {
                const uint64_t C = len[i], w = want ? want[i] : 0u;
                if (nofit) st = RLE_STATUS_NOFIT;
                else if (C > kMaxBufferBytes || w > kMaxBufferBytes) st = RLE_STATUS_TOOLARGE;
                else if ((uintptr_t)(src + off[i]) & 15u) st = RLE_STATUS_MISALIGNED;
            }
            status[i] = st;
        }
    }
    if (nofit) return;
    const uint64_t lo = dst_base + (uint64_t)blockIdx.x * span;
    if (lo >= tot) return;
    const uint64_t hi = tot - lo < span ? tot : lo + span;
    for (u32 i0 = relocate_find(new_off, n, lo, lane); i0 < n; i0 += kWave) {
        const u32 f = i0 + lane < n ? i0 + lane : n - 1u;
        const uint64_t o_l = new_off[f], cap_l = new_cap[f], C_l = len[f], so_l = off[f];
        const u32 cnt = n - i0 < kWave ? n - i0 : kWave;
        for (u32 j = 0; j < cnt; ++j) {
            const uint64_t o = readlane64(o_l, j);
            if (o >= hi) return;
            if (readlane64(cap_l, j) == 0u) continue;
            const uint64_t C = readlane64(C_l, j), so = readlane64(so_l, j);
            if ((uintptr_t)(src + so) & 15u) continue;   // RLE_STATUS_MISALIGNED: the slot stays as it is
            const uint64_t end = o + ((C + 15u) & ~(uint64_t)15u);   // (C <= cap <= RLE_MAX_BUFFER_BYTES)
            const uint64_t from = o > lo ? o : lo, to = end < hi ? end : hi;
            if (from >= to) continue;
            const u32x4* __restrict__ s16 = reinterpret_cast<const u32x4*>(src + so);
            u32x4* __restrict__ d16 = reinterpret_cast<u32x4*>(dst + o);
            const u32 k1 = (u32)((to - o) / 16u);
            const u32 keep = (u32)C & 15u, kp = keep ? (u32)(C / 16u) : 0xFFFFFFFFu;   // the partial chunk
            for (u32 k = (u32)((from - o) / 16u) + tid; k < k1; k += kRelPass) {
                u32x4 v[4];
#pragma unroll
                for (u32 q = 0; q < 4u; ++q) {
                    const u32 c = k + kRelBlock * q;
                    if (c < k1) v[q] = kNt ? __builtin_nontemporal_load(s16 + c) : s16[c];
                }
#pragma unroll
                for (u32 q = 0; q < 4u; ++q) {
                    const u32 c = k + kRelBlock * q;
                    if (c < k1) {
                        const u32x4 x = c == kp ? relocate_mask(v[q], keep) : v[q];
                        if (kNt) __builtin_nontemporal_store(x, d16 + c);
                        else d16[c] = x;
                    }
                }
            }
        }
    }
}

// CUs of the current device (256 where none is usable), asked once per device.
inline uint32_t relocate_cus() {
    static std::atomic<int> cache[16];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 256u;
    int k = dev < 16 ? cache[dev].load(std::memory_order_relaxed) : 0;
    if (k <= 0) {
        if (hipDeviceGetAttribute(&k, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || k <= 0) k = 256;
        if (dev < 16) cache[dev].store(k, std::memory_order_relaxed);
    }
    return (uint32_t)k;
}
inline int relocate_layout_launch(const uint64_t* d_len, const uint64_t* d_want, const uint32_t* d_sel,
                                  uint64_t dst_base, uint64_t* d_new_off, uint64_t* d_new_cap, uint64_t* d_total,
                                  uint32_t n, void* stream) {
    hipLaunchKernelGGL(relocate_layout_kernel, dim3(1), dim3(kLayoutBlock), 0, (hipStream_t)stream, d_len, d_want, d_sel,
                       dst_base, d_new_off, d_new_cap, d_total, n);
    return hipGetLastError() == hipSuccess ? RLE_OK : RLE_E_HIP;
}
}  // namespace rle

extern "C" uint64_t rle_relocate_span_bytes(uint64_t room_bytes) {
    const uint64_t parts = 8ull * rle::relocate_cus();
    const uint64_t per = room_bytes / parts + (room_bytes % parts ? 1u : 0u);
    const uint64_t span = (per + rle::kRelSpanMin - 1u) & ~(rle::kRelSpanMin - 1u);
    return span < rle::kRelSpanMin ? rle::kRelSpanMin : span;
}

extern "C" int rle_relocate_layout_device(const uint64_t* d_len, const uint64_t* d_want, const uint32_t* d_sel,
                                          uint64_t dst_base, uint64_t* d_new_off, uint64_t* d_new_cap,
                                          uint64_t* d_total, uint32_t n, void* stream) {
    if (!d_total || (dst_base & 15u) || n > rle::kMaxGrid) return RLE_E_INVAL;
    if (n != 0 && (!d_len || !d_new_off || !d_new_cap)) return RLE_E_INVAL;
    return rle::relocate_layout_launch(d_len, d_want, d_sel, dst_base, d_new_off, d_new_cap, d_total, n,
                                       stream);   // (n == 0: *d_total = dst_base)
}

extern "C" int rle_relocate_batch_device(const void* d_src, const uint64_t* d_off, const uint64_t* d_len,
                                         const uint64_t* d_want, const uint32_t* d_sel, void* d_dst,
                                         uint64_t dst_base, uint64_t dst_cap, uint64_t* d_new_off,
                                         uint64_t* d_new_cap, uint64_t* d_total, uint32_t* d_status, uint32_t n,
                                         void* stream) {
    if (n == 0)
        return d_total ? rle::relocate_layout_launch(nullptr, nullptr, nullptr, dst_base, nullptr, nullptr, d_total, 0u,
                                                     stream)
                       : (int)RLE_OK;
    if (!d_src || !d_off || !d_len || !d_dst || !d_new_off || !d_new_cap || !d_total) return RLE_E_INVAL;
    if (((uintptr_t)d_dst & 15u) || (dst_base & 15u) || dst_base > dst_cap || n > rle::kMaxGrid) return RLE_E_INVAL;
    if (const int rc = rle::relocate_layout_launch(d_len, d_want, d_sel, dst_base, d_new_off, d_new_cap, d_total, n,
                                                   stream))
        return rc;
    // the span and the grid from the room alone (frozen under capture); one workgroup at least, for the
    // status words; non-temporal by rle_copy_device's rule
    const uint64_t room = dst_cap - dst_base, span = rle_relocate_span_bytes(room);
    const uint64_t want = room / span + (room % span ? 1u : 0u);
    const uint32_t grid = (uint32_t)(want < 1u ? 1u : want);   // (<= 8 * CUs)
    auto kern = room >= (256ull << 20) ? rle::relocate_copy_kernel<true> : rle::relocate_copy_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(rle::kRelBlock), 0, (hipStream_t)stream, (const uint8_t*)d_src, d_off,
                       d_len, d_want, d_sel, (uint8_t*)d_dst, dst_base, dst_cap, d_new_off, d_new_cap, d_total, d_status,
                       n, span);
    return hipGetLastError() == hipSuccess ? RLE_OK : RLE_E_HIP;
}
