// Choosing eviction victims (include/rle_mi355x.h: rle_evict_select_device, rle_evict_gather_device;
// DESIGN.md §4e): the selection over sizes and policy keys that live on the device, in one launch of one
// workgroup (totals, a weighted radix select of the threshold key, the cut among its ties, compaction,
// the sort into eviction order), the gather of the victims' table rows, and their entries.
// Included by csrc/rle_kernels.hip behind rle_relocate.h.
#pragma once

namespace rle {

constexpr u32 kEvictBins = 256u;        // one byte of the key per select pass
constexpr u32 kEvictSortLds = 4096u;    // victims sorted in LDS (48 KiB of keys and indices); more: in d_victims
constexpr u32 kEvictGatherBlock = 256u;

struct EvictIn {
    const uint64_t* key;
    const uint64_t* len;
    const uint64_t* want;
    const uint32_t* live;
    const uint32_t* spare;
    bool slots;   // RLE_EVICT_SLOTS
};
// File i by the header's definitions: what it counts (0 when it is not live; rle_relocate_layout_device's
// max(want, len), rounded up to 16 under RLE_EVICT_SLOTS, modulo 2^64 where `big` refuses the call anyway).
struct EvictFile {
    uint64_t key, size;
    bool live, elig, big;
};
__device__ __forceinline__ EvictFile evict_file(const EvictIn& a, u32 i) {
    const uint64_t len = a.len[i], want = a.want ? a.want[i] : 0u, m = want > len ? want : len;
    EvictFile f;
    f.key = a.key[i];
    f.live = !a.live || a.live[i] != 0u;
    f.elig = f.live && !(a.spare && a.spare[i] != 0u);
    f.big = f.live && m > kMaxBufferBytes;
    f.size = !f.live ? 0u : a.slots ? (m + 15u) & ~(uint64_t)15u : m;
    return f;
}

// Block scan of (bytes, count) pairs over the workgroup's kLayoutBlock threads: the exclusive prefix
// of the calling thread and the sums over all threads.  readn_layout_body's pieces: a wave scan by DPP,
// the wave sums exchanged through LDS in two sets taken in turn (`turn` counts the calls: one barrier
// each).  Called by all threads of the workgroup together.
struct EvictScan {
    uint64_t eb;   // bytes before this thread
    u32 ec;        // count before this thread
    uint64_t tb;   // bytes of all threads
    u32 tc;        // count of all threads
};
__device__ __forceinline__ EvictScan evict_scan(uint64_t b, u32 c, u32& turn) {
    __shared__ uint64_t wb[2][kLayoutWaves];
    __shared__ u32 wc[2][kLayoutWaves];
    const u32 lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave, set = turn++ & 1u;
    uint64_t sb = b;
    sb = dpp_add64<kRowShr1>(sb);
    sb = dpp_add64<kRowShr2>(sb);
    sb = dpp_add64<kRowShr4>(sb);
    sb = dpp_add64<kRowShr8>(sb);
    sb = dpp_add64<kRowBcast15, 0xa>(sb);
    sb = dpp_add64<kRowBcast31, 0xc>(sb);
    const u32 sc = wave_scan_incl(c, 0u, OpAdd());
    if (lane == kWave - 1) {
        wb[set][wv] = sb;
        wc[set][wv] = sc;
    }
    __syncthreads();
    EvictScan r{sb - b, sc - c, 0u, 0u};
    for (u32 w = 0; w < kLayoutWaves; ++w) {
        const uint64_t xb = wb[set][w];
        const u32 xc = wc[set][w];
        if (w < wv) {
            r.eb += xb;
            r.ec += xc;
        }
        r.tb += xb;
        r.tc += xc;
    }
    return r;
}
// Both remaining needs are met by these sums.
__device__ __forceinline__ bool evict_covers(uint64_t b, u32 c, uint64_t need_b, u32 need_c) {
    return b >= need_b && c >= need_c;
}

// Sorts m elements ascending with the bitonic network of ascending comparators (each merge opens with
// the flip i <-> i ^ (k - 1), then the halvings i <-> i ^ j), padded to the next power of two by virtual
// +inf elements at and past m: a pair whose upper partner is there is skipped.  less(x, y): element x
// sorts before element y; swap(x, y) exchanges them.  One barrier per step; the pairs of a step are
// disjoint and each is handled by the thread that owns its lower index.
template <class Less, class Swap>
__device__ __forceinline__ void evict_bitonic(u32 m, Less less, Swap swap) {
    u32 pow2 = 1u;
    while (pow2 < m) pow2 <<= 1;
    for (u32 k = 2u; k <= pow2; k <<= 1)
        for (u32 j = k >> 1; j != 0u; j >>= 1) {
            for (u32 i = threadIdx.x; i < m; i += kLayoutBlock) {
                const u32 l = j == k >> 1 ? i ^ (k - 1u) : i ^ j;
                if (l > i && l < m && less(l, i)) swap(i, l);
            }
            __syncthreads();
        }
}

// ================================================================ selection (rle_evict_select_device)
// One workgroup.  Every loop is bounded by n (no wrap: the launcher bounds n by kMaxGrid), thread t
// takes the files t, t + kLayoutBlock, ... in every pass, so d_keep[i] is written by one thread only.
__global__ __launch_bounds__(kLayoutBlock) void evict_select_kernel(EvictIn a, uint64_t max_bytes, uint32_t max_files,
                                                                    uint32_t* __restrict__ keep, uint32_t* victims,
                                                                    uint64_t* __restrict__ summary, uint32_t n) {
    __shared__ unsigned long long hist_b[kEvictBins];
    __shared__ u32 hist_c[kEvictBins];
    __shared__ uint64_t sort_key[kEvictSortLds];
    __shared__ u32 sort_idx[kEvictSortLds];
    __shared__ unsigned long long s_or, s_and, s_need_b;
    __shared__ u32 s_need_c, s_pick;
    const u32 t = threadIdx.x;
    u32 turn = 0u;

    // 1. the totals over live and over eligible files, and d_keep as if nothing went
    uint64_t lb = 0u, eb = 0u, kor = 0u, kand = ~(uint64_t)0u;
    u32 lc = 0u, ec = 0u;
    bool big = false;
#pragma unroll 4
    for (u32 i = t; i < n; i += kLayoutBlock) {
        const EvictFile f = evict_file(a, i);
        keep[i] = f.live ? 1u : 0u;
        lb += f.size;
        lc += f.live ? 1u : 0u;
        big |= f.big;
        if (f.elig) {
            eb += f.size;
            ec += 1u;
            kor |= f.key;
            kand &= f.key;
        }
    }
    const EvictScan live = evict_scan(lb, lc, turn), elig = evict_scan(eb, ec, turn);
    const bool toolarge = __syncthreads_or(big) != 0;
    uint64_t need_b = live.tb > max_bytes ? live.tb - max_bytes : 0u;
    u32 need_c = max_files != 0u && live.tc > max_files ? live.tc - max_files : 0u;
    const u32 status = toolarge                                       ? RLE_STATUS_TOOLARGE
                       : !evict_covers(elig.tb, elig.tc, need_b, need_c) ? RLE_STATUS_NOFIT
                                                                         : RLE_STATUS_OK;
    if (status != RLE_STATUS_OK || (need_b == 0u && need_c == 0u)) {   // refused, or the store fits
        if (t == 0) {
            summary[0] = status;
            summary[1] = 0u;
            summary[2] = summary[3] = live.tb;
            summary[4] = summary[5] = live.tc;
        }
        return;
    }

    // 2. the threshold key, byte by byte from the first byte that the eligible keys do not share
    if (t == 0) {
        s_or = 0u;
        s_and = ~0ull;
    }
    __syncthreads();
    atomicOr(&s_or, (unsigned long long)kor);
    atomicAnd(&s_and, (unsigned long long)kand);
    __syncthreads();
    const uint64_t differ = s_or ^ s_and;
    int p = differ ? (63 - __clzll((long long)differ)) >> 3 : -1;
    uint64_t prefix = p == 7 ? 0u : (uint64_t)s_and >> (8 * (p + 1)) << (8 * (p + 1));   // bytes p and below: 0
    for (; p >= 0; --p) {
        if (t < kEvictBins) {
            hist_b[t] = 0u;
            hist_c[t] = 0u;
        }
        __syncthreads();
        const u32 sh = 8u * (u32)p;
#pragma unroll 2
        for (u32 i = t; i < n; i += kLayoutBlock) {
            const EvictFile f = evict_file(a, i);
            if (f.elig && (p == 7 || (f.key >> (sh + 8u)) == (prefix >> (sh + 8u)))) {
                const u32 bin = (u32)(f.key >> sh) & (kEvictBins - 1u);
                atomicAdd(&hist_b[bin], (unsigned long long)f.size);
                atomicAdd(&hist_c[bin], 1u);
            }
        }
        __syncthreads();
        const uint64_t hb = t < kEvictBins ? hist_b[t] : 0u;
        const u32 hc = t < kEvictBins ? hist_c[t] : 0u;
        const EvictScan s = evict_scan(hb, hc, turn);
        // the first bin up to which both needs are covered: the bins below it go whole
        if (t < kEvictBins && evict_covers(s.eb + hb, s.ec + hc, need_b, need_c) &&
            !evict_covers(s.eb, s.ec, need_b, need_c)) {
            s_pick = t;
            s_need_b = need_b > s.eb ? need_b - s.eb : 0u;
            s_need_c = need_c > s.ec ? need_c - s.ec : 0u;
        }
        __syncthreads();
        prefix |= (uint64_t)s_pick << sh;
        need_b = s_need_b;
        need_c = s_need_c;
    }

    // 3. among the files with the threshold key, in index order: the last one taken
    uint64_t cb = 0u;
    u32 cc = 0u;
    for (u32 i0 = 0u; i0 < n; i0 += kLayoutBlock) {
        const u32 i = i0 + t;
        bool tie = false;
        uint64_t size = 0u;
        if (i < n) {
            const EvictFile f = evict_file(a, i);
            tie = f.elig && f.key == prefix;
            size = tie ? f.size : 0u;
        }
        const EvictScan s = evict_scan(size, tie ? 1u : 0u, turn);
        const uint64_t xb = cb + s.eb;
        const u32 xc = cc + s.ec;
        if (tie && evict_covers(xb + size, xc + 1u, need_b, need_c) && !evict_covers(xb, xc, need_b, need_c)) s_pick = i;
        cb += s.tb;
        cc += s.tc;
        if (evict_covers(cb, cc, need_b, need_c)) break;
    }
    __syncthreads();
    const u32 last = s_pick;

    // 4. d_keep, and the victims compacted in index order
    u32 m = 0u;
    uint64_t gone = 0u;
    for (u32 i0 = 0u; i0 < n; i0 += kLayoutBlock) {
        const u32 i = i0 + t;
        bool v = false;
        uint64_t size = 0u, key = 0u;
        if (i < n) {
            const EvictFile f = evict_file(a, i);
            v = f.elig && (f.key < prefix || (f.key == prefix && i <= last));
            size = v ? f.size : 0u;
            key = f.key;
        }
        const EvictScan s = evict_scan(size, v ? 1u : 0u, turn);
        if (v) {
            const u32 at = m + s.ec;
            keep[i] = 0u;
            victims[at] = i;
            if (at < kEvictSortLds) {
                sort_key[at] = key;
                sort_idx[at] = i;
            }
        }
        m += s.tc;
        gone += s.tb;
    }
    __syncthreads();

    // 5. eviction order: ascending by (key, index)
    if (m <= kEvictSortLds) {
        evict_bitonic(
            m,
            [&](u32 x, u32 y) {
                return sort_key[x] < sort_key[y] || (sort_key[x] == sort_key[y] && sort_idx[x] < sort_idx[y]);
            },
            [&](u32 x, u32 y) {
                const uint64_t k = sort_key[x];
                const u32 v = sort_idx[x];
                sort_key[x] = sort_key[y];
                sort_idx[x] = sort_idx[y];
                sort_key[y] = k;
                sort_idx[y] = v;
            });
        for (u32 j = t; j < m; j += kLayoutBlock) victims[j] = sort_idx[j];
    } else {
        evict_bitonic(
            m,
            [&](u32 x, u32 y) {
                const u32 vx = victims[x], vy = victims[y];
                const uint64_t kx = a.key[vx], ky = a.key[vy];
                return kx < ky || (kx == ky && vx < vy);
            },
            [&](u32 x, u32 y) {
                const u32 v = victims[x];
                victims[x] = victims[y];
                victims[y] = v;
            });
    }
    if (t == 0) {
        summary[0] = RLE_STATUS_OK;
        summary[1] = m;
        summary[2] = live.tb;
        summary[3] = live.tb - gone;
        summary[4] = live.tc;
        summary[5] = live.tc - m;
    }
}

// ================================================================ the victims' rows (rle_evict_gather_device)
struct EvictTables {
    const uint64_t* in[8];
    uint64_t* out[8];
};
// Thread j below min(m, cap), m read from the summary: row j of every output table from the row of
// victim j (eviction order) or m - 1 - j (reply order).
__global__ __launch_bounds__(kEvictGatherBlock) void evict_gather_kernel(const uint32_t* __restrict__ victims,
                                                                         const uint64_t* __restrict__ summary,
                                                                         uint32_t reply, EvictTables tb, uint32_t ntables,
                                                                         uint32_t cap) {
    const uint64_t j = (uint64_t)blockIdx.x * kEvictGatherBlock + threadIdx.x, m = summary[1];
    if (j >= cap || j >= m) return;
    const u32 v = victims[reply ? m - 1u - j : j];
#pragma unroll
    for (u32 k = 0; k < 8u; ++k)
        if (k < ntables) tb.out[k][j] = tb.in[k][v];
}
}  // namespace rle

extern "C" int rle_evict_select_device(const uint64_t* d_key, const uint64_t* d_len, const uint64_t* d_want,
                                       const uint32_t* d_live, const uint32_t* d_spare, uint64_t max_bytes,
                                       uint32_t max_files, uint32_t flags, uint32_t* d_keep, uint32_t* d_victims,
                                       uint64_t* d_summary, uint32_t n, void* stream) {
    if (!d_summary || (flags & ~(uint32_t)RLE_EVICT_SLOTS) || n > rle::kMaxGrid) return RLE_E_INVAL;
    if (n != 0 && (!d_key || !d_len || !d_keep || !d_victims)) return RLE_E_INVAL;
    const rle::EvictIn in{d_key, d_len, d_want, d_live, d_spare, (flags & RLE_EVICT_SLOTS) != 0u};
    hipLaunchKernelGGL(rle::evict_select_kernel, dim3(1), dim3(rle::kLayoutBlock), 0, (hipStream_t)stream, in, max_bytes,
                       max_files, d_keep, d_victims, d_summary, n);   // (n == 0: the summary, all zero)
    return hipGetLastError() == hipSuccess ? RLE_OK : RLE_E_HIP;
}

extern "C" int rle_evict_gather_device(const uint32_t* d_victims, const uint64_t* d_summary, uint32_t order,
                                       const uint64_t* const* tables_in, uint64_t* const* tables_out, uint32_t ntables,
                                       uint32_t cap, void* stream) {
    if (!d_victims || !d_summary || !tables_in || !tables_out || ntables == 0u || ntables > 8u) return RLE_E_INVAL;
    if (order != RLE_EVICT_ORDER_EVICTION && order != RLE_EVICT_ORDER_REPLY) return RLE_E_INVAL;
    rle::EvictTables tb{};
    for (uint32_t k = 0; k < ntables; ++k) {
        if (!tables_in[k] || !tables_out[k]) return RLE_E_INVAL;
        tb.in[k] = tables_in[k];
        tb.out[k] = tables_out[k];
    }
    if (cap == 0u) return RLE_OK;
    const uint32_t grid = (cap - 1u) / rle::kEvictGatherBlock + 1u;
    hipLaunchKernelGGL(rle::evict_gather_kernel, dim3(grid), dim3(rle::kEvictGatherBlock), 0, (hipStream_t)stream,
                       d_victims, d_summary, order == RLE_EVICT_ORDER_REPLY ? 1u : 0u, tb, ntables, cap);
    return hipGetLastError() == hipSuccess ? RLE_OK : RLE_E_HIP;
}
