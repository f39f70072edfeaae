// rle_fileops.hip — device side of the fused append (RLEappend in
// csrc/rle_dropin.cpp): locating the final run of the decoded old content and building the
// 16-byte splice head the incremental re-encode starts from.
//
// The write path of the reference (src/filesystemApi.c:766-775) decodes the whole stored file,
// appends the new bytes and re-encodes all of it.  The encoder's tokens depend only on runs
// (src/rleCompression.c:13-41: every maximal run of length L is cut into floor((L-1)/9) tokens
// of 9 and one final token of r = L - 9 floor((L-1)/9) in 1..9 bytes), so encode(old ‖ new) is
// encode(old) without its final token, followed by encode(c^r ‖ new), c the last byte of old.
// Only the final run's remainder r has to be known; the old stream's tokens before it are kept.
// The second half of the file is the same append on streams that stay in device memory, without
// decoding them.  The tail scan (rle_tail_batch_device) has one wave parse a stream; its segmented
// form for large stored streams (rle_tail_batch_device_seg) takes the segmented decode's summaries
// and a per-stream scan of its own, and both walk their tiles with tail_tile and close with
// tail_close.  The append in place comes in three modes (AppMode): plain (rle_append_batch_device:
// the slot holds the worst case), size (rle_append_size_batch_device: the new length before anything
// is stored) and fit (rle_append_fit_batch_device: into a slot that merely fits).  Every mode accepts
// a file with app_accept and closes it with app_close; append_kernel<mode> is the one-wave form, and
// the segmented form for large new content (the _seg entries: several waves per file, on the
// segmented encode's device code) is append_seg_entry_kernel<mode> and append_seg_scan_kernel<mode>
// around the summary and write kernels that all modes share.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rle_seg_device.h"
#include "rle_mi355x.h"

namespace rle {

// Start of the final run of mid[0, U): 1 + the last position whose byte differs from mid[U-1]
// (0 when the whole buffer is one run), as an atomicMax into *start (zeroed by the launcher).
// Threads take 16-byte chunks from the end of the buffer backwards; a wave stops as soon as the
// start already found lies past its next chunk, so only the final run (plus one chunk per
// thread) is read.
__global__ __launch_bounds__(256) void last_run_kernel(const uint8_t* __restrict__ mid, uint64_t U,
                                                       unsigned long long* __restrict__ start) {
    const uint8_t c = mid[U - 1];
    const uint64_t nchunks = (U + 15) / 16;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t cc = 0x01010101u * c;
    for (uint64_t q0 = (uint64_t)blockIdx.x * blockDim.x; q0 < nchunks; q0 += stride) {
        // chunks q0 .. q0+255 of this block cover positions below 16 (nchunks - q0); skip the
        // rest of the walk once the final run is known to start above them
        const uint64_t top = 16 * (nchunks - q0);
        if (__hip_atomic_load(start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= top) break;
        const uint64_t q = q0 + threadIdx.x;
        if (q >= nchunks) continue;
        const uint64_t chunk = nchunks - 1 - q;
        const uint4 v = *reinterpret_cast<const uint4*>(mid + 16 * chunk);
        const uint32_t w[4] = {v.x ^ cc, v.y ^ cc, v.z ^ cc, v.w ^ cc};
        int last = -1;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const bool ne = ((w[k >> 2] >> (8 * (k & 3))) & 0xFFu) != 0u;
            if (ne && 16 * chunk + (uint64_t)k < U) last = k;
        }
        if (last >= 0) atomicMax(start, (unsigned long long)(16 * chunk + (uint64_t)last + 1));
    }
}

// Splice head: head[0, 16) = (16 - r) filler bytes ‖ c^r, with r = ((U - start) - 1) % 9 + 1.
// The filler alternates c^1, c^2 (adjacent bytes differ, none equals c), so it encodes to
// itself, one single-byte token per byte, and the head's final r bytes start a fresh run:
// encode(head ‖ new) = filler ‖ encode(c^r ‖ new).  res[0] = r, res[1..2] = a copy of the head.
__global__ void splice_head_kernel(const uint8_t* __restrict__ mid, uint64_t U,
                                   const unsigned long long* __restrict__ start, uint8_t* __restrict__ head,
                                   uint64_t* __restrict__ res) {
    const uint32_t lane = threadIdx.x;
    const uint8_t c = mid[U - 1];
    const uint64_t L = U - *start;
    const uint32_t r = (uint32_t)((L - 1) % 9) + 1;
    if (lane < 16) {
        const uint8_t v = lane >= 16 - r ? c : (uint8_t)(c ^ ((lane & 1) ? 2 : 1));
        head[lane] = v;
        reinterpret_cast<uint8_t*>(res + 1)[lane] = v;
    }
    if (lane == 0) res[0] = r;
}

}  // namespace rle

// Both kernels of rle_append_prepare_device, with the run-start accumulator (*d_start, zero on
// entry) and the results (res[0] = r, res[1..2] = head) where the caller wants them (the drop-in
// keeps them inside its single-copy call buffers).  Not in the public headers.
int rle_append_prepare_launch(const void* d_mid, uint64_t U, void* d_head, unsigned long long* d_start,
                              uint64_t* d_res, hipStream_t s) {
    const uint64_t nchunks = (U + 15) / 16;
    uint64_t blocks = (nchunks + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(rle::last_run_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, (const uint8_t*)d_mid, U,
                       d_start);
    hipLaunchKernelGGL(rle::splice_head_kernel, dim3(1), dim3(64), 0, s, (const uint8_t*)d_mid, U, d_start,
                       (uint8_t*)d_head, d_res);
    return hipGetLastError() == hipSuccess ? RLE_OK : RLE_E_HIP;
}

extern "C" int rle_append_prepare_device(const void* d_mid, uint64_t U, void* d_head, uint64_t* d_meta,
                                         void* stream) {
    if (U == 0 || !d_mid || !d_head || !d_meta) return RLE_E_INVAL;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_meta, 0, sizeof(uint64_t), s) != hipSuccess) return RLE_E_HIP;
    return rle_append_prepare_launch(d_mid, U, d_head, reinterpret_cast<unsigned long long*>(d_meta), d_meta + 1, s);
}

// ================================================================ append to stored streams
// rle_tail_batch_device / rle_append_batch_device (include/rle_mi355x.h): the append of the write
// path on streams that stay compressed in device memory.  encode(x ‖ new) is encode(x) up to its
// final token (offset t, byte c, count r) followed by encode(c^r ‖ new) (tests/test_append_model.py),
// so an append needs (t, r) and the new bytes only.  The tail scan finds (t, r) with the decoder's
// forward token-phase parse (C bytes read, nothing written); the append re-emits the final token
// with the new bytes that extend it and then runs the encode tile walk over the new bytes alone,
// entering it the way a segment of the segmented encode is entered (csrc/rle_segmented.hip
// enc_seg_write): run start, previous byte and output offset given, the first and the last
// 16-byte chunk of its output finished with byte stores.
namespace rle {

constexpr u32 kFileWaves = 4;
constexpr u32 kFileBlock = kWave * kFileWaves;

// rle_append_slot_bytes, on both sides: C + rle_max_compressed_size(A + 9) rounded up to 16, or 0
// past the per-buffer limit.
__host__ __device__ inline uint64_t append_slot_bytes(uint64_t C, uint64_t A) {
    if (C > RLE_MAX_BUFFER_BYTES || A > RLE_MAX_BUFFER_BYTES) return 0u;
    const uint64_t u = A + 9u;
    const uint64_t s = (C + u + u / 2u + 15u) & ~(uint64_t)15u;
    return s > RLE_MAX_BUFFER_BYTES ? 0u : s;
}

// The last token start of the tile at pos (S80: 0x80 per start among the owned positions), into
// `last` when the tile has one.
__device__ __forceinline__ void tail_tile_last(const DecLen& ln, u32 pos, const DecK& kc, u32& last) {
    constexpr uint64_t kOwned = (1ull << kOwnLanes) - 1ull;
    const u32 sa = __builtin_amdgcn_udot4(ln.S80[1], kc.C2, __builtin_amdgcn_udot4(ln.S80[0], kc.C1, 0u, false), false);
    const u32 sb = __builtin_amdgcn_udot4(ln.S80[3], kc.C2, __builtin_amdgcn_udot4(ln.S80[2], kc.C1, 0u, false), false);
    const u32 S16 = ((sa >> 7) | (sb << 1)) & 0xFFFFu;
    const uint64_t has = __builtin_amdgcn_ballot_w64(S16 != 0u) & kOwned;
    if (has) {
        const u32 hl = 63u - (u32)__builtin_clzll(has);
        last = pos + 16u * hl + 31u - (u32)__builtin_clz(readlane(S16, hl));
    }
}
// One tile of a tail scan's walk, at pos of a C-byte stream and entered in token phase d: the decode's
// tile (LDS-DMA, dec_prepare, dec_lengths) without its scatter, staging and stores.  The count-digit
// validation (a 3-byte token whose digit is not '2'..'9', or lies past C while its second byte does
// not, stops the walk: ~0u), the decoded length of the tokens starting in the tile (kSum: added to
// U), the last token start, and the phase leaving the tile.  Bytes at or past C read as zero
// (dec_prepare), and a token starting at C - 1 is one byte long whatever they are (dec_lengths).
template <bool kSum>
__device__ __forceinline__ u32 tail_tile(const uint8_t* cslot, const Refill& next, u32 pos, u32 C, u32 lane,
                                         const DecEntry* tbl, const DecK& kc, u32& d, u32& last, uint64_t& U) {
    constexpr uint64_t kOwned = (1ull << kOwnLanes) - 1ull;
    const u32x4 cur = *reinterpret_cast<const u32x4*>(cslot + 16u * lane);
    next();   // the slot is free once read
    const DecPrep pr = dec_prepare(cur, pos, C, C, lane, tbl, kc);
    const DecLen ln = dec_lengths(pr, d);
    if (__builtin_amdgcn_ballot_w64(ln.serial_lane) & kOwned) return ~0u;
    if (kSum) U += readlane(wave_scan_incl(ln.nout, 0u, OpAdd()), kOwnLanes - 1u);
    tail_tile_last(ln, pos, kc, last);
    d = bfe(readlane(pr.incl, kOwnLanes - 1u), 8u * d, 8);
    return 0u;
}
// The closing rule of both scans: the parse of a C-byte stream (C > 0) ends at C exactly when its
// final token, starting at `last`, is y[C-1] alone or "v v digit" with a digit 1..9.  The tail word,
// or 0 (RLE_STATUS_NOTCANON).
__device__ __forceinline__ uint64_t tail_close(const uint8_t* src, u32 C, u32 last) {
    u32 r = 1u;
    if (last + 1u != C) r = uniform((u32)src[C - 1u]) - 0x30u;
    if ((last + 1u != C && last + 3u != C) || r < 1u || r > 9u) return 0u;
    return (uint64_t)last | ((uint64_t)r << 32);
}

// One wave per stream walks all of its tiles.
__global__ __launch_bounds__(kFileBlock) void tail_scan_kernel(const uint8_t* __restrict__ in,
                                                               const uint64_t* __restrict__ off,
                                                               const uint64_t* __restrict__ len,
                                                               uint64_t* __restrict__ tail,
                                                               uint64_t* __restrict__ ulen,
                                                               uint32_t* __restrict__ status, uint32_t n) {
    __shared__ __attribute__((aligned(16))) uint8_t slots_all[kFileWaves * 2 * kSlot];
    __shared__ __attribute__((aligned(16))) DecEntry tbl[256];
    const u32 lane = threadIdx.x & (kWave - 1);
    const u32 wid = uniform(threadIdx.x / kWave);
    for (u32 k = threadIdx.x; k < 256u; k += kFileBlock) tbl[k] = kDecTable.e[k];
    __syncthreads();
    const u32 b = blockIdx.x * kFileWaves + wid;
    if (b >= n) return;
    const uint64_t C64 = len[b], ioff = off[b];
    const uint8_t* src = in + ioff;
    u32 bad = ((uintptr_t)src & 15u) ? RLE_STATUS_MISALIGNED : 0u;
    if (C64 > kMaxBufferBytes) bad |= RLE_STATUS_TOOLARGE;
    uint64_t w = 0u, U = 0u;
    if (!bad && C64) {
        const u32 C = (u32)C64;
        const u32x4 rsi = make_rsrc(src, (C + 15u) & ~15u);
        const uint8_t* slots = slots_all + wid * 2 * kSlot;
        const DecK kc = dec_k();
        u32 d = 0u, last = 0u;
        const bool stopped = walk_tiles(rsi, 0u, ntiles_for(C), lane, slots, [&](u32 t, const uint8_t* cs, const Refill& nx) {
            return tail_tile<true>(cs, nx, t * kTileStep, C, lane, tbl, kc, d, last, U);
        });
        vm_drain();
        if (!stopped) w = tail_close(src, C, last);
        if (!w) {
            bad = RLE_STATUS_NOTCANON;
            U = 0u;
        }
    }
    if (lane == 0) {
        tail[b] = w;
        if (ulen) ulen[b] = U;
        if (status) status[b] = bad;
    }
}

// The three forms of the append, one-wave and segmented: rle_append_batch_device (kPlain: the slot
// must hold the worst case), rle_append_size_batch_device (kSize: the new length C' to need_out,
// nothing else stored) and rle_append_fit_batch_device (kFit: the only capacity condition is
// cap >= C', and C' goes to need_out).
enum class AppMode { kPlain, kSize, kFit };

// Acceptance of one file, before anything of it is stored: the slot bytes (TOOLARGE when there are
// none), the addresses and, kPlain only, cap >= slot bytes (MISALIGNED), then the tail word against
// the stream's last bytes (NOTCANON), which are read here, ahead of the first store.  kUniform: the
// caller is a whole wave on one file and the bytes read are made wave-uniform.
struct AppFile {
    u32 bad, c, t, r;   // status bits; the final token's byte, offset and count (an empty stream: zeros)
    uint64_t slot;      // rle_append_slot_bytes(C, A)
};
template <AppMode kMode, bool kUniform>
__device__ __forceinline__ AppFile app_accept(uint64_t C64, uint64_t A64, uint64_t w, uint64_t cp, const uint8_t* dst,
                                              const uint8_t* nw) {
    const auto byte = [&](u32 i) { return kUniform ? uniform((u32)dst[i]) : (u32)dst[i]; };
    AppFile f{0u, 0u, (u32)w, (u32)(w >> 32), append_slot_bytes(C64, A64)};
    f.bad = f.slot ? 0u : RLE_STATUS_TOOLARGE;
    if ((((uintptr_t)dst | (uintptr_t)nw) & 15u) || (kMode == AppMode::kPlain && f.slot && cp < f.slot))
        f.bad |= RLE_STATUS_MISALIGNED;
    if (f.bad) return f;
    if (w == 0u) {
        if (C64) f.bad = RLE_STATUS_NOTCANON;
    } else if ((w >> 36) || f.r < 1u || f.r > 9u || C64 != (uint64_t)f.t + (f.r == 1u ? 1u : 3u)) {
        f.bad = RLE_STATUS_NOTCANON;
    } else {
        f.c = byte(f.t);
        if (f.r > 1u && (byte(f.t + 1u) != f.c || byte(f.t + 2u) != 0x30u + f.r)) f.bad = RLE_STATUS_NOTCANON;
    }
    return f;
}
// What a file that is left as it is receives: need_out (kSize, kFit) and the status.
template <AppMode kMode>
__device__ __forceinline__ void app_leave(u32 b, uint64_t need, u32 st, uint64_t* need_out, uint32_t* status) {
    if constexpr (kMode != AppMode::kPlain) need_out[b] = need;
    if (status) status[b] = st;
}
// The closing of an append, by lane 0: everything the file's words receive.  cnew: the new length;
// frs: the start of the final run of the virtual buffer's Uv positions; ulnew: the new decoded length.
template <AppMode kMode>
__device__ __forceinline__ void app_close(u32 b, u32 cnew, u32 frs, u32 Uv, uint64_t ulnew, uint64_t* len,
                                          uint64_t* tail, uint64_t* ulen, uint64_t* need_out, uint32_t* status) {
    const u32 rn = (Uv - frs - 1u) % 9u + 1u;   // the new final token's count
    len[b] = cnew;
    tail[b] = (uint64_t)(cnew - (rn == 1u ? 1u : 3u)) | ((uint64_t)rn << 32);
    if (ulen) ulen[b] = ulnew;
    app_leave<kMode>(b, cnew, RLE_STATUS_OK, need_out, status);
}

// One tile of the append's walk: enc_tile with, on the last tile, the start of the buffer's final
// run (the last run boundary below U; enc_tile_an's own EncState.rs counts the positions past U as
// boundaries there).
__device__ __forceinline__ u32 app_tile(const uint8_t* cslot, const Refill& next, u32 pos, u32 U, u32 lane,
                                        uint8_t* stage, uint8_t* dst, u32x4 rso, EncState& st, const EncK& kc,
                                        const u32* elut, u32& final_rs) {
    const u32x4 cur = *reinterpret_cast<const u32x4*>(cslot + 16u * lane);
    next();   // the slot is free once read
    const EncAn an = enc_analyze_bounds<false>(cur, uint2{0u, 0u}, pos, U, U, lane, st.prev_top, kc);
    if (pos + kTileStep >= U) {
        const u32 left = an.p0 < U ? U - an.p0 : 0u;
        const u32 Bv = lane < kOwnLanes ? an.B & lowmask(left < 16u ? left : 16u) : 0u;
        const u32 lb = Bv ? an.p0 + 31u - (u32)__builtin_clz(Bv) : 0u;
        const u32 m = readlane(wave_scan_incl(lb, 0u, OpMax()), kWave - 1u);
        final_rs = m > st.rs ? m : st.rs;
    }
    return enc_tile_an<false, true>(an, uint2{0u, 0u}, pos, U, U, lane, stage, dst, rso, st, kc, elut);
}

// One wave per file, in each mode.  The walks run over a virtual buffer: 16 head positions (the final
// token's c^r at 16 - r .. 15, never read) followed by the new bytes at 16 .., entered at position 16
// with the run start 16 - r, the previous byte c and the output offset behind the final token as it
// stands with the count r + e (e: the leading new bytes equal to c, up to 9 - r).  An empty stream is
// a plain encode of the new bytes from position 0.
//   size walk   (kSize always; kFit when cap is below the slot bytes, so a file whose slot holds the
//               worst case costs what kPlain costs; kPlain never) a segment summary of the whole range
//               [vs, Uv) (enc_seg_summarize: the tiles' analysis, no staging and no stores), entered
//               with the previous byte c and the run phase r - 1 at position 15 and closed as
//               enc_seg_window closes a segment: C' = the offset behind the final token, the tokens
//               starting in the entering run piece (enc_piece_count), the tokens from the first
//               boundary on.  kSize ends here, and so does a kFit file with cap < C' (NOFIT): nothing
//               of either is stored, and kSize keeps no staging and no selector table in LDS.
//   write walk  (kPlain, kFit) the final token again when e > 0, then the encode tiles.  It starts
//               only when every memory operation of the size walk has completed (vm_drain:
//               walk_tiles counts from zero).
template <AppMode kMode>
__global__ __launch_bounds__(kFileBlock) void append_kernel(uint8_t* streams, const uint64_t* __restrict__ off,
                                                            uint64_t* len, const uint64_t* __restrict__ cap,
                                                            uint64_t* ulen, uint64_t* tail,
                                                            const uint8_t* __restrict__ newb,
                                                            const uint64_t* __restrict__ new_off,
                                                            const uint64_t* __restrict__ new_len,
                                                            uint64_t* __restrict__ need_out, uint32_t* status,
                                                            uint32_t n) {
    constexpr bool kStores = kMode != AppMode::kSize, kSizes = kMode != AppMode::kPlain;
    __shared__ __attribute__((aligned(16))) uint8_t slots_all[kFileWaves * 2 * kSlot];
    __shared__ __attribute__((aligned(16))) uint8_t stage_all[kStores ? kFileWaves * kEncStage : 16];
    __shared__ __attribute__((aligned(16))) u32 elut[kStores ? kInsWaveWords : 4];   // enc_tile_fast's selectors
    const u32 lane = threadIdx.x & (kWave - 1);
    const u32 wid = uniform(threadIdx.x / kWave);
    if constexpr (kStores) {
        for (u32 k = threadIdx.x; k < kInsWaveWords; k += kFileBlock) elut[k] = kEncInsLut.s[k];
        __syncthreads();
    }
    const u32 b = blockIdx.x * kFileWaves + wid;
    if (b >= n) return;
    // every word of the file is loaded here, before the walks' hand-counted memory operations
    const uint64_t C64 = len[b], A64 = new_len[b], w = tail[b], soff = off[b], noff = new_off[b];
    const uint64_t cp = kStores ? cap[b] : 0u;
    const uint64_t ul = (kStores && ulen) ? ulen[b] : 0u;
    uint8_t* dst = streams + soff;
    const uint8_t* nw = newb + noff;
    const AppFile f = app_accept<kMode, true>(C64, A64, w, cp, dst, nw);
    const u32 C = (u32)C64, A = (u32)A64, t = f.t, r = f.r, c = f.c;
    if (f.bad || A == 0u) {   // refused (need 0), or nothing to append (need C): the file is left as it is
        if (lane == 0) app_leave<kMode>(b, f.bad ? 0u : C64, f.bad, need_out, status);
        return;
    }
    u32 vs = 0u, outp = 0u, rs = 0u, e = 0u;
    if (C) {
        const u32 lim = A < 9u - r ? A : 9u - r;
        const bool eq = lane < lim && nw[lane] == (uint8_t)c;
        e = (u32)__builtin_ctzll(__builtin_amdgcn_ballot_w64(!eq));   // <= lim <= 8
        vs = 16u;
        outp = t + (r + e == 1u ? 1u : 3u);
        rs = 16u - r;
    }
    const u32 Uv = vs + A;
    const uint8_t* vsrc = reinterpret_cast<const uint8_t*>((uintptr_t)nw - vs);
    const uint8_t* slots = slots_all + wid * 2 * kSlot;
    u32 bound = (u32)f.slot;   // the bytes of the slot the stores may reach
    if constexpr (kSizes) {
        if (!kStores || cp < f.slot) {
            const uint4 sm = enc_seg_summarize(vsrc, Uv, vs, Uv, lane, slots, SegEntry{vs != 0u, c});
            const u32 piece = vs ? enc_piece_count(uniform(sm.x), r - 1u, uniform(sm.w)) : 0u;
            const u32 cnew = outp + piece + uniform(sm.z);
            if (!kStores || cp < cnew) {
                if (lane == 0) app_leave<kMode>(b, cnew, kStores ? RLE_STATUS_NOFIT : RLE_STATUS_OK, need_out, status);
                return;
            }
            bound = (u32)cp;
            vm_drain();   // the write walk counts its own operations only
        }
    }
    if constexpr (kStores) {
        if (e && lane < 3u) dst[t + lane] = (uint8_t)(lane < 2u ? c : 0x30u + r + e);
        const u32x4 rsi = make_rsrc(vsrc, (Uv + 15u) & ~15u);
        const u32x4 rso = make_rsrc(dst, bound);
        uint8_t* stage = stage_all + wid * kEncStage;
        EncState st{outp, outp & ~15u, c << 24, rs, outp & 15u, false, {}};
        const EncK kc = enc_k();
        u32 final_rs = rs;
        walk_tiles(rsi, vs, ntiles_for(A), lane, slots, [&](u32 k, const uint8_t* cs, const Refill& nx) {
            return app_tile(cs, nx, vs + k * kTileStep, Uv, lane, stage, dst, rso, st, kc, elut, final_rs);
        });
        // the final partial chunk (< 16 bytes, staging chunk 1): byte stores, nothing below the walk's
        // first output byte and nothing past the new length
        if (lane >= st.head && lane < st.out_pos - st.flushed) dst[st.flushed + lane] = stage[16u + lane];
        if (lane == 0) app_close<kMode>(b, st.out_pos, final_rs, Uv, ul + A, len, tail, ulen, need_out, status);
    }
}

// ================================================================ segmented append
// rle_append_batch_device_seg and the _seg forms of the size and fit entries: the same append with
// several waves per file, for new content that is large next to the batch (one wave walks a 1 MiB
// append tile after tile while the chip idles).  The new bytes are cut into the segmented encode's
// segments (seg_count over new_len; the prologue and the plan and map launches of
// csrc/rle_segmented.hip) and go through its summary and write passes themselves
// (enc_seg_summary_pass, enc_seg_write_pass of rle_seg_device.h, which the encode's kernels call
// too), in the one-wave append's virtual coordinates: 16 head positions that are never read, then the
// new bytes.  What differs from an encode is the state entering a file's first segment
// (tests/append_seg_model.py), and all of it reaches the shared passes through the view of a file
// that app_view makes from the entry record:
//   entry    one lane per file accepts it (app_accept) before anything is stored and records c, r, e
//            (the leading new bytes that extend the final token), vs (16, or 0 for an empty stream,
//            which is a plain encode), t, the bound of the stores and the refusal status;
//   summary  the first segment's previous byte is the recorded c, not src[p0 - 1] (the view's entry);
//   scan     the append's own kernel: the encode's window (enc_seg_window) with the carry seeded
//            with the run start 16 - r and the output offset behind the final token; it knows C'
//            (kSize: need_out and the status, and no write launch follows; kFit: a file whose bound
//            is below C' is refused, NOFIT), and the wave rewrites the final token when e > 0 and
//            closes the file (app_close);
//   write    offsets from the plan, entering values and the output bound from the view: d_len and
//            d_tail are outputs of the scan by then and are never read again.
// Dependencies cross kernel boundaries only: no look-back, no ticket, nothing waits.
constexpr u32 kEntryBlock = 256;
struct AppEntry {
    u32 c, r, e, vs, bad, t, need;
};
__device__ __forceinline__ AppEntry app_entry(const uint4* entry, u32 b) {
    const uint4 v = entry[b];
    const u32 x = uniform(v.x);
    return AppEntry{x & 0xFFu, (x >> 8) & 0xFFu, (x >> 16) & 0xFFu, x >> 24, uniform(v.y), uniform(v.z), uniform(v.w)};
}
// File b as the encode's passes see it (streams: the write pass only): the virtual buffer of vs head
// positions and the new bytes, its first segment entered with the stored stream's final byte c, the
// output bounded by the recorded bound; it takes part when the entry kernel accepted it and there is
// something to append.
__device__ __forceinline__ EncView app_view(const uint4* entry, uint8_t* streams, const uint64_t* off,
                                            const uint8_t* newb, const uint64_t* new_off, const uint64_t* new_len,
                                            u32 b) {
    const AppEntry en = app_entry(entry, b);
    const uint64_t A64 = new_len[b];
    const uint8_t* src = reinterpret_cast<const uint8_t*>((uintptr_t)(newb + new_off[b]) - en.vs);
    return EncView{src, streams ? streams + off[b] : nullptr, en.vs + (u32)A64, en.vs, SegEntry{en.vs != 0u, en.c},
                   en.need, !en.bad && A64 != 0u};
}

// The entry record of file b.  The recorded bound is min(cap, slot bytes) (kSize, which has no cap:
// the slot bytes; kPlain: a file with cap below the slot bytes is refused), which the kFit scan
// compares C' with and the writers' store descriptor is made from.
template <AppMode kMode>
__global__ __launch_bounds__(kEntryBlock) void append_seg_entry_kernel(
    const uint8_t* __restrict__ streams, const uint64_t* __restrict__ off, const uint64_t* __restrict__ len,
    const uint64_t* __restrict__ cap, const uint64_t* __restrict__ tail, const uint8_t* __restrict__ newb,
    const uint64_t* __restrict__ new_off, const uint64_t* __restrict__ new_len, u32 n, uint4* __restrict__ entry) {
    const u32 b = blockIdx.x * kEntryBlock + threadIdx.x;
    if (b >= n) return;
    const uint64_t C64 = len[b], A64 = new_len[b], cp = kMode == AppMode::kSize ? ~0ull : cap[b];
    const uint8_t* nw = newb + new_off[b];
    const AppFile f = app_accept<kMode, false>(C64, A64, tail[b], cp, streams + off[b], nw);
    u32 x = 0u;
    if (!f.bad && C64) {
        const u32 lim = A64 < 9u - f.r ? (u32)A64 : 9u - f.r;
        u32 e = 0u;
        while (e < lim && nw[e] == f.c) ++e;
        x = f.c | (f.r << 8) | (e << 16) | (16u << 24);
    }
    entry[b] = make_uint4(x, f.bad, f.t, (u32)(cp < f.slot ? cp : f.slot));
}

__global__ __launch_bounds__(kSegBlock) void append_seg_summary_kernel(const uint8_t* __restrict__ newb,
                                                                       const uint64_t* __restrict__ new_off,
                                                                       const uint64_t* __restrict__ new_len, u32 n,
                                                                       const u32* __restrict__ seg_first,
                                                                       const u32* __restrict__ seg_buf, u32 maxseg,
                                                                       u32 sb, const uint4* __restrict__ entry,
                                                                       uint4* __restrict__ summ) {
    __shared__ __attribute__((aligned(16))) uint8_t slots_all[kSegWaves * 2 * kSlot];
    enc_seg_summary_pass(SegCut{seg_first, seg_buf, new_len, n, maxseg, sb}, summ, slots_all,
                         [=](u32 b) { return app_view(entry, nullptr, nullptr, newb, new_off, new_len, b); });
}

// One wave per file: the encode's scan from the append's entering state, C' = the offset it ends
// at, and everything the file's words receive.  A file that is left as it is (refused, nothing to
// append, kSize, or a kFit file whose bound is below C') has nothing stored but need_out and the
// status and is kept from the write pass (kFlagSkip); kSize writes no plan.
template <AppMode kMode>
__global__ __launch_bounds__(kSegBlock) void append_seg_scan_kernel(
    uint8_t* streams, const uint64_t* __restrict__ off, uint64_t* len, uint64_t* ulen, uint64_t* tail,
    const uint64_t* __restrict__ new_len, uint64_t* __restrict__ need_out, uint32_t* status, u32 n,
    const u32* __restrict__ seg_first, u32 maxseg, u32 sb, const uint4* __restrict__ entry,
    const uint4* __restrict__ summ, uint2* __restrict__ plan, u32* __restrict__ bflag) {
    constexpr bool kStores = kMode != AppMode::kSize, kSizes = kMode != AppMode::kPlain;
    const u32 lane = threadIdx.x & (kWave - 1);
    const u32 b = blockIdx.x * kSegWaves + uniform(threadIdx.x / kWave);
    if (b >= n) return;
    const AppEntry en = app_entry(entry, b);
    const uint64_t A64 = new_len[b];
    const uint64_t ul = (kStores && ulen) ? ulen[b] : 0u;
    const u32 s0 = seg_lo(seg_first, b), s1 = seg_hi(seg_first, b, new_len, sb);
    const u32 bad = en.bad | (s1 > maxseg ? (u32)RLE_STATUS_TOOLARGE : 0u);
    if (bad || A64 == 0u) {   // refused (need 0), or nothing to append (need C)
        if (lane == 0) {
            app_leave<kMode>(b, (bad || !kSizes) ? 0u : len[b], bad, need_out, status);
            bflag[b] = kFlagSkip;
        }
        return;
    }
    const u32 A = (u32)A64, rr = en.r + en.e;
    // entering the first segment: the final token's run c^r ends at virtual position 15, and the
    // output goes on behind that token as it stands once the e bytes are counted into it
    EncCarry cy{en.vs ? 17u - en.r : 0u, en.vs ? en.t + (rr == 1u ? 1u : 3u) : 0u};
    for (u32 base = s0; base < s1; base += kWave) {
        const u32 g = base + lane;
        const bool valid = g < s1;
        const uint4 sm = valid ? summ[g] : make_uint4(0u, 0u, 0u, 0u);
        const uint2 pl = enc_seg_window(sm, valid, en.vs + (g - s0) * sb, cy);
        if (kStores && valid) plan[g] = pl;
    }
    if (kSizes && (!kStores || cy.off > en.need)) {
        if (lane == 0) {
            app_leave<kMode>(b, cy.off, kStores ? (u32)RLE_STATUS_NOFIT : (u32)RLE_STATUS_OK, need_out, status);
            bflag[b] = kFlagSkip;
        }
        return;
    }
    if constexpr (kStores) {
        uint8_t* dst = streams + off[b];
        if (en.e && lane < 3u) dst[en.t + lane] = (uint8_t)(lane < 2u ? en.c : 0x30u + rr);
        if (lane == 0) {
            app_close<kMode>(b, cy.off, cy.lb1 ? cy.lb1 - 1u : 0u, en.vs + A, ul + A, len, tail, ulen, need_out, status);
            bflag[b] = 0u;
        }
    }
}

__global__ __launch_bounds__(kSegBlock) void append_seg_write_kernel(uint8_t* streams, const uint64_t* __restrict__ off,
                                                                     const uint8_t* __restrict__ newb,
                                                                     const uint64_t* __restrict__ new_off,
                                                                     const uint64_t* __restrict__ new_len, u32 n,
                                                                     const u32* __restrict__ seg_first,
                                                                     const u32* __restrict__ seg_buf, u32 maxseg,
                                                                     u32 sb, const uint4* __restrict__ entry,
                                                                     const uint2* __restrict__ plan,
                                                                     const u32* __restrict__ bflag,
                                                                     const uint4* __restrict__ summ) {
    __shared__ __attribute__((aligned(16))) uint8_t slots_all[kSegWaves * 2 * kSlot];
    __shared__ __attribute__((aligned(16))) uint8_t stage_all[kSegWaves * kEncStage];
    __shared__ __attribute__((aligned(16))) u32 elut[kInsWaveWords];
    enc_seg_write_pass(SegCut{seg_first, seg_buf, new_len, n, maxseg, sb}, SegScanned{plan, bflag, summ}, slots_all,
                       stage_all, elut, [=](u32 b) { return app_view(entry, streams, off, newb, new_off, new_len, b); });
}

// ================================================================ segmented tail scan
// rle_tail_batch_device_seg: the tail scan with several waves per stream (one wave walks the 1041
// dependent tiles of a 1 MiB stream while the chip idles).  The stream is cut into the segmented
// decode's segments and summarised by its summary launch itself (seg_launch_dec_summary: per segment
// and entry phase 0..2 the decoded bytes, the exit phase and whether the parse stops: dec_lengths'
// serial_lane on an owned lane, tail_tile's test).  The scan below, one wave per stream, makes the
// per-stream checks, composes the phase maps over windows of 64 segments, sums the counts of the
// phases taken (64 bits across windows: U is the result here and may pass 4 GiB) and refuses the
// stream when a taken phase stops.  The cut puts the final token's start into the last segment (it
// absorbs a remainder of 1-2 bytes), so the same wave then walks that one segment, at most 17 tiles,
// from its now known entry phase with tail_tile for the last token start, and closes with tail_close.
// Nothing is recorded per stream, so the workspace is the decode's.  Dependencies cross kernel
// boundaries only.  The algebra: tests/tail_seg_model.py.
__global__ __launch_bounds__(kSegBlock) void tail_seg_scan_kernel(const uint8_t* __restrict__ in,
                                                                  const uint64_t* __restrict__ off,
                                                                  const uint64_t* __restrict__ len,
                                                                  uint64_t* __restrict__ tail,
                                                                  uint64_t* __restrict__ ulen,
                                                                  uint32_t* __restrict__ status, u32 n,
                                                                  const u32* __restrict__ seg_first, u32 maxseg,
                                                                  u32 sb, const uint4* __restrict__ summ) {
    __shared__ __attribute__((aligned(16))) uint8_t slots_all[kSegWaves * 2 * kSlot];
    __shared__ __attribute__((aligned(16))) DecEntry tbl[256];
    const u32 lane = threadIdx.x & (kWave - 1);
    const u32 wid = uniform(threadIdx.x / kWave);
    for (u32 k = threadIdx.x; k < 256u; k += kSegBlock) tbl[k] = kDecTable.e[k];
    __syncthreads();
    const u32 b = blockIdx.x * kSegWaves + wid;
    if (b >= n) return;
    const uint64_t C64 = len[b];
    const uint8_t* src = in + off[b];
    const u32 s0 = seg_lo(seg_first, b), s1 = seg_hi(seg_first, b, len, sb);
    u32 bad = ((uintptr_t)src & 15u) ? RLE_STATUS_MISALIGNED : 0u;
    if (C64 > kMaxBufferBytes || s1 > maxseg) bad |= RLE_STATUS_TOOLARGE;
    uint64_t w = 0u, U = 0u;
    if (!bad && C64) {
        const u32 C = (u32)C64;
        u32 e = 0u, elast = 0u;   // the phase entering the window, and the one entering the last segment
        bool stop = false;
        for (u32 base = s0; base < s1; base += kWave) {
            const u32 g = base + lane;
            const bool valid = g < s1;
            const uint4 sm = valid ? summ[g] : make_uint4(0u, 0u, 0u, 0u);
            const u32 sel = valid ? (bfe(sm.w, 0, 2) | (bfe(sm.w, 2, 2) << 8) | (bfe(sm.w, 4, 2) << 16) | (3u << 24)) : kMapId;
            const u32 incl = wave_scan_incl(sel, kMapId, OpMap());
            const u32 ein = bfe(from_prev_lane(incl, kMapId), 8u * e, 8);   // the segment's taken entry phase
            const u32 cnt = valid ? (ein == 0u ? sm.x : (ein == 1u ? sm.y : sm.z)) : 0u;
            stop |= __builtin_amdgcn_ballot_w64(valid && ((sm.w >> (8u + ein)) & 1u)) != 0ull;
            U += wave_sum(cnt);   // a window decodes to less than 64 * 17 * 3024 bytes
            elast = readlane(ein, s1 - 1u - base < kWave ? s1 - 1u - base : kWave - 1u);
            e = bfe(readlane(incl, 63), 8u * e, 8);
        }
        u32 q0, q1;
        seg_range(s1 - 1u - s0, s1 - s0, C, sb, q0, q1);
        u32 last = q0 + elast, d = elast;
        if (!stop) {
            const u32x4 rsi = make_rsrc(src, (C + 15u) & ~15u);
            const DecK kc = dec_k();
            stop = walk_tiles(rsi, q0, ntiles_for(q1 - q0), lane, slots_all + wid * 2 * kSlot,
                              [&](u32 t, const uint8_t* cs, const Refill& nx) {
                return tail_tile<false>(cs, nx, q0 + t * kTileStep, C, lane, tbl, kc, d, last, U);
            });
            vm_drain();
        }
        if (!stop) w = tail_close(src, C, last);
        if (!w) {
            bad = RLE_STATUS_NOTCANON;
            U = 0u;
        }
    }
    if (lane == 0) {
        tail[b] = w;
        if (ulen) ulen[b] = U;
        if (status) status[b] = bad;
    }
}

}  // namespace rle

using rle::AppMode;

extern "C" size_t rle_append_slot_bytes(uint64_t C, uint64_t A) { return (size_t)rle::append_slot_bytes(C, A); }

extern "C" int rle_tail_batch_device(const void* d_in, const uint64_t* d_off, const uint64_t* d_len, uint64_t* d_tail,
                                     uint64_t* d_ulen, uint32_t* d_status, uint32_t n, void* stream) {
    if (n == 0) return RLE_OK;
    if (!d_in || !d_off || !d_len || !d_tail) return RLE_E_INVAL;
    hipLaunchKernelGGL(rle::tail_scan_kernel, dim3((n + rle::kFileWaves - 1u) / rle::kFileWaves), dim3(rle::kFileBlock),
                       0, (hipStream_t)stream, (const uint8_t*)d_in, d_off, d_len, d_tail, d_ulen, d_status, n);
    return hipGetLastError() == hipSuccess ? RLE_OK : RLE_E_HIP;
}

// The one-wave append in one mode.  kSize stores to d_need and d_status only and reads neither d_cap
// nor d_ulen; kPlain never touches d_need.
template <AppMode kMode>
static int append_wave(const void* d_streams, const uint64_t* d_off, const uint64_t* d_len, const uint64_t* d_cap,
                       uint64_t* d_ulen, const uint64_t* d_tail, const void* d_new, const uint64_t* d_new_off,
                       const uint64_t* d_new_len, uint64_t* d_need, uint32_t* d_status, uint32_t n, void* stream) {
    hipLaunchKernelGGL(rle::append_kernel<kMode>, dim3((n + rle::kFileWaves - 1u) / rle::kFileWaves),
                       dim3(rle::kFileBlock), 0, (hipStream_t)stream, (uint8_t*)const_cast<void*>(d_streams), d_off,
                       const_cast<uint64_t*>(d_len), d_cap, d_ulen, const_cast<uint64_t*>(d_tail), (const uint8_t*)d_new,
                       d_new_off, d_new_len, d_need, d_status, n);
    return hipGetLastError() == hipSuccess ? RLE_OK : RLE_E_HIP;
}

extern "C" int rle_append_batch_device(void* d_streams, const uint64_t* d_off, uint64_t* d_len, const uint64_t* d_cap,
                                       uint64_t* d_ulen, uint64_t* d_tail, const void* d_new,
                                       const uint64_t* d_new_off, const uint64_t* d_new_len, uint32_t* d_status,
                                       uint32_t n, void* stream) {
    if (n == 0) return RLE_OK;
    if (!d_streams || !d_off || !d_len || !d_cap || !d_tail || !d_new || !d_new_off || !d_new_len) return RLE_E_INVAL;
    return append_wave<AppMode::kPlain>(d_streams, d_off, d_len, d_cap, d_ulen, d_tail, d_new, d_new_off, d_new_len,
                                        nullptr, d_status, n, stream);
}

// The workspace: the segmented encode's carve-up, then one 16-byte entry record per file.
extern "C" size_t rle_append_seg_workspace_bytes(uint32_t n, uint64_t total_new_bytes) {
    rle::SegShape sh;
    rle::seg_prologue(nullptr, 0, n, total_new_bytes, sizeof(uint4) * (size_t)n, &sh);
    return sh.bytes;
}

// The segmented append in one mode: prologue, plan and map, entry, summary, scan, and the write
// unless the mode is kSize (which reads neither d_cap nor d_ulen and stores to d_need and d_status
// only).
template <AppMode kMode>
static int append_seg(const void* d_streams, const uint64_t* d_off, const uint64_t* d_len, const uint64_t* d_cap,
                      uint64_t* d_ulen, const uint64_t* d_tail, const void* d_new, const uint64_t* d_new_off,
                      const uint64_t* d_new_len, uint64_t* d_need, uint32_t* d_status, uint32_t n,
                      uint64_t total_new_bytes, void* d_workspace, size_t workspace_bytes, void* stream) {
    rle::SegShape sh;
    const size_t records = sizeof(uint4) * (size_t)n;   // one entry record per file behind the encode's tables
    if (const int rc = rle::seg_prologue(d_workspace, workspace_bytes, n, total_new_bytes, records, &sh)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    uint4* const entry = static_cast<uint4*>(sh.extra);
    uint8_t* streams = (uint8_t*)const_cast<void*>(d_streams);
    const uint8_t* newb = (const uint8_t*)d_new;
    rle::seg_launch_plan_map(d_new_len, n, sh, s);
    hipLaunchKernelGGL(rle::append_seg_entry_kernel<kMode>, dim3((n + rle::kEntryBlock - 1u) / rle::kEntryBlock),
                       dim3(rle::kEntryBlock), 0, s, streams, d_off, d_len, d_cap, d_tail, newb, d_new_off, d_new_len, n,
                       entry);
    hipLaunchKernelGGL(rle::append_seg_summary_kernel, dim3(sh.grid), dim3(rle::kSegBlock), 0, s, newb, d_new_off,
                       d_new_len, n, sh.seg_first, sh.seg_buf, sh.maxseg, sh.sb, entry, sh.summ);
    hipLaunchKernelGGL(rle::append_seg_scan_kernel<kMode>, dim3(rle::seg_buf_grid(n)), dim3(rle::kSegBlock), 0, s,
                       streams, d_off, const_cast<uint64_t*>(d_len), d_ulen, const_cast<uint64_t*>(d_tail), d_new_len,
                       d_need, d_status, n, sh.seg_first, sh.maxseg, sh.sb, entry, sh.summ, sh.plan, sh.bflag);
    if (kMode != AppMode::kSize)
        hipLaunchKernelGGL(rle::append_seg_write_kernel, dim3(sh.grid), dim3(rle::kSegBlock), 0, s, streams, d_off, newb,
                           d_new_off, d_new_len, n, sh.seg_first, sh.seg_buf, sh.maxseg, sh.sb, entry, sh.plan, sh.bflag,
                           sh.summ);
    return hipGetLastError() == hipSuccess ? RLE_OK : RLE_E_HIP;
}

extern "C" int rle_append_batch_device_seg(void* d_streams, const uint64_t* d_off, uint64_t* d_len,
                                           const uint64_t* d_cap, uint64_t* d_ulen, uint64_t* d_tail,
                                           const void* d_new, const uint64_t* d_new_off, const uint64_t* d_new_len,
                                           uint32_t* d_status, uint32_t n, uint64_t total_new_bytes,
                                           void* d_workspace, size_t workspace_bytes, void* stream) {
    if (n == 0) return RLE_OK;
    if (!d_streams || !d_off || !d_len || !d_cap || !d_tail || !d_new || !d_new_off || !d_new_len) return RLE_E_INVAL;
    return append_seg<AppMode::kPlain>(d_streams, d_off, d_len, d_cap, d_ulen, d_tail, d_new, d_new_off, d_new_len,
                                       nullptr, d_status, n, total_new_bytes, d_workspace, workspace_bytes, stream);
}

extern "C" int rle_append_size_batch_device(const void* d_streams, const uint64_t* d_off, const uint64_t* d_len,
                                            const uint64_t* d_tail, const void* d_new, const uint64_t* d_new_off,
                                            const uint64_t* d_new_len, uint64_t* d_need, uint32_t* d_status,
                                            uint32_t n, void* stream) {
    if (n == 0) return RLE_OK;
    if (!d_streams || !d_off || !d_len || !d_tail || !d_new || !d_new_off || !d_new_len || !d_need) return RLE_E_INVAL;
    return append_wave<AppMode::kSize>(d_streams, d_off, d_len, nullptr, nullptr, d_tail, d_new, d_new_off, d_new_len,
                                       d_need, d_status, n, stream);
}

extern "C" int rle_append_fit_batch_device(void* d_streams, const uint64_t* d_off, uint64_t* d_len,
                                           const uint64_t* d_cap, uint64_t* d_ulen, uint64_t* d_tail,
                                           const void* d_new, const uint64_t* d_new_off, const uint64_t* d_new_len,
                                           uint64_t* d_need, uint32_t* d_status, uint32_t n, void* stream) {
    if (n == 0) return RLE_OK;
    if (!d_streams || !d_off || !d_len || !d_cap || !d_tail || !d_new || !d_new_off || !d_new_len || !d_need)
        return RLE_E_INVAL;
    return append_wave<AppMode::kFit>(d_streams, d_off, d_len, d_cap, d_ulen, d_tail, d_new, d_new_off, d_new_len,
                                      d_need, d_status, n, stream);
}

extern "C" int rle_append_size_batch_device_seg(const void* d_streams, const uint64_t* d_off, const uint64_t* d_len,
                                                const uint64_t* d_tail, const void* d_new, const uint64_t* d_new_off,
                                                const uint64_t* d_new_len, uint64_t* d_need, uint32_t* d_status,
                                                uint32_t n, uint64_t total_new_bytes, void* d_workspace,
                                                size_t workspace_bytes, void* stream) {
    if (n == 0) return RLE_OK;
    if (!d_streams || !d_off || !d_len || !d_tail || !d_new || !d_new_off || !d_new_len || !d_need) return RLE_E_INVAL;
    return append_seg<AppMode::kSize>(d_streams, d_off, d_len, nullptr, nullptr, d_tail, d_new, d_new_off, d_new_len,
                                      d_need, d_status, n, total_new_bytes, d_workspace, workspace_bytes, stream);
}

extern "C" int rle_append_fit_batch_device_seg(void* d_streams, const uint64_t* d_off, uint64_t* d_len,
                                               const uint64_t* d_cap, uint64_t* d_ulen, uint64_t* d_tail,
                                               const void* d_new, const uint64_t* d_new_off, const uint64_t* d_new_len,
                                               uint64_t* d_need, uint32_t* d_status, uint32_t n,
                                               uint64_t total_new_bytes, void* d_workspace, size_t workspace_bytes,
                                               void* stream) {
    if (n == 0) return RLE_OK;
    if (!d_streams || !d_off || !d_len || !d_cap || !d_tail || !d_new || !d_new_off || !d_new_len || !d_need)
        return RLE_E_INVAL;
    return append_seg<AppMode::kFit>(d_streams, d_off, d_len, d_cap, d_ulen, d_tail, d_new, d_new_off, d_new_len,
                                     d_need, d_status, n, total_new_bytes, d_workspace, workspace_bytes, stream);
}

// The workspace: the segmented decode's carve-up, nothing of the scan's own.
extern "C" size_t rle_tail_seg_workspace_bytes(uint32_t n, uint64_t total_in_bytes) {
    rle::SegShape sh;
    rle::seg_prologue(nullptr, 0, n, total_in_bytes, 0, &sh);
    return sh.bytes;
}

extern "C" int rle_tail_batch_device_seg(const void* d_in, const uint64_t* d_off, const uint64_t* d_len,
                                         uint64_t* d_tail, uint64_t* d_ulen, uint32_t* d_status, uint32_t n,
                                         uint64_t total_in_bytes, void* d_workspace, size_t workspace_bytes,
                                         void* stream) {
    if (n == 0) return RLE_OK;
    if (!d_in || !d_off || !d_len || !d_tail) return RLE_E_INVAL;
    rle::SegShape sh;
    if (const int rc = rle::seg_prologue(d_workspace, workspace_bytes, n, total_in_bytes, 0, &sh)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const uint8_t* in = (const uint8_t*)d_in;
    rle::seg_launch_plan_map(d_len, n, sh, s);
    rle::seg_launch_dec_summary(in, d_off, d_len, n, sh, s);
    hipLaunchKernelGGL(rle::tail_seg_scan_kernel, dim3(rle::seg_buf_grid(n)), dim3(rle::kSegBlock), 0, s, in, d_off,
                       d_len, d_tail, d_ulen, d_status, n, sh.seg_first, sh.maxseg, sh.sb, sh.summ);
    return hipGetLastError() == hipSuccess ? RLE_OK : RLE_E_HIP;
}
