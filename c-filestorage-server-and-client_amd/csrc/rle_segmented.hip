// rle_segmented.hip — the codec for LARGE buffers: several waves per buffer.
//
// A one-wave-per-buffer launch walks a buffer's tiles one after another, so a single big buffer
// (the drop-in's one-call-per-file path, src/filesystemApi.c:766-775, or the large end of a
// mixed batch) runs at one wave's speed.  Here every buffer is cut into segments of 4..16 tiles
// (1008 input bytes each; the launcher aims at ~16 segments per CU) that separate waves process.
// The only state crossing a segment boundary is
// (the algebra, checked against the oracle on CPU: tests/seg_model.py, tests/test_seg_model.py):
//   encode  the run phase entering the segment.  A segment summary holds the offset L0 of its
//           first run boundary, its last boundary lb, whether a boundary-free segment's run
//           continues past it, and the compressed bytes of the tokens from L0 on; a per-buffer
//           scan turns them into each segment's entering run start rs (a running max of lb) and
//           output offset (the entering piece's tokens have a closed form in L0 and the phase).
//   decode  the token phase entering the segment (0..2).  A segment summary holds, for each of
//           the three possible entry phases, the exit phase, the decoded byte count and whether
//           the tiled path would decline; the per-buffer scan composes the exit maps (v_perm
//           selectors, like the in-wave scan) and sums the counts of the phases actually taken.
// Five launches per direction: plan (segments per buffer, exclusive scan), map (each segment's
// buffer), summary (waves over all segments), scan (one wave per buffer), write (waves over all
// segments, the tile steps of rle_device.h with absolute positions, an owned end and a first
// chunk shared with the previous segment written bytewise; encode writes a segment without a run
// boundary from its entering state alone).  Same output as rle_kernels.hip.
// The segment cut and the encode's per-segment device code (summary, scan window, writers) live in
// rle_seg_device.h, which the segmented append (csrc/rle_fileops.hip) builds on as well.
#include "rle_seg_device.h"
#include "rle_reply.h"   // the read-N entries' sequence (rle_readn_batch_device_seg, rle_readn_reply_device_seg)

namespace rle {

// decode write pass staging (chunks per wave, rle_device.h kDecChunks): the launcher takes the
// one-pass 192-chunk kernel when every segment is resident at once, else the 96-chunk one (7 instead
// of 4 workgroups per CU; r3s A/B: 1 MiB random -9 %, mixed batch -27 %, one 64 MiB file +7 % with 96)
constexpr u32 kSegDecChunksOne = RLE_DEC_CHUNKS, kSegDecChunksMany = 96;
// The write passes take the fast tile paths (round 3) and the segments last-summarised first
// (memory-side cache reuse; r3w, same process: configs[2] mixed batch encode -6 %, decode -2 %, 1 MiB
// kinds +-1 %); the summaries count uniform / literal tiles without the full analysis (round 3) and
// sum their lanes' counts once per segment, not per tile (round 5).

// seg_first[i] = segments of buffers < i; seg_first[n] = total.  One workgroup.
__global__ __launch_bounds__(1024) void seg_plan_kernel(const uint64_t* __restrict__ len, u32 n, u32 sb,
                                                        u32* __restrict__ seg_first) {
    __shared__ u32 part[1024];
    const u32 t = threadIdx.x;
    const u32 per = (n + 1023u) / 1024u;
    const u32 b0 = t * per < n ? t * per : n;
    const u32 b1 = b0 + per < n ? b0 + per : n;
    u32 s = 0;
    for (u32 i = b0; i < b1; ++i) s += seg_count(len32(len[i]), sb);
    part[t] = s;
    __syncthreads();
    for (u32 off = 1; off < 1024u; off <<= 1) {
        const u32 v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    u32 base = t ? part[t - 1] : 0u;
    for (u32 i = b0; i < b1; ++i) {
        seg_first[i] = base;
        base += seg_count(len32(len[i]), sb);
    }
    if (t == 1023u) seg_first[n] = part[1023];
}

// seg_buf[g] = the buffer holding segment g, for every segment (one binary search per segment, all
// in parallel), so the persistent summary and write waves find a segment's buffer with one load
constexpr u32 kMapBlock = 256;
__global__ __launch_bounds__(kMapBlock) void seg_map_kernel(const u32* __restrict__ seg_first, u32 n, u32 maxseg,
                                                           u32* __restrict__ seg_buf) {
    const u32 g = blockIdx.x * kMapBlock + threadIdx.x;
    const u32 total = seg_first[n] < maxseg ? seg_first[n] : maxseg;
    if (g >= total) return;
    u32 lo = 0, hi = n;
    while (hi - lo > 1u) {
        const u32 mid = (lo + hi) >> 1;
        if (seg_first[mid] <= g) lo = mid;
        else hi = mid;
    }
    seg_buf[g] = lo;
}
// ================================================================ ENCODE
// Buffer b as the passes of rle_seg_device.h see it (out: the write pass only): all of it is cut
// into segments, no entry state, the default output bound.
__device__ __forceinline__ EncView enc_view(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                            uint8_t* out, const uint64_t* out_off, u32 b) {
    const uint64_t U64 = in_len[b];
    const uint8_t* src = in + in_off[b];
    return EncView{src, out ? out + out_off[b] : nullptr, (u32)U64, 0u, SegEntry{false, 0u}, 0u,
                   U64 > 0 && U64 <= kMaxBufferBytes && !((uintptr_t)src & 15u)};
}

__global__ __launch_bounds__(kSegBlock) void enc_seg_summary_kernel(const uint8_t* __restrict__ in,
                                                                    const uint64_t* __restrict__ in_off,
                                                                    const uint64_t* __restrict__ in_len, u32 n,
                                                                    const u32* __restrict__ seg_first, const u32* __restrict__ seg_buf, u32 maxseg, u32 sb,
                                                                    uint4* __restrict__ summ) {
    __shared__ __attribute__((aligned(16))) uint8_t slots_all[kSegWaves * 2 * kSlot];
    enc_seg_summary_pass(SegCut{seg_first, seg_buf, in_len, n, maxseg, sb}, summ, slots_all,
                         [=](u32 b) { return enc_view(in, in_off, in_len, nullptr, nullptr, b); });
}

// one wave per buffer: entering run start and output offset of every segment, C of the buffer
__global__ __launch_bounds__(kSegBlock) void enc_seg_scan_kernel(const uint8_t* __restrict__ in,
                                                                 const uint64_t* __restrict__ in_off,
                                                                 const uint64_t* __restrict__ in_len,
                                                                 uint8_t* __restrict__ out,
                                                                 const uint64_t* __restrict__ out_off,
                                                                 uint64_t* __restrict__ out_len,
                                                                 uint32_t* __restrict__ status, u32 n,
                                                                 const u32* __restrict__ seg_first, u32 maxseg, u32 sb,
                                                                 const uint4* __restrict__ summ, uint2* __restrict__ plan,
                                                                 u32* __restrict__ bflag) {
    const u32 lane = threadIdx.x & (kWave - 1);
    const u32 b = blockIdx.x * kSegWaves + uniform(threadIdx.x / kWave);
    if (b >= n) return;
    const uint64_t U64 = in_len[b];
    const uint8_t* src = in + in_off[b];
    uint8_t* dst = out + out_off[b];
    const u32 s0 = seg_lo(seg_first, b), s1 = seg_hi(seg_first, b, in_len, sb);
    u32 bad = (((uintptr_t)src | (uintptr_t)dst) & 15u) ? RLE_STATUS_MISALIGNED : 0u;
    if (U64 > kMaxBufferBytes || s1 > maxseg) bad |= RLE_STATUS_TOOLARGE;
    if (bad) {
        if (lane == 0) {
            out_len[b] = 0;
            if (status) status[b] = bad;
            bflag[b] = kFlagSkip;
        }
        return;
    }
    EncCarry c{0u, 0u};
    for (u32 base = s0; base < s1; base += kWave) {
        const u32 g = base + lane;
        const bool valid = g < s1;
        const uint4 sm = valid ? summ[g] : make_uint4(0u, 0u, 0u, 0u);
        const uint2 pl = enc_seg_window(sm, valid, (g - s0) * sb, c);
        if (valid) plan[g] = pl;
    }
    if (lane == 0) {
        out_len[b] = c.off;
        if (status) status[b] = RLE_STATUS_OK;
        bflag[b] = 0u;
    }
}

__global__ __launch_bounds__(kSegBlock) void enc_seg_write_kernel(const uint8_t* __restrict__ in,
                                                                  const uint64_t* __restrict__ in_off,
                                                                  const uint64_t* __restrict__ in_len,
                                                                  uint8_t* __restrict__ out,
                                                                  const uint64_t* __restrict__ out_off, u32 n,
                                                                  const u32* __restrict__ seg_first, const u32* __restrict__ seg_buf, u32 maxseg, u32 sb,
                                                                  const uint2* __restrict__ plan,
                                                                  const u32* __restrict__ bflag,
                                                                  const uint4* __restrict__ summ) {
    __shared__ __attribute__((aligned(16))) uint8_t slots_all[kSegWaves * 2 * kSlot];
    __shared__ __attribute__((aligned(16))) uint8_t stage_all[kSegWaves * kEncStage];
    __shared__ __attribute__((aligned(16))) u32 elut[kInsWaveWords];
    enc_seg_write_pass(SegCut{seg_first, seg_buf, in_len, n, maxseg, sb}, SegScanned{plan, bflag, summ}, slots_all,
                       stage_all, elut, [=](u32 b) { return enc_view(in, in_off, in_len, out, out_off, b); });
}

// ================================================================ DECODE
// Decoded bytes of a non-tail tile entered at phase d when every pair token in it is "v v 2" (random
// and text-like data): then each token's output is its own bytes with the count digit deleted, so
// the count is the owned positions minus the pairs' digits minus the tile's first d positions (the
// literal path's count, dec_tile_fast, without its stores or its per-lane limits).  kNotFast when a
// pair has another count (the caller then runs dec_lengths).  About 40 VALU against ~100 for
// dec_lengths + its sum.
// kLane: the lane's own count (the caller sums the lanes once per segment).
template <bool kLane = false>
__device__ __forceinline__ u32 dec_count_literal(const DecPrep& pr, u32 d, u32 lane, const DecK& kc) {
    constexpr uint64_t kOwned = (1ull << kOwnLanes) - 1ull;
    const u32* w = pr.w;
    const u32 NE16 = (pr.xa >> 7) | (pr.xb << 1);
    // cheap reject first (runs): at most 2 equal neighbours per owned lane
    if (__builtin_amdgcn_ballot_w64(__builtin_popcount(~NE16 & 0xFFFFu) > 2) & kOwned) return kNotFast;
    const u32 dl = bfe(pr.excl, 8u * d, 8);
    const u32 mid = __builtin_amdgcn_perm(0u, pr.ta.y, 0x0C0C0C00u | dl);
    const u32 sa = __builtin_amdgcn_perm(0u, pr.ta.x, 0x0C0C0C00u | dl);
    const u32 sb = __builtin_amdgcn_perm(0u, pr.tb.x, 0x0C0C0C00u | mid);
    const u32 P16 = (sa | (sb << 8)) & ~NE16 & 0xFFFFu;   // pair starts
    const u32 dg[4] = {alignbyte(w[1], w[0], 2), alignbyte(w[2], w[1], 2), alignbyte(w[3], w[2], 2),
                       alignbyte(pr.la, w[3], 2)};
    u32 nz[4];
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
        const u32 t = dg[k] ^ 0x32323232u;
        nz[k] = bitop3<kOrAnd>(faddi<0x7F7F7F7Fu>(t & kc.K7F), t, kc.K80);
    }
    const u32 za = __builtin_amdgcn_udot4(nz[1], kc.C2, __builtin_amdgcn_udot4(nz[0], kc.C1, 0u, false), false);
    const u32 zb = __builtin_amdgcn_udot4(nz[3], kc.C2, __builtin_amdgcn_udot4(nz[2], kc.C1, 0u, false), false);
    const u32 NZ16 = (za >> 7) | (zb << 1);   // digit position j + 2 holds something other than '2'
    const u32 prevP = from_prev_lane(P16, 0u);
    u32 del = ((P16 << 2) | (prevP >> 14)) & 0xFFFFu;
    if (lane == 0u) del |= lowmask(d);
    const u32 K = lane < kOwnLanes ? (~del & 0xFFFFu) : ((prevP >> 15) & 1u);
    if (__builtin_amdgcn_ballot_w64((P16 & NZ16) != 0u) & kOwned) return kNotFast;
    return kLane ? (u32)__builtin_popcount(K) : wave_sum((u32)__builtin_popcount(K));
}

// Whether every token starting in this tile (entry phase d, starts S80 from dec_lengths) carries
// one byte v, the byte of the tile's first token.
__device__ __forceinline__ bool dec_tile_single(const DecPrep& pr, const DecLen& ln, u32 d, const DecK& kc, u32& v) {
    v = (readlane(pr.w[0], 0) >> (8u * d)) & 0xFFu;
    const u32 vv = rep4(v);
    u32 bad = 0;
#pragma unroll
    for (u32 k = 0; k < 4; ++k) {
        const u32 t = pr.w[k] ^ vv;
        bad |= bitop3<kOrAnd>(faddi<0x7F7F7F7Fu>(t & kc.K7F), t, kc.K80) & ln.S80[k];
    }
    return !owned_any(bad != 0u);
}

// One segment's decode summary: for each entry phase 0..2, the decoded bytes (.x .y .z) and, in .w,
// the exit phases (2 bits each), the phases whose tiled path declines (bits 8..10) and the phases
// from which every token carries one byte (bits 11..13: the segment decodes to copies of that byte,
// the one at its first token; dec_seg_fill writes them without reading the segment).  C > 0.
__device__ __forceinline__ uint4 dec_seg_summarize(const uint8_t* src, u32 C, u32 q0, u32 q1, u32 lane,
                                                   const uint8_t* slots, const DecEntry* tbl) {
    const u32x4 rsi = make_rsrc(src, (C + 15u) & ~15u);
    u32 d0 = 0u, d1 = 1u, d2 = 2u, c0 = 0u, c1 = 0u, c2 = 0u, badm = 0u;
    u32 uni = 7u, v0 = 0u, v1 = 0u, v2 = 0u;   // single-byte phases and their bytes
    u32 accm = 0u;       // the lane's decoded bytes over the tiles after the phases merged (summed once)
    bool badl = false;   // ... and whether the lane declined in one of them
    const DecK kc = dec_k();
    walk_seg(rsi, q0, ntiles_for(q1 - q0), lane, slots, [&](u32 t, const uint8_t* cs, const Refill& nx) {
        const u32x4 cur = *reinterpret_cast<const u32x4*>(cs + 16u * lane);
        nx();
        const u32 pos = q0 + t * kTileStep;
        const DecPrep pr = dec_prepare(cur, pos, C, q1, lane, tbl, kc);
        const u32 m63 = readlane(pr.incl, kOwnLanes - 1u);   // lane 63: lookahead only
        if (d0 == d1 && d1 == d2) {   // the three entry phases have merged: one evaluation
            u32 tot = !pr.tail ? dec_count_literal<true>(pr, d0, lane, kc) : kNotFast;
            if (tot == kNotFast) {
                const DecLen ln = dec_lengths(pr, d0);
                // the lane's count and decline, summed once per segment
                tot = lane < kOwnLanes ? ln.nout : 0u;
                badl |= lane < kOwnLanes && ln.serial_lane;
                if (uni) {
                    u32 v;
                    const bool one = dec_tile_single(pr, ln, d0, kc, v);
                    if (!one || v != v0) uni &= ~1u;
                    if (!one || v != v1) uni &= ~2u;
                    if (!one || v != v2) uni &= ~4u;
                }
            } else {
                uni = 0u;   // a literal tile (its own bytes, "v v 2" pairs): not counted as single-byte
            }
            accm += tot;
            d0 = d1 = d2 = bfe(m63, 8u * d0, 8);
        } else {
            const DecLen l0 = dec_lengths(pr, d0);
            c0 += owned_sum(l0.nout);
            badm |= owned_any(l0.serial_lane) ? 1u : 0u;
            const DecLen l1 = dec_lengths(pr, d1);
            c1 += owned_sum(l1.nout);
            badm |= owned_any(l1.serial_lane) ? 2u : 0u;
            const DecLen l2 = dec_lengths(pr, d2);
            c2 += owned_sum(l2.nout);
            badm |= owned_any(l2.serial_lane) ? 4u : 0u;
            if (uni) {
                u32 v;
                bool one = dec_tile_single(pr, l0, d0, kc, v);
                if (!one || (t && v != v0)) uni &= ~1u;
                v0 = t ? v0 : v;
                one = dec_tile_single(pr, l1, d1, kc, v);
                if (!one || (t && v != v1)) uni &= ~2u;
                v1 = t ? v1 : v;
                one = dec_tile_single(pr, l2, d2, kc, v);
                if (!one || (t && v != v2)) uni &= ~4u;
                v2 = t ? v2 : v;
            }
            d0 = bfe(m63, 8u * d0, 8);
            d1 = bfe(m63, 8u * d1, 8);
            d2 = bfe(m63, 8u * d2, 8);
        }
        return 0u;
    });
    const u32 cm = wave_sum(accm);
    c0 += cm; c1 += cm; c2 += cm;
    badm |= __builtin_amdgcn_ballot_w64(badl) ? 7u : 0u;
    return make_uint4(c0, c1, c2, d0 | (d1 << 2) | (d2 << 4) | (badm << 8) | (uni << 11));
}
// the summary of an empty stream: counts 0, exit = entry
constexpr uint4 kDecEmpty = {0u, 0u, 0u, 0u | (1u << 2) | (2u << 4)};

__global__ __launch_bounds__(kSegBlock) void dec_seg_summary_kernel(const uint8_t* __restrict__ in,
                                                                    const uint64_t* __restrict__ in_off,
                                                                    const uint64_t* __restrict__ in_len, u32 n,
                                                                    const u32* __restrict__ seg_first, const u32* __restrict__ seg_buf, u32 maxseg, u32 sb,
                                                                    uint4* __restrict__ summ) {
    __shared__ __attribute__((aligned(16))) uint8_t slots_all[kSegWaves * 2 * kSlot];
    __shared__ DecEntry tbl[256];
    const u32 lane = threadIdx.x & (kWave - 1);
    const u32 wid = uniform(threadIdx.x / kWave);
    for (u32 k = threadIdx.x; k < 256u; k += kSegBlock) tbl[k] = dec_entry_from(kDecTable.e[k]);
    __syncthreads();
    const uint8_t* slots = slots_all + wid * 2 * kSlot;
    seg_walk<false>(SegCut{seg_first, seg_buf, in_len, n, maxseg, sb}, wid, SegScanned{}, [&](const Seg& s) {
        const uint64_t C64 = in_len[s.b];
        const uint8_t* src = in + in_off[s.b];
        uint4 res = kDecEmpty;
        if (C64 > 0 && C64 <= kMaxBufferBytes && !((uintptr_t)src & 15u)) {
            u32 q0, q1;
            seg_range(s.g - s.s0, s.nseg, (u32)C64, sb, q0, q1);
            res = dec_seg_summarize(src, (u32)C64, q0, q1, lane, slots, tbl);
        }
        if (lane == 0) summ[s.g] = res;
    });
}

// The carried state of a decode scan over a buffer's segments: the entry phase, the output offset
// and whether the buffer needs the exact serial path (a taken phase declines, or the stream decodes
// past U).  One window of up to 64 consecutive segments (lane i: segment base + i, summary sm); each
// lane gets its segment's entry phase and output offset; c advances past the window.
struct DecCarry {
    u32 e, off;
    bool serial;
};
__device__ __forceinline__ uint2 dec_seg_window(uint4 sm, bool valid, u32 U, DecCarry& c) {
    const u32 sel = valid ? (bfe(sm.w, 0, 2) | (bfe(sm.w, 2, 2) << 8) | (bfe(sm.w, 4, 2) << 16) | (3u << 24)) : kMapId;
    const u32 incl = wave_scan_incl(sel, kMapId, OpMap());
    const u32 e = bfe(from_prev_lane(incl, kMapId), 8u * c.e, 8);
    const u32 cnt = valid ? (e == 0u ? sm.x : (e == 1u ? sm.y : sm.z)) : 0u;
    c.serial |= __builtin_amdgcn_ballot_w64(valid && ((sm.w >> (8u + e)) & 1u)) != 0;
    const u32 oincl = wave_scan_incl(cnt, 0u, OpAdd());
    const uint2 r = make_uint2(e, c.off + oincl - cnt);
    c.e = bfe(readlane(incl, 63), 8u * c.e, 8);
    const u32 add = readlane(oincl, 63);
    if (add > U - (c.off < U ? c.off : U)) c.serial = true;   // decodes past U
    c.off += add;
    return r;
}

// The scan, one wave per buffer: entry phase and output offset of every segment; serial when the
// taken path declines anywhere or decodes past U.  The aligned and the packed form (kPacked:
// rle_decode_packed_batch_device_seg, rle_readn_batch_device_seg, destinations at any byte) differ in
// what they refuse.  Aligned: a stream or a destination off 16 bytes, or out_cap below U.  Packed: the
// stream's address alone is tested, cap = U; with total (the read-N form: the reply's length, written
// by the layout launch ahead of this one) every file is RLE_STATUS_NOFIT when it passes reply_cap.
// The plan is in file-relative output offsets, and dec_seg_window's "decodes past U" test on U, in
// both.
template <bool kPacked>
__device__ __forceinline__ void dec_seg_scan_body(const uint8_t* in, const uint64_t* in_off, const uint64_t* in_len,
                                                  uint8_t* out, const uint64_t* out_off, const uint64_t* out_len,
                                                  const uint64_t* out_cap, uint32_t* status, u32 n,
                                                  const u32* seg_first, u32 maxseg, u32 sb, const uint4* summ,
                                                  uint2* plan, u32* bflag, const uint64_t* total,
                                                  uint64_t reply_cap) {
    const u32 lane = threadIdx.x & (kWave - 1);
    const u32 b = blockIdx.x * kSegWaves + uniform(threadIdx.x / kWave);
    if (b >= n) return;
    const uint64_t C64 = in_len[b], U64 = out_len[b];
    const uint64_t cap = !kPacked && out_cap ? out_cap[b] : U64;
    const uint64_t tot = kPacked && total ? *total : 0u;
    const uint8_t* src = in + in_off[b];
    const uintptr_t dst = kPacked ? 0u : (uintptr_t)(out + out_off[b]);
    const u32 s0 = seg_lo(seg_first, b), s1 = seg_hi(seg_first, b, in_len, sb);
    u32 bad = ((((uintptr_t)src | dst) & 15u) || cap < U64) ? RLE_STATUS_MISALIGNED : 0u;
    if (C64 > kMaxBufferBytes || U64 > kMaxBufferBytes || s1 > maxseg) bad |= RLE_STATUS_TOOLARGE;
    if (kPacked && tot > reply_cap) bad = RLE_STATUS_NOFIT;
    if (bad) {
        if (lane == 0) {
            if (status) status[b] = bad;
            bflag[b] = kFlagSkip;
        }
        return;
    }
    const u32 U = (u32)U64;
    DecCarry c{0u, 0u, false};
    for (u32 base = s0; base < s1; base += kWave) {
        const u32 g = base + lane;
        const bool valid = g < s1;
        const uint4 sm = valid ? summ[g] : make_uint4(0u, 0u, 0u, 0u);
        const uint2 pl = dec_seg_window(sm, valid, U, c);
        if (valid) plan[g] = pl;
    }
    if (lane == 0) bflag[b] = c.serial ? kFlagSerial : 0u;
}
__global__ __launch_bounds__(kSegBlock) void dec_seg_scan_kernel(const uint8_t* __restrict__ in,
                                                                 const uint64_t* __restrict__ in_off,
                                                                 const uint64_t* __restrict__ in_len,
                                                                 uint8_t* __restrict__ out,
                                                                 const uint64_t* __restrict__ out_off,
                                                                 const uint64_t* __restrict__ out_len,
                                                                 const uint64_t* __restrict__ out_cap,
                                                                 uint32_t* __restrict__ status, u32 n,
                                                                 const u32* __restrict__ seg_first, u32 maxseg, u32 sb,
                                                                 const uint4* __restrict__ summ, uint2* __restrict__ plan,
                                                                 u32* __restrict__ bflag) {
    dec_seg_scan_body<false>(in, in_off, in_len, out, out_off, out_len, out_cap, status, n, seg_first, maxseg, sb, summ,
                             plan, bflag, nullptr, 0u);
}
__global__ __launch_bounds__(kSegBlock) void dec_seg_scan_packed_kernel(const uint8_t* __restrict__ in,
                                                                        const uint64_t* __restrict__ in_off,
                                                                        const uint64_t* __restrict__ in_len,
                                                                        const uint64_t* __restrict__ out_len,
                                                                        uint32_t* __restrict__ status, u32 n,
                                                                        const u32* __restrict__ seg_first, u32 maxseg,
                                                                        u32 sb, const uint4* __restrict__ summ,
                                                                        uint2* __restrict__ plan, u32* __restrict__ bflag,
                                                                        const uint64_t* __restrict__ total,
                                                                        uint64_t reply_cap) {
    dec_seg_scan_body<true>(in, in_off, in_len, nullptr, nullptr, out_len, nullptr, status, n, seg_first, maxseg, sb,
                            summ, plan, bflag, total, reply_cap);
}

// A segment whose tokens all carry one byte v (summary bit 11 + e; never a stream's last segment,
// whose end dec_finish handles) decodes to cnt copies of v: written without reading the segment,
// aligned 16-byte chunks and, at both ends (shared with the neighbouring segments), single bytes.
__device__ RLE_SEG_UNIFORM_ATTR void dec_seg_fill(uint8_t* dst, u32 U, u32 off, u32 cnt, u32 v, u32 lane) {
    const u32 end = off + cnt;
    const u32 a0 = (off + 15u) & ~15u, a1 = end & ~15u;
    const u32 vv = rep4(v);
    for (u32 c0 = a0; c0 < a1; c0 += 16u * kWave) {
        const u32 c = c0 + 16u * lane;
        if (c < a1) *reinterpret_cast<u32x4*>(dst + c) = u32x4{vv, vv, vv, vv};
    }
    const u32 h1 = a0 < end ? a0 : end;
    if (lane < 16u && off + lane < h1) dst[off + lane] = (uint8_t)v;
    const u32 t0 = a1 > a0 ? a1 : a0;
    if (lane < 16u && t0 + lane < end) dst[t0 + lane] = (uint8_t)v;
}

// One segment's output: the tile walk from entry phase e and output offset off; the stream's last
// segment (last) also writes the bytes up to U and the status (st_b, when given).
template <u32 kChunks>
__device__ __forceinline__ void dec_seg_write(const uint8_t* src, uint8_t* dst, u32 C, u32 U, u32 q0, u32 q1, u32 e,
                                              u32 off, bool last, u32 lane, const uint8_t* slots, uint8_t* stage,
                                              const DecEntry* tbl, const u32x4* clut, uint32_t* st_b) {
    const u32x4 rsi = make_rsrc(src, (C + 15u) & ~15u);
    const u32x4 rso = make_rsrc(dst, U);
    DecState st{off, off & ~15u, e, 0u, 0u, off & 15u, 0u, false, {}};
    const DecK kc = dec_k();
    const bool serial = walk_seg(rsi, q0, ntiles_for(q1 - q0), lane, slots, [&](u32 t, const uint8_t* cs, const Refill& nx) {
        // the fast tile paths (round 3): past the segment's shared first chunk, and the literal
        // path only on tiles a later tile of this segment follows (dec_tile)
        return dec_tile<true, kChunks, false>(cs, nx, q0 + t * kTileStep, C, q1, U, lane, tbl, stage, dst, rso, st, kc,
                                               clut);
    });
    dec_finish(st, last ? U : st.out_pos, lane, stage, rso, dst);
    if (last && lane == 0 && st_b) *st_b = serial ? (RLE_STATUS_SERIAL | RLE_STATUS_OVERFLOW) : dec_tiled_status(st, U);
}

template <u32 kSegDecChunks>
__global__ __launch_bounds__(kSegBlock) void dec_seg_write_kernel(const uint8_t* __restrict__ in,
                                                                  const uint64_t* __restrict__ in_off,
                                                                  const uint64_t* __restrict__ in_len,
                                                                  uint8_t* __restrict__ out,
                                                                  const uint64_t* __restrict__ out_off,
                                                                  const uint64_t* __restrict__ out_len,
                                                                  const uint64_t* __restrict__ out_cap,
                                                                  uint32_t* __restrict__ status, u32 n,
                                                                  const u32* __restrict__ seg_first, const u32* __restrict__ seg_buf, u32 maxseg, u32 sb,
                                                                  const uint2* __restrict__ plan,
                                                                  const u32* __restrict__ bflag,
                                                                  const uint4* __restrict__ summ) {
    __shared__ __attribute__((aligned(16))) uint8_t slots_all[kSegWaves * 2 * kSlot];
    constexpr u32 kStage = 32u * kSegDecChunks;
    __shared__ __attribute__((aligned(128))) uint8_t stage_all[kSegWaves * kStage];
    __shared__ DecEntry tbl[256];
    __shared__ u32x4 clut[kCompactEntries];   // dec_tile_fast's selectors
    const u32 lane = threadIdx.x & (kWave - 1);
    const u32 wid = uniform(threadIdx.x / kWave);
    for (u32 k = threadIdx.x; k < 256u; k += kSegBlock) tbl[k] = dec_entry_from(kDecTable.e[k]);
    for (u32 k = threadIdx.x; k < kCompactEntries; k += kSegBlock)
        clut[k] = u32x4{kCompactLut.s[4u * k], kCompactLut.s[4u * k + 1u], kCompactLut.s[4u * k + 2u],
                        kCompactLut.s[4u * k + 3u]};
    uint8_t* stage = stage_all + wid * kStage;
    const uint8_t* slots = slots_all + wid * 2 * kSlot;
    for (u32 k = lane; k < kStage / 16u; k += kWave)
        reinterpret_cast<u32x4*>(stage)[k] = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    const SegScanned scanned{plan, bflag, summ};
    seg_walk<true>(SegCut{seg_first, seg_buf, in_len, n, maxseg, sb}, wid, scanned, [&](const Seg& s) {
        const u32 g = s.g, b = s.b, s0 = s.s0, nseg = s.nseg;
        const uint2 pl = s.pl;
        const uint4 sm = s.sm;
        const u32 C = (u32)in_len[b], U = (u32)out_len[b];
        const uint8_t* src = in + in_off[b];
        uint8_t* dst = out + out_off[b];
        if (s.flag & kFlagSerial) {   // one wave decodes the whole buffer exactly
            if (g == s0) {
                const uint64_t cap = out_cap ? out_cap[b] : (uint64_t)U;
                const u32 stat = dec_serial(src, C, U, cap, dst, lane, stage, kStage);
                if (lane == 0 && status) status[b] = stat;
            }
            return;
        }
        u32 q0, q1;
        seg_range(g - s0, nseg, C, sb, q0, q1);
        if (g + 1u != s0 + nseg) {   // one byte throughout: no second read
            const u32 e = uniform(pl.x);
            if ((uniform(sm.w) >> (11u + e)) & 1u) {
                const u32 cnt = uniform(e == 0u ? sm.x : (e == 1u ? sm.y : sm.z));
                dec_seg_fill(dst, U, uniform(pl.y), cnt, src[q0 + e], lane);
                return;
            }
        }
        dec_seg_write<kSegDecChunks>(src, dst, C, U, q0, q1, uniform(pl.x), uniform(pl.y), g + 1u == s0 + nseg,
                                     lane, slots, stage, tbl, clut, status ? status + b : nullptr);
    });
}

// The packed write pass (rle_decode_packed_batch_device_seg, rle_readn_batch_device_seg: destinations
// at any byte) is a kernel of its own over the same device functions (dec_seg_fill, dec_seg_write).
// One body for both write passes was measured and not kept: with it one aligned cell, 1 x 64 KiB
// runs50, was slower in 2 of 8 passes where no control cell was in more than 1, and
// dec_seg_write_kernel is what the benchmark runs (profiles/readn_fold_ab.md).
// The write pass based the way decode_packed_kernel (rle_kernels.hip) bases one wave's walk: per file
// head = the destination's low four bits, base = dst - head, and the output descriptor covers
// [base, base + head + U) (head + U < 2^31).  A segment whose scanned offset is off enters at
// head + off: DecState.head = (head + off) & 15 and the flushed position is that offset rounded down
// to 16 (dec_seg_write), so the file's first segment gets the packed decode's entry (st.head = head,
// phase 0) and every later one the entry it has in an aligned slot, shifted by head.  The stream's last
// segment closes with dec_finish to head + U, its last chunk by bytes, and takes its status from
// dec_tiled_status against head + U.  No 16-byte store of a segment covers a byte outside that
// segment's output (tests/readn_pack_seg_model.py).  A file the scan flagged serial is decoded by its
// first segment's wave with dec_serial_packed: dec_serial's aligned zero fill would cover the
// neighbours' bytes at both ends.
template <u32 kSegDecChunks>
__global__ __launch_bounds__(kSegBlock) void dec_seg_write_packed_kernel(const uint8_t* __restrict__ in,
                                                                         const uint64_t* __restrict__ in_off,
                                                                         const uint64_t* __restrict__ in_len,
                                                                         uint8_t* __restrict__ out,
                                                                         const uint64_t* __restrict__ out_off,
                                                                         const uint64_t* __restrict__ out_len,
                                                                         uint32_t* __restrict__ status, u32 n,
                                                                         const u32* __restrict__ seg_first,
                                                                         const u32* __restrict__ seg_buf, u32 maxseg,
                                                                         u32 sb, const uint2* __restrict__ plan,
                                                                         const u32* __restrict__ bflag,
                                                                         const uint4* __restrict__ summ) {
    __shared__ __attribute__((aligned(16))) uint8_t slots_all[kSegWaves * 2 * kSlot];
    constexpr u32 kStage = 32u * kSegDecChunks;
    __shared__ __attribute__((aligned(128))) uint8_t stage_all[kSegWaves * kStage];
    __shared__ DecEntry tbl[256];
    __shared__ u32x4 clut[kCompactEntries];   // dec_tile_fast's selectors
    const u32 lane = threadIdx.x & (kWave - 1);
    const u32 wid = uniform(threadIdx.x / kWave);
    for (u32 k = threadIdx.x; k < 256u; k += kSegBlock) tbl[k] = dec_entry_from(kDecTable.e[k]);
    for (u32 k = threadIdx.x; k < kCompactEntries; k += kSegBlock)
        clut[k] = u32x4{kCompactLut.s[4u * k], kCompactLut.s[4u * k + 1u], kCompactLut.s[4u * k + 2u],
                        kCompactLut.s[4u * k + 3u]};
    uint8_t* stage = stage_all + wid * kStage;
    const uint8_t* slots = slots_all + wid * 2 * kSlot;
    for (u32 k = lane; k < kStage / 16u; k += kWave)
        reinterpret_cast<u32x4*>(stage)[k] = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    const SegScanned scanned{plan, bflag, summ};
    seg_walk<true>(SegCut{seg_first, seg_buf, in_len, n, maxseg, sb}, wid, scanned, [&](const Seg& s) {
        const u32 g = s.g, b = s.b, s0 = s.s0, nseg = s.nseg;
        const uint2 pl = s.pl;
        const uint4 sm = s.sm;
        const u32 C = (u32)in_len[b], U = (u32)out_len[b];
        const uint8_t* src = in + in_off[b];
        uint8_t* dst = out + out_off[b];
        if (s.flag & kFlagSerial) {   // one wave decodes the whole file exactly
            if (g == s0) {
                const u32 stat = dec_serial_packed(src, C, U, dst, lane, stage, kStage);
                if (lane == 0 && status) status[b] = stat;
            }
            return;
        }
        const u32 head = uniform((u32)(uintptr_t)dst & 15u);
        uint8_t* base = dst - head;
        const u32 E = head + U, off = head + uniform(pl.y);
        u32 q0, q1;
        seg_range(g - s0, nseg, C, sb, q0, q1);
        if (g + 1u != s0 + nseg) {   // one byte throughout: no second read
            const u32 e = uniform(pl.x);
            if ((uniform(sm.w) >> (11u + e)) & 1u) {
                const u32 cnt = uniform(e == 0u ? sm.x : (e == 1u ? sm.y : sm.z));
                dec_seg_fill(base, E, off, cnt, src[q0 + e], lane);
                return;
            }
        }
        dec_seg_write<kSegDecChunks>(src, base, C, E, q0, q1, uniform(pl.x), off, g + 1u == s0 + nseg, lane, slots,
                                     stage, tbl, clut, status ? status + b : nullptr);
    });
}

}  // namespace rle

// ================================================================ C-ABI launchers
#include <map>
#include <mutex>
#include <utility>

namespace {
// The workspace (seg_first, per-segment summaries and plans, per-buffer flags) belongs to the
// caller (rle_seg_workspace_bytes), like a cub temp-storage argument: the library keeps no
// device memory between calls and nothing tied to a stream or thread.  Host-side cache: CUs.
struct CuCache {
    std::mutex m;
    std::map<int, int> cus;
};
CuCache& cu_cache() {
    static CuCache* p = new CuCache();   // never destroyed: launches may run during exit
    return *p;
}
int device_cus(int* ncu) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return RLE_E_HIP;
    CuCache& P = cu_cache();
    std::lock_guard<std::mutex> g(P.m);
    auto c = P.cus.find(dev);
    if (c == P.cus.end()) {
        int k = 0;
        if (hipDeviceGetAttribute(&k, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || k <= 0) k = 256;
        c = P.cus.emplace(dev, k).first;
    }
    *ncu = c->second;
    return RLE_OK;
}
inline size_t al(size_t x) { return (x + 255u) & ~(size_t)255u; }
// upper bound on the segments of n buffers holding total bytes (each segment but a buffer's
// last covers sb bytes)
inline uint32_t max_segments(uint32_t n, uint64_t total, uint32_t sb) {
    const uint64_t m = total / (sb - 2u) + n;
    return m > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)m;
}
// segment length in bytes: about 16 segments per CU over the batch, 4..16 tiles each
// (longer segments, caps of 32 / 64 tiles, measured slower on the mixed batch: r5w)
inline uint32_t seg_bytes(uint64_t total, int ncu) {
    const uint64_t tiles = (total + rle::kTileStep - 1) / rle::kTileStep;
    uint64_t per = tiles / ((uint64_t)ncu * 16u);
    per = per < rle::kSegTilesMin ? rle::kSegTilesMin : (per > rle::kSegTilesMax ? rle::kSegTilesMax : per);
    return (uint32_t)per * rle::kTileStep;
}
// persistent grids: enough workgroups to fill every CU (RLE_SEG_OCC per CU), never more than the
// segments
#ifndef RLE_SEG_OCC   // 24 since r3s (was 4): workgroups past residency queue behind the first ones
#define RLE_SEG_OCC 24
#endif
inline uint32_t seg_grid(uint32_t maxseg, int ncu) {
    const uint32_t need = (maxseg + rle::kSegWaves - 1) / rle::kSegWaves;
    const uint32_t fill = (uint32_t)ncu * RLE_SEG_OCC;
    const uint32_t g = need < fill ? need : fill;
    return g ? g : 1u;
}
// The launch shape: segment length, segment bound, grid, and the carve-up of the workspace at base.
rle::SegShape seg_shape(char* base, uint32_t n, uint64_t total, int ncu, size_t extra) {
    rle::SegShape sh;
    sh.ncu = ncu;
    sh.sb = seg_bytes(total, ncu);
    sh.maxseg = max_segments(n, total, sh.sb);
    sh.grid = seg_grid(sh.maxseg, ncu);
    const size_t m = sh.maxseg;
    size_t o = 0;
    const auto take = [&](size_t bytes) {
        char* const p = base ? base + o : nullptr;
        o += al(bytes);
        return p;
    };
    sh.seg_first = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * ((size_t)n + 1)));
    sh.seg_buf = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * m));
    sh.summ = reinterpret_cast<uint4*>(take(sizeof(uint4) * m));
    sh.plan = reinterpret_cast<uint2*>(take(sizeof(uint2) * m));
    sh.bflag = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * (size_t)n));
    // reserved, unused: three retired tables whose bytes stay in the published workspace size
    take(al(sizeof(uint32_t) * m) + al(sizeof(uint4) * m) + al(sizeof(uint32_t)));
    sh.extra = take(extra);
    sh.bytes = o;
    return sh;
}
}  // namespace

namespace rle {
int seg_prologue(void* d_workspace, size_t workspace_bytes, uint32_t n, uint64_t total, size_t extra, SegShape* sh) {
    int ncu = 0;
    const int have = device_cus(&ncu);
    *sh = seg_shape(static_cast<char*>(d_workspace), n, total, have == RLE_OK ? ncu : 256, extra);
    if (!d_workspace || workspace_bytes < sh->bytes) return RLE_E_INVAL;
    if (have != RLE_OK) return have;
    if (n == 1u) sh->seg_first = sh->seg_buf = nullptr;
    return RLE_OK;
}
void seg_launch_plan_map(const uint64_t* len, uint32_t n, const SegShape& sh, hipStream_t s) {
    if (!sh.seg_first) return;
    hipLaunchKernelGGL(seg_plan_kernel, dim3(1), dim3(1024), 0, s, len, n, sh.sb, sh.seg_first);
    hipLaunchKernelGGL(seg_map_kernel, dim3((sh.maxseg + kMapBlock - 1) / kMapBlock), dim3(kMapBlock), 0, s,
                       sh.seg_first, n, sh.maxseg, sh.seg_buf);
}
void seg_launch_dec_summary(const uint8_t* in, const uint64_t* off, const uint64_t* len, uint32_t n,
                            const SegShape& sh, hipStream_t s) {
    hipLaunchKernelGGL(dec_seg_summary_kernel, dim3(sh.grid), dim3(kSegBlock), 0, s, in, off, len, n, sh.seg_first,
                       sh.seg_buf, sh.maxseg, sh.sb, sh.summ);
}
}  // namespace rle

extern "C" size_t rle_seg_workspace_bytes(uint32_t n, uint64_t total_in_bytes) {
    rle::SegShape sh;
    rle::seg_prologue(nullptr, 0, n, total_in_bytes, 0, &sh);
    return sh.bytes;
}

// host only: the segment length a launch with this total_in_bytes takes (tests name it)
extern "C" uint32_t rle_seg_segment_bytes(uint64_t total_in_bytes) {
    rle::SegShape sh;
    rle::seg_prologue(nullptr, 0, 1, total_in_bytes, 0, &sh);
    return sh.sb;
}

extern "C" int rle_encode_batch_device_seg(const void* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                           void* d_out, const uint64_t* d_out_off, uint64_t* d_out_len,
                                           uint32_t* d_status, uint32_t n, uint64_t total_in_bytes, void* d_workspace,
                                           size_t workspace_bytes, void* stream) {
    if (n == 0) return RLE_OK;
    if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_len) return RLE_E_INVAL;
    rle::SegShape sh;
    if (const int rc = rle::seg_prologue(d_workspace, workspace_bytes, n, total_in_bytes, 0, &sh)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const uint8_t* in = (const uint8_t*)d_in;
    uint8_t* out = (uint8_t*)d_out;
    rle::seg_launch_plan_map(d_in_len, n, sh, s);
    hipLaunchKernelGGL(rle::enc_seg_summary_kernel, dim3(sh.grid), dim3(rle::kSegBlock), 0, s, in, d_in_off, d_in_len,
                       n, sh.seg_first, sh.seg_buf, sh.maxseg, sh.sb, sh.summ);
    hipLaunchKernelGGL(rle::enc_seg_scan_kernel, dim3(rle::seg_buf_grid(n)), dim3(rle::kSegBlock), 0, s, in, d_in_off,
                       d_in_len, out, d_out_off, d_out_len, d_status, n, sh.seg_first, sh.maxseg, sh.sb, sh.summ,
                       sh.plan, sh.bflag);
    hipLaunchKernelGGL(rle::enc_seg_write_kernel, dim3(sh.grid), dim3(rle::kSegBlock), 0, s, in, d_in_off, d_in_len,
                       out, d_out_off, n, sh.seg_first, sh.seg_buf, sh.maxseg, sh.sb, sh.plan, sh.bflag, sh.summ);
    return hipGetLastError() == hipSuccess ? RLE_OK : RLE_E_HIP;
}

extern "C" int rle_decode_batch_device_seg(const void* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                           void* d_out, const uint64_t* d_out_off, const uint64_t* d_out_len,
                                           const uint64_t* d_out_cap, uint32_t* d_status, uint32_t n,
                                           uint64_t total_in_bytes, void* d_workspace, size_t workspace_bytes,
                                           void* stream) {
    if (n == 0) return RLE_OK;
    if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_len) return RLE_E_INVAL;
    rle::SegShape sh;
    if (const int rc = rle::seg_prologue(d_workspace, workspace_bytes, n, total_in_bytes, 0, &sh)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    const uint8_t* in = (const uint8_t*)d_in;
    uint8_t* out = (uint8_t*)d_out;
    rle::seg_launch_plan_map(d_in_len, n, sh, s);
    rle::seg_launch_dec_summary(in, d_in_off, d_in_len, n, sh, s);
    hipLaunchKernelGGL(rle::dec_seg_scan_kernel, dim3(rle::seg_buf_grid(n)), dim3(rle::kSegBlock), 0, s, in, d_in_off,
                       d_in_len, out, d_out_off, d_out_len, d_out_cap, d_status, n, sh.seg_first, sh.maxseg, sh.sb,
                       sh.summ, sh.plan, sh.bflag);
    const bool one_round = sh.maxseg <= (uint32_t)sh.ncu * 16u;   // the 192-chunk kernel's residency
    hipLaunchKernelGGL(one_round ? rle::dec_seg_write_kernel<rle::kSegDecChunksOne>
                                 : rle::dec_seg_write_kernel<rle::kSegDecChunksMany>,
                       dim3(sh.grid), dim3(rle::kSegBlock), 0, s, in, d_in_off, d_in_len, out, d_out_off, d_out_len,
                       d_out_cap, d_status, n, sh.seg_first, sh.seg_buf, sh.maxseg, sh.sb, sh.plan, sh.bflag, sh.summ);
    return hipGetLastError() == hipSuccess ? RLE_OK : RLE_E_HIP;
}

namespace {
// The segmented packed decode's launches, shared by rle_decode_packed_batch_device_seg (d_total NULL)
// and rle_readn_batch_device_seg (behind its layout launch): the segmented decode's plan, map and
// summary, which read only the streams, then the packed scan and write; the staging choice is the
// segmented decode's for the same maxseg.
int packed_seg_launch(const void* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len, void* d_out,
                      const uint64_t* d_out_off, const uint64_t* d_out_len, uint32_t* d_status, uint32_t n,
                      const uint64_t* d_total, uint64_t out_cap, const rle::SegShape& sh, hipStream_t s) {
    const uint8_t* in = (const uint8_t*)d_in;
    uint8_t* out = (uint8_t*)d_out;
    rle::seg_launch_plan_map(d_in_len, n, sh, s);
    rle::seg_launch_dec_summary(in, d_in_off, d_in_len, n, sh, s);
    hipLaunchKernelGGL(rle::dec_seg_scan_packed_kernel, dim3(rle::seg_buf_grid(n)), dim3(rle::kSegBlock), 0, s, in,
                       d_in_off, d_in_len, d_out_len, d_status, n, sh.seg_first, sh.maxseg, sh.sb, sh.summ, sh.plan,
                       sh.bflag, d_total, out_cap);
    const bool one_round = sh.maxseg <= (uint32_t)sh.ncu * 16u;
    hipLaunchKernelGGL(one_round ? rle::dec_seg_write_packed_kernel<rle::kSegDecChunksOne>
                                 : rle::dec_seg_write_packed_kernel<rle::kSegDecChunksMany>,
                       dim3(sh.grid), dim3(rle::kSegBlock), 0, s, in, d_in_off, d_in_len, out, d_out_off, d_out_len,
                       d_status, n, sh.seg_first, sh.seg_buf, sh.maxseg, sh.sb, sh.plan, sh.bflag, sh.summ);
    return hipGetLastError() == hipSuccess ? RLE_OK : RLE_E_HIP;
}
// The read-N sequence (rle_reply.h) over the segmented launches: the workspace check ahead of the
// layout launch, and packed_seg_launch into the places it wrote.
int readn_seg_run(const rle::ReadN& a, uint32_t* d_status, uint64_t total_in_bytes, void* d_workspace,
                  size_t workspace_bytes) {
    rle::SegShape sh;
    return rle::readn_run(
        a, [&] { return rle::seg_prologue(d_workspace, workspace_bytes, a.n, total_in_bytes, 0, &sh); },
        [&] {
            return packed_seg_launch(a.streams, a.off, a.len, a.out, a.place, a.ulen, d_status, a.n, a.total, a.out_cap,
                                     sh, (hipStream_t)a.stream);
        });
}
}  // namespace

extern "C" size_t rle_decode_packed_seg_workspace_bytes(uint32_t n, uint64_t total_in_bytes) {
    return rle_seg_workspace_bytes(n, total_in_bytes);
}

extern "C" int rle_decode_packed_batch_device_seg(const void* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                                  void* d_out, const uint64_t* d_out_off, const uint64_t* d_out_len,
                                                  uint32_t* d_status, uint32_t n, uint64_t total_in_bytes,
                                                  void* d_workspace, size_t workspace_bytes, void* stream) {
    if (n == 0) return RLE_OK;
    if (!d_in || !d_in_off || !d_in_len || !d_out || !d_out_off || !d_out_len) return RLE_E_INVAL;
    rle::SegShape sh;
    if (const int rc = rle::seg_prologue(d_workspace, workspace_bytes, n, total_in_bytes, 0, &sh)) return rc;
    return packed_seg_launch(d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_len, d_status, n, nullptr, 0u, sh,
                             (hipStream_t)stream);
}

extern "C" int rle_readn_batch_device_seg(const void* d_streams, const uint64_t* d_off, const uint64_t* d_len,
                                          const uint64_t* d_ulen, const uint64_t* d_gap, void* d_out, uint64_t out_cap,
                                          uint64_t* d_place, uint64_t* d_total, uint32_t* d_status, uint32_t n,
                                          uint64_t total_in_bytes, void* d_workspace, size_t workspace_bytes,
                                          void* stream) {
    return readn_seg_run(rle::ReadN{d_streams, d_off, d_len, d_ulen, d_gap, d_out, out_cap, d_place, d_total, n, nullptr,
                                    stream},
                         d_status, total_in_bytes, d_workspace, workspace_bytes);
}

extern "C" int rle_readn_reply_device_seg(const void* d_streams, const uint64_t* d_off, const uint64_t* d_len,
                                          const uint64_t* d_ulen, const void* d_paths, const uint64_t* d_path_off,
                                          const uint64_t* d_path_len, void* d_out, uint64_t out_cap,
                                          uint64_t* d_place, uint64_t* d_total, uint32_t* d_status, uint32_t form,
                                          uint32_t n, uint64_t total_in_bytes, void* d_workspace,
                                          size_t workspace_bytes, void* stream) {
    const rle::ReplyHeaders hdr{d_paths, d_path_off, d_path_len, form};
    return readn_seg_run(rle::ReadN{d_streams, d_off, d_len, d_ulen, nullptr, d_out, out_cap, d_place, d_total, n, &hdr,
                                    stream},
                         d_status, total_in_bytes, d_workspace, workspace_bytes);
}
