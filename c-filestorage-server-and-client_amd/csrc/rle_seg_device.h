// rle_seg_device.h — the device code of the segmented encode that more than one translation unit
// uses: the segment cut (seg_count, seg_range), the persistent walk over a launch's segments
// (seg_walk), a segment's summary, the per-buffer scan window, the two segment writers, and the
// encode's summary and write passes over a per-buffer view (EncView).  csrc/rle_segmented.hip builds
// the segmented codec from it, and csrc/rle_fileops.hip the segmented append
// (rle_append_batch_device_seg), whose view enters a file's first segment with the state an append
// carries and runs every later segment as the encode does.  The host side at the end declares the
// launch shape and prologue that every segmented entry point shares, and the decode's summary launch,
// which the segmented tail scan (rle_tail_batch_device_seg, csrc/rle_fileops.hip) makes as well.
// The algebra: tests/seg_model.py, tests/append_seg_model.py, tests/tail_seg_model.py.
#pragma once
#include "rle_device.h"

namespace rle {

// Segment length: seg_tiles tiles of 1008 input bytes, a kernel argument chosen by the launcher
// (4..16 tiles: about 16 segments per CU over the batch).
#ifndef RLE_SEG_TILES_MAX   // 16 since r3s (was 64): more, shorter segments fill the chip better
#define RLE_SEG_TILES_MAX 16
#endif
constexpr u32 kSegTilesMin = 4, kSegTilesMax = RLE_SEG_TILES_MAX;
constexpr u32 kSegWaves = 4;
constexpr u32 kSegBlock = kWave * kSegWaves;
constexpr u32 kNone = 0xFFFFFFFFu;
// per-buffer flags (workspace) written by the scans, read by the writers
constexpr u32 kFlagSkip = 1u;     // bad buffer: status already written
constexpr u32 kFlagSerial = 2u;   // decode: the exact serial path handles the whole buffer
// Segments of an n-byte buffer: n = q S + r gives q + (r >= 3) segments (at least one); the last
// absorbs a remainder of 1-2 bytes, so a stream's final token never starts a segment of its own.
__device__ __forceinline__ u32 seg_count(u32 n, u32 sb) {
    const u32 k = (u32)(((uint64_t)n + sb - 3u) / sb);
    return k ? k : 1u;
}
__device__ __forceinline__ u32 len32(uint64_t n) { return n > kMaxBufferBytes ? 0u : (u32)n; }

// A launch of one buffer (the drop-in's single large calls) skips the plan and map launches: the
// launcher passes seg_first = seg_buf = nullptr, and every segment is buffer 0's, its segments
// [0, seg_count(in_len[0])) (round 5).
__device__ __forceinline__ u32 seg_total(const u32* seg_first, u32 n, const uint64_t* len, u32 sb) {
    return seg_first ? uniform(seg_first[n]) : seg_count(len32(len[0]), sb);
}
__device__ __forceinline__ u32 seg_of(const u32* seg_buf, u32 g) { return seg_buf ? uniform(seg_buf[g]) : 0u; }
__device__ __forceinline__ u32 seg_lo(const u32* seg_first, u32 b) { return seg_first ? uniform(seg_first[b]) : 0u; }
__device__ __forceinline__ u32 seg_hi(const u32* seg_first, u32 b, const uint64_t* len, u32 sb) {
    return seg_first ? uniform(seg_first[b + 1]) : seg_count(len32(len[0]), sb);
}
__device__ __forceinline__ void seg_range(u32 i, u32 nseg, u32 n, u32 sb, u32& p0, u32& p1) {
    p0 = i * sb;
    p1 = (i + 1u == nseg) ? n : p0 + sb;
}

// The persistent walk of every summary and write kernel (encode, decode, append) over a launch's
// segments: wave wid of workgroup k takes segments 4 k + wid, + 4 gridDim.x, ... below the segment
// bound, and the body gets each one with its buffer b and that buffer's segments [s0, s0 + nseg).
// The summaries go forward.  The writes (kWrite) go last-summarised first (memory-side cache reuse,
// r3w), get the segment's own plan and summary words, loaded with its buffer index, not after it,
// and the buffer's flags, and never see a segment of a buffer the scan refused (kFlagSkip).
struct SegCut {   // the cut as the kernels are told it: tables (null for one buffer), lengths, bounds
    const u32* seg_first;
    const u32* seg_buf;
    const uint64_t* len;
    u32 n, maxseg, sb;
};
struct SegScanned {   // what the scan left for the write pass
    const uint2* plan;
    const u32* bflag;
    const uint4* summ;
};
struct Seg {
    u32 g, b, s0, nseg;
    u32 flag;   // the write passes only, as pl and sm
    uint2 pl;
    uint4 sm;
};
template <bool kWrite, class Body>
__device__ __forceinline__ void seg_walk(const SegCut& k, u32 wid, const SegScanned& w, Body body) {
    u32 total = seg_total(k.seg_first, k.n, k.len, k.sb);
    total = total < k.maxseg ? total : k.maxseg;
    for (u32 g0 = blockIdx.x * kSegWaves + wid; g0 < total; g0 += gridDim.x * kSegWaves) {
        Seg s{};
        s.g = kWrite ? total - 1u - g0 : g0;
        if (kWrite) {
            s.pl = w.plan[s.g];
            s.sm = w.summ[s.g];
        }
        s.b = seg_of(k.seg_buf, s.g);
        if (kWrite) {
            s.flag = uniform(w.bflag[s.b]);
            if (s.flag & kFlagSkip) continue;
        }
        s.s0 = seg_lo(k.seg_first, s.b);
        s.nseg = seg_hi(k.seg_first, s.b, k.len, k.sb) - s.s0;
        body(s);
    }
}

__device__ __forceinline__ u32 wave_sum(u32 x) { return readlane(wave_scan_incl(x, 0u, OpAdd()), 63); }
// over the tile-owning lanes 0..62 (lane 63 holds the lookahead only)
__device__ __forceinline__ u32 owned_sum(u32 x) { return readlane(wave_scan_incl(x, 0u, OpAdd()), kOwnLanes - 1u); }
__device__ __forceinline__ bool owned_any(bool x) {
    return (__builtin_amdgcn_ballot_w64(x) & ((1ull << kOwnLanes) - 1ull)) != 0ull;
}

// A segment's tile walk: walk_tiles (rle_device.h) through the wave's two LDS-DMA slots.  (Its own
// inlined function: the segment kernels' instruction order depends on it, checked in the listings.)
template <class Step>
__device__ __forceinline__ bool walk_seg(u32x4 rs, u32 start, u32 ntiles, u32 lane, const uint8_t* slots, Step step) {
    return walk_tiles(rs, start, ntiles, lane, slots, step);
}

// compressed bytes of the tokens starting in a segment's entering run piece (length L0) when the
// byte before the segment has run phase q; cont: the piece's run continues past the segment
__device__ __forceinline__ u32 enc_piece_count(u32 L0, u32 q, u32 cont) {
    const u32 k0 = q >= 8u ? 0u : 8u - q;
    if (L0 <= k0) return 0u;
    const u32 n = (L0 - 1u - k0) / 9u + 1u;
    const bool last_is_start = (L0 - 1u - k0) % 9u == 0u;
    return 3u * n - ((last_is_start && !cont) ? 2u : 0u);
}

// The byte in front of a segment, when it is not src[p0 - 1]: the first segment of an append's new
// bytes starts at p0 = 16 of a virtual buffer whose 16 head positions are never read (they lie in
// front of the caller's buffer), and the byte before it is the stored stream's final byte c.
struct SegEntry {
    bool given;
    u32 prev;   // the byte, when given
};
__device__ __forceinline__ u32 seg_prev_top(const uint8_t* src, u32 p0, SegEntry en) {
    if (en.given) return en.prev << 24;
    return p0 ? (u32)src[p0 - 1u] << 24 : 0u;
}

// One segment's encode summary (L0, lb + 1 or 0, rest, cont; see the top of rle_segmented.hip): a
// walk over its tiles, analysis only.  U > 0, src 16-byte aligned.
__device__ __forceinline__ uint4 enc_seg_summarize(const uint8_t* src, u32 U, u32 p0, u32 p1, u32 lane,
                                                   const uint8_t* slots, SegEntry en = SegEntry{false, 0u}) {
    const u32x4 rsi = make_rsrc(src, (U + 15u) & ~15u);
    u32 prev_top = seg_prev_top(src, p0, en);
    u32 rs = p0, fb = kNone, lb = kNone, rest = 0;
    u32 restl = 0u, lbl = 0u;   // the lane's token bytes and its last boundary + 1 (0: none), summed once per segment
    const EncK kc = enc_k();
    walk_seg(rsi, p0, ntiles_for(p1 - p0), lane, slots, [&](u32 t, const uint8_t* cs, const Refill& nx) {
        const u32x4 cur = *reinterpret_cast<const u32x4*>(cs + 16u * lane);
        nx();
        const u32 pos = p0 + t * kTileStep;
        // (tried only when the run entering the tile is already 16 bytes long, a scalar test
        // that keeps the check off random and short-run tiles)
        if (pos != 0u && pos - rs >= 16u && pos + kTileStep < p1) {
            // a tile inside a run (every byte, and the first lookahead byte, equal to the byte
            // before the tile; never the buffer's first tile, whose position 0 is a boundary
            // whatever its byte): no boundary, so fb, lb and rs stay; the tokens count only past
            // the segment's first boundary, all 3-byte (the run goes on), one every 9 bytes
            // from the run start rs.  About 10 VALU against enc_analyze's ~75.
            const u32 v = uniform(readlane(cur.x, 0)) & 0xFFu;
            if ((prev_top >> 24) == v) {
                const u32 vrep = v * 0x01010101u;
                const bool diff = lane < kOwnLanes
                                      ? ((cur.x ^ vrep) | (cur.y ^ vrep) | (cur.z ^ vrep) | (cur.w ^ vrep)) != 0u
                                      : ((cur.x ^ vrep) & 0xFFu) != 0u;
                if (!__builtin_amdgcn_ballot_w64(diff)) {
                    if (fb != kNone) {
                        const u32 f = pos + (9u - (pos - rs) % 9u) % 9u;   // first token start
                        if (f < pos + kTileStep) rest += 3u * ((pos + kTileStep - 1u - f) / 9u + 1u);
                    }
                    return 0u;
                }
            }
        }
        const EncAn an = enc_analyze<false>(cur, uint2{0u, 0u}, pos, U, p1, lane, prev_top, rs, kc);
        // run boundaries inside the segment: the first one (L0) and the last one (lb)
        const u32 Bo = an.B & an.validm;
        // the first boundary on the scalar unit until found; the last one per lane (tiles come in
        // order, so a lane's latest is its last), the lanes' maximum taken once per segment (round 5:
        // the per-tile wave reductions it replaced measured within +-2 %)
        if (fb == kNone) {
            const uint64_t bl = __builtin_amdgcn_ballot_w64(Bo != 0u);
            if (bl) fb = readlane(an.p0 + (u32)__builtin_ctz(Bo | 0x10000u), (u32)__builtin_ctzll(bl));
        }
        lbl = Bo ? an.p0 + 32u - (u32)__builtin_clz(Bo) : lbl;
        // tokens at or after the first boundary do not depend on the entering run phase
        u32 fbm = 0u;
        if (fb != kNone) fbm = fb <= an.p0 ? 0xFFFFu : (fb >= an.p0 + 16u ? 0u : ~lowmask(fb - an.p0) & 0xFFFFu);
        restl += bcnt(an.T & fbm, 0u) + 2u * bcnt(an.P & fbm, 0u);
        prev_top = readlane(an.top, kOwnLanes - 1u);
        const u32 i63 = readlane(an.incl, kOwnLanes - 1u);
        rs = i63 > rs ? i63 : rs;
        return 0u;
    });
    rest += wave_sum(restl);
    const u32 m = readlane(wave_scan_incl(lbl, 0u, OpMax()), kWave - 1u);
    if (m) lb = m - 1u;
    const u32 L0 = fb == kNone ? p1 - p0 : fb - p0;
    const u32 cont = (fb == kNone && p1 < U && src[p1] == src[p1 - 1u]) ? 1u : 0u;
    return make_uint4(L0, lb == kNone ? 0u : lb + 1u, rest, cont);
}

// The carried state of an encode scan over a buffer's segments: max (lb + 1) so far, and the output
// offset.  One window of up to 64 consecutive segments (lane i: segment base + i, summary sm, first
// position p0), entered with c: each lane's entering run start and output offset; c advances past
// the window.
struct EncCarry {
    u32 lb1, off;
};
__device__ __forceinline__ uint2 enc_seg_window(uint4 sm, bool valid, u32 p0, EncCarry& c) {
    const u32 incl = wave_scan_incl(valid ? sm.y : 0u, 0u, OpMax());
    const u32 ex = from_prev_lane(incl, 0u);
    const u32 rsp1 = ex > c.lb1 ? ex : c.lb1;
    const u32 rs = rsp1 ? rsp1 - 1u : 0u;
    const u32 piece = (valid && p0 > 0u) ? enc_piece_count(sm.x, mod9(p0 - 1u - rs), sm.w) : 0u;
    const u32 cnt = valid ? piece + sm.z : 0u;
    const u32 oincl = wave_scan_incl(cnt, 0u, OpAdd());
    const uint2 r = make_uint2(rs, c.off + oincl - cnt);
    const u32 i63 = readlane(incl, 63);
    c.lb1 = i63 > c.lb1 ? i63 : c.lb1;
    c.off += readlane(oincl, 63);
    return r;
}

// One segment's output: the tile walk from its entering run start rs and output offset off.
// obound: the bytes of dst the stores may reach (0: the encode's U + U / 2; the append passes its
// slot, whose output starts behind the stored stream).
__device__ __forceinline__ void enc_seg_write(const uint8_t* src, uint8_t* dst, u32 U, u32 p0, u32 p1, u32 rs,
                                              u32 off, u32 lane, const uint8_t* slots, uint8_t* stage,
                                              const u32* elut, SegEntry en = SegEntry{false, 0u}, u32 obound = 0u) {
    const u32x4 rsi = make_rsrc(src, (U + 15u) & ~15u);
    const u32x4 rso = make_rsrc(dst, obound ? obound : U + U / 2u);
    EncState st{off, off & ~15u, seg_prev_top(src, p0, en), rs, off & 15u, false, {}};
    const EncK kc = enc_k();
    walk_seg(rsi, p0, ntiles_for(p1 - p0), lane, slots, [&](u32 t, const uint8_t* cs, const Refill& nx) {
        // the fast tile paths (round 3; until then only the one-wave kernels took them): past the
        // segment's shared first chunk and before its last tile, as in a one-wave walk
        return enc_tile<false, true>(cs, nx, p0 + t * kTileStep, U, p1, lane, stage, dst, rso, st, kc, elut);
    });
    // the final partial chunk (< 16 bytes, staging chunk 1): byte stores, nothing past this
    // segment's output and nothing before it
    if (lane >= st.head && lane < st.out_pos - st.flushed) dst[st.flushed + lane] = stage[16u + lane];
    wave_lds_sync();
}

// A segment without a run boundary (every byte equals the byte before the segment, v: zero-filled
// data, long runs) encodes to "v v '9'" tokens every 9 bytes from the entering run start rs; only
// the last token's count depends on the input, through the (up to 8) run bytes after the segment.
// Its output is written from that alone, without reading the segment a second time (the summary
// pass has read it): aligned 16-byte chunks of the 3-periodic pattern, and the partial chunks at
// both ends, which the neighbouring segments share, bytewise.  (Round 3.)
#define RLE_SEG_UNIFORM_ATTR __attribute__((noinline))   // out of the write loop's hot code (r3x)
__device__ RLE_SEG_UNIFORM_ATTR void enc_seg_uniform(const uint8_t* src, uint8_t* dst, u32 U, u32 p0, u32 p1, u32 rs,
                                                u32 off, u32 lane) {
    const u32 v = src[p0];
    const bool eq = lane < 8u && p1 + lane < U && src[p1 + lane] == v;
    const u32 ext = (u32)__builtin_ctzll(__builtin_amdgcn_ballot_w64(!eq));   // run bytes past p1, <= 8
    const u32 f = p0 + (9u - (p0 - rs) % 9u) % 9u;   // the segment's first token start
    if (f >= p1) return;                             // none: the previous segment's token covers it
    const u32 ns = (p1 - 1u - f) / 9u + 1u;
    const u32 sl = f + 9u * (ns - 1u);
    const u32 cl = p1 + ext - sl < 9u ? p1 + ext - sl : 9u;   // the last token's count
    const u32 tot = 3u * (ns - 1u) + (cl >= 2u ? 3u : 1u);
    const u32 end = off + tot;
    const u32 ld = (cl >= 2u && cl < 9u) ? tot - 1u : ~0u;   // the output byte holding a count other than 9
    const u32 vv = rep4(v), d9 = 0x39393939u;
    auto byte_at = [&](u32 k) { return k % 3u != 2u ? v : (k == ld ? 0x30u + cl : 0x39u); };
    // aligned interior chunks [a0, a1)
    const u32 a0 = (off + 15u) & ~15u, a1 = end & ~15u;
    for (u32 c0 = a0; c0 < a1; c0 += 16u * kWave) {
        const u32 c = c0 + 16u * lane;
        const u32 k0 = c - off, ph = k0 % 3u;
        u32 o[4];
#pragma unroll
        for (u32 q = 0; q < 4u; ++q) {
            u32 mk[3];
#pragma unroll
            for (u32 p = 0; p < 3u; ++p) {
                u32 m = 0;
                for (u32 b = 0; b < 4u; ++b)
                    if ((p + 4u * q + b) % 3u == 2u) m |= 0xFFu << (8u * b);
                mk[p] = m;
            }
            const u32 dm = ph == 0u ? mk[0] : ph == 1u ? mk[1] : mk[2];
            o[q] = (vv & ~dm) | (d9 & dm);
        }
        const u32 kd = ld - k0;   // the odd count digit, when it falls in this chunk
        if (kd < 16u) {
            const u32 sh = 8u * (kd & 3u), q = kd >> 2;
            const u32 dv = (0x30u + cl) << sh, msk = 0xFFu << sh;
            o[0] = q == 0u ? (o[0] & ~msk) | dv : o[0];
            o[1] = q == 1u ? (o[1] & ~msk) | dv : o[1];
            o[2] = q == 2u ? (o[2] & ~msk) | dv : o[2];
            o[3] = q == 3u ? (o[3] & ~msk) | dv : o[3];
        }
        if (c < a1) *reinterpret_cast<u32x4*>(dst + c) = u32x4{o[0], o[1], o[2], o[3]};
    }
    // the partial chunks at both ends
    const u32 h1 = a0 < end ? a0 : end;
    if (lane < 16u && off + lane < h1) dst[off + lane] = (uint8_t)byte_at(lane);
    const u32 t0 = a1 > a0 ? a1 : a0;
    if (lane < 16u && t0 + lane < end) dst[t0 + lane] = (uint8_t)byte_at(t0 + lane - off);
}

// One buffer as the encode's summary and write passes see it.  The segmented encode and the
// segmented append run the same two passes and differ only in this view, which each kernel makes
// from its own arguments (view(b)): the encode's has vs = 0, no entry and the default bound; the
// append's is a virtual buffer whose first vs positions lie in front of the new bytes and whose
// first segment is entered with the stored stream's final byte.
struct EncView {
    const uint8_t* src;   // position 0 (the append: new bytes - vs, never read below vs)
    uint8_t* dst;         // the write pass only
    u32 U, vs;            // length, and the first position that is cut into segments
    SegEntry en;          // entering the buffer's first segment
    u32 need;             // the bytes of dst the stores may reach (0: U + U / 2)
    bool live;            // the summary pass only: the buffer takes part (else its summaries are 0)
};

template <class View>
__device__ __forceinline__ void enc_seg_summary_pass(const SegCut& k, uint4* summ, const uint8_t* slots_all, View view) {
    const u32 lane = threadIdx.x & (kWave - 1);
    const u32 wid = uniform(threadIdx.x / kWave);
    const uint8_t* slots = slots_all + wid * 2 * kSlot;
    seg_walk<false>(k, wid, SegScanned{}, [&](const Seg& s) {
        const EncView v = view(s.b);
        uint4 res = make_uint4(0u, 0u, 0u, 0u);
        if (v.live) {
            u32 p0, p1;
            seg_range(s.g - s.s0, s.nseg, v.U - v.vs, k.sb, p0, p1);
            res = enc_seg_summarize(v.src, v.U, v.vs + p0, v.vs + p1, lane, slots,
                                    SegEntry{s.g == s.s0 && v.en.given, v.en.prev});
        }
        if (lane == 0) summ[s.g] = res;
    });
}

// (slots_all, stage_all, elut: the kernel's LDS, kSegWaves * 2 * kSlot, kSegWaves * kEncStage bytes
// and kInsWaveWords words, enc_tile_fast's selectors)
template <class View>
__device__ __forceinline__ void enc_seg_write_pass(const SegCut& k, const SegScanned& w, const uint8_t* slots_all,
                                                   uint8_t* stage_all, u32* elut, View view) {
    const u32 lane = threadIdx.x & (kWave - 1);
    const u32 wid = uniform(threadIdx.x / kWave);
    uint8_t* stage = stage_all + wid * kEncStage;
    const uint8_t* slots = slots_all + wid * 2 * kSlot;
    for (u32 i = threadIdx.x; i < kInsWaveWords; i += kSegBlock) elut[i] = kEncInsLut.s[i];
    __syncthreads();
    seg_walk<true>(k, wid, w, [&](const Seg& s) {
        const EncView v = view(s.b);
        u32 p0, p1;
        seg_range(s.g - s.s0, s.nseg, v.U - v.vs, k.sb, p0, p1);
        p0 += v.vs;
        p1 += v.vs;
        // no run boundary in the segment: for an append's first segment too (the new bytes only
        // continue the stored run), but never position 0 of a buffer
        if (p0 > 0u && uniform(s.sm.y) == 0u && uniform(s.sm.x) == p1 - p0) {
            enc_seg_uniform(v.src, v.dst, v.U, p0, p1, uniform(s.pl.x), uniform(s.pl.y), lane);
            return;
        }
        enc_seg_write(v.src, v.dst, v.U, p0, p1, uniform(s.pl.x), uniform(s.pl.y), lane, slots, stage, elut,
                      SegEntry{s.g == s.s0 && v.en.given, v.en.prev}, v.need);
    });
}

}  // namespace rle

// ---------------------------------------------------------------- host side (csrc/rle_segmented.hip)
// What a segmented launch over n buffers holding `total` bytes looks like: CUs (256 on a machine
// without a device), segment length, segment bound, persistent grid, and the 256-byte-aligned
// carve-up of the caller's workspace: the tables, then `extra` bytes of the caller's own.  Every
// pointer is null when the workspace is (sizes only).
namespace rle {
struct SegShape {
    int ncu;
    uint32_t sb, maxseg, grid;
    uint32_t* seg_first;   // null for one buffer too: the kernels take its segments from its length
    uint32_t* seg_buf;     // per-segment buffer index (seg_map_kernel)
    uint4* summ;
    uint2* plan;
    uint32_t* bflag;
    void* extra;
    size_t bytes;
};
// The prologue of every segmented entry point, after n == 0 and the NULL checks of its own pointers:
// the shape of this n and total over the workspace, then everything decidable on the host first
// (RLE_E_INVAL for a NULL or short workspace), then the device query's error (RLE_E_HIP).  The size
// queries call it without a workspace and read sh->bytes.
int seg_prologue(void* d_workspace, size_t workspace_bytes, uint32_t n, uint64_t total, size_t extra, SegShape* sh);
// The plan and map launches over `len` into seg_first and seg_buf of the shape; none for one buffer.
void seg_launch_plan_map(const uint64_t* len, uint32_t n, const SegShape& sh, hipStream_t s);
// The decode's summary launch over the streams `in + off[i]` of `len[i]` bytes into the shape's
// summaries (dec_seg_summary_kernel: per segment and entry phase 0..2 the decoded bytes in .x .y .z,
// the exit phases in .w bits 0..5 and the phases whose parse stops in bits 8..10).  The segmented
// tail scan (csrc/rle_fileops.hip) reads the same words.
void seg_launch_dec_summary(const uint8_t* in, const uint64_t* off, const uint64_t* len, uint32_t n,
                            const SegShape& sh, hipStream_t s);
inline uint32_t seg_buf_grid(uint32_t n) { return (n + kSegWaves - 1u) / kSegWaves; }   // one wave per buffer
}  // namespace rle
