// rle_route.h — which path a drop-in call of given sizes takes (rle_dropin.cpp): the size constants,
// the settings the decision reads, and one pure function per entry point.  No HIP here: a plain C++
// compiler builds it, and tests/test_route.py pins the decisions on a machine without a GPU.
// What depends on device or process state is not part of a route and stays with the calls: the
// cooperative kernels' own admission (rle_*_coop_one returning 0), whether a call that wants
// registration gets it (reg_likely, LargeCall::registered), live_pages.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rle_coop_limits.h"

namespace rle {

// Small-call threshold: up to this many input bytes the worst-case output is copied back in the
// same round trip as its size (one stream sync instead of two).
constexpr size_t kOneTripBytes = 128u << 10;
// From these sizes one call is cut into segments processed by separate waves
// (rle_*_batch_device_seg) instead of one wave walking the whole buffer.
constexpr size_t kSegEncodeBytes = 48u << 10;
constexpr size_t kSegDecodeBytes = 32u << 10;

// The thread's mapped pinned buffer of the zero-copy calls: input, launch words, output.  Input up
// to 256 KiB, output up to 384 KiB (r5n / r5o, profiles/r5o_zc_size.md: past the cooperative kernels'
// reach the segmented kernels on the mapped buffer beat the two copies of the staged path up to
// 256 KiB, e.g. a 96 KiB compress 43 against 68 us; 80 KiB of input until round 5's r5n)
#ifndef RLE_ZC_IN_KIB
#define RLE_ZC_IN_KIB 256
#endif
constexpr size_t kZcIn = 0, kZcWords = (size_t)RLE_ZC_IN_KIB << 10, kZcOut = kZcWords + (4u << 10),
                 kZcBytes = kZcOut + (kZcWords * 3 / 2 > (204u << 10) ? kZcWords * 3 / 2 : (204u << 10));
static_assert(kZcWords >= kCoopDecMaxIn, "zero-copy input region");
constexpr size_t kZcMaxIn = kZcWords, kZcMaxOut = kZcBytes - kZcOut;   // one zero-copy call's bytes

// A chunk of an RLEdecompressN batch through the mapped buffer: at most kZcNFiles files, each
// decoding to at most kZcNMaxU bytes.  (Files up to 16 KiB: a 64 KiB file's one-wave decode writing
// over PCIe took 200 µs per chunk of five, r6aa: 64 x 64 KiB zero 2266 µs against 456 staged.)
constexpr size_t kZcNFiles = 56;   // 36 bytes of launch words each, below kZcWords + 2048 (kZcMail)
constexpr size_t kZcNMaxU = 16384;

// What the routes read of the library's settings (init_once fills it from the environment).
struct Settings {
    // Small calls run zero-copy by default: the kernel reads the caller's bytes from, and writes its
    // result into, this thread's mapped pinned buffer over PCIe, with no copy commands at all (4 KiB:
    // 19 / 20 us per compress / decompress call against 21 / 23 with one H2D + one D2H;
    // profiles/r1e_small.md).  RLE_MI355X_SMALL=copy selects the copying form.
    bool zerocopy = true;
    // Zero-copy calls from this many bytes (encode: U, decode: C) run the segmented kernels on the mapped
    // buffer instead of one wave walking it, and the zero-copy form then takes calls up to 256 KiB in
    // (RLE_MI355X_ZC_SEG=<bytes>; 0 = never).  profiles/r4f_callrate_zcseg.txt, µs per call on 1 / 8
    // threads: 40 KB 42.2 / 91.7 against 66.1 / 151.3 for one wave over the mapped buffer; 24 KiB
    // 41.2 / 91.1 against 34.8 / 64.2 (the five launches cost more than a short walk).
    size_t zc_seg = 32u << 10;
    // ... except the calls one cooperative workgroup takes (rle_coop_limits.h: encode up to 64 KiB,
    // decode up to 80 tiles decoding to 64 KiB; rounds of 16 waves, one launch, polled like the smaller
    // calls).  RLE_MI355X_ZC_COOP=0: the segmented kernels from zc_seg as before (round 5 A/B).
    bool zc_coop = true;
    // From reg_min bytes a call wants its buffers registered for its duration (rle_dropin.cpp,
    // LargeCall; RLE_MI355X_REG_MIN; 0 = never; past the zero-copy calls: r6m / r6o).
    size_t reg_min = kZcMaxIn + 1;
    int fake_devs = 0;   // test build: contexts without HIP objects (RLE_MI355X_FAKE_DEVICES); none registers
};

// The body that runs an RLEcompress / RLEdecompress.
enum class Body : uint8_t {
    MappedOne,   // mapped buffer, one launch: the cooperative workgroup, else one wave (polled)
    MappedSeg,   // mapped buffer, the segmented kernels (one stream sync)
    Staged,      // one H2D, one one-wave launch, one D2H (RLE_MI355X_SMALL=copy)
    Large,       // device buffers: the caller's bytes by DMA or the runtime's pageable copies
};
// A buffer in device memory (queue_encode / queue_decode, the registered calls): the segmented
// kernels or one wave, and whether an encode's worst-case output travels with its size.
struct DeviceForm {
    bool seg, one_trip;
};
constexpr DeviceForm encode_form(size_t n) { return {n >= kSegEncodeBytes, n <= kOneTripBytes}; }
constexpr DeviceForm decode_form(size_t C) { return {C >= kSegDecodeBytes, false}; }

struct CallRoute {
    bool reg;         // registration wanted: tried first when reg_likely(), then body
    Body body;
    DeviceForm dev;   // of the registered and the Large bodies
};
// What one cooperative workgroup takes, by size (its occupancy admission is rle_coop.hip's own).
constexpr bool coop_encodes(size_t U, const Settings& s) { return s.zc_coop && U <= kCoopEncMaxBytes; }
constexpr bool coop_decodes(size_t C, size_t U, const Settings& s) {
    return s.zc_coop && C <= kCoopDecMaxIn && U <= kCoopDecUmax;
}
constexpr Body small_body(bool seg, const Settings& s) {
    return !s.zerocopy ? Body::Staged : seg ? Body::MappedSeg : Body::MappedOne;
}

// RLEcompress of U > 0 bytes.  (Registered encodes are segmented; the cooperative kernel's stay zero-copy.)
constexpr CallRoute route_compress(size_t U, const Settings& s) {
    const bool reg = s.reg_min && !s.fake_devs && U >= s.reg_min && U >= kSegEncodeBytes && !coop_encodes(U, s);
    const bool small = U < kSegEncodeBytes || (s.zc_seg && s.zerocopy && U <= kZcMaxIn);
    const bool seg = s.zc_seg && U >= s.zc_seg && !coop_encodes(U, s);
    return {reg, small ? small_body(seg, s) : Body::Large, encode_form(U)};
}

// RLEdecompress of C > 0 stream bytes into U + E.  As it stands a call can both want registration
// and be within the mapped buffer's reach (total >= reg_min while C <= kZcMaxIn and total <=
// kZcMaxOut: ADVICE r6 item 1); it runs registered when it gets the registration, else mapped.
constexpr CallRoute route_decompress(size_t C, size_t U, size_t E, const Settings& s) {
    const size_t total = U + E;
    const bool reg = s.reg_min && !s.fake_devs && (C >= s.reg_min || total >= s.reg_min) && !coop_decodes(C, U, s);
    const bool small = (C < kSegDecodeBytes && total <= kOneTripBytes) ||
                       (s.zc_seg && s.zerocopy && C <= kZcMaxIn && total <= kZcMaxOut);
    const bool seg = s.zc_seg && C >= s.zc_seg && !coop_decodes(C, U, s);
    return {reg, small ? small_body(seg, s) : Body::Large, decode_form(C)};
}

// RLEappend of A bytes to a stream of C bytes decoding to U > 0.
enum class AppendRoute : uint8_t {
    Mapped,        // decode + encode of the whole on the mapped buffer: what the cooperative or one-wave kernels take
    SmallSplice,   // the splice in one H2D and one D2H: one-wave decode, one-wave encode of the tail
    LargeSplice,   // the splice through device buffers (a LargeCall)
};
// max_whole / max_tail: the caller's rle_max_compressed_size(U + A) / (16 + A) (defined by the kernels alone).
constexpr AppendRoute route_append(size_t C, size_t U, size_t A, size_t max_whole, size_t max_tail, const Settings& s) {
    const bool dec = C < kSegDecodeBytes || coop_decodes(C, U, s);
    const bool enc = U + A < kSegEncodeBytes || coop_encodes(U + A, s);
    if (s.zerocopy && C != 0 && dec && enc && C <= kZcWords && U + A <= kZcMaxOut && max_whole <= kZcWords)
        return AppendRoute::Mapped;
    if (C && C < kSegDecodeBytes && 16 + A < kSegEncodeBytes && max_tail <= kOneTripBytes)
        return AppendRoute::SmallSplice;
    return AppendRoute::LargeSplice;
}

// One file (C > 0) of an RLEdecompressN batch that fits the bounded staging.
enum class NFileRoute : uint8_t {
    Mapped,      // in a chunk through the mapped buffer: a one-wave or cooperative decode
    Staged,      // in a staged chunk, the one-wave launch
    StagedSeg,   // in a staged chunk, the segmented launch
};
constexpr NFileRoute route_n_file(size_t C, size_t U, const Settings& s) {
    return s.zerocopy && C < kSegDecodeBytes && U <= kZcNMaxU ? NFileRoute::Mapped
           : C >= kSegDecodeBytes                               ? NFileRoute::StagedSeg
                                                                : NFileRoute::Staged;
}

}  // namespace rle
