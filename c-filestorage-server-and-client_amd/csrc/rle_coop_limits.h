// rle_coop_limits.h — the largest single buffers the cooperative kernels (rle_coop.hip) take in one
// workgroup: rounds of 16 one-wave tiles (1024 input bytes per encode tile, 1008 stream bytes per
// decode tile) and a decode staging of at most 64 KiB of output (LDS).  The drop-in
// (rle_dropin.cpp) sends zero-copy calls within them to the sized launch, where they run as one
// workgroup, instead of the segmented kernels.
//
// And which of the kernels' instantiations ("forms") given sizes select: coop_enc_form /
// coop_dec_form, the one table all four launchers of rle_coop.hip dispatch from (batched and by
// value).  No HIP in this header: tests/native/coop_form_check.cpp builds it with plain g++ and
// tests/test_coop_form.py pins every threshold.
#pragma once
#include <stdint.h>

namespace rle {
constexpr uint32_t kCoopMaxWaves = 16;
constexpr uint32_t kCoopEncRounds = 4, kCoopDecRounds = 5;
constexpr uint64_t kCoopEncMaxBytes = 1024ull * kCoopMaxWaves * kCoopEncRounds;   // 64 KiB
constexpr uint64_t kCoopDecMaxIn = 1008ull * kCoopMaxWaves * kCoopDecRounds;      // 80640
constexpr uint64_t kCoopDecUmax = 65536;
constexpr uint32_t kCoopEncTile = 1024, kCoopDecTile = 1008;   // rle_device.h kEncStep / kTileStep

// A form: R rounds of W waves (decode: a staging of Umax output bytes).  W == 0: the sizes do not
// qualify (a single tile or less, or past the limits above) and nothing cooperative is launched.
struct CoopEncForm {
    uint32_t W, R;
};
struct CoopDecForm {
    uint32_t W, Umax, R;
};

// Encode: the largest input length of the batch (or the one buffer's length).
constexpr CoopEncForm coop_enc_form(uint64_t max_len) {
    if (max_len > kCoopEncMaxBytes || max_len <= kCoopEncTile) return {0, 0};
    const uint32_t tiles = (uint32_t)((max_len + kCoopEncTile - 1) / kCoopEncTile);
    if (tiles <= 2) return {2, 1};
    if (tiles <= 3) return {3, 1};
    if (tiles <= 4) return {4, 1};
    if (tiles <= 6) return {6, 1};
    if (tiles <= 8) return {8, 1};
    if (tiles <= 12) return {12, 1};
    if (tiles <= 16) return {16, 1};
    if (tiles <= 32) return {16, 2};
    return {16, 4};
}

// Decode: the largest stream length and the largest decoded length of the batch (or the one
// buffer's C and U).
constexpr CoopDecForm coop_dec_form(uint64_t max_in_len, uint64_t max_out_len) {
    if (max_in_len > kCoopDecMaxIn || max_in_len <= kCoopDecTile || max_out_len > kCoopDecUmax) return {0, 0, 0};
    const uint32_t tiles = (uint32_t)((max_in_len + kCoopDecTile - 1) / kCoopDecTile);
    if (max_out_len > 32768u) return {16, 65536, 5};   // 32-64 KiB: rounds of 16 tiles
    if (max_out_len > 16384u) {
        if (tiles <= 4) return {4, 32768, 1};
        if (tiles <= 8) return {8, 32768, 1};
        if (tiles <= 16) return {16, 32768, 1};
        if (tiles <= 48) return {16, 32768, 3};
        return {16, 32768, 4};   // (a worst-case 32 KiB stream: up to 49 tiles)
    }
    if (tiles > 16) return {16, 16384, 2};   // (random 16 KiB: 17 tiles)
    if (max_out_len <= 4096u) {
        if (tiles <= 2) return {2, 4096, 1};
        if (tiles <= 3) return {3, 4096, 1};
        if (tiles <= 5) return {5, 4096, 1};
        return {8, 4096, 1};
    }
    if (tiles <= 2) return {2, 16384, 1};
    if (tiles <= 3) return {3, 16384, 1};
    if (tiles <= 5) return {5, 16384, 1};
    if (tiles <= 8) return {8, 16384, 1};
    if (tiles <= 12) return {12, 16384, 1};
    return {16, 16384, 1};
}
}  // namespace rle
