/*
 * rle_mi355x.h — batched, device-resident entry points of the MI355X RLE block codec.
 *
 * These are the batch forms of the reference codec (src/rleCompression.c:9-62, declared at
 * include/rleCompression.h:4-5 of samul-1/C-FileStorage-Server-and-Client): the same token
 * grammar, byte-identical output, applied to B independent buffers in one launch.  The
 * reference has no batch API; its natural batch is readNFilesHandler's decode loop
 * (src/filesystemApi.c:680-687), and the eviction decode loop (src/server.c:314-323).
 *
 * All pointers named d_* are device (HBM) pointers; `stream` is a hipStream_t passed as
 * void* (NULL = the default stream).  Calls are asynchronous on that stream.  Return value:
 * RLE_OK, or a negative RLE_E_* host-side error (nothing was launched).
 *
 * Layout rules:
 *  - buffer i occupies d_in + d_in_off[i] .. + d_in_len[i]; d_in + d_in_off[i] and
 *    d_out + d_out_off[i] must be 16-byte aligned (else d_status[i] = RLE_STATUS_MISALIGNED
 *    and that buffer is skipped);
 *  - encode: the output slot of buffer i must hold rle_max_compressed_size(d_in_len[i])
 *    bytes; exactly d_out_len[i] = C bytes are written;
 *  - decode: d_in_len[i] = C (compressed), d_out_len[i] = U (decoded size, as the reference's
 *    uncompressedSize).  d_out_cap[i] (NULL: = U) is the writable slot size, U <= cap (a slot
 *    with cap < U is refused like a misaligned one: d_status[i] = RLE_STATUS_MISALIGNED, nothing
 *    written); the first U bytes are always written.  Bytes of a slot past U are written only for streams
 *    the encoder never emits and only where the reference would write them (its
 *    extraAllocation region).
 *
 * Graph capture (tests/test_gpu_graph_replay.py): the batch entry points -- rle_encode_batch_device,
 * rle_decode_batch_device, their *_sized and *_sized_flags forms, the *_seg forms,
 * rle_tail_batch_device_seg (tests/test_gpu_tail_seg_replay.py),
 * rle_append_batch_device, rle_append_batch_device_seg, rle_append_size_batch_device,
 * rle_append_size_batch_device_seg, rle_append_fit_batch_device, rle_append_fit_batch_device_seg
 * (tests/test_gpu_append_fit_replay.py), rle_decode_packed_batch_device, rle_readn_layout_device,
 * rle_readn_batch_device (tests/test_gpu_readn_pack_replay.py; n and out_cap are frozen, lengths, gaps,
 * offsets and data are read again and d_place, d_total and the status words written again by each
 * replay), rle_decode_packed_batch_device_seg, rle_readn_batch_device_seg
 * (tests/test_gpu_readn_pack_seg_replay.py; the same, with the segment length and table sizes frozen
 * from total_in_bytes), rle_readn_headers_device, rle_readn_reply_device, rle_readn_reply_device_seg
 * (tests/test_gpu_readn_reply_replay.py; n, form and out_cap are frozen, names and lengths are read
 * again), rle_relocate_layout_device, rle_relocate_batch_device (tests/test_gpu_relocate_replay.py; n,
 * dst_base, dst_cap and with them the span and the grid are frozen, lengths, wants, masks, offsets and
 * data are read again and d_new_off, d_new_cap, d_total and the status words written again by each
 * replay), rle_evict_select_device, rle_evict_gather_device (tests/test_gpu_evict_replay.py; n, the
 * limits, flags, order, cap, ntables and the table pointers are frozen, keys, sizes, masks and the
 * summary are read again and d_keep, d_victims, d_summary and the gathered rows written again by each
 * replay) and rle_append_prepare_device -- may be called on a stream that is being captured, in the default
 * (global) capture mode, and the graph replayed any number of times.  The host freezes at capture
 * what it decides itself: the kernel form (from n, the max_* hints and the cooperative mode), the
 * grid, the segment length and table sizes (from the total_* hint), every pointer including the
 * workspace, and rle_append_prepare_device's U.  Everything else is read from device memory on each
 * replay: offsets, lengths, capacities, tail words and the data may all be rewritten between replays,
 * within the hints given at capture; every status word, length and table is written again by each
 * replay.  The caller keeps every buffer it passed, the workspace included, alive and out of other
 * launches' hands while the graph exists.  A decode of more than 4096 buffers does not use the
 * stream's cached issue-order array under capture: the graph holds its own allocation and release of
 * the array (stream-ordered memory nodes) around the sort and decode kernels.
 */
#ifndef RLE_MI355X_H
#define RLE_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* host-side return codes */
#define RLE_OK          0
#define RLE_E_INVAL    (-1)   /* bad argument */
#define RLE_E_HIP      (-2)   /* a HIP runtime call failed */
#define RLE_E_NODEV    (-3)   /* no usable gfx950 device */

/* Largest buffer (input or decoded) one kernel handles: in-buffer offsets are 32-bit. */
#define RLE_MAX_BUFFER_BYTES 0x7FFFFFF0u

/* per-buffer status bits (d_status[i]) */
#define RLE_STATUS_OK          0u
#define RLE_STATUS_OVERFLOW    1u      /* decode: stream writes past cap (reference: heap overflow); truncated */
#define RLE_STATUS_MISALIGNED  2u      /* input or output slot not 16-byte aligned; buffer skipped */
#define RLE_STATUS_TOOLARGE    4u      /* buffer larger than RLE_MAX_BUFFER_BYTES (2 GiB); buffer skipped */
#define RLE_STATUS_SERIAL      0x100u  /* info: stream decoded by the exact serial path (not encoder output) */
#define RLE_STATUS_SHORT       0x400u  /* info: the stream decodes to fewer than U bytes, the rest is zero
                                          (not encoder output) */
#define RLE_STATUS_INTERNAL    0x800u  /* the segmented kernels' carry wait ran out (never expected): output
                                          not trusted */
#define RLE_STATUS_NOTCANON    0x1000u /* tail scan / append: the stream, or the tail word given for it, is not
                                          what the encoder emits; nothing written */
#define RLE_STATUS_NOFIT       0x2000u /* fit append: the slot is smaller than the stream the append would
                                          leave; nothing written, d_need[i] says how much it takes.
                                          rle_readn_batch_device: the reply is longer than out_cap; nothing
                                          written, *d_total says how much it takes */

/* Worst-case compressed size of U bytes (every run of length 2: 3 bytes per 2 input bytes). */
size_t rle_max_compressed_size(size_t U);

/* Batched encode (RLEcompress, src/rleCompression.c:9-45) of n buffers.
 * d_status may be NULL. */
int rle_encode_batch_device(const void* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                            void* d_out, const uint64_t* d_out_off, uint64_t* d_out_len,
                            uint32_t* d_status, uint32_t n, void* stream);

/* Batched decode (RLEdecompress, src/rleCompression.c:47-62) of n buffers.
 * d_out_cap and d_status may be NULL.  Batches of more than 4096 buffers are issued longest first:
 * a small sort launch writes an issue-order array that the library keeps per (device, stream) and
 * reuses (the first call on a stream allocates it, stream-ordered); calls from several host threads
 * on one stream are serialised while they enqueue. */
int rle_decode_batch_device(const void* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                            void* d_out, const uint64_t* d_out_off, const uint64_t* d_out_len,
                            const uint64_t* d_out_cap, uint32_t* d_status, uint32_t n, void* stream);

/* The same two launches with the batch's largest sizes known on the host (max_in_len >= every
 * d_in_len[i]; decode: max_out_len >= every d_out_len[i]).  Few small buffers (encode:
 * 1 KiB < max_in_len <= 64 KiB; decode: 1008 < max_in_len <= 80640 and max_out_len <= 64 KiB; and
 * no more workgroups than the chip holds at once, from the occupancy API) then run the cooperative
 * kernels, one workgroup per buffer and one wave per tile, so a buffer's tiles run side by side
 * instead of one after another (a single file, a small readN).  Other batches (or
 * RLE_MI355X_COOP=0) take the kernels above.  Output and status are the same bytes. */
int rle_encode_batch_device_sized(const void* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                  void* d_out, const uint64_t* d_out_off, uint64_t* d_out_len,
                                  uint32_t* d_status, uint32_t n, uint64_t max_in_len, void* stream);
int rle_decode_batch_device_sized(const void* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                  void* d_out, const uint64_t* d_out_off, const uint64_t* d_out_len,
                                  const uint64_t* d_out_cap, uint32_t* d_status, uint32_t n,
                                  uint64_t max_in_len, uint64_t max_out_len, void* stream);

/* The sized launches with launch flags.  RLE_LAUNCH_STATUS_FLAG (needs d_status): each buffer's
 * status word is stored last, behind a system-scope release of every output byte and d_out_len
 * word of that buffer, so a host that placed d_out / d_status in mapped pinned memory
 * (hipHostMallocMapped) and preset the status words to a value no status takes (e.g. 0xFFFFFFFF)
 * can poll them instead of synchronizing the stream: once a status word changes, the buffer's
 * output is readable from the host.  The drop-in's small zero-copy calls work this way (saves
 * ~4.5 us per call against hipStreamSynchronize, profiles/r4a_sync_probe.txt).  Other flag bits:
 * RLE_E_INVAL. */
#define RLE_LAUNCH_STATUS_FLAG 2u
int rle_encode_batch_device_sized_flags(const void* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                        void* d_out, const uint64_t* d_out_off, uint64_t* d_out_len,
                                        uint32_t* d_status, uint32_t n, uint64_t max_in_len, uint32_t flags,
                                        void* stream);
int rle_decode_batch_device_sized_flags(const void* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                        void* d_out, const uint64_t* d_out_off, const uint64_t* d_out_len,
                                        const uint64_t* d_out_cap, uint32_t* d_status, uint32_t n,
                                        uint64_t max_in_len, uint64_t max_out_len, uint32_t flags, void* stream);

/* Synthetic batch generator: xorshift64 (13,7,17), state seed
 * 0x9E3779B97F4A7C15 + index, one step per byte; kind 0 zero, 1 random, 2 runs50,
 * 3 runs90, 4 pairs.  d_kind / d_index may be NULL (kind 1, index = i). */
int rle_gen_synthetic_device(void* d_out, const uint64_t* d_off, const uint64_t* d_len,
                             const uint32_t* d_kind, const uint64_t* d_index, uint32_t n, void* stream);

/* Host-path accounting of the drop-in RLEcompress/RLEdecompress (process-wide): bytes the callers
 * passed in and got back, bytes moved host->device / device->host, and wall time spent staging
 * into pinned memory, on the device round trip (H2D + kernel + D2H, stream-synchronised) and
 * copying out to the caller's malloc block.  reset != 0 zeroes the counters after reading. */
typedef struct {
    uint64_t calls_compress, calls_decompress;
    uint64_t bytes_in, bytes_out, bytes_h2d, bytes_d2h;
    uint64_t ns_stage_in, ns_device, ns_stage_out;
    uint64_t calls_append;   /* RLEappend (include/rle_fileops.h); RLEdecompressN counts per file */
    uint64_t calls_coalesced, launches_coalesced;   /* always 0: call coalescing is retired, the layout
                                                       stays */
    uint64_t calls_registered;     /* large calls run on the caller's registered memory (RLE_MI355X_REG_MIN) */
    uint64_t calls_reg_fallback;   /* ... and those that took the staging instead (registration refused or
                                      overlapping another call's) */
    uint64_t calls_append_spliced;   /* RLEappend calls that kept the old stream up to its final token and
                                        re-encoded only the final run's remainder and the new bytes; the
                                        other appends re-encoded the whole content */
} rle_dropin_stats_t;
int rle_mi355x_dropin_stats(rle_dropin_stats_t* out, int reset);

/* Runs the cross-lane (DPP) primitive self-test on the current device; 0 = pass. */
int rle_mi355x_selftest(void);

/* Large buffers: the same batched encode / decode with every buffer cut into segments of 4..16
 * tiles of 1008 input bytes (about 16 segments per CU over the batch) processed by separate waves
 * (per-segment summaries, a per-buffer scan of the run / token phase crossing segment boundaries,
 * then per-segment writes: four launches).  Same arguments, results and status codes as
 * rle_encode_batch_device / rle_decode_batch_device, plus:
 *   total_in_bytes  >= the sum of the n input lengths (sizes the segment tables; a buffer whose
 *                   segments do not fit gets RLE_STATUS_TOOLARGE)
 *   d_workspace     caller-owned device memory of at least rle_seg_workspace_bytes(n,
 *                   total_in_bytes) bytes, 256-byte aligned, not used by another launch in flight
 * Decided on the host before anything is launched: n == 0 is RLE_OK; a NULL d_in, d_in_off, d_in_len,
 * d_out, d_out_off, d_out_len or d_workspace, or workspace_bytes below that size, is RLE_E_INVAL.
 * Use it when buffers are large relative to the batch (one big file, a mixed 4 KiB - 1 MiB batch);
 * RLEcompress / RLEdecompress use it from 48 KiB (encode input) / 32 KiB (decode input).
 * Replaces src/rleCompression.c:9-62 like the entries above. */
size_t rle_seg_workspace_bytes(uint32_t n, uint64_t total_in_bytes);
/* Host only, launches nothing: the segment length in bytes (a whole number of 1008-byte tiles) that
 * a segmented launch with this total_in_bytes takes on the current device:
 * clamp(ceil(total_in_bytes / 1008) / (16 * CUs), 4, 16) tiles, 256 CUs assumed when no device is
 * usable.  The same value sizes rle_seg_workspace_bytes.  Tests use it to name the segment edges. */
uint32_t rle_seg_segment_bytes(uint64_t total_in_bytes);
int rle_encode_batch_device_seg(const void* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                void* d_out, const uint64_t* d_out_off, uint64_t* d_out_len,
                                uint32_t* d_status, uint32_t n, uint64_t total_in_bytes,
                                void* d_workspace, size_t workspace_bytes, void* stream);
int rle_decode_batch_device_seg(const void* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                void* d_out, const uint64_t* d_out_off, const uint64_t* d_out_len,
                                const uint64_t* d_out_cap, uint32_t* d_status, uint32_t n,
                                uint64_t total_in_bytes, void* d_workspace, size_t workspace_bytes,
                                void* stream);

/* Fused append, device half (used by RLEappend, include/rle_fileops.h).
 * d_mid holds the decoded old content, U >= 1 bytes, 16-byte aligned.  Finds the final run of
 * d_mid (byte c, length L), r = (L - 1) % 9 + 1 (the size of the reference encoder's last token of
 * that run, src/rleCompression.c:22-39), and writes the 16-byte splice head
 *   d_head[0, 16) = (16 - r) filler bytes ‖ c^r
 * whose filler encodes to itself byte for byte, so encode(head ‖ new) = filler ‖ encode(c^r ‖ new).
 * d_meta (4 u64, device): [0] final run start, [1] r, [2..3] a copy of the head.  Asynchronous on
 * `stream`; RLE_E_INVAL when U == 0. */
int rle_append_prepare_device(const void* d_mid, uint64_t U, void* d_head, uint64_t* d_meta, void* stream);

/* ---- append to stored streams, on the device, without decoding them ---------
 * The write path of the reference appends by decode, append, re-encode (src/filesystemApi.c:766-775).
 * For streams kept compressed in device memory the same result needs only the stream's final token
 * and the new bytes: encode(x ‖ new) = y[0, t) ‖ encode(c^r ‖ new), with y = encode(x), t the
 * offset of y's final token, c = y[t] and r that token's count.
 *
 * The tail word, one uint64_t per stream: bits 0..31 = t, bits 32..35 = r (1 for a one-byte token,
 * 2..9 for "v v digit"), every other bit zero; RLE_TAIL_EMPTY (0) is the empty stream (C = 0). */
#define RLE_TAIL_EMPTY      ((uint64_t)0)
#define RLE_TAIL_OFFSET(w)  ((uint32_t)((uint64_t)(w) & 0xFFFFFFFFu))
#define RLE_TAIL_COUNT(w)   ((uint32_t)(((uint64_t)(w) >> 32) & 0xFu))

/* Host only, launches nothing: the slot capacity an append of A bytes to a C-byte stream may need,
 * C + rle_max_compressed_size(A + 9) rounded up to 16 (t < C and r <= 9, so the new length is at most
 * t + rle_max_compressed_size(r + A)); 0 when that passes RLE_MAX_BUFFER_BYTES. */
size_t rle_append_slot_bytes(uint64_t C, uint64_t A);

/* Tail scan of n streams (stream i: d_in + d_off[i], d_len[i] = C bytes, 16-byte aligned, readable
 * up to C rounded up to 16), one wave per stream: the decoder's forward token parse, reading C
 * bytes and writing only the results.  Bytes at or past C are not part of the stream: a token
 * starting at C - 1 is one byte whatever lies in the padding.
 *     j = 0; U = 0
 *     while j < C:
 *         if j + 1 < C and y[j] == y[j+1]:
 *             if j + 2 >= C or not ('2' <= y[j+2] <= '9'): NOTCANON
 *             t, r = j, y[j+2] - '0'; U += r; j += 3
 *         else:
 *             t, r = j, 1;            U += 1; j += 1
 * RLE_STATUS_OK: d_tail[i] = t | r << 32 and d_ulen[i] = U (64-bit: it may exceed 2 GiB); C = 0 is
 * OK with tail 0 and ulen 0.  RLE_STATUS_NOTCANON, RLE_STATUS_MISALIGNED (the stream's address) and
 * RLE_STATUS_TOOLARGE (C > RLE_MAX_BUFFER_BYTES): tail 0 and ulen 0.  d_ulen and d_status may be
 * NULL.  One wave per stream walks the stream's tiles one after another: for streams that are large
 * next to the batch, rle_tail_batch_device_seg below spreads the same scan over many waves. */
int rle_tail_batch_device(const void* d_in, const uint64_t* d_off, const uint64_t* d_len, uint64_t* d_tail,
                          uint64_t* d_ulen, uint32_t* d_status, uint32_t n, void* stream);

/* The same scan with several waves per stream ("segmented scan"): each stream is cut
 * into the segments of rle_decode_batch_device_seg (rle_seg_segment_bytes(total_in_bytes) bytes each,
 * the last one taking a remainder of 1-2 bytes) and goes through its summary launch; one wave per
 * stream then composes the segments' token phases, sums the decoded length in 64 bits, and walks
 * the stream's last segment, where the final token starts, for the tail word.  The parse, the tail
 * word, d_ulen, the status bits and the results of refused streams (tail 0, ulen 0) are those of
 * rle_tail_batch_device, word for word; d_ulen and d_status may be NULL.  Plus:
 *   total_in_bytes  >= the sum of the n stream lengths (sizes the segment tables; a stream whose
 *                   segments do not fit gets RLE_STATUS_TOOLARGE, tail 0, ulen 0)
 *   d_workspace     caller-owned device memory of at least rle_tail_seg_workspace_bytes(n,
 *                   total_in_bytes) = rle_seg_workspace_bytes(n, total_in_bytes) bytes (the decode's
 *                   tables; the scan keeps no record of its own), 256-byte aligned, not used by
 *                   another launch in flight
 * Decided on the host before anything is launched: n == 0 is RLE_OK; a NULL d_in, d_off, d_len,
 * d_tail or d_workspace, or workspace_bytes below that size, is RLE_E_INVAL.
 * rle_tail_batch_device never routes here: the caller picks the form.
 * Measured on one MI355X (profiles/tail_seg.json), one-wave against segmented: one
 * 1 MiB stream 531-533 us against 13-19 us, 64 of them 568-573 us against 38-47 us, one 64 KiB stream
 * 36-37 us against 12-14 us; 4096 streams of 4 KiB 10-12 us against 29-33 us and 4096 streams of 64 KiB
 * 81-87 us against 89-107 us, where the one-wave form wins.  The crossover follows the number of
 * streams, not their size: use this form for a few dozen streams or fewer of tens of KiB and more;
 * a batch of a thousand streams fills the chip with one wave each. */
size_t rle_tail_seg_workspace_bytes(uint32_t n, uint64_t total_in_bytes);
int rle_tail_batch_device_seg(const void* d_in, const uint64_t* d_off, const uint64_t* d_len, uint64_t* d_tail,
                              uint64_t* d_ulen, uint32_t* d_status, uint32_t n, uint64_t total_in_bytes,
                              void* d_workspace, size_t workspace_bytes, void* stream);

/* Append in place, one wave per file: file i's stream is d_streams + d_off[i], d_len[i] = C bytes in
 * a slot of d_cap[i] bytes; its new content is d_new + d_new_off[i], d_new_len[i] = A bytes (readable
 * up to A rounded up to 16; bytes past A are ignored); d_tail[i] = the stream's tail word (from
 * rle_tail_batch_device, or carried from the previous append).  d_ulen and d_status may be NULL.
 * Accepted when the tail word is RLE_TAIL_EMPTY with C = 0, or describes the stream's last bytes
 * (r = 1: t + 1 = C; else t + 3 = C, y[t] = y[t+1] and y[t+2] = '0' + r).  Then the slot becomes
 * y[0, t) ‖ encode(c^r ‖ new) (an empty stream: encode(new)): no byte below t and no byte at or past
 * the new length C' changes; d_len[i] = C', d_ulen[i] += A, d_tail[i] = the new stream's tail word.
 * A = 0 is OK and changes nothing.
 * Refused, with the slot, d_len, d_ulen and d_tail untouched:
 *   RLE_STATUS_NOTCANON    the tail word does not describe the stream
 *   RLE_STATUS_MISALIGNED  the stream or the new content is not 16-byte aligned, or
 *                          d_cap[i] < rle_append_slot_bytes(C, A) (as the decode treats cap < U)
 *   RLE_STATUS_TOOLARGE    rle_append_slot_bytes(C, A) == 0
 * Parity (as include/rle_fileops.h states for RLEappend): for encoder output the result is byte-
 * identical to the reference composition RLEcompress(RLEdecompress(y) ‖ new).  A hand-made stream that
 * passes the scan keeps its non-canonical prefix: "aa2aa2" + "a" gives "aa2" ‖ encode("aaa") =
 * "aa2aa3", where the reference composition re-encodes all of it to "aa5". */
int rle_append_batch_device(void* d_streams, const uint64_t* d_off, uint64_t* d_len, const uint64_t* d_cap,
                            uint64_t* d_ulen, uint64_t* d_tail, const void* d_new, const uint64_t* d_new_off,
                            const uint64_t* d_new_len, uint32_t* d_status, uint32_t n, void* stream);

/* The same append with several waves per file ("segmented form"): each file's new
 * bytes are cut into the segments of rle_encode_batch_device_seg (rle_seg_segment_bytes(
 * total_new_bytes) bytes each, counted over d_new_len) and go through its summary, scan and write
 * launches, the first segment entered with the state the append carries (c, r, the offset behind
 * the final token), every later one as an encode segment.  Arguments, accepted and refused cases,
 * status bits and results are those of rle_append_batch_device, byte for byte, plus:
 *   total_new_bytes  >= the sum of the n new lengths (sizes the segment tables; a file whose
 *                    segments do not fit gets RLE_STATUS_TOOLARGE and is left untouched)
 *   d_workspace      caller-owned device memory of at least rle_append_seg_workspace_bytes(n,
 *                    total_new_bytes) bytes (the encode's tables and one 16-byte entry record per
 *                    file), 256-byte aligned, not used by another launch in flight
 * Decided on the host before anything is launched: n == 0 is RLE_OK; a NULL d_streams, d_off, d_len,
 * d_cap, d_tail, d_new, d_new_off, d_new_len or d_workspace, or workspace_bytes below that size, is
 * RLE_E_INVAL.
 * rle_append_batch_device never routes here: the caller picks the form.  Use this one when the new
 * content is large next to the batch: one big write, or a batch with files of tens of KiB and more.
 * Measured on one MI355X (profiles/append_seg.json), one-wave against segmented: one
 * 1 MiB append 838-1579 us against 22-23 us, 64 of them 876-1628 us against 72-97 us, one 64 KiB append
 * 57-103 us against 20 us; 4096 appends of 4 KiB 17-23 us against 45-50 us, where the one-wave form
 * wins.  The crossover lies between a few KiB and tens of KiB of new content per file.
 * RLEappend (include/rle_fileops.h) does not use this one. */
size_t rle_append_seg_workspace_bytes(uint32_t n, uint64_t total_new_bytes);
int rle_append_batch_device_seg(void* d_streams, const uint64_t* d_off, uint64_t* d_len, const uint64_t* d_cap,
                                uint64_t* d_ulen, uint64_t* d_tail, const void* d_new, const uint64_t* d_new_off,
                                const uint64_t* d_new_len, uint32_t* d_status, uint32_t n,
                                uint64_t total_new_bytes, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- sizing an append before it is written ("Sizing an append before it is written")
 * The reference looks at the new compressed size before it stores anything: a result larger than the
 * store is refused and the file stays as it was, and other files are evicted until the new size fits
 * (src/filesystemApi.c:777-798); only then is the content swapped (:811-814).  The appends above
 * write in place and need a slot for the worst case.  These four give the exact new length first and
 * append into a slot that merely fits.
 *
 * Contract, the same in all four.  Arguments are those of rle_append_batch_device (the size entries
 * have no d_cap and no d_ulen, and write to nothing but d_need and d_status); d_need is required,
 * d_status and d_ulen may be NULL.  Per file, in this order:
 *   RLE_STATUS_TOOLARGE    rle_append_slot_bytes(C, A) == 0: the worst case must fit 32-bit offsets
 *   RLE_STATUS_MISALIGNED  the stream or the new content is not 16-byte aligned (addresses only)
 *   RLE_STATUS_NOTCANON    the tail word does not describe the stream's last bytes
 *   A == 0                 RLE_STATUS_OK, nothing changes, d_need[i] = C; d_cap[i] is not consulted
 *   otherwise              C' = the exact length of y[0, t) ‖ encode(c^r ‖ new), d_need[i] = C'.
 *                          Size entries: RLE_STATUS_OK.  Fit entries: RLE_STATUS_OK when d_cap[i] >= C'
 *                          (exact, not rounded), and then everything rle_append_batch_device writes
 *                          is written, byte for byte and word for word; else RLE_STATUS_NOFIT.
 * After every refusal, NOFIT included, the slot (the final token's three bytes too), d_len, d_ulen and
 * d_tail are untouched; d_need[i] = 0 after TOOLARGE, MISALIGNED and NOTCANON, and C' after NOFIT.
 * No byte at or past C' changes: a file that fits exactly may have another file's bytes right behind
 * C'.  The store descriptor is bounded by min(d_cap[i], rle_append_slot_bytes(C, A)).
 *
 * One-wave forms: one wave per file.  The size entry walks the new bytes once (the encode's analysis:
 * no staging, no stores).  The fit entry does the same and then, when the file fits, the append's
 * write walk; a file with d_cap[i] >= rle_append_slot_bytes(C, A) cannot overflow, skips the size walk
 * and costs what rle_append_batch_device costs.  Segmented forms: the launches of
 * rle_append_batch_device_seg (plan, map, entry, summary, scan, write; the size form has no write
 * launch), its workspace (rle_append_seg_workspace_bytes(n, total_new_bytes)) and its host-side
 * returns: n == 0 is RLE_OK; a NULL required pointer (d_need among them) or workspace, or
 * workspace_bytes below that size, is RLE_E_INVAL; a file past the tables gets RLE_STATUS_TOOLARGE
 * (d_need[i] = 0).  No entry routes to another form: the caller picks, as above.
 * Size and then fit when the slot may have to move or the store's limit decides (refuse, evict or
 * relocate between the two calls); fit alone when a slot that is too small is the rare case, and
 * d_need of the NOFIT files says what to relocate them to.
 * Measured on one MI355X against the plain append in the same process (profiles/append_fit.json,
 * DESIGN.md §4b): 4096 appends of 4 KiB, size 12 us against 17-22 us, fit into exact slots 21-26 us,
 * fit into worst-case slots 17-22 us; 64 appends of 1 MiB (segmented), size 37 us against 69-92 us,
 * fit in either kind of slot within the rounds' spread of the plain append. */
int rle_append_size_batch_device(const void* d_streams, const uint64_t* d_off, const uint64_t* d_len,
                                 const uint64_t* d_tail, const void* d_new, const uint64_t* d_new_off,
                                 const uint64_t* d_new_len, uint64_t* d_need, uint32_t* d_status, uint32_t n,
                                 void* stream);
int rle_append_size_batch_device_seg(const void* d_streams, const uint64_t* d_off, const uint64_t* d_len,
                                     const uint64_t* d_tail, const void* d_new, const uint64_t* d_new_off,
                                     const uint64_t* d_new_len, uint64_t* d_need, uint32_t* d_status, uint32_t n,
                                     uint64_t total_new_bytes, void* d_workspace, size_t workspace_bytes,
                                     void* stream);
int rle_append_fit_batch_device(void* d_streams, const uint64_t* d_off, uint64_t* d_len, const uint64_t* d_cap,
                                uint64_t* d_ulen, uint64_t* d_tail, const void* d_new, const uint64_t* d_new_off,
                                const uint64_t* d_new_len, uint64_t* d_need, uint32_t* d_status, uint32_t n,
                                void* stream);
int rle_append_fit_batch_device_seg(void* d_streams, const uint64_t* d_off, uint64_t* d_len, const uint64_t* d_cap,
                                    uint64_t* d_ulen, uint64_t* d_tail, const void* d_new,
                                    const uint64_t* d_new_off, const uint64_t* d_new_len, uint64_t* d_need,
                                    uint32_t* d_status, uint32_t n, uint64_t total_new_bytes, void* d_workspace,
                                    size_t workspace_bytes, void* stream);

/* ---- reading stored streams into a packed reply -----------------------------------
 * The reference's batched readers build one reply buffer, file after file: readNFilesHandler
 * (src/filesystemApi.c:663-691) writes "%010ld%s%010ld" (path length, path, content length) and the
 * decoded content directly behind it, then the next header, growing the buffer as it goes (:665-673);
 * the eviction loop (src/server.c:314-323) sends its victims the same way.  Contents start at
 * whatever byte the header ends on, and their lengths live where the tail scan and the appends keep
 * them: on the device.  These three decode into such a reply without aligned slots, without a copy of
 * the lengths to the host and without a gather.
 *
 * rle_decode_packed_batch_device: rle_decode_batch_device with d_out_cap = NULL (cap = U, the
 * reference readers' extraAllocation = 0) and no alignment rule on d_out + d_out_off[i].  File i
 * writes exactly the bytes [d_out_off[i], d_out_off[i] + U) of d_out, U = d_out_len[i], and no other
 * byte: files may abut, and the up to 15 bytes in front of a destination and behind its end that
 * share a 16-byte chunk with it are other files' (or the caller's headers) and stay as they are; the
 * first and the last chunk of a file are written with byte stores only.  Input rules, results and
 * status words are the decode's, word for word, with cap = U: the stream's address is 16-byte aligned,
 * bytes at or past C read as zero; for streams the encoder never emits, RLE_STATUS_SERIAL, _OVERFLOW
 * and _SHORT with the reference's bytes in [0, U) and the zero fill of a short stream.
 * Refused, the file's range untouched: RLE_STATUS_MISALIGNED (the stream's address only) and
 * RLE_STATUS_TOOLARGE (C or U past RLE_MAX_BUFFER_BYTES).  d_status may be NULL.
 * Decided on the host before anything is launched: n == 0 is RLE_OK; a NULL d_in, d_in_off, d_in_len,
 * d_out, d_out_off or d_out_len is RLE_E_INVAL.
 * One wave per file, the decode's tile walk entered like a segment of rle_decode_batch_device_seg at
 * the destination's offset in its 16-byte chunk; the store policy is the decode's for the same n.
 * There is no issue-order sort in this form (a batch of more than 4096 files runs in index order)
 * and no cooperative form; the segmented form is rle_decode_packed_batch_device_seg below.
 *
 * rle_readn_layout_device: the reply's layout from the lengths on the device, in 64 bits:
 *   d_place[i] = sum over k < i of (d_gap[k] + d_ulen[k]) + d_gap[i]      (where file i's content goes)
 *   *d_total   = sum over all n of (d_gap[k] + d_ulen[k])                  (the reply's length)
 * d_gap[i] is the header the caller puts in front of file i (the reference reply: 20 + strlen(path));
 * d_gap == NULL means no gaps.  One launch of one workgroup, no workspace, no allocation and no host
 * synchronisation.  On the host: a NULL d_total, or with n > 0 a NULL d_ulen or d_place, is
 * RLE_E_INVAL; n == 0 writes *d_total = 0 and is RLE_OK.
 *
 * rle_readn_batch_device: both, in two launches: the layout into d_place and d_total, then the packed
 * decode of stream i (d_streams + d_off[i], d_len[i] = C bytes) to d_out + d_place[i], d_ulen[i]
 * bytes.  The decode reads *d_total: when *d_total > out_cap (the bytes d_out holds) every file gets
 * RLE_STATUS_NOFIT and no byte of d_out is written; d_place and *d_total are written all the same, so
 * the caller can allocate *d_total bytes and call again (the reference's realloc growth).  Otherwise
 * results and statuses are rle_decode_packed_batch_device's.  The gap bytes are never written: the
 * caller fills its headers before or after the call (rle_readn_reply_device below writes them from
 * device state).  On the host: n == 0 is RLE_OK (and writes
 * *d_total = 0 when d_total is given); a NULL d_streams, d_off, d_len, d_ulen, d_out, d_place or
 * d_total is RLE_E_INVAL; d_gap and d_status may be NULL.
 *
 * Measured on one MI355X (profiles/readn_pack.json), rle_readn_batch_device against
 * what a caller had to do before (d_ulen copied to the host and summed there, rle_decode_batch_device
 * into aligned slots, one device gather into the reply): 64 files of 4 KiB 17-18 us against 43-44 us,
 * 4096 of 4 KiB 22-26 us against 66-69 us, 64 of 64 KiB 63-96 us against 85-116 us, 4096 of 64 KiB
 * 147-167 us against 334-345 us: faster on every shape measured.  Against rle_decode_batch_device
 * alone (aligned slots, offsets known on the host) the packed reply costs 4-8 us more per call at
 * 4 KiB per file and 6-15 us more at 64 KiB (the layout launch, and the byte stores at both ends of
 * every file): a caller that can use aligned slots decodes fastest there. */
int rle_decode_packed_batch_device(const void* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                   void* d_out, const uint64_t* d_out_off, const uint64_t* d_out_len,
                                   uint32_t* d_status, uint32_t n, void* stream);
int rle_readn_layout_device(const uint64_t* d_ulen, const uint64_t* d_gap, uint64_t* d_place,
                            uint64_t* d_total, uint32_t n, void* stream);
int rle_readn_batch_device(const void* d_streams, const uint64_t* d_off, const uint64_t* d_len,
                           const uint64_t* d_ulen, const uint64_t* d_gap, void* d_out, uint64_t out_cap,
                           uint64_t* d_place, uint64_t* d_total, uint32_t* d_status, uint32_t n, void* stream);

/* ---- segmented packed read-N: several waves per stored stream ("Segmented form")
 * rle_decode_packed_batch_device_seg and rle_readn_batch_device_seg are rle_decode_packed_batch_device
 * and rle_readn_batch_device for streams that are large next to the batch: each stream is cut into
 * the segments of rle_decode_batch_device_seg (rle_seg_segment_bytes(total_in_bytes) bytes each) that
 * separate waves decode.  Launches: plan and map (none for n == 1), the decode's summary, a scan with
 * the packed decode's refusals, and a write pass in which every segment enters at the destination's
 * offset in its 16-byte chunk plus its scanned output offset; the read-N form runs the layout launch
 * of rle_readn_layout_device first, and its scan reads *d_total.  Arguments, results and status words
 * are those of the one-wave forms, byte for byte and word for word: file i writes exactly
 * [d_out_off[i], d_out_off[i] + U) and no other byte, files may abut at any destination phase, the
 * stream's address is 16-byte aligned, bytes at or past C read as zero; RLE_STATUS_SERIAL, _OVERFLOW,
 * _SHORT, _MISALIGNED, _TOOLARGE and (read-N) _NOFIT as above, the range untouched after a refusal.
 * Plus:
 *   total_in_bytes   >= the sum of the n stream lengths (sizes the segment tables; a stream whose
 *                    segments do not fit gets RLE_STATUS_TOOLARGE and its range stays untouched)
 *   d_workspace      caller-owned device memory of at least rle_decode_packed_seg_workspace_bytes(n,
 *                    total_in_bytes) = rle_seg_workspace_bytes(n, total_in_bytes) bytes, 256-byte
 *                    aligned, not used by another launch in flight; the form keeps no record of its own
 * Decided on the host before anything is launched: n == 0 is RLE_OK (the read-N form then writes
 * *d_total = 0 when d_total is given); a NULL d_in, d_in_off, d_in_len, d_out, d_out_off or d_out_len
 * (decode), a NULL d_streams, d_off, d_len, d_ulen, d_out, d_place or d_total (read-N), a NULL
 * d_workspace, or workspace_bytes below that size, is RLE_E_INVAL.  d_gap and d_status may be NULL.
 * Graph capture: the rules of the other _seg entries (tests/test_gpu_readn_pack_seg_replay.py): n,
 * out_cap, the segment length, the table sizes and every pointer are frozen at capture; lengths, gaps,
 * offsets and data are read again, and d_place, *d_total and every status word written again, by each
 * replay.
 * No entry routes to another form: the caller picks.  RLEdecompressN does not use these.
 * Use these when the reply holds files of tens of KiB and more and there are at most a few hundred of
 * them.  Measured on one MI355X (profiles/readn_pack_seg.json),
 * rle_readn_batch_device_seg against rle_readn_batch_device: one 1 MiB file 24-30 us against 814-1331
 * us, 64 of them 76-128 us against 869-1382 us, one 64 KiB file 24-29 us against 58-94 us, 64 of them
 * 31-39 us against 64-99 us; 4096 files of 4 KiB 53-64 us against 21-28 us and 4096 of 64 KiB 204-284
 * us against 146-178 us, where the one-wave form wins.  Against rle_decode_batch_device_seg alone
 * (aligned slots, offsets known on the host) the packed reply costs 3-10 us more per call (1.02-1.26
 * times), whatever the file size. */
size_t rle_decode_packed_seg_workspace_bytes(uint32_t n, uint64_t total_in_bytes);
int rle_decode_packed_batch_device_seg(const void* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                       void* d_out, const uint64_t* d_out_off, const uint64_t* d_out_len,
                                       uint32_t* d_status, uint32_t n, uint64_t total_in_bytes,
                                       void* d_workspace, size_t workspace_bytes, void* stream);
int rle_readn_batch_device_seg(const void* d_streams, const uint64_t* d_off, const uint64_t* d_len,
                               const uint64_t* d_ulen, const uint64_t* d_gap, void* d_out, uint64_t out_cap,
                               uint64_t* d_place, uint64_t* d_total, uint32_t* d_status, uint32_t n,
                               uint64_t total_in_bytes, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- the whole read-N reply: headers and terminator from device state ("Headers and
 * terminator")
 * The entries above leave the gaps to the caller, and the second number of each header is the file's
 * decoded length, which lives in d_ulen on the device.  These four write the wire reply itself, so
 * that one call and one copy of *d_total bytes to the host give what the reference hands to writen;
 * nothing is copied to the host or synchronised on the way.  What the caller still does itself: keep
 * the path table on the device (upload it when names change), and the one D2H copy of the reply.
 *
 * The path table: file i's name is the d_path_len[i] bytes at d_paths + d_path_off[i], at any
 * alignment, without a NUL; the bytes are copied as they are.
 *
 * form:
 *   RLE_REPLY_READN  header "%010ld%s%010ld" (path length, path, content length), 20 + d_path_len[i]
 *                    bytes: readNFilesHandler (src/filesystemApi.c:675-679) and the eviction loop's
 *                    SEND_EVICTED_FILE (src/server.c:53-58)
 *   RLE_REPLY_READ   header "%010ld" (content length), 10 bytes: READ_FILE's reply
 *                    (src/server.c:262-264); d_paths, d_path_off and d_path_len are not read and may
 *                    be NULL
 *   RLE_REPLY_END    or-ed to RLE_REPLY_READN only: the reference's NO_MORE_CONTENT, the ten bytes
 *                    "0000000000" (src/server.c:122, :285, :326), follows the last file and is
 *                    counted in *d_total
 * Any other bit, or RLE_REPLY_END with RLE_REPLY_READ, is RLE_E_INVAL.
 * A field holds ten digits: of a value of 10^10 or more (a d_path_len or d_ulen no real reply has)
 * the low ten decimal digits are written, where the reference's snprintf would write more than ten.
 * Keeping d_path_len sane is the caller's duty; a d_ulen past RLE_MAX_BUFFER_BYTES is
 * RLE_STATUS_TOOLARGE in the decode anyway.
 *
 * rle_reply_header_bytes (host only): the header's length, 20 + path_len or 10; 0 for a bad form.
 *
 * rle_readn_headers_device: the header writer alone, for places the caller already has (beside
 * rle_readn_layout_device with d_gap[i] = rle_reply_header_bytes(form, d_path_len[i])).  File i's
 * header goes to exactly [d_place[i] - gap_i, d_place[i]) of d_out and no other byte is touched: the
 * bytes that share a 16-byte chunk with it are other files' and are written with byte stores only.
 * With RLE_REPLY_END the terminator goes to the ten bytes at d_place[n-1] + d_ulen[n-1] (at 0 for
 * n == 0).  One launch, one wave per file.  On the host: n == 0 without RLE_REPLY_END is RLE_OK and
 * launches nothing; a bad form, a NULL d_out, with n > 0 a NULL d_ulen or d_place, and in the READN
 * form with n > 0 a NULL d_paths, d_path_off or d_path_len, is RLE_E_INVAL.
 *
 * rle_readn_reply_device: the reply in three launches: the layout with the gaps derived on the device
 * from d_path_len (and the terminator's ten bytes in *d_total), rle_readn_batch_device's packed
 * decode, and the headers and the terminator.  Content bytes and status words are those of
 * rle_readn_batch_device, word for word.  Headers are written for every file whenever the reply
 * fits: a file whose decode is refused (RLE_STATUS_MISALIGNED, _TOOLARGE) or flagged (_SERIAL,
 * _OVERFLOW, _SHORT) still gets its header, since its name and length are known, and its status word
 * tells the rest.  When *d_total > out_cap every file is RLE_STATUS_NOFIT and no byte of d_out is
 * written, neither header nor terminator; d_place and *d_total are written all the same.
 * n == 0: without RLE_REPLY_END RLE_OK (and *d_total = 0 when d_total is given); with it the reply is
 * the terminator alone, *d_total = 10, under the same rule for out_cap (d_out and d_total required).
 * On the host: a bad form, a NULL d_streams, d_off, d_len, d_ulen, d_out, d_place or d_total, and in
 * the READN form a NULL d_paths, d_path_off or d_path_len, is RLE_E_INVAL before any launch; d_status
 * may be NULL.
 *
 * rle_readn_reply_device_seg: the same over the launches of rle_readn_batch_device_seg, with its
 * total_in_bytes and its workspace (rle_decode_packed_seg_workspace_bytes(n, total_in_bytes); a NULL
 * or short workspace is RLE_E_INVAL; none is needed for n == 0).  Reply, d_place, *d_total and status
 * words equal the one-wave entry's.
 *
 * Graph capture (tests/test_gpu_readn_reply_replay.py): n, form, out_cap and every pointer (and for
 * the _seg form the segment length, the table sizes and the workspace) are frozen; lengths, names,
 * offsets and data are read again by each replay.
 *
 * Measured on one MI355X (profiles/readn_reply.json and _run2.json, two fresh runs),
 * 49-byte headers and the terminator.  Against rle_readn_batch_device(_seg) alone the headers and
 * their launch cost 2.1-6.3 us per call (medians; within the spreads on 22 of 32 rows), whatever the
 * bytes decoded.  Against what a caller had to do before (d_ulen copied to the host with a
 * synchronise, headers formatted there and copied into the gaps, then rle_readn_batch_device): 1 and
 * 64 files of 4 KiB 17-24 us against 46-58 us, 4096 of 4 KiB 24-32 us against 227-241 us, 1 and 64
 * files of 64 KiB 59-101 us against 93-139 us, 4096 of 64 KiB 152-185 us against 353-393 us; _seg: one
 * 1 MiB file 24-30 us against 56-65 us, 64 of them 76-103 us against 110-146 us.  The host-header
 * route won on no shape measured. */
#define RLE_REPLY_READN 0u
#define RLE_REPLY_READ  1u
#define RLE_REPLY_END   0x100u
size_t rle_reply_header_bytes(uint32_t form, uint64_t path_len);
int rle_readn_headers_device(const void* d_paths, const uint64_t* d_path_off, const uint64_t* d_path_len,
                             const uint64_t* d_ulen, void* d_out, const uint64_t* d_place, uint32_t form,
                             uint32_t n, void* stream);
int rle_readn_reply_device(const void* d_streams, const uint64_t* d_off, const uint64_t* d_len,
                           const uint64_t* d_ulen, const void* d_paths, const uint64_t* d_path_off,
                           const uint64_t* d_path_len, void* d_out, uint64_t out_cap, uint64_t* d_place,
                           uint64_t* d_total, uint32_t* d_status, uint32_t form, uint32_t n, void* stream);
int rle_readn_reply_device_seg(const void* d_streams, const uint64_t* d_off, const uint64_t* d_len,
                               const uint64_t* d_ulen, const void* d_paths, const uint64_t* d_path_off,
                               const uint64_t* d_path_len, void* d_out, uint64_t out_cap, uint64_t* d_place,
                               uint64_t* d_total, uint32_t* d_status, uint32_t form, uint32_t n,
                               uint64_t total_in_bytes, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- relocating stored streams: slots from sizes, one copy -------------------------
 * The reference's write path ends by swapping in a freshly allocated block of exactly C' bytes and
 * freeing the victims' (src/filesystemApi.c:811-814).  For streams kept in device arenas the same step
 * is a move: after the size query, the files whose slots are too small go to slots of d_need bytes;
 * after an eviction or a removeFile, the survivors are packed and the victims' slots given up.  These
 * entries lay the new slots out from sizes that live on the device and move the streams there in one
 * copy launch, with no copy of the sizes to the host and no synchronise.
 *
 * Selection and slot size, the same in both entries.  File i is selected when d_sel == NULL or
 * d_sel[i] != 0; an unselected file is an evicted or removed one, or one that stays where it is.
 * want_i = d_want ? d_want[i] : 0.  A selected file takes a slot of
 *   cap_i = round_up_16(max(want_i, d_len[i]))
 * bytes; an unselected file, and a selected one with max(want_i, d_len[i]) > RLE_MAX_BUFFER_BYTES, takes
 * none (cap_i = 0).  The size query's d_need serves as d_want as it is: a file whose append was refused
 * has d_need = 0 and keeps a slot for the stream it has, and A == 0 gives d_need = C.
 *
 * rle_relocate_layout_device: the slots, in 64 bits:
 *   d_new_off[i] = dst_base + sum over k < i of cap_k      (non-decreasing)
 *   d_new_cap[i] = cap_i                                   (0: file i has no new place)
 *   *d_total     = dst_base + sum over all n of cap_k      (the end of the last slot)
 * all three written for every file.  One launch of one workgroup, no workspace, no allocation and no
 * host synchronisation.  Use it alone to ask how large the new arena must be before allocating it, or
 * to pack the survivors of an eviction.  On the host: a NULL d_total, with n > 0 a NULL d_len,
 * d_new_off or d_new_cap, dst_base not a multiple of 16, or n past the library's launch bound (2^30) is
 * RLE_E_INVAL; n == 0 writes *d_total = dst_base and is RLE_OK.
 *
 * rle_relocate_batch_device: two launches, the layout and then one copy launch.  The copy reads
 * *d_total: when *d_total > dst_cap every selected file gets RLE_STATUS_NOFIT and no byte of d_dst is
 * written; d_new_off, d_new_cap and *d_total are written all the same (rle_readn_batch_device's rule).
 * Otherwise, per file, in this order:
 *   unselected                RLE_STATUS_OK, nothing written
 *   RLE_STATUS_TOOLARGE       selected, d_len[i] or want_i past RLE_MAX_BUFFER_BYTES: no slot, nothing
 *                             written
 *   RLE_STATUS_MISALIGNED     d_src + d_off[i] is not 16-byte aligned: the slot stays reserved and
 *                             untouched
 *   RLE_STATUS_OK             the slot is d_dst + d_new_off[i]: [0, C) is the stream (C = d_len[i]),
 *                             [C, round_up_16(C)) is zero, [round_up_16(C), cap_i) is untouched
 * No other byte changes: no byte of d_dst below dst_base, at or past *d_total or in another file's
 * slot, no byte of d_src; d_off, d_len and the caller's d_ulen and d_tail are not written.  The tail
 * word's offset is relative to the stream and carries over as it is: the caller goes on with
 * d_off <- d_new_off and d_cap <- d_new_cap.  The source is read up to round_up_16(C), which the
 * store's slot rule makes readable.  d_want, d_sel and d_status may be NULL.
 * The caller's duties: the destination range [dst_base, *d_total) of d_dst overlaps no selected source
 * stream (two arenas, or one arena with dst_base past its used end; an in-place slide is not offered:
 * it needs an order between workgroups), and d_new_off and d_new_cap do not alias d_off
 * or d_len.
 * On the host: n == 0 is RLE_OK and writes *d_total = dst_base when d_total is given; a NULL d_src,
 * d_off, d_len, d_dst, d_new_off, d_new_cap or d_total, a d_dst that is not 16-byte aligned, dst_base
 * not a multiple of 16, or dst_base > dst_cap is RLE_E_INVAL before any launch.
 *
 * The copy is balanced over destination bytes, not over files: with room = dst_cap - dst_base,
 * workgroup w of ceil(room / span) owns the destination bytes [dst_base + w * span, + span) below
 * *d_total, span = rle_relocate_span_bytes(room) = max(16 KiB, ceil(room / (8 * CUs))) rounded up to
 * 16 KiB (256 CUs assumed when no device is usable), and returns at once when that range is empty.  It
 * finds the file that owns its first byte by a 64-way search over d_new_off and walks forward from
 * there; a slot across a span edge is written by both neighbours, each 16-byte chunk by exactly one.
 * So dst_cap also sizes the grid: pass the room this relocation may take, not the size of the arena.
 * Loads and stores are non-temporal from a room of 256 MiB (rle_copy_device's rule), decided on the
 * host.
 *
 * rle_relocate_span_bytes (host only, launches nothing): that span for a room of room_bytes on the
 * current device.  Tests use it to name the span edges.
 *
 * Measured on one MI355X (profiles/relocate.json and _run2.json, two fresh runs), with
 * slots as tight as the streams and with worst-case append slots (2.5 times the stream: mostly gaps).
 * Against rle_copy_device of the same number of copied bytes in one contiguous range, the ceiling: one
 * stream of 4 KiB, 64 KiB or 1 MiB 12-20 us against 8-13 us, 4096 streams of 4 KiB 20-40 us against
 * 9-17 us, 64 of 1 MiB 29-39 us against 25-29 us, 4096 of 64 KiB 109-139 us against 88-96 us: 1.16-1.44
 * times the plain copy on the two largest shapes and 1.5-2.5 times on the small ones (the layout
 * launch, the search, and at 4 KiB one load in flight per lane and slot); 0.48-0.61 of 8 TB/s on the
 * two largest shapes, where the plain copy reaches 0.60-0.76.  Against what a caller had to do before
 * (d_len and d_want copied to the host with a synchronise, the slots laid out there, the offsets
 * uploaded, one hipMemcpyAsync device-to-device per file): one stream 12-20 us against 43-63 us, 64
 * streams of 4 KiB or 64 KiB 13-25 us against 233-263 us, 64 of 1 MiB 29-39 us against 234-252 us, 4096
 * streams 20-139 us against 12.4-16.1 ms.  The host route won on no shape measured. */
uint64_t rle_relocate_span_bytes(uint64_t room_bytes);
int rle_relocate_layout_device(const uint64_t* d_len, const uint64_t* d_want, const uint32_t* d_sel,
                               uint64_t dst_base, uint64_t* d_new_off, uint64_t* d_new_cap,
                               uint64_t* d_total, uint32_t n, void* stream);
int rle_relocate_batch_device(const void* d_src, const uint64_t* d_off, const uint64_t* d_len,
                              const uint64_t* d_want, const uint32_t* d_sel,
                              void* d_dst, uint64_t dst_base, uint64_t dst_cap,
                              uint64_t* d_new_off, uint64_t* d_new_cap, uint64_t* d_total,
                              uint32_t* d_status, uint32_t n, void* stream);

/* ---- choosing eviction victims: in policy order until it fits -----------------------
 * The reference decides evictions between the size and the swap of a write, in writeToFileHandler:
 *   while (currStorageSize - contentSize + newCompressedSize > maxStorageSize) victim = getVictim(store, fptr)
 * (src/filesystemApi.c:784-798), and in openFileHandler when the file count is at its limit (:477-480).
 * getVictim (:41-64, comparators in src/cacheFns.c:9-21) picks the file with the smallest policy key --
 * the insertion time for FIFO, lastRef for LRU, refCount for LFU -- the earliest in list order among
 * equals, and never the file being written.  The sizes that decide it (d_len, and the d_need of the
 * pending appends) live on the device; these entries take the decision there, so that the write path's
 * "size -> refuse / evict / relocate -> fit" runs without copying a size to the host.
 *
 * rle_evict_select_device.  Definitions:
 *   live      d_live == NULL or d_live[i] != 0
 *   spared    d_spare != NULL and d_spare[i] != 0: the files this batch writes to (getVictim's `spare`)
 *   eligible  live and not spared
 *   size_i    max(d_want ? d_want[i] : 0, d_len[i]); under RLE_EVICT_SLOTS rounded up to 16.  This is the
 *             rule of rle_relocate_layout_device, so the size query's d_need serves as d_want as it is.
 *             A file that is not live counts nothing.
 *   order     the eligible files ascending by (d_key[i], i).  Keys compare as plain unsigned 64-bit
 *             integers (the reference's comparators return a time_t or size_t difference as int; that
 *             truncation is not reproduced).  The index stands for the reference's list order: with all
 *             keys equal the order is FIFO over the list.
 * The victims are the shortest prefix of that order after whose removal both hold:
 *   bytes = the sum of size_i over the live files <= max_bytes, and
 *   max_files == 0, or the number of live files <= max_files.
 * This is the reference's while (... > maxStorageSize): a store that fits exactly evicts nothing.
 * openFileHandler's single victim is max_files = maxFileNum - 1 with max_bytes = UINT64_MAX.
 * Outputs, all written by every call:
 *   d_keep[i]         1 for a live file that stays, 0 for a victim or a file that is not live: usable as
 *                     d_sel of rle_relocate_batch_device as it is
 *   d_victims[0, m)   the victims' indices in eviction order; entries at and past m are not written
 *   d_summary[0..5]   status, m, bytes before, bytes after, live files before, live files after
 * Refusals: the status goes to d_summary[0], m = 0, d_keep[i] = live_i, after = before, and d_victims is
 * left untouched:
 *   RLE_STATUS_TOOLARGE  some live file has max(want, len) > RLE_MAX_BUFFER_BYTES.  (Without one every
 *                        sum stays below 2^62; with one the byte sums are taken modulo 2^64.)
 *   RLE_STATUS_NOFIT     removing every eligible file still leaves the store over a limit: the
 *                        reference's E2BIG, and the case in which its assert(victim) would fire
 * On the host, before any launch: n == 0 is RLE_OK and writes the summary (all zero), so d_summary is
 * required even then; a NULL d_summary, with n > 0 a NULL d_key, d_len, d_keep or d_victims, a flag bit
 * other than RLE_EVICT_SLOTS, or n past the library's launch bound (2^30) is RLE_E_INVAL.  d_want, d_live
 * and d_spare may be NULL.  d_keep must not alias d_live or d_spare.
 * The caller keeps: the keys (when they are updated), LFU's reset of every refCount after an eviction
 * (:800-805), and everything the host does with the victims' names.
 *
 * One launch of one workgroup of 1024 threads, no workspace, no allocation, no host synchronisation; no
 * workgroup waits for anything and every loop is bounded by n.  One pass over the files sums bytes and
 * counts over the live and the eligible files; a store that fits, and a refusal, end there.  Else the
 * threshold key is found by a weighted radix select over the bytes of the key from the first byte the
 * eligible keys do not share (a 256-bin LDS histogram of byte sums and counts per pass, both remaining
 * needs reduced by the bins below the chosen one), an index-order scan over the files with that key
 * finds the last one taken, the victims are compacted in index order and then sorted by (key, index)
 * with a bitonic network: in LDS for m <= 4096, over d_victims in global memory beyond (slow, correct).
 *
 * rle_evict_gather_device: the victims' rows of up to 8 tables of 64-bit words, in one launch with a
 * grid over cap.  tables_in and tables_out are host arrays of ntables (1..8) device pointers, passed to
 * the kernel by value.  With m = d_summary[1] read on the device, for j < min(m, cap) and every table k:
 *   tables_out[k][j] = tables_in[k][v],  v = d_victims[j]          (RLE_EVICT_ORDER_EVICTION)
 *                                        v = d_victims[m - 1 - j]  (RLE_EVICT_ORDER_REPLY)
 * Entries at and past m are not written.  The reply order is the reversed one: the reference builds
 * evictedList by push-front (:792-793) and sends it from its head (src/server.c:314-323), last evicted
 * first.  With d_off, d_len, d_ulen, d_path_off and d_path_len as the tables, the outputs are the
 * arguments of rle_readn_reply_device(..., RLE_REPLY_READN | RLE_REPLY_END, n = m, ...): the reference's
 * eviction reply.  The host must read m and the victim list before it can call the reply with n = m: one
 * small device-to-host copy of d_summary and d_victims.  The host needs the list anyway, to drop the
 * victims' names, log EVICTED and notify waiting clients; the sizes, the keys and the tables never
 * leave the device.  After the eviction a victim's row of the caller's tables is dead: the relocation
 * gives it no slot (d_new_cap[i] = 0), and what a later append reports for it says nothing.
 * The caller's duty for a dead row (a victim, or a file it removed), before the next batched call over the
 * tables and after the gather has taken the victims' rows: d_len[i] = 0, d_ulen[i] = 0, d_tail[i] =
 * RLE_TAIL_EMPTY (one masked multiply by d_keep on the device), and d_new_len[i] = 0 in every later batch.
 * Every entry then reads nothing through the row's stale d_off (a zero length is no access: the scans
 * answer tail 0, ulen 0, RLE_STATUS_OK, the size and fit entries d_need = 0, RLE_STATUS_OK, the relocation
 * gives no slot), d_want, d_off and d_cap may stay whatever they were, and the row revived (d_live[i] = 1,
 * a key) is the empty stream, which an append accepts.  A row left with its old d_len and d_tail is read
 * at d_off[i] + t by the next size or fit call, and d_off[i] is by then the next file's offset or *d_total;
 * with d_len zeroed but d_tail kept the row's first append after a revival is RLE_STATUS_NOTCANON.
 * On the host, checked in this order: a NULL d_victims, d_summary, tables_in or
 * tables_out, ntables of 0 or above 8, an unknown order, or a NULL table pointer is RLE_E_INVAL; then
 * cap == 0 is RLE_OK and launches nothing.
 *
 * Graph capture (tests/test_gpu_evict_replay.py): n, max_bytes, max_files, flags, order, cap, ntables
 * and every pointer (the table pointers among them) are frozen at capture; keys, sizes, masks and the
 * summary are read again, and every output written again, by each replay.
 *
 * Measured on one MI355X (profiles/evict.json and _run2.json, two fresh runs), against
 * what a caller had to do before (keys, sizes and masks copied to the host with a synchronise, a numpy
 * lexsort and cumsum there, the keep mask and five gathered tables uploaded).  The selection alone: a
 * store that fits 17-26 us at 64 files, 16-36 us at 4096, 107-158 us at 65536, against 107-143 us,
 * 149-244 us and 3.1-6.8 ms; 1 % or 10 % evicted 20-47 us, 39-58 us and 316-620 us against 126-395 us,
 * 181-331 us and 3.2-4.3 ms; every eligible file evicted 24-40 us at 64 files and 112-125 us at 4096
 * (3712 victims, the LDS sort) against 127-300 us and 206-689 us.  With the gather 5-14 us more where
 * the selection is short.  The host route won on one shape: all 59392 eligible of 65536 files evicted
 * at once, the sort in global memory, 4.05-4.07 ms against 3.5-8.3 ms (3.59 ms in the quiet run).  A
 * caller that expects to evict tens of thousands of files in one step should take the host route
 * there; below a few thousand victims the device route was faster at every n measured. */
#define RLE_EVICT_SLOTS 1u        /* count round_up_16(size): what rle_relocate_layout_device lays out.
                                     Without it: exact bytes, the reference's currStorageSize */
#define RLE_EVICT_SUMMARY_WORDS 6
#define RLE_EVICT_ORDER_EVICTION 0u
#define RLE_EVICT_ORDER_REPLY    1u   /* reversed: evictedList is built by push-front (:792-793) and sent from
                                         its head (src/server.c:314-323), last evicted first */
int rle_evict_select_device(const uint64_t* d_key, const uint64_t* d_len, const uint64_t* d_want,
                            const uint32_t* d_live, const uint32_t* d_spare,
                            uint64_t max_bytes, uint32_t max_files, uint32_t flags,
                            uint32_t* d_keep, uint32_t* d_victims, uint64_t* d_summary,
                            uint32_t n, void* stream);
int rle_evict_gather_device(const uint32_t* d_victims, const uint64_t* d_summary, uint32_t order,
                            const uint64_t* const* tables_in, uint64_t* const* tables_out,
                            uint32_t ntables, uint32_t cap, void* stream);

/* Diagnostic builds only (RLE_STAMPS=1, never the product library): per-segment decode cycle sums
 * over all waves: [tile wait, scan, scatter, flush reads, flush fill, flush store, flush re-zero,
 * move/drain/finish, waves]; RLE_E_INVAL otherwise. */
int rle_mi355x_stamps(unsigned long long* out9, int reset);

/* Diagnostic builds only (RLE_TIMELINE=1, never the product library): per-buffer wave timelines of
 * the one-wave batch kernels, 16384 x 16 u64 (s_memrealtime at entry, walk start, tiles 0..7, end;
 * HW_ID, XCC_ID); RLE_E_INVAL otherwise. */
int rle_mi355x_timeline(unsigned long long* out, int reset);

/* ---- multi-GPU exchange (csrc/rle_dist.hip) -------------------------------
 * The one exchange of a batch sharded round-robin over N GPUs (shard.py, bench.py --gpus N): each
 * rank's per-buffer compressed sizes all-gathered over RCCL and scanned into offsets in the global
 * stream (global buffer i = k * world + r is rank r's k-th buffer).  No reference interface: the
 * reference server is single-host, single-process (src/server.c); this replaces the Python
 * all_gather + cumsum of shard.global_offsets with one host call.  RCCL is resolved at run time from
 * the process's librccl.so.1 (or rccl_path when non-NULL).
 *   rle_dist_unique_id: a communicator id (128 bytes) on one rank, to be broadcast to all ranks.
 *   rle_dist_init: this rank's communicator (once per process).
 *   rle_dist_gather_offsets: on `stream`, after the work issued on it so far: all-gather
 *     d_sizes[n] into d_gathered[world * n] (rank major), then the exclusive scan in global order
 *     into d_offsets[world * n].
 *   rle_dist_offsets_device: the scan alone, on `stream` (tests).  Two launches over the whole
 *     chip, with the tile sums in the caller's workspace d_ws of ws_bytes >=
 *     rle_dist_workspace_bytes(n) bytes (0 for n <= 512: d_ws may be NULL; 8-byte aligned).  Scans
 *     that may run at once need workspaces of their own; a captured graph keeps the pointer, so the
 *     caller keeps the workspace alive while the graph exists.  RLE_E_INVAL when it is too small.
 *   rle_dist_available: RLE_OK when the RCCL symbols resolve in this process (a preflight that every
 *     rank runs before any rank enters the blocking rle_dist_init).
 *   rle_dist_finalize: destroys the communicator. */
int rle_dist_available(const char* rccl_path);
int rle_dist_unique_id(void* out, size_t len, const char* rccl_path);
int rle_dist_init(const void* id, size_t len, int rank, int world, const char* rccl_path);
size_t rle_dist_workspace_bytes(uint32_t n);
int rle_dist_gather_offsets(const int64_t* d_sizes, uint32_t n, int64_t* d_gathered, int64_t* d_offsets, void* d_ws,
                            size_t ws_bytes, void* stream);
int rle_dist_offsets_device(const int64_t* d_gathered, uint32_t world, uint32_t n, int64_t* d_offsets, void* d_ws,
                            size_t ws_bytes, void* stream);
/* rle_dist_gather_offsets off the codec's stream: after the work issued on codec_stream so far, the
 * gather + scan run on comm_stream into the caller's result buffers of `slot` (0 or 1, alternating
 * per step); codec_stream is made to wait only for the previous call's exchange (the other slot),
 * so the caller may rewrite the other slot's sizes in its next step.  Each slot needs its own workspace
 * (d_ws, as rle_dist_gather_offsets).  Calls must alternate the slots (a repeated slot is
 * RLE_E_INVAL); one communicator and one stream pair per process; not thread-safe. */
int rle_dist_gather_offsets_async(const int64_t* d_sizes, uint32_t n, int64_t* d_gathered, int64_t* d_offsets,
                                  void* d_ws, size_t ws_bytes, void* codec_stream, void* comm_stream, int slot);
int rle_dist_finalize(void);

/* Tests: the cooperative mode of the sized entry points, in-process (0 never, 1 whenever the sizes
 * qualify, -1 residency-gated default; RLE_MI355X_COOP sets the initial mode).  RLE_E_INVAL
 * otherwise. */
int rle_mi355x_set_coop_mode(int mode);

/* Host only, launches nothing: which cooperative kernel form the sized entry points (and the
 * drop-in's single calls) select for these sizes.  decode == 0: max_in_len is the encode's largest
 * input length (max_out_len ignored, *umax = 0); otherwise the decode's largest stream and decoded
 * lengths.  Returns 1 and the form -- *rounds rounds of *waves waves, decode: a staging of *umax
 * output bytes -- or 0 (all three 0) when the sizes do not qualify.  Whether a launch then runs the
 * form still depends on the cooperative mode and the residency admission.  Null pointers are
 * skipped.  Tests use it to assert which form a launch ran. */
int rle_mi355x_coop_form(int decode, uint64_t max_in_len, uint64_t max_out_len, uint32_t* waves,
                         uint32_t* umax, uint32_t* rounds);

/* Tests / A-B: waves per workgroup of the large-batch decode in rounds (0 off, 4, 8 or 16): batches
 * of more than 4096 buffers through the sized entry points whose max_in_len is at least 8 decode
 * tiles (8064 bytes) decode one workgroup per buffer, its waves on consecutive tiles.
 * RLE_MI355X_DEC_ROUND sets the initial value; -1 only reads it.  Returns the previous setting, or
 * RLE_E_INVAL. */
int rle_mi355x_set_dec_round(int waves);

/* Large decodes (more than 4096 buffers) keep their issue-order array per (device, stream handle),
 * up to 16 of them, the least recently used handed over when a new stream needs one; every array
 * is used in turn across the queues a handle may name (hipStreamPerThread, a reused handle).  This
 * frees the array kept for `stream` on the current device, behind the work already issued on it. */
int rle_decode_release_stream(void* stream);

/* Measurement only (not the codec): copies nbytes (a multiple of 16, both pointers 16-byte aligned)
 * from d_src to d_dst on `stream` with a hand-written 16-byte-per-lane streaming kernel; bench.py
 * times it as the practical HBM ceiling of SURVEY.md §8(d).  RLE_E_INVAL on bad sizes. */
int rle_copy_device(void* d_dst, const void* d_src, uint64_t nbytes, void* stream);

/* Measurement only (not the codec): the large-batch decode's memory traffic without its token work:
 * each of the n buffers (decode_batch arguments) read in decode tiles and U bytes written, one wave
 * per buffer, the decode's occupancy and issue order.  bench.py times it beside the north-star decode
 * as the ceiling of that access pattern.  The output bytes are not a decode. */
int rle_decode_pattern_device(const void* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len, void* d_out,
                              const uint64_t* d_out_off, const uint64_t* d_out_len, uint32_t n, void* stream);

/* The drop-in's background start-up (HIP runtime, warm thread contexts) at library load: 1 when this
 * process started it, 0 otherwise.  It starts in a program that links the library (the reference
 * server, INTEGRATION.md §2: the library is among the main program's DT_NEEDED entries) or whenever
 * RLE_MI355X_PREINIT > 0; a process that dlopen()s the library (Python ctypes) does no GPU work
 * before its first codec call unless RLE_MI355X_PREINIT asks for it.  No reference interface. */
int rle_mi355x_preinit_state(void);

/* Number of visible HIP devices (0 when none). */
int rle_mi355x_device_count(void);

const char* rle_mi355x_version(void);

#ifdef __cplusplus
}
#endif
#endif
