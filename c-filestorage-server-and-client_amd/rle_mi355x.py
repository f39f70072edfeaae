"""ctypes binding of librle_mi355x.so — the MI355X RLE block codec.

Mirrors the reference codec interface (samul-1/C-FileStorage-Server-and-Client
include/rleCompression.h:4-5, src/rleCompression.c:9-62): `compress` / `decompress`
call the drop-in RLEcompress / RLEdecompress exactly as src/filesystemApi.c does, and the
`*_batch` functions expose the batched device-resident API of include/rle_mi355x.h on
torch device tensors (PyTorch is only the allocator/stream plumbing here).

The library is required: there is no Python or CPU fallback.  Loading fails loudly when
librle_mi355x.so has not been built (`python -c "import __graft_entry__ as g; g.build()"`).
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "librle_mi355x.so")
# A/B experiments only (tools/ab.sh): load an experimental build instead of the product library
LIB_PATH = os.environ.get("RLE_MI355X_LIB", LIB_PATH)
INCLUDE_DIR = os.path.join(os.path.dirname(HERE), "include")

RLE_OK = 0
RLE_E_INVAL = -1
RLE_STATUS_OK = 0
RLE_STATUS_OVERFLOW = 1
RLE_STATUS_MISALIGNED = 2
RLE_STATUS_TOOLARGE = 4
RLE_STATUS_SERIAL = 0x100
RLE_STATUS_SHORT = 0x400
RLE_STATUS_INTERNAL = 0x800
RLE_STATUS_NOTCANON = 0x1000
RLE_STATUS_NOFIT = 0x2000
RLE_TAIL_EMPTY = 0
RLE_MAX_BUFFER_BYTES = 0x7FFFFFF0
RLE_LAUNCH_STATUS_FLAG = 2
RLE_REPLY_READN = 0
RLE_REPLY_READ = 1
RLE_REPLY_END = 0x100
RLE_EVICT_SLOTS = 1
RLE_EVICT_SUMMARY_WORDS = 6
RLE_EVICT_ORDER_EVICTION = 0
RLE_EVICT_ORDER_REPLY = 1

_u64p = ctypes.c_void_p
_lib = None
_libc = ctypes.CDLL("libc.so.6")
_libc.free.argtypes = [ctypes.c_void_p]


class RLEError(RuntimeError):
    pass


class DropinStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("calls_compress", "calls_decompress", "bytes_in", "bytes_out",
                                               "bytes_h2d", "bytes_d2h", "ns_stage_in", "ns_device",
                                               "ns_stage_out", "calls_append", "calls_coalesced",
                                               "launches_coalesced", "calls_registered", "calls_reg_fallback",
                                               "calls_append_spliced")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def lib():
    """Load (once) and return the codec library."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RLEError(f"{LIB_PATH} is missing: the HIP codec has not been built")
    L = ctypes.CDLL(LIB_PATH, use_errno=True)   # errno of the drop-in calls (ENOMEM, EFBIG, EINVAL)
    vp, u32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
    L.rle_max_compressed_size.restype = sz
    L.rle_max_compressed_size.argtypes = [sz]
    L.rle_encode_batch_device.restype = ctypes.c_int
    L.rle_encode_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, vp]
    L.rle_decode_batch_device.restype = ctypes.c_int
    L.rle_decode_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32, vp]
    u64 = ctypes.c_uint64
    L.rle_encode_batch_device_sized.restype = ctypes.c_int
    L.rle_encode_batch_device_sized.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u64, vp]
    L.rle_decode_batch_device_sized.restype = ctypes.c_int
    L.rle_decode_batch_device_sized.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32, u64, u64, vp]
    L.rle_encode_batch_device_sized_flags.restype = ctypes.c_int
    L.rle_encode_batch_device_sized_flags.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u64, u32, vp]
    L.rle_decode_batch_device_sized_flags.restype = ctypes.c_int
    L.rle_decode_batch_device_sized_flags.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32, u64, u64, u32, vp]
    L.rle_seg_workspace_bytes.restype = sz
    L.rle_seg_workspace_bytes.argtypes = [u32, ctypes.c_uint64]
    L.rle_encode_batch_device_seg.restype = ctypes.c_int
    L.rle_encode_batch_device_seg.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, ctypes.c_uint64, vp, sz, vp]
    L.rle_decode_batch_device_seg.restype = ctypes.c_int
    L.rle_decode_batch_device_seg.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u32, ctypes.c_uint64, vp, sz, vp]
    L.rle_gen_synthetic_device.restype = ctypes.c_int
    L.rle_gen_synthetic_device.argtypes = [vp, vp, vp, vp, vp, u32, vp]
    L.rle_mi355x_selftest.restype = ctypes.c_int
    L.rle_mi355x_selftest.argtypes = []
    L.rle_mi355x_device_count.restype = ctypes.c_int
    L.rle_mi355x_device_count.argtypes = []
    L.rle_mi355x_version.restype = ctypes.c_char_p
    L.rle_mi355x_version.argtypes = []
    L.rle_mi355x_dropin_stats.restype = ctypes.c_int
    L.rle_mi355x_dropin_stats.argtypes = [ctypes.POINTER(DropinStats), ctypes.c_int]
    L.RLEcompress.restype = ctypes.c_void_p
    L.RLEcompress.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(sz)]
    L.RLEdecompress.restype = ctypes.c_void_p
    L.RLEdecompress.argtypes = [ctypes.c_char_p, sz, sz, sz]
    L.RLEappend.restype = ctypes.c_void_p
    L.RLEappend.argtypes = [ctypes.c_char_p, sz, sz, ctypes.c_char_p, sz, ctypes.POINTER(sz)]
    L.RLEdecompressN.restype = ctypes.c_int
    L.RLEdecompressN.argtypes = [sz, vp, vp, vp, vp]
    L.rle_append_prepare_device.restype = ctypes.c_int
    L.rle_append_prepare_device.argtypes = [vp, ctypes.c_uint64, vp, vp, vp]
    L.rle_append_slot_bytes.restype = sz
    L.rle_append_slot_bytes.argtypes = [u64, u64]
    L.rle_tail_batch_device.restype = ctypes.c_int
    L.rle_tail_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, u32, vp]
    L.rle_append_batch_device.restype = ctypes.c_int
    L.rle_append_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp]
    L.rle_append_seg_workspace_bytes.restype = sz
    L.rle_append_seg_workspace_bytes.argtypes = [u32, u64]
    L.rle_append_batch_device_seg.restype = ctypes.c_int
    L.rle_append_batch_device_seg.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u64, vp, sz, vp]
    L.rle_append_size_batch_device.restype = ctypes.c_int
    L.rle_append_size_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp]
    L.rle_append_size_batch_device_seg.restype = ctypes.c_int
    L.rle_append_size_batch_device_seg.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u64, vp, sz, vp]
    L.rle_append_fit_batch_device.restype = ctypes.c_int
    L.rle_append_fit_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp]
    L.rle_append_fit_batch_device_seg.restype = ctypes.c_int
    L.rle_append_fit_batch_device_seg.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u64, vp, sz, vp]
    L.rle_decode_packed_batch_device.restype = ctypes.c_int
    L.rle_decode_packed_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, vp]
    L.rle_readn_layout_device.restype = ctypes.c_int
    L.rle_readn_layout_device.argtypes = [vp, vp, vp, vp, u32, vp]
    L.rle_readn_batch_device.restype = ctypes.c_int
    L.rle_readn_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, u32, vp]
    L.rle_decode_packed_seg_workspace_bytes.restype = sz
    L.rle_decode_packed_seg_workspace_bytes.argtypes = [u32, u64]
    L.rle_decode_packed_batch_device_seg.restype = ctypes.c_int
    L.rle_decode_packed_batch_device_seg.argtypes = [vp, vp, vp, vp, vp, vp, vp, u32, u64, vp, sz, vp]
    L.rle_readn_batch_device_seg.restype = ctypes.c_int
    L.rle_readn_batch_device_seg.argtypes = [vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, u32, u64, vp, sz, vp]
    L.rle_reply_header_bytes.restype = sz
    L.rle_reply_header_bytes.argtypes = [u32, u64]
    L.rle_readn_headers_device.restype = ctypes.c_int
    L.rle_readn_headers_device.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, vp]
    L.rle_readn_reply_device.restype = ctypes.c_int
    L.rle_readn_reply_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, u32, u32, vp]
    L.rle_readn_reply_device_seg.restype = ctypes.c_int
    L.rle_readn_reply_device_seg.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, u32, u32, u64, vp, sz, vp]
    L.rle_relocate_span_bytes.restype = u64
    L.rle_relocate_span_bytes.argtypes = [u64]
    L.rle_relocate_layout_device.restype = ctypes.c_int
    L.rle_relocate_layout_device.argtypes = [vp, vp, vp, u64, vp, vp, vp, u32, vp]
    L.rle_relocate_batch_device.restype = ctypes.c_int
    L.rle_relocate_batch_device.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, vp, vp, vp, vp, u32, vp]
    L.rle_evict_select_device.restype = ctypes.c_int
    L.rle_evict_select_device.argtypes = [vp, vp, vp, vp, vp, u64, u32, u32, vp, vp, vp, u32, vp]
    L.rle_evict_gather_device.restype = ctypes.c_int
    L.rle_evict_gather_device.argtypes = [vp, vp, u32, vp, vp, u32, u32, vp]
    L.rle_tail_seg_workspace_bytes.restype = sz
    L.rle_tail_seg_workspace_bytes.argtypes = [u32, u64]
    L.rle_tail_batch_device_seg.restype = ctypes.c_int
    L.rle_tail_batch_device_seg.argtypes = [vp, vp, vp, vp, vp, vp, u32, u64, vp, sz, vp]
    L.rle_mi355x_set_coop_mode.restype = ctypes.c_int
    L.rle_mi355x_set_coop_mode.argtypes = [ctypes.c_int]
    u32p = ctypes.POINTER(u32)
    L.rle_mi355x_coop_form.restype = ctypes.c_int
    L.rle_mi355x_coop_form.argtypes = [ctypes.c_int, u64, u64, u32p, u32p, u32p]
    # the by-value cooperative launches of the drop-in's single calls (csrc/rle_coop.hip; test helpers)
    L.rle_encode_coop_one.restype = ctypes.c_int
    L.rle_encode_coop_one.argtypes = [vp, vp, u64, vp, vp, u32, vp]
    L.rle_decode_coop_one.restype = ctypes.c_int
    L.rle_decode_coop_one.argtypes = [vp, vp, u64, u64, u64, vp, u32, vp]
    L.rle_decode_release_stream.restype = ctypes.c_int
    L.rle_decode_release_stream.argtypes = [vp]
    L.rle_mi355x_set_dec_round.restype = ctypes.c_int
    L.rle_mi355x_set_dec_round.argtypes = [ctypes.c_int]
    L.rle_copy_device.restype = ctypes.c_int
    L.rle_copy_device.argtypes = [vp, vp, ctypes.c_uint64, vp]
    L.rle_decode_pattern_device.restype = ctypes.c_int
    L.rle_decode_pattern_device.argtypes = [vp] * 6 + [ctypes.c_uint32, vp]
    for f, a in (("rle_dist_available", [ctypes.c_char_p]),
                 ("rle_dist_unique_id", [vp, sz, ctypes.c_char_p]),
                 ("rle_dist_init", [vp, sz, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]),
                 ("rle_dist_gather_offsets", [vp, u32, vp, vp, vp, sz, vp]),
                 ("rle_dist_gather_offsets_async", [vp, u32, vp, vp, vp, sz, vp, vp, ctypes.c_int]),
                 ("rle_dist_offsets_device", [vp, u32, u32, vp, vp, sz, vp]),
                 ("rle_dist_finalize", [])):
        getattr(L, f).restype = ctypes.c_int
        getattr(L, f).argtypes = a
    L.rle_dist_workspace_bytes.restype = sz
    L.rle_dist_workspace_bytes.argtypes = [u32]
    _lib = L
    return L


def max_compressed_size(U: int) -> int:
    return int(lib().rle_max_compressed_size(U))


def round16(x: int) -> int:
    return (x + 15) & ~15


# ------------------------------------------------------------------ drop-in (host) API
def compress(data: bytes) -> bytes:
    """RLEcompress (src/rleCompression.c:9-45) through the drop-in C ABI."""
    c = ctypes.c_size_t(0)
    p = lib().RLEcompress(data, len(data), ctypes.byref(c))
    if not p:
        raise MemoryError("RLEcompress returned NULL")
    out = ctypes.string_at(p, c.value) if c.value else b""
    _libc.free(p)
    return out


def decompress(stream: bytes, U: int, E: int = 0) -> bytes:
    """RLEdecompress (src/rleCompression.c:47-62): U decoded bytes followed by E zero bytes."""
    p = lib().RLEdecompress(stream, len(stream), U, E)
    if not p:
        raise MemoryError("RLEdecompress returned NULL")
    out = ctypes.string_at(p, U + E) if U + E else b""
    _libc.free(p)
    return out


def append(content: bytes, U: int, new: bytes) -> bytes:
    """RLEappend (include/rle_fileops.h): the write path of src/filesystemApi.c:766-775
    -- decode(content, U) ‖ new, re-encoded -- as one fused device round trip."""
    c = ctypes.c_size_t(0)
    p = lib().RLEappend(content, len(content), U, new, len(new), ctypes.byref(c))
    if not p:
        raise MemoryError("RLEappend returned NULL")
    out = ctypes.string_at(p, c.value) if c.value else b""
    _libc.free(p)
    return out


def decompress_n(streams, usizes):
    """RLEdecompressN (include/rle_fileops.h): the n decodes of readNFiles
    (src/filesystemApi.c:675-687) / eviction (src/server.c:314-323) in one launch, into caller buffers."""
    n = len(streams)
    if n != len(usizes):
        raise ValueError("streams and usizes differ in length")
    keep = [ctypes.create_string_buffer(s, len(s) + 1) for s in streams]
    outs = [ctypes.create_string_buffer(max(int(u), 1)) for u in usizes]
    data = (ctypes.c_void_p * max(n, 1))(*[ctypes.addressof(b) for b in keep])
    cs = (ctypes.c_size_t * max(n, 1))(*[len(s) for s in streams])
    us = (ctypes.c_size_t * max(n, 1))(*[int(u) for u in usizes])
    op = (ctypes.c_void_p * max(n, 1))(*[ctypes.addressof(b) for b in outs])
    rc = lib().RLEdecompressN(n, data, cs, us, op)
    if rc != 0:
        raise RLEError(f"RLEdecompressN failed (errno {ctypes.get_errno()})")
    return [o.raw[:int(u)] for o, u in zip(outs, usizes)]


# ------------------------------------------------------------------ batch layout helpers
def layout(sizes, align=16, pad=0):
    """Offsets of buffers packed back to back, each start 16-byte aligned (plus `pad` spare bytes
    after each buffer); returns (offs, total)."""
    offs, pos = [], 0
    for s in sizes:
        offs.append(pos)
        pos += (int(s) + align - 1) // align * align + pad
    return offs, max(pos, align)


def compressed_slots(sizes, pad=0):
    """Worst-case-capacity output slots for encoding buffers of the given sizes."""
    return layout([max_compressed_size(int(s)) for s in sizes], pad=pad)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


STREAM_PER_THREAD = 2   # hipStreamPerThread ((hipStream_t)2, hip_runtime_api.h)


def _stream_ptr(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    if isinstance(stream, int):   # a raw handle (tests: hipStreamPerThread)
        return ctypes.c_void_p(stream)
    return ctypes.c_void_p(stream.cuda_stream)


def release_stream(stream):
    """Free the issue-order array the library keeps for `stream` (rle_decode_release_stream)."""
    _check(lib().rle_decode_release_stream(_stream_ptr(stream)), "rle_decode_release_stream")


def encode_batch(d_in, in_off, in_len, d_out, out_off, out_len, status=None, stream=None, max_len=None, flags=0):
    """Batched encode on device tensors (uint8 data; int64 offsets/lengths; int32 status).  With
    max_len (>= every in_len) the sized entry point runs, which takes the cooperative kernels for
    batches of small buffers; flags (RLE_LAUNCH_STATUS_FLAG) selects the *_sized_flags form."""
    n = in_off.numel()
    if flags:
        rc = lib().rle_encode_batch_device_sized_flags(_ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out),
                                                       _ptr(out_off), _ptr(out_len), _ptr(status), n,
                                                       int(max_len), int(flags), _stream_ptr(stream))
    elif max_len is None:
        rc = lib().rle_encode_batch_device(_ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out), _ptr(out_off),
                                           _ptr(out_len), _ptr(status), n, _stream_ptr(stream))
    else:
        rc = lib().rle_encode_batch_device_sized(_ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out), _ptr(out_off),
                                                 _ptr(out_len), _ptr(status), n, int(max_len), _stream_ptr(stream))
    if rc != RLE_OK:
        raise RLEError(f"rle_encode_batch_device failed: {rc}")


def decode_batch(d_in, in_off, in_len, d_out, out_off, out_len, out_cap=None, status=None, stream=None,
                 max_in_len=None, max_out_len=None, flags=0):
    """Batched decode on device tensors.  With max_in_len / max_out_len (>= every in_len / out_len)
    the sized entry point runs (cooperative kernels for batches of small buffers); flags
    (RLE_LAUNCH_STATUS_FLAG) selects the *_sized_flags form."""
    n = in_off.numel()
    if flags:
        rc = lib().rle_decode_batch_device_sized_flags(_ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out),
                                                       _ptr(out_off), _ptr(out_len), _ptr(out_cap), _ptr(status), n,
                                                       int(max_in_len), int(max_out_len), int(flags),
                                                       _stream_ptr(stream))
    elif max_in_len is None or max_out_len is None:
        rc = lib().rle_decode_batch_device(_ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out), _ptr(out_off),
                                           _ptr(out_len), _ptr(out_cap), _ptr(status), n, _stream_ptr(stream))
    else:
        rc = lib().rle_decode_batch_device_sized(_ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out), _ptr(out_off),
                                                 _ptr(out_len), _ptr(out_cap), _ptr(status), n, int(max_in_len),
                                                 int(max_out_len), _stream_ptr(stream))
    if rc != RLE_OK:
        raise RLEError(f"rle_decode_batch_device failed: {rc}")


def seg_workspace(n: int, total_in_bytes: int, device=None):
    """A device workspace for the segmented entry points (caller-owned, reusable across calls on
    one stream)."""
    import torch
    nb = int(lib().rle_seg_workspace_bytes(n, int(total_in_bytes)))
    return torch.empty(nb + 256, dtype=torch.uint8, device=device if device is not None else "cuda")


def seg_segment_bytes(total_in_bytes: int) -> int:
    """The segment length (bytes, a multiple of 1008) a segmented launch with this total_in_bytes
    takes on the current device (rle_seg_segment_bytes; host only, 256 CUs without a device)."""
    f = lib().rle_seg_segment_bytes
    f.restype, f.argtypes = ctypes.c_uint32, [ctypes.c_uint64]
    return int(f(int(total_in_bytes)))


def _ws_ptr(ws):
    a = ws.data_ptr()
    return ctypes.c_void_p((a + 255) & ~255), ws.numel() - ((-a) & 255)


def encode_batch_seg(d_in, in_off, in_len, d_out, out_off, out_len, status=None, total_in_bytes=None,
                     workspace=None, stream=None):
    """Segmented batched encode (several waves per buffer; for large buffers).  The default
    total_in_bytes (the sum of in_len, read back from the device) synchronises, and the default
    workspace is allocated here: a call captured into a graph must pass both."""
    n = in_off.numel()
    total = int(in_len.sum().item()) if total_in_bytes is None else int(total_in_bytes)
    ws = workspace if workspace is not None else seg_workspace(n, total, d_in.device)
    wp, wn = _ws_ptr(ws)
    rc = lib().rle_encode_batch_device_seg(_ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out), _ptr(out_off),
                                           _ptr(out_len), _ptr(status), n, total, wp, wn, _stream_ptr(stream))
    if rc != RLE_OK:
        raise RLEError(f"rle_encode_batch_device_seg failed: {rc}")


def decode_batch_seg(d_in, in_off, in_len, d_out, out_off, out_len, out_cap=None, status=None,
                     total_in_bytes=None, workspace=None, stream=None):
    """Segmented batched decode (several waves per buffer; for large buffers).  The default
    total_in_bytes (the sum of in_len, read back from the device) synchronises, and the default
    workspace is allocated here: a call captured into a graph must pass both."""
    n = in_off.numel()
    total = int(in_len.sum().item()) if total_in_bytes is None else int(total_in_bytes)
    ws = workspace if workspace is not None else seg_workspace(n, total, d_in.device)
    wp, wn = _ws_ptr(ws)
    rc = lib().rle_decode_batch_device_seg(_ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out), _ptr(out_off),
                                           _ptr(out_len), _ptr(out_cap), _ptr(status), n, total, wp, wn,
                                           _stream_ptr(stream))
    if rc != RLE_OK:
        raise RLEError(f"rle_decode_batch_device_seg failed: {rc}")


def gen_synthetic(d_out, off, length, kind=None, index=None, stream=None):
    n = off.numel()
    rc = lib().rle_gen_synthetic_device(_ptr(d_out), _ptr(off), _ptr(length), _ptr(kind), _ptr(index), n,
                                        _stream_ptr(stream))
    if rc != RLE_OK:
        raise RLEError(f"rle_gen_synthetic_device failed: {rc}")


def append_prepare(d_mid, U, d_head, d_meta, stream=None):
    """rle_append_prepare_device (include/rle_fileops.h): the final run of d_mid[0, U) and the 16-byte
    splice head of the incremental append.  d_mid: uint8, readable up to round16(U); d_head: 16 bytes;
    d_meta: 4 int64 (run start, r, the head again)."""
    rc = lib().rle_append_prepare_device(_ptr(d_mid), int(U), _ptr(d_head), _ptr(d_meta), _stream_ptr(stream))
    if rc != RLE_OK:
        raise RLEError(f"rle_append_prepare_device failed: {rc}")


def append_slot_bytes(C: int, A: int) -> int:
    """rle_append_slot_bytes: the slot capacity an append of A bytes to a C-byte stream may need
    (C + max_compressed_size(A + 9), rounded up to 16); 0 past RLE_MAX_BUFFER_BYTES.  Host only."""
    return int(lib().rle_append_slot_bytes(int(C), int(A)))


def tail_word(t: int, r: int) -> int:
    """The tail word of a stream whose final token starts at offset t with count r."""
    return int(t) | (int(r) << 32)


def tail_offset(w: int) -> int:
    return int(w) & 0xFFFFFFFF


def tail_count(w: int) -> int:
    return (int(w) >> 32) & 0xF


def _seg_defaults(n, lengths, total, ws, make_ws, device):
    """(total, ws) of a _seg call of the tail scan or the append: total None is the sum of lengths,
    read back from the device (which synchronises); ws None is a fresh workspace from make_ws."""
    total = int(lengths.sum().item()) if total is None else int(total)
    return total, ws if ws is not None else make_ws(n, total, device)


def _default_tail(tail, d_streams, off, length, stream):
    """The tail words of an append: the tensor given, or a fresh one filled by a scan of the streams
    (tail_batch) first."""
    if tail is None:
        import torch
        tail = torch.zeros(off.numel(), dtype=torch.int64, device=d_streams.device)
        tail_batch(d_streams, off, length, tail, None, None, stream)
    return tail


def tail_batch(d_in, off, length, tail, ulen=None, status=None, stream=None):
    """rle_tail_batch_device on device tensors (uint8 streams; int64 offsets, lengths, tail words and
    decoded lengths; int32 status): the tail word t | r << 32 and the decoded length of every stream,
    reading the streams only."""
    _check(lib().rle_tail_batch_device(_ptr(d_in), _ptr(off), _ptr(length), _ptr(tail), _ptr(ulen), _ptr(status),
                                       off.numel(), _stream_ptr(stream)), "rle_tail_batch_device")


def tail_seg_workspace(n: int, total_in_bytes: int, device=None):
    """A device workspace for tail_batch_seg (caller-owned, reusable across calls on one stream)."""
    import torch
    nb = int(lib().rle_tail_seg_workspace_bytes(n, int(total_in_bytes)))
    return torch.empty(nb + 256, dtype=torch.uint8, device=device if device is not None else "cuda")


def tail_batch_seg(d_in, off, length, tail, ulen=None, status=None, total_in_bytes=None, ws=None, stream=None):
    """rle_tail_batch_device_seg: tail_batch with several waves per stream, for streams that are large
    next to the batch.  total_in_bytes (>= the sum of length; default: that sum) sizes the segment
    tables; ws: from tail_seg_workspace (default: a fresh one).  The default total_in_bytes
    synchronises (the sum is read back from the device): a call captured into a graph must pass
    total_in_bytes and ws."""
    n = off.numel()
    total, ws = _seg_defaults(n, length, total_in_bytes, ws, tail_seg_workspace, d_in.device)
    _check(lib().rle_tail_batch_device_seg(_ptr(d_in), _ptr(off), _ptr(length), _ptr(tail), _ptr(ulen), _ptr(status),
                                           n, total, *_ws_ptr(ws), _stream_ptr(stream)), "rle_tail_batch_device_seg")


def append_batch(d_streams, off, length, cap, ulen, d_new, new_off, new_len, status=None, tail=None, stream=None):
    """rle_append_batch_device on device tensors: new_len[i] bytes at d_new + new_off[i] appended to
    the stream in the slot d_streams + off[i] (length[i] bytes of cap[i]), in place; length, ulen
    (may be None) and tail are updated.  tail=None: the tail words come from a scan of the streams
    first (tail_batch) into a fresh tensor.  Returns the tail tensor, to be carried into the next
    append."""
    tail = _default_tail(tail, d_streams, off, length, stream)
    _check(lib().rle_append_batch_device(_ptr(d_streams), _ptr(off), _ptr(length), _ptr(cap), _ptr(ulen), _ptr(tail),
                                         _ptr(d_new), _ptr(new_off), _ptr(new_len), _ptr(status), off.numel(),
                                         _stream_ptr(stream)), "rle_append_batch_device")
    return tail


def append_seg_workspace(n: int, total_new_bytes: int, device=None):
    """A device workspace for append_batch_seg (caller-owned, reusable across calls on one stream)."""
    import torch
    nb = int(lib().rle_append_seg_workspace_bytes(n, int(total_new_bytes)))
    return torch.empty(nb + 256, dtype=torch.uint8, device=device if device is not None else "cuda")


def append_batch_seg(d_streams, off, length, cap, ulen, d_new, new_off, new_len, status=None, total_new_bytes=None,
                     workspace=None, tail=None, stream=None):
    """rle_append_batch_device_seg: append_batch with several waves per file, for new content that is
    large next to the batch.  total_new_bytes (>= the sum of new_len; default: that sum) sizes the
    segment tables; workspace: from append_seg_workspace (default: a fresh one).  Returns the tail
    tensor, as append_batch does.  The default total_new_bytes synchronises (the sum is read back
    from the device) and the default tail launches a scan into a new tensor: a call captured into a
    graph must pass total_new_bytes, workspace and tail."""
    n = off.numel()
    tail = _default_tail(tail, d_streams, off, length, stream)
    total, ws = _seg_defaults(n, new_len, total_new_bytes, workspace, append_seg_workspace, d_streams.device)
    _check(lib().rle_append_batch_device_seg(_ptr(d_streams), _ptr(off), _ptr(length), _ptr(cap), _ptr(ulen),
                                             _ptr(tail), _ptr(d_new), _ptr(new_off), _ptr(new_len), _ptr(status), n,
                                             total, *_ws_ptr(ws), _stream_ptr(stream)), "rle_append_batch_device_seg")
    return tail


def append_size(d_streams, off, length, tail, d_new, new_off, new_len, need, status=None, stream=None):
    """rle_append_size_batch_device: need[i] = the length append_batch would leave in length[i], and
    nothing else is written (need: int64; tail: the streams' tail words, required)."""
    _check(lib().rle_append_size_batch_device(_ptr(d_streams), _ptr(off), _ptr(length), _ptr(tail), _ptr(d_new),
                                              _ptr(new_off), _ptr(new_len), _ptr(need), _ptr(status), off.numel(),
                                              _stream_ptr(stream)), "rle_append_size_batch_device")
    return need


def append_size_seg(d_streams, off, length, tail, d_new, new_off, new_len, need, status=None, total_new_bytes=None,
                    workspace=None, stream=None):
    """rle_append_size_batch_device_seg: append_size with several waves per file.  total_new_bytes and
    workspace as in append_batch_seg (a captured call must pass both)."""
    n = off.numel()
    total, ws = _seg_defaults(n, new_len, total_new_bytes, workspace, append_seg_workspace, d_new.device)
    _check(lib().rle_append_size_batch_device_seg(_ptr(d_streams), _ptr(off), _ptr(length), _ptr(tail), _ptr(d_new),
                                                  _ptr(new_off), _ptr(new_len), _ptr(need), _ptr(status), n, total,
                                                  *_ws_ptr(ws), _stream_ptr(stream)),
           "rle_append_size_batch_device_seg")
    return need


def append_fit(d_streams, off, length, cap, ulen, d_new, new_off, new_len, need, status=None, tail=None, stream=None):
    """rle_append_fit_batch_device: append_batch whose capacity rule is cap[i] >= the new length
    (exact); need[i] receives that length, and a file that does not fit is refused with
    RLE_STATUS_NOFIT, untouched.  tail=None: from a scan first, as in append_batch.  Returns the tail
    tensor."""
    tail = _default_tail(tail, d_streams, off, length, stream)
    _check(lib().rle_append_fit_batch_device(_ptr(d_streams), _ptr(off), _ptr(length), _ptr(cap), _ptr(ulen),
                                             _ptr(tail), _ptr(d_new), _ptr(new_off), _ptr(new_len), _ptr(need),
                                             _ptr(status), off.numel(), _stream_ptr(stream)),
           "rle_append_fit_batch_device")
    return tail


def append_fit_seg(d_streams, off, length, cap, ulen, d_new, new_off, new_len, need, status=None,
                   total_new_bytes=None, workspace=None, tail=None, stream=None):
    """rle_append_fit_batch_device_seg: append_fit with several waves per file.  total_new_bytes,
    workspace and tail as in append_batch_seg (a captured call must pass all three)."""
    n = off.numel()
    tail = _default_tail(tail, d_streams, off, length, stream)
    total, ws = _seg_defaults(n, new_len, total_new_bytes, workspace, append_seg_workspace, d_streams.device)
    _check(lib().rle_append_fit_batch_device_seg(_ptr(d_streams), _ptr(off), _ptr(length), _ptr(cap), _ptr(ulen),
                                                 _ptr(tail), _ptr(d_new), _ptr(new_off), _ptr(new_len), _ptr(need),
                                                 _ptr(status), n, total, *_ws_ptr(ws), _stream_ptr(stream)),
           "rle_append_fit_batch_device_seg")
    return tail


def decode_packed(d_in, in_off, in_len, d_out, out_off, out_len, status=None, stream=None):
    """rle_decode_packed_batch_device on device tensors: decode_batch with cap = U whose destinations
    d_out + out_off[i] may lie at any byte; file i writes exactly out_len[i] bytes there and nothing
    else, so files may abut."""
    _check(lib().rle_decode_packed_batch_device(_ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out), _ptr(out_off),
                                                _ptr(out_len), _ptr(status), in_off.numel(), _stream_ptr(stream)),
           "rle_decode_packed_batch_device")


def readn_layout(ulen, gap, place, total, stream=None):
    """rle_readn_layout_device: place[i] = sum over k < i of (gap[k] + ulen[k]) + gap[i] and total[0] =
    the sum over all files (int64 device tensors; gap may be None: no gaps), in one launch."""
    _check(lib().rle_readn_layout_device(_ptr(ulen), _ptr(gap), _ptr(place), _ptr(total), ulen.numel(),
                                         _stream_ptr(stream)), "rle_readn_layout_device")


def readn_batch(d_streams, off, length, ulen, gap, d_out, place, total, status=None, out_cap=None, stream=None):
    """rle_readn_batch_device: readn_layout, then decode_packed of the streams to d_out + place[i].
    out_cap (default: d_out's size) is the reply's capacity: a reply longer than that leaves d_out
    untouched, every status RLE_STATUS_NOFIT, and place / total say what it takes."""
    cap = d_out.numel() if out_cap is None else int(out_cap)
    _check(lib().rle_readn_batch_device(_ptr(d_streams), _ptr(off), _ptr(length), _ptr(ulen), _ptr(gap), _ptr(d_out),
                                        cap, _ptr(place), _ptr(total), _ptr(status), off.numel(),
                                        _stream_ptr(stream)), "rle_readn_batch_device")


def decode_packed_seg_workspace(n: int, total_in_bytes: int, device=None):
    """A device workspace for decode_packed_seg and readn_batch_seg (caller-owned, reusable across
    calls on one stream)."""
    import torch
    nb = int(lib().rle_decode_packed_seg_workspace_bytes(n, int(total_in_bytes)))
    return torch.empty(nb + 256, dtype=torch.uint8, device=device if device is not None else "cuda")


def decode_packed_seg(d_in, in_off, in_len, d_out, out_off, out_len, status=None, total_in_bytes=None, ws=None,
                      stream=None):
    """rle_decode_packed_batch_device_seg: decode_packed with several waves per stream, for streams
    that are large next to the batch.  total_in_bytes (>= the sum of in_len; default: that sum) sizes
    the segment tables; ws: from decode_packed_seg_workspace (default: a fresh one).  The default
    total_in_bytes synchronises (the sum is read back from the device): a call captured into a graph
    must pass total_in_bytes and ws."""
    n = in_off.numel()
    total, ws = _seg_defaults(n, in_len, total_in_bytes, ws, decode_packed_seg_workspace, d_in.device)
    _check(lib().rle_decode_packed_batch_device_seg(_ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out), _ptr(out_off),
                                                    _ptr(out_len), _ptr(status), n, total, *_ws_ptr(ws),
                                                    _stream_ptr(stream)), "rle_decode_packed_batch_device_seg")


def readn_batch_seg(d_streams, off, length, ulen, gap, d_out, place, total, status=None, out_cap=None,
                    total_in_bytes=None, ws=None, stream=None):
    """rle_readn_batch_device_seg: readn_batch with several waves per stream (readn_layout, then
    decode_packed_seg to d_out + place[i]); out_cap as in readn_batch, total_in_bytes and ws as in
    decode_packed_seg."""
    n = off.numel()
    cap = d_out.numel() if out_cap is None else int(out_cap)
    tin, ws = _seg_defaults(n, length, total_in_bytes, ws, decode_packed_seg_workspace, d_streams.device)
    _check(lib().rle_readn_batch_device_seg(_ptr(d_streams), _ptr(off), _ptr(length), _ptr(ulen), _ptr(gap), _ptr(d_out),
                                            cap, _ptr(place), _ptr(total), _ptr(status), n, tin, *_ws_ptr(ws),
                                            _stream_ptr(stream)), "rle_readn_batch_device_seg")


def reply_header_bytes(form: int, path_len: int = 0) -> int:
    """rle_reply_header_bytes: the header's length in front of a file, 20 + path_len (RLE_REPLY_READN)
    or 10 (RLE_REPLY_READ); 0 for a bad form."""
    return int(lib().rle_reply_header_bytes(form, int(path_len)))


def readn_headers(d_paths, path_off, path_len, ulen, d_out, place, form=RLE_REPLY_READN, stream=None):
    """rle_readn_headers_device: file i's header into d_out[place[i] - gap_i : place[i]] from the path
    table (d_paths uint8, path_off / path_len int64; None in the READ form) and ulen on the device;
    with RLE_REPLY_END the ten '0' behind the last file.  No other byte is written."""
    _check(lib().rle_readn_headers_device(_ptr(d_paths), _ptr(path_off), _ptr(path_len), _ptr(ulen), _ptr(d_out),
                                          _ptr(place), form, ulen.numel(), _stream_ptr(stream)),
           "rle_readn_headers_device")


def readn_reply(d_streams, off, length, ulen, d_paths, path_off, path_len, d_out, place, total, status=None,
                form=RLE_REPLY_READN, out_cap=None, stream=None):
    """rle_readn_reply_device: the whole wire reply -- the layout with the header lengths derived from
    path_len, readn_batch's packed decode, the headers and (RLE_REPLY_END) the terminator -- on one
    stream; total[0] bytes of d_out are the reply.  out_cap as in readn_batch."""
    cap = d_out.numel() if out_cap is None else int(out_cap)
    _check(lib().rle_readn_reply_device(_ptr(d_streams), _ptr(off), _ptr(length), _ptr(ulen), _ptr(d_paths),
                                        _ptr(path_off), _ptr(path_len), _ptr(d_out), cap, _ptr(place), _ptr(total),
                                        _ptr(status), form, off.numel(), _stream_ptr(stream)),
           "rle_readn_reply_device")


def readn_reply_seg(d_streams, off, length, ulen, d_paths, path_off, path_len, d_out, place, total, status=None,
                    form=RLE_REPLY_READN, out_cap=None, total_in_bytes=None, ws=None, stream=None):
    """rle_readn_reply_device_seg: readn_reply over readn_batch_seg's launches; total_in_bytes and ws as
    in decode_packed_seg."""
    n = off.numel()
    cap = d_out.numel() if out_cap is None else int(out_cap)
    tin, ws = _seg_defaults(n, length, total_in_bytes, ws, decode_packed_seg_workspace, d_streams.device)
    _check(lib().rle_readn_reply_device_seg(_ptr(d_streams), _ptr(off), _ptr(length), _ptr(ulen), _ptr(d_paths),
                                            _ptr(path_off), _ptr(path_len), _ptr(d_out), cap, _ptr(place),
                                            _ptr(total), _ptr(status), form, n, tin, *_ws_ptr(ws),
                                            _stream_ptr(stream)), "rle_readn_reply_device_seg")


def relocate_span_bytes(room: int) -> int:
    """rle_relocate_span_bytes: the destination bytes one workgroup of relocate_batch's copy owns for
    a room (dst_cap - dst_base) of this many bytes: a multiple of 16 KiB, about room / (8 * CUs).
    Host only, 256 CUs without a device."""
    return int(lib().rle_relocate_span_bytes(int(room)))


def relocate_layout(length, want, sel, new_off, new_cap, total, dst_base=0, stream=None):
    """rle_relocate_layout_device: new slots from sizes on the device, in one launch: a selected file
    (sel None: all; else int32, non-zero) takes new_cap[i] = max(want[i], length[i]) rounded up to 16
    (want None: 0), any other file 0; new_off[i] = dst_base + the caps before it and total[0] = the end
    of the last slot (int64 device tensors)."""
    _check(lib().rle_relocate_layout_device(_ptr(length), _ptr(want), _ptr(sel), int(dst_base), _ptr(new_off),
                                            _ptr(new_cap), _ptr(total), length.numel(), _stream_ptr(stream)),
           "rle_relocate_layout_device")


def relocate_batch(d_src, off, length, d_dst, new_off, new_cap, total, want=None, sel=None, status=None, dst_base=0,
                   dst_cap=None, stream=None):
    """rle_relocate_batch_device: relocate_layout, then one copy of every selected stream
    (d_src + off[i], length[i] bytes) to its new slot d_dst + new_off[i].  dst_cap (default: d_dst's
    size) bounds the end of the last slot and, with dst_base, sizes the grid: pass the room this
    relocation may take.  Slots that end past it leave d_dst untouched, every selected file
    RLE_STATUS_NOFIT, and new_off / new_cap / total say what it takes."""
    cap = d_dst.numel() if dst_cap is None else int(dst_cap)
    _check(lib().rle_relocate_batch_device(_ptr(d_src), _ptr(off), _ptr(length), _ptr(want), _ptr(sel), _ptr(d_dst),
                                           int(dst_base), cap, _ptr(new_off), _ptr(new_cap), _ptr(total), _ptr(status),
                                           off.numel(), _stream_ptr(stream)), "rle_relocate_batch_device")


def evict_select(key, length, keep, victims, summary, want=None, live=None, spare=None, max_bytes=(1 << 64) - 1,
                 max_files=0, flags=0, stream=None):
    """rle_evict_select_device: the eviction victims from keys and sizes on the device, in one launch:
    the eligible files (live None: all, else int32 non-zero; spare None: none spared) in ascending
    (key[i], i) order, unsigned, until the live files' sizes (max(want[i], length[i]), want None: 0;
    rounded up to 16 under RLE_EVICT_SLOTS) sum to max_bytes at most and, with max_files != 0, the live
    files are max_files at most.  keep[i] (int32) = 1 for a live file that stays, victims[0:m] (int32)
    the victims in eviction order, summary (int64, RLE_EVICT_SUMMARY_WORDS) = status, m, bytes before
    and after, live files before and after.  key, length, want: int64 device tensors, read as unsigned."""
    _check(lib().rle_evict_select_device(_ptr(key), _ptr(length), _ptr(want), _ptr(live), _ptr(spare), int(max_bytes),
                                         int(max_files), int(flags), _ptr(keep), _ptr(victims), _ptr(summary),
                                         length.numel(), _stream_ptr(stream)), "rle_evict_select_device")


def evict_gather(victims, summary, tables_in, tables_out, order=RLE_EVICT_ORDER_EVICTION, cap=None, stream=None):
    """rle_evict_gather_device: row j of every tables_out[k] from row victims[j] (or, in
    RLE_EVICT_ORDER_REPLY, victims[m - 1 - j]) of tables_in[k], for j < min(m, cap) with m = summary[1]
    read on the device; 1 to 8 int64 tables; cap (default: the first output table's size) bounds the
    rows written."""
    k = len(tables_in)
    if len(tables_out) != k:
        raise RLEError("rle_evict_gather_device: as many output tables as input tables")
    cap = (tables_out[0].numel() if k else 0) if cap is None else int(cap)
    tin = (ctypes.c_void_p * max(k, 1))(*[t.data_ptr() for t in tables_in])
    tout = (ctypes.c_void_p * max(k, 1))(*[t.data_ptr() for t in tables_out])
    _check(lib().rle_evict_gather_device(_ptr(victims), _ptr(summary), int(order), tin, tout, k, cap,
                                         _stream_ptr(stream)), "rle_evict_gather_device")


def copy_device(dst, src, nbytes, stream=None):
    """rle_copy_device: the hand-written 16-byte-per-lane streaming copy bench.py times as the
    practical HBM ceiling (not part of the codec).  nbytes must be a multiple of 16."""
    rc = lib().rle_copy_device(_ptr(dst), _ptr(src), int(nbytes), _stream_ptr(stream))
    if rc != RLE_OK:
        raise RLEError(f"rle_copy_device failed: {rc}")


def decode_pattern(d_in, in_offs, in_lens, d_out, out_offs, out_lens, stream=None):
    """rle_decode_pattern_device: the large-batch decode's memory traffic (tiles of C in, U out, one
    wave per buffer, the decode's occupancy and issue order) without its token work; bench.py times
    it as the ceiling of that access pattern.  Not a decode: d_out receives the tiles' bytes."""
    rc = lib().rle_decode_pattern_device(_ptr(d_in), _ptr(in_offs), _ptr(in_lens), _ptr(d_out), _ptr(out_offs),
                                         _ptr(out_lens), in_offs.numel(), _stream_ptr(stream))
    if rc != RLE_OK:
        raise RLEError(f"rle_decode_pattern_device failed: {rc}")


def set_coop_mode(mode: int):
    """Tests: the cooperative small-buffer kernels never (0), always when the sizes qualify (1), or
    when the launch is resident at once (-1, the default; RLE_MI355X_COOP sets it at load)."""
    if lib().rle_mi355x_set_coop_mode(int(mode)) != RLE_OK:
        raise RLEError(f"bad cooperative mode {mode}")


def coop_enc_form(max_len: int):
    """The cooperative encode form (W, R) the launchers select for this largest input length, or None
    when it does not qualify (rle_mi355x_coop_form; host only, launches nothing)."""
    w, u, r = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    ok = lib().rle_mi355x_coop_form(0, int(max_len), 0, ctypes.byref(w), ctypes.byref(u), ctypes.byref(r))
    return (w.value, r.value) if ok else None


def coop_dec_form(max_in_len: int, max_out_len: int):
    """The cooperative decode form (W, Umax, R) for these largest stream and decoded lengths, or None."""
    w, u, r = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    ok = lib().rle_mi355x_coop_form(1, int(max_in_len), int(max_out_len), ctypes.byref(w), ctypes.byref(u),
                                    ctypes.byref(r))
    return (w.value, u.value, r.value) if ok else None


def encode_coop_one(d_src, d_dst, U, d_out_len, d_status, flags=0, stream=None) -> int:
    """Tests: rle_encode_coop_one, the by-value cooperative encode of one buffer (d_src readable up to
    round16(U), d_dst of max_compressed_size(U) bytes, both 16-byte aligned; d_out_len one int64,
    d_status one int32).  Returns 1 launched, 0 the size does not qualify (nothing launched)."""
    rc = lib().rle_encode_coop_one(_ptr(d_src), _ptr(d_dst), int(U), _ptr(d_out_len), _ptr(d_status), int(flags),
                                   _stream_ptr(stream))
    if rc < 0:
        raise RLEError(f"rle_encode_coop_one failed: {rc}")
    return rc


def decode_coop_one(d_src, d_dst, C, U, cap, d_status, flags=0, stream=None) -> int:
    """Tests: rle_decode_coop_one, the by-value cooperative decode of one stream (d_src readable up to
    round16(C), d_dst of cap >= U bytes).  Returns 1 launched, 0 the sizes do not qualify."""
    rc = lib().rle_decode_coop_one(_ptr(d_src), _ptr(d_dst), int(C), int(U), int(cap), _ptr(d_status), int(flags),
                                   _stream_ptr(stream))
    if rc < 0:
        raise RLEError(f"rle_decode_coop_one failed: {rc}")
    return rc


def set_dec_round(waves: int) -> int:
    """Waves per workgroup of the large-batch decode in rounds (csrc/rle_round.h): 0 off, 4, 8 or
    16 (RLE_MI355X_DEC_ROUND sets it at load); -1 only reads.  Returns the previous setting."""
    rc = lib().rle_mi355x_set_dec_round(int(waves))
    if rc < 0:
        raise RLEError(f"bad decode round width {waves}")
    return rc


def selftest() -> int:
    return int(lib().rle_mi355x_selftest())


def device_count() -> int:
    return int(lib().rle_mi355x_device_count())


def version() -> str:
    return lib().rle_mi355x_version().decode()


def dropin_stats(reset=False) -> dict:
    """Host-path accounting of the drop-in calls made in this process (include/rle_mi355x.h)."""
    st = DropinStats()
    rc = lib().rle_mi355x_dropin_stats(ctypes.byref(st), 1 if reset else 0)
    if rc != RLE_OK:
        raise RLEError(f"rle_mi355x_dropin_stats failed: {rc}")
    return st.as_dict()


# ------------------------------------------------------------------ multi-GPU exchange (csrc/rle_dist.hip)
def _check(rc, what):
    if rc != RLE_OK:
        raise RLEError(f"{what} failed: {rc}")


def _torch_rccl_path():
    """torch's own librccl (the copy torch.distributed's "nccl" backend loaded), so the exchange uses
    the same RCCL library as the process group."""
    import torch
    p = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
    return p.encode() if os.path.exists(p) else None


def dist_available():
    """Raises unless RCCL resolves in this process (the preflight of shard.NativeExchange)."""
    _check(lib().rle_dist_available(_torch_rccl_path()), "rle_dist_available")


def dist_unique_id() -> bytes:
    buf = ctypes.create_string_buffer(128)
    _check(lib().rle_dist_unique_id(buf, 128, _torch_rccl_path()), "rle_dist_unique_id")
    return buf.raw


def dist_init(uid: bytes, rank: int, world: int):
    _check(lib().rle_dist_init(uid, len(uid), rank, world, _torch_rccl_path()), "rle_dist_init")


def dist_workspace(n: int, device):
    """The scan workspace of one exchange of n sizes per rank (rle_dist_workspace_bytes): an int64
    device tensor (at least one element), to be kept alive as long as any call or graph uses it.
    Exchanges that may run at once need one each."""
    words = max(1, int(lib().rle_dist_workspace_bytes(int(n))) // 8)
    import torch
    return torch.empty(words, dtype=torch.int64, device=device)


def _ws(ws):
    return (_ptr(ws), ws.numel() * ws.element_size()) if ws is not None else (None, 0)


# Workspaces made for calls that pass none: the scan kernels run on `stream` (or the
# comm stream, or a captured graph replays them) after the call returns, so a temporary torch tensor
# could be handed to another tensor by the caching allocator while they still use it.  One workspace
# per (device, stream, slot) instead, kept for the life of the process: calls on one stream run in
# order, and calls that may run at once (different streams or slots) get different workspaces.  It
# grows when a larger n needs more (keyed on n as well, callers whose n changed from step
# to step grew device memory without bound); the replaced tensor is marked as used by the stream
# (record_stream), so the allocator hands it out again only after the work issued on it so far.
_WS_CACHE = {}


def _default_ws(n, device, stream, slot):
    import torch
    dev = torch.device(device)
    key = (dev.type, dev.index, _stream_ptr(stream).value or 0, slot)
    need = max(1, int(lib().rle_dist_workspace_bytes(int(n))) // 8)
    ws = _WS_CACHE.get(key)
    if ws is None or ws.numel() < need:
        if ws is not None:
            s = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.current_stream(dev)
            ws.record_stream(s)
        ws = _WS_CACHE[key] = dist_workspace(n, dev)
    return ws


def dist_gather_offsets(sizes, gathered, offsets, stream=None, ws=None):
    """One exchange step (rle_dist_gather_offsets) on `stream`: sizes (int64[n], device) all-gathered
    and scanned into offsets (int64[world * n]) in the global stream order; ws: dist_workspace(n)
    (None: a workspace of this module's own for this stream, kept alive, _default_ws)."""
    if ws is None:
        ws = _default_ws(sizes.numel(), sizes.device, stream, "gather")
    _check(lib().rle_dist_gather_offsets(_ptr(sizes), sizes.numel(), _ptr(gathered), _ptr(offsets), *_ws(ws),
                                         _stream_ptr(stream)), "rle_dist_gather_offsets")


def dist_gather_offsets_async(sizes, gathered, offsets, codec_stream, comm_stream, slot: int, ws=None):
    """The exchange on comm_stream after the work issued on codec_stream (rle_dist_gather_offsets_async);
    codec_stream waits only for the previous call's exchange (the other slot).  Slots must alternate;
    ws: this slot's dist_workspace(n) (None: this module's own for the comm stream and slot)."""
    if ws is None:
        ws = _default_ws(sizes.numel(), sizes.device, comm_stream, ("async", int(slot)))
    _check(lib().rle_dist_gather_offsets_async(_ptr(sizes), sizes.numel(), _ptr(gathered), _ptr(offsets), *_ws(ws),
                                               _stream_ptr(codec_stream), _stream_ptr(comm_stream), int(slot)),
           "rle_dist_gather_offsets_async")


def dist_offsets(gathered, world: int, n: int, offsets, stream=None, ws=None):
    if ws is None:
        ws = _default_ws(n, gathered.device, stream, "offsets")
    _check(lib().rle_dist_offsets_device(_ptr(gathered), world, n, _ptr(offsets), *_ws(ws), _stream_ptr(stream)),
           "rle_dist_offsets_device")


def dist_finalize():
    _check(lib().rle_dist_finalize(), "rle_dist_finalize")
