"""GPU tests: every device entry point replayed from a captured graph, against the oracle.

The rest of the suite launches each call once, eagerly, into fresh tensors.  Here a launch is
captured once (torch.cuda.graph on a side stream, a linear chain, the default capture error mode:
no form needed `relaxed`) and replayed over data sets that differ in every buffer, so everything
the host decided at capture -- form, grid, size hints, segment length, the workspace carve-up -- is
frozen, and everything else has to come from device memory on every run.  Protocol of every test
(run_protocol): an eager warm-up with data set 0; the capture; one replay per further data set with
the inputs rewritten in the same device tensors and the outputs poisoned (0xA5 data, 0xFFFFFFFF
status, -1 lengths); the same call eagerly; the graph destroyed; the call eagerly once more.  After
every run each buffer's bytes, length and status are the oracle's, every other byte of the output
arena is still poison, and no non-empty buffer equals what the previous data set expected there.

Data sets move every buffer across the form's edges (long, one tile, empty, long again), and hold
one refused buffer (decode: cap < U; encode: a misaligned input) that is accepted in the sets
around it, so a status word goes both ways.  The CPU side of this (consecutive sets differ in
every non-empty buffer) is asserted before anything is launched (assert_sets_differ).

Large-batch decode (n > 4096): the captured launch takes order_acquire's per-launch
hipMallocAsync / hipFreeAsync pair (csrc/rle_kernels.hip); the eager launches around it the cached
array of the stream."""
import numpy as np
import pytest
import torch

import append_tail_gpu as G
import append_tail_model as M
import coop_forms as CF
import rle_mi355x as R
import rle_oracle as O
import stream_family as F
from test_gpu_parity import DEV, POISON, _input_image

pytestmark = pytest.mark.gpu
INFO = R.RLE_STATUS_OVERFLOW | R.RLE_STATUS_SERIAL | R.RLE_STATUS_SHORT
KINDS = 5   # O.gen: zero, random, runs50, runs90, pairs


# ------------------------------------------------------------------ data
class Buf:
    """One buffer of one data set.  data: the launch's input bytes; want: the output's bytes (empty
    when refused); decode: U and cap as passed; refused: the launch must answer MISALIGNED and write
    nothing (decode: cap < U; encode: the input offset is moved off its alignment); serial: a stream
    the encoder never writes (status SERIAL, the bytes of the exact decode)."""
    __slots__ = ("data", "want", "U", "cap", "refused", "serial")

    def __init__(self, data, want, U=None, cap=None, refused=False, serial=False):
        self.data, self.want, self.U, self.cap = bytes(data), bytes(want), U, cap
        self.refused, self.serial = refused, serial


def enc_buf(x, refused=False):
    return Buf(x, b"" if refused else O.encode(x), refused=refused)


_FILL = bytes(F._FILL)


def stream_of_len(C, kind, index):
    """(y, x): an encoder stream of exactly C bytes and its content: the oracle's encode of
    generated data, as long as fits, then literals that no neighbour pairs up with."""
    if C == 0:
        return b"", b""
    u = C * 6 // 10
    while u and len(O.encode(O.gen(kind, index, u + u // 5 + 1))) <= C:
        u += u // 5 + 1
    x0 = O.gen(kind, index, u)
    y0 = O.encode(x0)
    k = next(i for i in range(3) if not x0 or _FILL[i] != x0[-1])
    fill = bytes(_FILL[(k + j) % 3] for j in range(C - len(y0)))
    x, y = x0 + fill, y0 + fill
    assert len(y) == C and O.encode(x) == y, (C, kind, index)
    return y, x


def dec_buf(C, kind, index, room=0, refused=False):
    """An accepted decode of a C-byte encoder stream into a slot of U + room bytes, or (refused) one
    with cap = U - 1."""
    y, x = stream_of_len(C, kind, index)
    if refused:
        assert len(x) >= 1
        return Buf(y, b"", U=len(x), cap=len(x) - 1, refused=True)
    return Buf(y, x, U=len(x), cap=len(x) + room)


def serial_buf(p, max_c):
    """A serial-class stream with its probe at stream position p and cap = U (stream_family)."""
    c = next(c for c in F.family(p) if c.serial and c.cap == c.U and c.U >= 16 and len(c.stream) <= max_c)
    ref, ost = O.decode(c.stream, c.U, c.cap)
    b = Buf(c.stream, ref, U=c.U, cap=c.cap, serial=True)
    return b, ost & 1


def assert_sets_differ(sets):
    """CPU: a result left over from the previous data set cannot pass for this one."""
    for k in range(len(sets)):   # (set 0 also follows the last one: the eager run behind the replays)
        for i, (a, b) in enumerate(zip(sets[k - 1], sets[k])):
            if len(b.want):
                assert a.want != b.want, (k, i, len(b.want))
    for k, s in enumerate(sets):   # a refused buffer is accepted in the sets on both sides
        for i, b in enumerate(s):
            if b.refused:
                assert not sets[k - 1][i].refused and not sets[(k + 1) % len(sets)][i].refused, (k, i)
                assert len(sets[k - 1][i].want) and len(sets[(k + 1) % len(sets)][i].want), (k, i)


# ------------------------------------------------------------------ the launch's fixed device tensors
class Stage:
    """The device tensors of one encode or decode launch, allocated once for the largest data set
    and rewritten per data set on `stream` (packed 16-byte-aligned slots, so the offsets move too)."""

    def __init__(self, kind, sets, stream):
        self.kind, self.stream, self.n = kind, stream, len(sets[0])
        assert all(len(s) == self.n for s in sets)
        need_in = max(self._layout(s)[1] for s in sets) + 64
        need_out = max(self._layout(s)[3] for s in sets) + 64
        i64 = dict(dtype=torch.int64, device=DEV)
        with torch.cuda.stream(stream):
            self.d_in = torch.zeros(need_in, dtype=torch.uint8, device=DEV)
            self.d_out = torch.empty(need_out, dtype=torch.uint8, device=DEV)
            self.in_off, self.in_len = torch.zeros(self.n, **i64), torch.zeros(self.n, **i64)
            self.out_off, self.out_len = torch.zeros(self.n, **i64), torch.zeros(self.n, **i64)
            self.cap = torch.zeros(self.n, **i64)
            self.status = torch.zeros(self.n, dtype=torch.int32, device=DEV)
        self.cur = None

    def _layout(self, bufs):
        in_offs, in_total = R.layout([len(b.data) for b in bufs])
        if self.kind == "enc":
            out_offs, out_total = R.compressed_slots([len(b.data) for b in bufs])
        else:
            out_offs, out_total = R.layout([max(b.cap, b.U) for b in bufs])
        return in_offs, in_total, out_offs, out_total

    def load(self, bufs):
        """The data set's inputs into the device tensors, and the outputs poisoned."""
        in_offs, host = _input_image([b.data for b in bufs], None)
        _, _, out_offs, out_total = self._layout(bufs)
        assert host.size <= self.d_in.numel() and out_total <= self.d_out.numel()
        if self.kind == "enc":
            in_offs = [o + (8 if b.refused else 0) for o, b in zip(in_offs, bufs)]

        def put(t, vals):
            t.copy_(torch.from_numpy(np.asarray(vals, dtype=np.int64)))

        with torch.cuda.stream(self.stream):
            self.d_in[:host.size].copy_(torch.from_numpy(host))
            put(self.in_off, in_offs)
            put(self.in_len, [len(b.data) for b in bufs])
            put(self.out_off, out_offs)
            self.d_out.fill_(POISON)
            self.status.fill_(-1)
            if self.kind == "enc":
                self.out_len.fill_(-1)
            else:
                put(self.out_len, [b.U for b in bufs])
                put(self.cap, [b.cap for b in bufs])
        self.cur = (bufs, list(out_offs))

    def check(self, label, stale=None, overflow=None):
        """After the launch: every buffer's bytes, length and status, and every other byte of the
        arena still poison.  stale: the previous data set, which no non-empty buffer may match."""
        bufs, out_offs = self.cur
        self.stream.synchronize()
        out = self.d_out.cpu().numpy()
        st = self.status.cpu().numpy().astype(np.uint32)
        lens = self.out_len.cpu().numpy()
        exp = np.full(out.size, POISON, np.uint8)
        for i, (b, o) in enumerate(zip(bufs, out_offs)):
            exp[o:o + len(b.want)] = np.frombuffer(b.want, np.uint8)
            s = int(st[i])
            if b.refused:
                assert s == R.RLE_STATUS_MISALIGNED, (label, i, hex(s))
            elif b.serial:
                assert s & R.RLE_STATUS_SERIAL and not s & ~INFO, (label, i, hex(s))
                if overflow is not None:
                    assert (s & R.RLE_STATUS_OVERFLOW) == overflow, (label, i, hex(s))
            else:
                assert s == R.RLE_STATUS_OK, (label, i, hex(s), len(b.data))
            if self.kind == "enc":
                assert int(lens[i]) == len(b.want), (label, i, int(lens[i]), len(b.want))
        diff = np.nonzero(out != exp)[0]
        if diff.size:
            p = int(diff[0])
            i = max([j for j, o in enumerate(out_offs) if o <= p], default=0)
            raise AssertionError(f"{label}: buffer {i} (input {len(bufs[i].data)} bytes, output {len(bufs[i].want)}), "
                                 f"byte +{p - out_offs[i]} is {out[p]:#x}, expected {exp[p]:#x}; {diff.size} bytes differ")
        if stale is not None:
            for i, (b, o, a) in enumerate(zip(bufs, out_offs, stale)):
                if len(b.want):
                    assert out[o:o + len(b.want)].tobytes() != a.want, (label, i, "stale")


def run_protocol(stage, launch, sets, overflow=None):
    """Warm-up, capture, one replay per further data set, eager, graph destroyed, eager (module
    docstring).  launch() issues the call on the current stream from the stage's tensors."""
    assert len(sets) >= 4
    assert_sets_differ(sets)
    s = stage.stream
    with torch.cuda.stream(s):
        stage.load(sets[0])
        launch()
        stage.check("warm-up", overflow=overflow)
        stage.load(sets[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    with torch.cuda.stream(s):
        for k in range(1, len(sets)):
            stage.load(sets[k])
            g.replay()
            stage.check(f"replay {k}", stale=sets[k - 1], overflow=overflow)
        stage.load(sets[0])
        launch()
        stage.check("eager after the replays", stale=sets[-1], overflow=overflow)
        g.reset()
        del g
        stage.load(sets[1])
        launch()
        stage.check("eager after the graph", stale=sets[0], overflow=overflow)


@pytest.fixture
def side():
    s = torch.cuda.Stream(device=DEV)
    yield s
    s.synchronize()


@pytest.fixture
def always_coop():
    R.set_coop_mode(1)
    yield
    R.set_coop_mode(-1)


def enc_launch(st, **kw):
    return lambda: R.encode_batch(st.d_in, st.in_off, st.in_len, st.d_out, st.out_off, st.out_len, st.status, **kw)


def dec_launch(st, **kw):
    return lambda: R.decode_batch(st.d_in, st.in_off, st.in_len, st.d_out, st.out_off, st.out_len, st.cap, st.status,
                                  **kw)


# ------------------------------------------------------------------ one wave per buffer
WAVE_N = 64
WAVE_SIZES = [4096, 1, 15, 1008, 17, 1007, 0, 1009, 2016, 16]
WAVE_ROT = (0, 3, 6, 8)   # buffer 0: 4096 -> 1008 -> 0 -> 2016 over the data sets
WAVE_REFUSED = 2          # in data set 2: 1007 -> (2016, refused) -> 4096
assert sorted(WAVE_SIZES) == [0, 1, 15, 16, 17, F.TILE - 1, F.TILE, F.TILE + 1, 2 * F.TILE, 4096]


def wave_size(k, i):
    return WAVE_SIZES[(i + WAVE_ROT[k]) % len(WAVE_SIZES)]


def wave_sets(kind):
    if kind == "enc":
        return [[enc_buf(O.gen((i // 10 + k) % KINDS, 1000 * k + i, wave_size(k, i)),
                         refused=(k == 2 and i == WAVE_REFUSED)) for i in range(WAVE_N)] for k in range(4)]
    return [[dec_buf(wave_size(k, i), (i // 10 + k) % KINDS, 2000 * k + i, room=16 * (i % 3),
                     refused=(k == 2 and i == WAVE_REFUSED)) for i in range(WAVE_N)] for k in range(4)]


def test_one_wave_encode(side):
    sets = wave_sets("enc")
    st = Stage("enc", sets, side)
    run_protocol(st, enc_launch(st), sets)


def test_one_wave_decode(side):
    sets = wave_sets("dec")
    st = Stage("dec", sets, side)
    run_protocol(st, dec_launch(st), sets)


# ------------------------------------------------------------------ more than 4096 buffers
LARGE_MAX_IN = 3 * F.TILE


def large_sets(n):
    """Nearly all buffers decode to 16-64 bytes; 32 streams of 1-3 tiles sit at positions that move
    with the data set, so the longest-first issue order is another one on every replay."""
    sets = []
    for k in range(4):
        long_at = {(37 + 611 * k + (n // 32) * j) % n: j for j in range(32)}
        assert len(long_at) == 32
        bufs = []
        for i in range(n):
            j = long_at.get(i)
            if j is not None:
                C = (F.TILE, F.TILE + 1, 2 * F.TILE, 3 * F.TILE)[j % 4] - (j // 4 if j % 4 == 3 else 0)
                bufs.append(dec_buf(C, 1 + j % 4, 7000 * k + i))
            else:
                bufs.append(dec_buf(16 + (i * 7 + k * 13) % 49, 1 + (i + k) % 4, 7000 * k + i, room=16 * (i % 2),
                                    refused=(k == 2 and i == 4096)))
        sets.append(bufs)
    assert max(len(b.data) for s in sets for b in s) == LARGE_MAX_IN and sets[2][4096].refused
    return sets


@pytest.mark.parametrize("n,sized", [(4097, False), (8195, True)])
def test_large_batch_decode(side, n, sized):
    """One buffer past a residency round, and past two rounds plus odd chunks of the 256-buffer
    local sort.  The captured launch allocates and frees its issue-order array inside the graph; the
    eager launches before and after it use the stream's cached array, released at the end."""
    assert n > 4096 and n % 256
    sets = large_sets(n)
    st = Stage("dec", sets, side)
    hints = dict(max_in_len=LARGE_MAX_IN, max_out_len=max(b.U for s in sets for b in s)) if sized else {}
    try:
        run_protocol(st, dec_launch(st, **hints), sets)
    finally:
        R.release_stream(side)


# ------------------------------------------------------------------ cooperative forms
def _coop_sizes(limit, tile):
    """n = 4 sizes per data set: 1 byte up to the hint, exactly the hint and one tile less."""
    return [[limit, 1, limit // 2 + 3, limit - tile],
            [limit - tile, limit, 17, tile + 1],
            [1, limit - tile, limit, 0],
            [tile, limit // 3, 1, limit]]


def coop_enc_sets(max_len):
    sizes = _coop_sizes(max_len, CF.ENC_TILE)
    return [[enc_buf(O.gen((i + k) % KINDS, 3000 * k + i, sizes[k][i]), refused=(k == 2 and i == 1)) for i in range(4)]
            for k in range(4)]


def coop_dec_sets(max_in, max_out):
    """Pairs and random data, the long streams all pairs (1.5 stream bytes per output byte): a
    stream of max_in bytes has to decode to no more than max_out."""
    sizes = _coop_sizes(max_in, F.TILE)
    sets = [[dec_buf(sizes[k][i], 4 if (i + k) % 2 == 0 or sizes[k][i] > max_out * 3 // 4 else 1, 4000 * k + i,
                     room=16 * (i % 2), refused=(k == 2 and i == 1)) for i in range(4)] for k in range(4)]
    assert max(b.U for s in sets for b in s) <= max_out and max(len(b.data) for s in sets for b in s) == max_in
    return sets


@pytest.mark.parametrize("flags", [0, R.RLE_LAUNCH_STATUS_FLAG])
@pytest.mark.parametrize("form", [(4, 1), (16, 2)])
def test_coop_encode(side, always_coop, form, flags):
    max_len = CF.enc_hints(form)[0]
    assert R.coop_enc_form(max_len) == form and (form[1] > 1) == (form == (16, 2))
    sets = coop_enc_sets(max_len)
    st = Stage("enc", sets, side)
    run_protocol(st, enc_launch(st, max_len=max_len, flags=flags), sets)


@pytest.mark.parametrize("flags", [0, R.RLE_LAUNCH_STATUS_FLAG])
@pytest.mark.parametrize("form,max_in", [((5, 4096, 1), 5040), ((16, 16384, 2), 20000)])
def test_coop_decode(side, always_coop, form, max_in, flags):
    max_out = form[1]
    assert R.coop_dec_form(max_in, max_out) == form and CF.dec_hints(form)[1][0] <= max_in <= CF.dec_hints(form)[0][0]
    sets = coop_dec_sets(max_in, max_out)
    st = Stage("dec", sets, side)
    run_protocol(st, dec_launch(st, max_in_len=max_in, max_out_len=max_out, flags=flags), sets)


# ------------------------------------------------------------------ segmented
def seg_hint(n):
    """(S, hint): the capture-time total_in_bytes of n buffers of up to five segments."""
    S = R.seg_segment_bytes(1)
    hint = 5 * S * n
    assert R.seg_segment_bytes(hint) == S
    return S, hint


def seg_sizes(n, S):
    """Per data set and buffer; a buffer's segment count shrinks and grows from set to set."""
    if n == 1:
        return [[5 * S], [S + 1], [S], [3 * S + 5], [0], [S - 1], [5 * S], [1]]
    return [[5 * S, S - 1, 3 * S + 5],
            [1, 3 * S + 5, 0],
            [S + 1, S, 5 * S],
            [3 * S + 5, 0, 1],
            [S + 1, 5 * S, S - 1]]


def seg_sets(kind, n):
    """(sets, hint, the serial stream's OVERFLOW bit).  Data set 1 holds the refused buffer (the last
    of n = 1, else buffer 1); decode: buffer 0 of data set 2 is a stream the encoder never writes,
    its probe on the first segment edge, and data set 3 holds an encoder stream there again."""
    S, hint = seg_hint(n)
    sizes = seg_sizes(n, S)
    overflow = None
    if kind == "enc":
        sets = [[enc_buf(O.gen((i + 2 * k) % KINDS, 5000 * k + i, sizes[k][i]), refused=(k == 1 and i == min(1, n - 1)))
                 for i in range(n)] for k in range(len(sizes))]
    else:
        sets = [[dec_buf(sizes[k][i], (i + 2 * k) % KINDS, 6000 * k + i, room=16 * ((i + k) % 2),
                         refused=(k == 1 and i == min(1, n - 1))) for i in range(n)] for k in range(len(sizes))]
        sets[2][0], overflow = serial_buf(S, 5 * S)
    assert max(sum(len(b.data) for b in s) for s in sets) <= hint
    return sets, hint, overflow


@pytest.mark.parametrize("n", [3, 1])
def test_segmented_encode(side, n):
    sets, hint, _ = seg_sets("enc", n)
    st = Stage("enc", sets, side)
    ws = R.seg_workspace(n, hint, DEV)
    run_protocol(st, lambda: R.encode_batch_seg(st.d_in, st.in_off, st.in_len, st.d_out, st.out_off, st.out_len,
                                                st.status, total_in_bytes=hint, workspace=ws), sets)


@pytest.mark.parametrize("n", [3, 1])
def test_segmented_decode(side, n):
    sets, hint, overflow = seg_sets("dec", n)
    st = Stage("dec", sets, side)
    ws = R.seg_workspace(n, hint, DEV)
    run_protocol(st, lambda: R.decode_batch_seg(st.d_in, st.in_off, st.in_len, st.d_out, st.out_off, st.out_len,
                                                st.cap, st.status, total_in_bytes=hint, workspace=ws), sets,
                 overflow=overflow)


# ------------------------------------------------------------------ appends: state carried on the device
class Appends:
    """n stored streams in slots sized for every append of the test, their d_len / d_ulen / d_tail
    kept on the device from launch to launch; the new bytes and their lengths are rewritten per
    launch.  The host follows with the content x ‖ new1 ‖ ... and checks the slots against the
    oracle's encode of it."""
    HEAD = 16   # bytes in front of every new buffer that no kernel reads

    def __init__(self, contents, rounds, stream):
        self.stream, self.n = stream, len(contents)
        self.x = [bytes(x) for x in contents]
        ys = [O.encode(x) for x in self.x]
        total = [sum(len(r[i]) for r in rounds) for i in range(self.n)]
        need = [R.append_slot_bytes(len(y), a) for y, a in zip(ys, total)]
        assert all(need)
        for i, x in enumerate(self.x):   # (CPU) no launch of the test runs a slot out of capacity
            for r in rounds:
                assert R.append_slot_bytes(len(O.encode(x)), len(r[i])) <= need[i], (i, len(x), len(r[i]), need[i])
                x = x + r[i]
        self.soffs, stotal = R.layout(need, pad=G.PAD)
        img = np.full(stotal + 64, G.POISON, np.uint8)
        for y, o in zip(ys, self.soffs):
            img[o:o + len(y)] = np.frombuffer(y, np.uint8)
        amax = max(len(a) for r in rounds for a in r)
        noffs, ntotal = R.layout([self.HEAD + amax] * self.n, pad=G.PAD)
        self.noffs = [o + self.HEAD for o in noffs]
        self.nimg = np.zeros(ntotal + 64, np.uint8)
        with torch.cuda.stream(stream):
            self.d_s = torch.from_numpy(img).to(DEV)
            self.d_n = torch.zeros(ntotal + 64, dtype=torch.uint8, device=DEV)
            self.off, self.cap, self.new_off = G.i64(self.soffs), G.i64(need), G.i64(self.noffs)
            self.d_len = G.i64([len(y) for y in ys])
            self.new_len = torch.zeros(self.n, dtype=torch.int64, device=DEV)
            self.d_ulen = torch.zeros(self.n, dtype=torch.int64, device=DEV)
            self.d_tail = torch.zeros(self.n, dtype=torch.int64, device=DEV)
            self.status = torch.zeros(self.n, dtype=torch.int32, device=DEV)
            # the tail scan, eagerly: what the captured appends carry on from
            R.tail_batch(self.d_s, self.off, self.d_len, self.d_tail, self.d_ulen, self.status)
        self.check("tail scan", None)

    def load(self, new):
        """The launch's new bytes (behind each, its last byte repeated: hostile padding) and lengths."""
        self.nimg[:] = 0
        for a, o in zip(new, self.noffs):
            self.nimg[o - self.HEAD:o] = 0xAA
            self.nimg[o:o + len(a)] = np.frombuffer(a, np.uint8)
            if a:
                self.nimg[o + len(a):o + len(a) + 24] = a[-1]
        with torch.cuda.stream(self.stream):
            self.d_n.copy_(torch.from_numpy(self.nimg))
            self.new_len.copy_(torch.from_numpy(np.asarray([len(a) for a in new], np.int64)))
            self.status.fill_(-1)
        self.new = new

    def check(self, label, new):
        """The slots hold the oracle's encode of the content so far; length, decoded length and tail
        word are those of a fresh scan; everything outside the streams is still poison."""
        self.stream.synchronize()
        before = [O.encode(x) for x in self.x]
        if new is not None:
            self.x = [x + a for x, a in zip(self.x, new)]
        got = self.d_s.cpu().numpy()
        ln, ul, tl = (t.cpu().numpy().astype(np.uint64) for t in (self.d_len, self.d_ulen, self.d_tail))
        st = self.status.cpu().numpy().astype(np.uint32)
        exp = np.full(got.size, G.POISON, np.uint8)
        for i, (x, o) in enumerate(zip(self.x, self.soffs)):
            y = O.encode(x)
            exp[o:o + len(y)] = np.frombuffer(y, np.uint8)
            assert st[i] == 0, (label, i, hex(st[i]))
            assert ln[i] == len(y) and ul[i] == len(x), (label, i, int(ln[i]), len(y), int(ul[i]), len(x))
            assert tl[i] == M.word_of(y), (label, i, hex(int(tl[i])), hex(M.word_of(y)))
            if new is not None:   # a file changes exactly when it got bytes
                assert (y != before[i]) == (len(new[i]) > 0), (label, i)
        diff = np.nonzero(got != exp)[0]
        assert not diff.size, (label, int(diff[0]), self.soffs, diff.size)
        # a fresh scan of the slots, on the device
        with torch.cuda.stream(self.stream):
            tail, ulen = torch.zeros_like(self.d_tail), torch.zeros_like(self.d_ulen)
            R.tail_batch(self.d_s, self.off, self.d_len, tail, ulen, None)
            self.stream.synchronize()
            assert torch.equal(tail, self.d_tail) and torch.equal(ulen, self.d_ulen), label


def append_rounds(contents, sizes, base):
    """rounds[k][i]: the new bytes of file i in launch k, sizes[(i + k) % len(sizes)] of them, in
    turn starting with the content's last byte (the final run goes on) and with another one."""
    last = [x[-1] if x else 0x61 for x in contents]
    rounds = []
    for k in range(6):
        new = []
        for i in range(len(contents)):
            a = bytearray(O.gen(1 + (i + k) % 4, base + 100 * k + i, sizes[(i + k) % len(sizes)]))
            if a:
                a[0] = last[i] if (i + k) % 2 == 0 else last[i] ^ 0x55
                if len(a) > 1 and (i + k) % 4 == 0:
                    a[1] = a[0]
                last[i] = a[-1]
            new.append(bytes(a))
        rounds.append(new)
    return rounds


def run_append_protocol(ap, launch, rounds):
    s = ap.stream
    with torch.cuda.stream(s):
        ap.load(rounds[0])
        launch()
        ap.check("warm-up", rounds[0])
        ap.load(rounds[0])   # (captured, not run)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch()
    with torch.cuda.stream(s):
        for k in (1, 2, 3):
            ap.load(rounds[k])
            g.replay()
            ap.check(f"replay {k}", rounds[k])
        ap.load(rounds[4])
        launch()
        ap.check("eager after the replays", rounds[4])
        g.reset()
        del g
        ap.load(rounds[5])
        launch()
        ap.check("eager after the graph", rounds[5])


def stored_contents(n):
    """Contents whose streams end in tokens of r = 1, 2, 9 and the empty stream, in turn."""
    ends = [b"q", b"zz", b"k" * 9, None]
    out = []
    for i in range(n):
        e = ends[i % 4]
        out.append(b"" if e is None else O.gen(1 + i % 4, 900 + i, 40 + 300 * (i // 4 % 8))[:-1] + b"\x01" + e)
    for x, r in zip(out, [1, 2, 9, 0] * n):
        assert (M.tail_of(O.encode(x))[1] if x else 0) == r
    return out


def test_append_in_place(side):
    xs = stored_contents(8)
    sizes = [0, 1, 9, F.TILE, F.TILE + 1]
    rounds = append_rounds(xs, sizes, 8000)
    assert all(any(len(a) == 0 for a in r) for r in rounds[1:4])
    ap = Appends(xs, rounds, side)
    run_append_protocol(ap, lambda: R.append_batch(ap.d_s, ap.off, ap.d_len, ap.cap, ap.d_ulen, ap.d_n, ap.new_off,
                                                   ap.new_len, ap.status, tail=ap.d_tail), rounds)


def test_append_segmented(side):
    n = 3
    xs = stored_contents(4)[:n]
    S = R.seg_segment_bytes(1)
    sizes = [1, S - 1, S + 1, 3 * S + 5]
    rounds = append_rounds(xs, sizes, 9000)
    hint = n * (3 * S + 5)
    assert R.seg_segment_bytes(hint) == S and max(sum(len(a) for a in r) for r in rounds) <= hint
    ap = Appends(xs, rounds, side)
    ws = R.append_seg_workspace(n, hint, DEV)
    run_append_protocol(ap, lambda: R.append_batch_seg(ap.d_s, ap.off, ap.d_len, ap.cap, ap.d_ulen, ap.d_n, ap.new_off,
                                                       ap.new_len, ap.status, total_new_bytes=hint, workspace=ws,
                                                       tail=ap.d_tail), rounds)


# ------------------------------------------------------------------ append prepare
def test_append_prepare(side):
    """rle_append_prepare_device holds a hipMemsetAsync (the run-start accumulator): replayed with
    final runs of L = 1, 9, 10 and the whole buffer, whose starts go down as well as up."""
    U = 5000
    runs = [10, 1, 9, 10, U, 1, 9]
    mids = []
    for k, L in enumerate(runs):
        c = 0x41 + k
        body = bytearray(O.gen(1, 300 + k, U - L))
        if body:
            body[-1] = c ^ 0x20
        mids.append(bytes(body) + bytes([c]) * L)
    with torch.cuda.stream(side):
        d_mid = torch.zeros(R.round16(U), dtype=torch.uint8, device=DEV)
        d_head = torch.zeros(16, dtype=torch.uint8, device=DEV)
        d_meta = torch.zeros(4, dtype=torch.int64, device=DEV)

    def load(k):
        with torch.cuda.stream(side):
            d_mid[:U].copy_(torch.from_numpy(np.frombuffer(mids[k], np.uint8).copy()))
            d_head.fill_(POISON)
            d_meta.fill_(-1)

    def launch():
        R.append_prepare(d_mid, U, d_head, d_meta)

    prev = [None]

    def check(label, k):
        side.synchronize()
        L, c = runs[k], mids[k][-1]
        r = (L - 1) % 9 + 1
        head, meta = d_head.cpu().numpy().tobytes(), d_meta.cpu().numpy()
        assert int(meta[0]) == U - L and int(meta[1]) == r, (label, meta[:2], U - L, r)
        assert meta[2:].tobytes() == head, label
        filler = head[:16 - r]
        assert head[16 - r:] == bytes([c]) * r and c not in filler, (label, head)
        new = b"\x07" + bytes([c]) * 3
        assert O.encode(filler) == filler and O.encode(head + new) == filler + O.encode(bytes([c]) * r + new), label
        assert head != prev[0], (label, "stale")
        prev[0] = head

    with torch.cuda.stream(side):
        load(0)
        launch()
        check("warm-up", 0)
        load(0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch()
    with torch.cuda.stream(side):
        for k in (1, 2, 3, 4):
            load(k)
            g.replay()
            check(f"replay {k}", k)
        load(5)
        launch()
        check("eager after the replays", 5)
        g.reset()
        del g
        load(6)
        launch()
        check("eager after the graph", 6)
