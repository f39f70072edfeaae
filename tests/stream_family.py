"""TEST INFRASTRUCTURE: a deterministic family of decode inputs the encoder never emits, placed at
chosen byte positions (lane, tile, segment, round and stream-end edges).  No GPU, no torch, no
numpy; its own xorshift PRNG, so the family is the same bytes on every Python.

A case is (stream, U, cap) with stream = prefix + probe + suffix:

  prefix  a valid encoder-style token stream of exactly p bytes, token-aligned at its end, whose
          last byte differs from the probe's value.  Four kinds: 0 literal-heavy over all 256
          values, 1 literals and pairs over {a b 5 9 0x00 0x80 z} with digits '2'..'9', 2 uniform
          "zz9" tokens (whole uniform tiles), 3 all pairs with digit '9' (3x expansion).
  probe   for a value v: 0 "vv2vv2", 1 "vv2v"+(v^1), 2 "vv5vv5vv5", 3 "vv9vv8vv9" (valid for the
          tiled decode but not canonical); 4..13 "vv"+d for the BAD_DIGITS; 14 "v", 15 "vv" (the
          stream is cut there: no suffix).
  suffix  empty, or about 1.5 KB of valid tokens (at least one more tile) whose first byte differs
          from the probe's last byte.
  U       from N, the decoded length under the reference's semantics (src/rleCompression.c:47-62,
          counts not capped): N, N - 1, N + 5 for a finite N; Nprefix + 40, Nprefix + 1 when a
          token is unbounded.
  cap     U + C + 16 (every token writes at most one byte past U); one U per stream is repeated
          with cap = U (N for the tiled-class probes: an exact fit; N - 1 or Nprefix + 1 for the
          others: the OVERFLOW truncation and status bit).

needs_serial(stream, U) is the routing rule documented at csrc/rle_device.h dec_serial: the tiled
decode declines a stream when some pair token, parsed from phase 0, has its second byte inside C
and a count digit past C or outside '2'..'9', or when N > U.  A final lone 0x00 byte pairs with
the zero padding and is not serial.

family(p) rotates the cross product (kind x value x probe x suffix) instead of taking it in full
(_combos);
Case.serial is the generator's own classification (from the structure of the case), which
tests/test_stream_family.py checks against needs_serial and against a brute-force walk.
"""
import hashlib

VALUES = (0x61, 0x35, 0x00, 0x80, 0x39)                                    # a 5 \0 \x80 9
BAD_DIGITS = (0x30, 0x31, 0x3A, 0x2F, 0x00, 0x7F, 0x80, 0xB5, 0xFF, 0x61)  # 0 1 : / ... a
NPROBES = 16
NKINDS = 4
TILE = 1008            # owned stream bytes of one decode tile
SEG = 64512            # a common multiple of the four-launch kernels' 4-, 8- and 16-tile segments
SEG_RES = 7056         # 7-tile segments (tests/test_gpu_seg_lengths.py runs them); once the retired resident kernels' length
_FILL = (0x71, 0x72, 0x73)   # q r s: literals no prefix alphabet pairs up and no probe value equals
_CARRIER = 2 * SEG + 8192
_MIXED = (0x61, 0x62, 0x35, 0x39, 0x00, 0x80, 0x7A)


class _XorShift:
    def __init__(self, seed):
        self.s = (0x9E3779B97F4A7C15 + seed) & 0xFFFFFFFFFFFFFFFF

    def next(self):
        x = self.s
        x ^= (x << 13) & 0xFFFFFFFFFFFFFFFF
        x ^= x >> 7
        x ^= (x << 17) & 0xFFFFFFFFFFFFFFFF
        self.s = x
        return x


class Case:
    """One decode input; unpacks as (stream, U, cap)."""
    __slots__ = ("stream", "U", "cap", "serial", "p", "kind", "probe", "value")

    def __init__(self, stream, U, cap, serial, p, kind, probe, value):
        self.stream, self.U, self.cap, self.serial = stream, U, cap, serial
        self.p, self.kind, self.probe, self.value = p, kind, probe, value

    def __iter__(self):
        return iter((self.stream, self.U, self.cap))

    def __repr__(self):
        return (f"Case(p={self.p}, kind={self.kind}, probe={self.probe}, v={self.value:#x}, C={len(self.stream)}, "
                f"U={self.U}, cap={self.cap}, serial={self.serial})")


def walk(y):
    """The token walk from phase 0.  Returns (N, bad): N the decoded length with no cap at U (None
    when some token's count is unbounded), bad whether some pair token has its second byte inside C
    and a count digit past C or outside '2'..'9'."""
    C = len(y)
    j = n = 0
    bad = unbounded = False
    while j < C:
        v = y[j]
        n += 1
        if j + 1 < C:
            if v != y[j + 1]:
                j += 1
                continue
            if j + 2 < C:
                d = y[j + 2]
                if 0x32 <= d <= 0x39:
                    n += d - 0x31
                else:
                    bad = True
                    if 0x3A <= d <= 0x7F:
                        n += d - 0x31          # a finite over-long count: 10..79 copies
                    elif d != 0x30 and d != 0x31:
                        unbounded = True       # (signed char)d - '0' < 0 wraps as size_t
            else:
                bad = unbounded = True          # the digit is the zero padding
            j += 3
        else:
            # the last byte: a literal, or (0x00) a pair with the zero padding whose fill to U writes
            # the zeros the output already holds
            j += 3 if v == 0 else 1
    return (None if unbounded else n), bad


def needs_serial(stream, U):
    N, bad = walk(stream)
    return bad or N is None or N > U


# ------------------------------------------------------------------ carriers
# One long token stream per prefix kind, with cum[i] = decoded length of carrier[:i] at the token
# boundaries i and -1 elsewhere; a prefix is a slice of it plus at most a few filler literals.
_carriers = {}


def _carrier(kind):
    c = _carriers.get(kind)
    if c is not None:
        return c
    rng = _XorShift(1000 + kind)
    out = bytearray()
    cum = [-1] * (_CARRIER + 4)
    n = 0
    prev = -1
    cum[0] = 0
    if kind == 2:
        ntok = _CARRIER // 3
        out = bytearray(b"zz9" * ntok)
        for t in range(1, ntok + 1):
            cum[3 * t] = 9 * t
    else:
        while len(out) < _CARRIER - 3:
            r = rng.next()
            if kind == 0:
                v = (r >> 16) & 0xFF
                pair = (r & 15) == 0
            elif kind == 1:
                v = _MIXED[(r >> 16) % 7]
                pair = (r & 3) < 2
            else:
                v = (r >> 16) & 0xFF
                pair = True
            if v == prev:
                v = (v + 1) & 0xFF if kind != 1 else _MIXED[(_MIXED.index(v) + 1) % 7]
            prev = v
            if pair:
                d = 9 if kind == 3 else 2 + ((r >> 8) & 7)
                out += bytes((v, v, 0x30 + d))
                n += d
            else:
                out.append(v)
                n += 1
            cum[len(out)] = n
    c = (bytes(out), cum)
    _carriers[kind] = c
    return c


def _filler(prev, avoid=-1):
    for f in _FILL:
        if f != prev and f != avoid:
            return f
    raise AssertionError


def prefix(kind, p, v):
    """(bytes of exactly p, decoded length): valid tokens, aligned at the end, last byte != v."""
    car, cum = _carrier(kind)
    b = p
    while b > 0 and (cum[b] < 0 or (b == p and car[b - 1] == v)):
        b -= 1
    out = bytearray(car[:b])
    prev = car[b - 1] if b else -1
    for _ in range(p - b):
        prev = _filler(prev)
        out.append(prev)
    assert p - b <= 8 and len(out) == p
    return bytes(out), cum[b] + (p - b)


_suffixes = {}


def _suffix_body(kind):
    s = _suffixes.get(kind)
    if s is None:
        car, cum = _carrier(kind)
        a = 3000
        while cum[a] < 0:
            a += 1
        e = a + 1500
        while cum[e] < 0:
            e -= 1
        s = _suffixes[kind] = (car[a:e], cum[e] - cum[a])
    return s


def suffix(kind, last):
    """(bytes, decoded length): a lead literal that differs from `last`, then ~1.5 KB of tokens."""
    body, n = _suffix_body(kind)
    return bytes((_filler(last, body[0]),)) + body, n + 1


def probe(pi, v):
    if pi == 0:
        return bytes((v, v, 0x32, v, v, 0x32))
    if pi == 1:
        return bytes((v, v, 0x32, v, v ^ 1))
    if pi == 2:
        return bytes((v, v, 0x35)) * 3
    if pi == 3:
        return bytes((v, v, 0x39, v, v, 0x38, v, v, 0x39))
    if pi < 14:
        return bytes((v, v, BAD_DIGITS[pi - 4]))
    return bytes((v,)) * (pi - 13)


def rot_for(p):
    """The rotation modulus at position p < 60000: about 1/rot of the cross product is taken (longer
    streams, fewer cases, so every test stays at a few seconds).  Past that, _combos takes eight
    streams per position."""
    return 6 if p < 8000 else 16


def _combos(p):
    """The (probe, suffix, kind, value index) combinations taken at position p.

    p < 60000: every rot-th combination of the cross product in mixed radix (probe, suffix, kind,
    value), the value lowest: rot = 6 = 5 + 1 and 16 = 3 * 5 + 1 step the value and the kind
    together, and the carries move the suffix and the probe.
    Longer streams: each dimension rotates on its own.  Position p takes the eight probes of its own
    parity (so any two neighbouring positions have all sixteen); the j-th of them goes with value
    (j + p) % 5, kind (j + p // 2) % 4 and suffix (j + p // 2) % 2, so one position has every value,
    every kind and both suffix settings, and a probe meets the other suffix setting two positions on.
    Cut probes end the stream: no suffix."""
    if p < 60000:
        rot = rot_for(p)
        out = []
        for idx in range((-p) % rot, NPROBES * 2 * NKINDS * len(VALUES), rot):
            pi, si = idx // 40, idx // 20 % 2
            if not (pi >= 14 and si):
                out.append((pi, si, idx // 5 % NKINDS, idx % 5))
        return out
    out = []
    for j in range(NPROBES // 2):
        pi = 2 * j + (p & 1)
        out.append((pi, 0 if pi >= 14 else (j + p // 2) % 2, (j + p // 2) % NKINDS, (j + p) % len(VALUES)))
    return out


_families = {}


def family(p):
    """The cases whose probe's first byte is at stream position p (a list, cached)."""
    fam = _families.get(p)
    if fam is not None:
        return fam
    fam = []
    pres = {}
    for pi, si, kind, vi in _combos(p):
        v = VALUES[vi]
        pre = pres.get((kind, v))
        if pre is None:
            pre = pres[(kind, v)] = prefix(kind, p, v)
        pb = probe(pi, v)
        npr, bad = walk(pb)
        tail, ntail = suffix(kind, pb[-1]) if si else (b"", 0)
        stream = pre[0] + pb + tail
        C = len(stream)
        if npr is None:
            N = None
            us = [pre[1] + 40, pre[1] + 1]
            exact = pre[1] + 1
        else:
            N = pre[1] + npr + ntail
            us = [N, N - 1, N + 5]
            exact = N - 1 if bad else N
        for U, cap in [(U, U + C + 16) for U in us] + [(exact, exact)]:
            fam.append(Case(stream, U, cap, bad or N is None or N > U, p, kind, pi, v))
    _families[p] = fam
    return fam


def cases(positions):
    out = []
    for p in positions:
        out += family(p)
    return out


def around(base, lo=-4, hi=2):
    return [base + d for d in range(lo, hi + 1)]


# ------------------------------------------------------------------ position groups (one per decode form's edges)
WAVE_GROUPS = {
    "lane": [0, 1, 2] + list(range(13, 19)),       # stream start; the lane edge (digit from the next lane)
    "tile1": around(TILE),
    "tile2": around(2 * TILE),
    "tile4": around(4 * TILE),
    "slot": list(range(1021, 1026)),               # the 1024-byte slot's end
}
COOP_GROUPS = {f"k{k}": around(k * TILE) for k in range(1, 8)}
COOP_GROUPS["round2"] = around(16 * TILE)          # past 16 tiles: a later round of the workgroup


def seg_positions(S):
    return around(S) + around(2 * S) + around(S + TILE, -2, 1)


SEG_TILES_BETWEEN = tuple(range(5, 16))   # segment lengths between the shortest (4 tiles) and the longest (16)


def seg_length_positions(m):
    """The first edge of m-tile segments, and for the two shortest odd lengths the second edge."""
    return around(m * TILE) + (around(2 * m * TILE) if m in (5, 7) else [])


def round_positions(waves):
    out = []
    for k in (1, waves - 1, waves, waves + 1):
        out += around(k * TILE)
    return out


def all_positions():
    ps = set()
    for g in (WAVE_GROUPS, COOP_GROUPS):
        for v in g.values():
            ps.update(v)
    for S in (SEG, SEG_RES):
        ps.update(seg_positions(S))
    for w in (4, 8, 16):
        ps.update(round_positions(w))
    for m in SEG_TILES_BETWEEN:
        ps.update(seg_length_positions(m))
    return sorted(ps)


def pin(fam, outputs):
    """sha256 over stream | U (8 bytes, little endian) | output of every case of one position."""
    h = hashlib.sha256()
    for c, out in zip(fam, outputs):
        assert len(out) == c.cap
        h.update(c.stream)
        h.update(c.U.to_bytes(8, "little"))
        h.update(out)
    return h.hexdigest()
