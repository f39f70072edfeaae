"""TEST INFRASTRUCTURE: labelled cases for every form of the cooperative kernels (csrc/rle_coop.hip:
one workgroup per buffer, one wave per tile, up to 5 rounds of 16 tiles).  No GPU, no torch, no
numpy: the oracle's generator, tests/stream_family.py and a few carriers of this module's own.

A form is a template instantiation: encode (W, R), decode (W, Umax, R); csrc/rle_coop_limits.h
chooses one from a launch's size hints.  enc_cases(form) / dec_cases(form) return the cases that
tests/test_gpu_coop_forms.py runs in one batch under the form's largest hint and again under its
smallest (enc_hints / dec_hints), so every wave count, staging size and round count sees:

  encode  every size 1024 k + (-1, 0, 1) up to the form's limit (waves that end early, a partly
          filled last round); runs ending at, crossing and starting at every wave and round edge,
          with lengths around the 9-byte token cut; runs that enter a round already started (the
          carried run start), cover a whole round, or span whole tiles inside a round; the staging's
          extremes (C = 1.5 U at the limit, C = U, all zero); digit-heavy repeats.
  decode  valid streams at the form's limits (U = Umax, C = 1008 W R, every round edge +-1, every
          reachable tile count); streams the encoder never emits (stream_family's probes) at tile
          edge 1, the last wave edge, every round edge and the last tile edge; one-tile streams
          with U = Umax; two buffers past the form (the in-kernel one-wave fallback).

Where stream_family's own prefixes cannot reach an edge inside the form (they expand, and the late
edges need at least as many stream bytes as output bytes), the prefix is built here: literals
(C = U) or "xx2" tokens (C = 1.5 U).  An edge that no stream reaches with a decoded length within
Umax is listed in EXEMPT with the reason; it still gets cases (all of the serial class: they decode
past U), so the wave on that edge parses a probe before the workgroup declines the stream.
tests/test_coop_forms.py checks all of this on the CPU.
"""
import rle_oracle as O
import stream_family as F

ENC_TILE, DEC_TILE = 1024, F.TILE
ROUND = 16   # tiles per round of the multi-round forms

ENC_FORMS = [(2, 1), (3, 1), (4, 1), (6, 1), (8, 1), (12, 1), (16, 1), (16, 2), (16, 4)]
DEC_FORMS = [(2, 4096, 1), (3, 4096, 1), (5, 4096, 1), (8, 4096, 1),
             (2, 16384, 1), (3, 16384, 1), (5, 16384, 1), (8, 16384, 1), (12, 16384, 1), (16, 16384, 1),
             (16, 16384, 2),
             (4, 32768, 1), (8, 32768, 1), (16, 32768, 1), (16, 32768, 3), (16, 32768, 4),
             (16, 65536, 5)]

# decode: ((largest max_in_len, max_out_len), (smallest: the previous thresholds plus one))
DEC_HINTS = {
    (2, 4096, 1): ((2016, 4096), (1009, 1)),
    (3, 4096, 1): ((3024, 4096), (2017, 1)),
    (5, 4096, 1): ((5040, 4096), (3025, 1)),
    (8, 4096, 1): ((8064, 4096), (5041, 1)),
    (2, 16384, 1): ((2016, 16384), (1009, 4097)),
    (3, 16384, 1): ((3024, 16384), (2017, 4097)),
    (5, 16384, 1): ((5040, 16384), (3025, 4097)),
    (8, 16384, 1): ((8064, 16384), (5041, 4097)),
    (12, 16384, 1): ((12096, 16384), (8065, 4097)),
    (16, 16384, 1): ((16128, 16384), (12097, 4097)),
    (16, 16384, 2): ((32256, 16384), (16129, 1)),
    (4, 32768, 1): ((4032, 32768), (1009, 16385)),
    (8, 32768, 1): ((8064, 32768), (4033, 16385)),
    (16, 32768, 1): ((16128, 32768), (8065, 16385)),
    (16, 32768, 3): ((48384, 32768), (16129, 16385)),
    (16, 32768, 4): ((64512, 32768), (48385, 16385)),
    (16, 65536, 5): ((80640, 65536), (1009, 32769)),
}

# Places of a decode form that no stream reaches with a decoded length within Umax: a valid token
# yields at most 1.5 stream bytes per output byte ("xx2"), so a stream of more than 1.5 Umax bytes
# decodes past Umax.  Keys: a tile edge k (the probe sits at 1008 k, so the bytes before it alone
# decode to at least 672 k), "limit" (a valid stream of 1008 W R bytes) or "round<r>" (valid streams
# around the round edge 16128 r).  Exempt edges carry serial-class cases only (U = Umax < N); exempt
# limits carry none.  tests/test_coop_forms.py counts these entries.
EXEMPT = {
    (8, 4096, 1): {7: "672 * 7 = 4704 > 4096", "limit": "8064 > 1.5 * 4096 = 6144"},
    (16, 16384, 2): {31: "672 * 31 = 20832 > 16384", "limit": "32256 > 1.5 * 16384 = 24576 (tiles 26-32)"},
    (16, 32768, 4): {63: "672 * 63 = 42336 > 32768", "limit": "64512 > 1.5 * 32768 = 49152 (tiles 50-64)"},
}


def enc_limit(form):
    return ENC_TILE * form[0] * form[1]


def enc_hints(form):
    """(largest, smallest) max_len that select the form."""
    limits = [ENC_TILE] + [enc_limit(f) for f in ENC_FORMS]
    return enc_limit(form), limits[ENC_FORMS.index(form)] + 1


def dec_limit(form):
    return DEC_TILE * form[0] * form[2]


def dec_hints(form):
    return DEC_HINTS[form]


def rotating_sample(items, key, n, rot):
    """n of items (all of them if there are fewer) for the one-call-each launches: the items grouped
    by key(item) and the groups taken in turn, one item each, until n are taken; a group is walked
    from a start that rotates with rot, in steps that spread over the group."""
    groups = {}
    for it in items:
        groups.setdefault(key(it), []).append(it)
    per = -(-n // len(groups))
    orders = []
    for g in sorted(groups, key=str):
        v = groups[g]
        step = max(1, len(v) // per)
        first = list(range(rot % step, len(v), step))
        orders.append([v[i] for i in first + [i for i in range(len(v)) if i not in set(first)]])
    out, depth = [], 0
    while len(out) < min(n, len(items)):
        for o in orders:
            if depth < len(o) and len(out) < n:
                out.append(o[depth])
        depth += 1
    return out


# ------------------------------------------------------------------ encode
class EncCase:
    """One encode input.  group: sizes | edge | carry | round | span | staging | digits | fallback;
    edge: the tile edge k of an `edge` case; fits: within the form (a `fallback` case is not)."""
    __slots__ = ("label", "data", "group", "edge", "fits")

    def __init__(self, label, data, group, edge=None, fits=True):
        self.label, self.data, self.group, self.edge, self.fits = label, bytes(data), group, edge, fits

    def __repr__(self):
        return f"EncCase({self.label}, U={len(self.data)})"


RUN_LENGTHS = (1, 2, 3, 8, 9, 10, 11, 17, 18, 19, 27, 28)
SIDES = ("ends", "crosses", "starts")


def enc_wave_edges(form):
    return list(range(1, form[0] * form[1]))


def enc_round_edges(form):
    return [ROUND * r for r in range(1, form[1])]


def enc_full_edges(form):
    """The edges that take the whole (length x side) cross product; the others a rotating third."""
    return sorted({1, form[0] - 1} | set(enc_round_edges(form)))


def _run_span(e, L, side):
    if side == "ends":
        return e - L, e
    if side == "starts":
        return e, e + L
    if L == 1:
        return e - 1, e + 1   # (the shortest run on both sides)
    return e - (L + 1) // 2, e - (L + 1) // 2 + L


def no_equal_neighbours(seed, n):
    """n random bytes, no two neighbours equal (C = U)."""
    x = bytearray(O.gen(1, seed, n))
    for i in range(1, n):
        if x[i] == x[i - 1]:
            x[i] = (x[i] + 1 + (i + 1 < n and x[i + 1] == (x[i] + 1) & 0xFF)) & 0xFF
    return bytes(x)


def exact_pairs(n):
    """n bytes of runs of exactly two (a last single byte when n is odd): C = 1.5 U."""
    out = bytearray()
    k = 0
    while len(out) < n:
        out += bytes((k * 37 & 0xFF,)) * 2
        k += 1
    return bytes(out[:n])


def repeat_heavy(seed, size):
    """Runs of 1..21 over a small alphabet heavy in digit bytes (the generator of
    tests/test_gpu_coop.py test_runs_and_digits_across_tile_edges, on this module's PRNG)."""
    rng = F._XorShift(seed)
    alpha = (b"a0123456789", b"\0\x01", b"33", b"ab", b"99")[rng.next() % 5]
    out = bytearray()
    while len(out) < size:
        r = rng.next()
        out += bytes((alpha[(r >> 8) % len(alpha)],)) * (1 + (r >> 32) % 21)
    return bytes(out[:size])


_enc_cache = {}


def enc_cases(form):
    """The encode cases of form (W, R), a list of EncCase (cached)."""
    if form in _enc_cache:
        return _enc_cache[form]
    W, R = form
    lim, nt = enc_limit(form), W * R
    seed = 100000 * W + 1000 * R
    out = []
    # sizes: the waves that end early, the last round partly filled
    sizes = {0, 1}
    for k in range(1, nt + 1):
        sizes.update(min(lim, ENC_TILE * k + d) for d in (-1, 0, 1))
    for i, s in enumerate(sorted(sizes)):
        out.append(EncCase(f"size-{s}", O.gen(1 + i % 4, seed + i, s), "sizes"))
    # runs at the wave and round edges
    combos = [(L, side) for L in RUN_LENGTHS for side in SIDES]
    full = enc_full_edges(form)
    nrun = 0
    for k in enc_wave_edges(form):
        e = ENC_TILE * k
        for ci, (L, side) in enumerate(combos):
            if k not in full and (ci // 3 + ci % 3 + k) % 3:
                continue   # (one side per length, the sides rotating with the length and the edge)
            n = min(lim, e + 40)
            x = bytearray(O.gen(1, 97 * e + ci, n))
            lo, hi = _run_span(e, L, side)
            hi = min(hi, n)
            x[lo:hi] = (b"7" if nrun % 2 else b"\0") * (hi - lo)
            nrun += 1
            out.append(EncCase(f"edge-k{k}-L{L}-{side}", x, "edge", edge=k))
    # runs that carry a start into a round
    for r in range(1, R):
        e = ENC_TILE * ROUND * r
        for ph in range(9):
            n = lim if ph % 2 == 0 else min(lim, e + ENC_TILE + 37 + ph)
            x = bytearray(O.gen(1, seed + 7 * e + ph, n))
            x[e - ph:n] = (b"7" if ph % 2 else b"\0") * (n - e + ph)
            out.append(EncCase(f"carry-r{r}-ph{ph}", x, "carry", edge=ROUND * r))
    if R == 4:   # the second round without a run boundary: rmax stays the carried start
        e, end = ENC_TILE * ROUND, 2 * ENC_TILE * ROUND
        for ph in range(9):
            n = end + 2000
            x = bytearray(O.gen(1, seed + 31 + ph, n))
            x[e - ph:end + 3 + ph] = (b"\0" if ph % 2 else b"7") * (end + 3 + ph - e + ph)
            out.append(EncCase(f"round-ph{ph}", x, "round"))
    # inside one round: a run from mid-tile over whole tiles (their xch entries are 0)
    for r in range(R):
        base = ENC_TILE * ROUND * r
        spans = [(base + 500, base + min(ENC_TILE * W, 3 * ENC_TILE + 17))]
        if W >= 4:
            spans.append((base + ENC_TILE * (W - 3) + 500, base + ENC_TILE * W))
        for i, (lo, hi) in enumerate(spans):
            n = min(lim, hi + 40)
            x = bytearray(O.gen(1, seed + 57 + 2 * r + i, n))
            x[lo:hi] = (b"7" if (r + i) % 2 else b"\0") * (hi - lo)
            out.append(EncCase(f"span-r{r}-{i}", x, "span"))
    # staging extremes
    out.append(EncCase("staging-pairs-U", O.gen(4, seed + 1, lim), "staging"))
    out.append(EncCase("staging-pairs-U-1", O.gen(4, seed + 2, lim - 1), "staging"))
    out.append(EncCase("staging-exact-pairs-U", exact_pairs(lim), "staging"))
    out.append(EncCase("staging-exact-pairs-U-1", exact_pairs(lim - 1), "staging"))
    out.append(EncCase("staging-literals", no_equal_neighbours(seed + 3, lim), "staging"))
    out.append(EncCase("staging-zero", bytes(lim), "staging"))
    # digit-heavy alphabets
    rng = F._XorShift(seed + 5)
    for i in range(24):
        s = lim - i if i < 2 else 900 + rng.next() % (lim - 899)
        out.append(EncCase(f"digits-{i}-{s}", repeat_heavy(seed + 100 + i, s), "digits"))
    # past the form's tiles under its hint: the in-kernel one-wave walk
    out.append(EncCase("fallback-tiles", O.gen(2, seed + 9, lim + 1500), "fallback", fits=False))
    _enc_cache[form] = out
    return out


# ------------------------------------------------------------------ decode
class DecCase:
    """One decode input; check() of tests/test_gpu_stream_family.py reads stream, U, cap, serial.
    group: valid | tiles | edge | short | fallback; edge / p: the tile edge and stream position of an
    `edge` case; valid: encoder output with U its decoded length; fits: within the form."""
    __slots__ = ("label", "stream", "U", "cap", "serial", "group", "edge", "p", "valid", "fits")

    def __init__(self, label, stream, U, cap, serial, group, edge=None, p=None, valid=False, fits=True):
        self.label, self.stream, self.U, self.cap, self.serial = label, stream, U, cap, serial
        self.group, self.edge, self.p, self.valid, self.fits = group, edge, p, valid, fits

    def __repr__(self):
        return f"DecCase({self.label}, C={len(self.stream)}, U={self.U}, cap={self.cap}, serial={self.serial})"


def dec_edges(form):
    """Tile edges that take non-encoder streams: 1, the last wave edge, every round edge, the last
    tile edge."""
    W, _, R = form
    return sorted({1, W - 1, W * R - 1} | {ROUND * r for r in range(1, R)})


def dec_round_edges(form):
    return [ROUND * r for r in range(1, form[2])]


# carriers of this module's prefixes: literals with no equal neighbours, and "xx2" tokens whose
# values cycle over bytes that are no probe value and no filler
_X2_VALUES = (0x62, 0x33, 0x01, 0xFF, 0x37, 0x7A, 0x20, 0x81, 0x32, 0x0A, 0xB4)
_CAR_LEN = 100000
_cars = {}


def _car(kind):
    if kind not in _cars:
        if kind == "lit":
            _cars[kind] = no_equal_neighbours(4242, _CAR_LEN)
        else:
            _cars[kind] = b"".join(bytes((v, v, 0x32)) for v in _X2_VALUES) * (_CAR_LEN // 33 + 1)
    return _cars[kind]


def own_prefix(kind, p, v):
    """(bytes of exactly p, decoded length): valid tokens, aligned at the end, last byte != v.
    kind "lit": literals (C = U); "x2": "xx2" tokens then up to two filler literals (C = 1.5 U)."""
    car = _car(kind)
    if kind == "lit":
        out = bytearray(car[:p])
        if p and out[-1] == v:
            out[-1] = F._filler(out[-2] if p > 1 else -1, v)
        return bytes(out), p
    k, f = divmod(p, 3)
    out = bytearray(car[:3 * k])
    prev = -1
    for _ in range(f):
        prev = F._filler(prev)
        out.append(prev)
    return bytes(out), 2 * k + f


def mixed_stream(C, Umax, flip=False):
    """A valid stream of exactly C bytes decoding to at most Umax bytes: "xx2" tokens and literals,
    as few pairs as a seventh of the bytes where that fits.  (stream, U), or None when C > 1.5 Umax."""
    pairs = max(C - Umax, C // 7)
    if 3 * pairs > C:
        return None
    lits = C - 3 * pairs
    x2, lit = _car("x2")[:3 * pairs], _car("lit")
    if flip and lits:   # literals first; the last one differs from the first pair's value
        a = lit[:lits]
        if pairs and a[-1] == x2[0]:
            a = a[:-1] + bytes((F._filler(a[-2] if lits > 1 else -1, x2[0]),))
        y = a + x2
    else:
        o = 0
        while pairs and lits and lit[o] == x2[3 * pairs - 3]:
            o += 1
        y = x2 + lit[o:o + lits]
    return y, 2 * pairs + lits


_walks = {}


def _walk_rest(pi, v, tk):
    """(probe + tail bytes, N, bad) of probe pi with value v and the suffix of kind tk (None: no
    suffix), N by stream_family.walk."""
    key = (pi, v, tk)
    if key not in _walks:
        pb = F.probe(pi, v)
        rest = pb + (F.suffix(tk, pb[-1])[0] if tk is not None else b"")
        _walks[key] = (rest,) + F.walk(rest)
    return _walks[key]


def _own_edge_cases(form, k, p, overlong):
    """Cases at position p from this module's prefixes: all 16 probes, with and without a suffix
    where that fits.  overlong (an EXEMPT edge): U = Umax, Umax - 1 below the decoded length."""
    W, Umax, R = form
    clim = dec_limit(form)
    out = []
    for pi in range(F.NPROBES):
        v = F.VALUES[(pi + p) % len(F.VALUES)]
        for si in (0, 1):
            if pi >= 14 and si:
                continue   # the cut probes end the stream
            rot = pi + p + si
            kinds = ("lit", "x2") if rot % 2 else ("x2", "lit")
            tails = [None] if not si else [(1, 0, 3)[(rot + j) % 3] for j in range(3)]
            chosen = None
            for pk in (("x2",) if overlong else kinds):
                for tk in tails:
                    pre, npre = own_prefix(pk, p, v)
                    rest, n, bad = _walk_rest(pi, v, tk)
                    need = npre + (n if n is not None else 1)
                    if p + len(rest) <= clim and (overlong or need <= Umax):
                        chosen = (pk, tk, pre, npre, rest, n, bad)
                        break
                if chosen:
                    break
            if not chosen:
                continue
            pk, tk, pre, npre, rest, n, bad = chosen
            stream = pre + rest
            C = len(stream)
            if overlong:
                assert n is None or npre + n > Umax
                variants = [(Umax, Umax + C + 16), (Umax - 1, Umax - 1 + C + 16), (Umax, Umax)]
                N = None
            elif n is None:
                N = None
                variants = [(npre + 40, npre + 40 + C + 16), (npre + 1, npre + 1 + C + 16), (npre + 1, npre + 1)]
            else:
                N = npre + n
                exact = N - 1 if bad else N
                variants = [(U, U + C + 16) for U in (N, N - 1, N + 5)] + [(exact, exact)]
            for U, cap in variants:
                if U > Umax:
                    continue
                serial = overlong or bad or N is None or N > U
                out.append(DecCase(f"own-k{k}-p{p}-{pk}-probe{pi}-s{si}-U{U}-cap{cap}", stream, U, cap, serial,
                                   "edge", edge=k, p=p))
    return out


_dec_cache = {}


def dec_cases(form):
    """The decode cases of form (W, Umax, R), a list of DecCase (cached)."""
    if form in _dec_cache:
        return _dec_cache[form]
    W, Umax, R = form
    clim, nt = dec_limit(form), W * R
    exempt = EXEMPT.get(form, {})
    out = []

    def valid(label, y, U, group="valid"):
        out.append(DecCase(label, y, U, U, False, group, valid=True))

    # U = Umax and Umax - 1 from runs (few tiles); where W R tiles of "vv9" tokens decode to less,
    # the largest U they reach
    for name, byte in (("zero", b"\0"), ("nines", b"9")):
        top = Umax if len(O.encode(byte * Umax)) <= clim else clim // 3 * 9
        for U in (top, top - 1):
            valid(f"valid-{name}-U{U}", O.encode(byte * U), U)
    # C = 1008 W R and around every round edge
    for name, e in [(f"round{r // ROUND}", DEC_TILE * r) for r in dec_round_edges(form)] + [("limit", clim)]:
        for d in (-1, 0, 1):
            C = e + d
            if C > clim:
                continue
            m = mixed_stream(C, Umax, flip=d == 0)
            if m is None:
                assert name in exempt, (form, name, C)
                continue
            valid(f"valid-{name}{d:+d}-C{C}", m[0], m[1])
    # one stream for every tile count valid data can reach at this Umax
    for t in range(1, nt + 1):
        C = DEC_TILE * (t - 1) + 1 + t * 331 % (DEC_TILE - 1)
        C = min(C, Umax + Umax // 2)
        if C <= DEC_TILE * (t - 1):
            continue   # (unreachable tile counts: the "limit" exemption's tiles)
        y, U = mixed_stream(C, Umax, flip=t % 2 == 1)
        valid(f"tiles-{t}-C{C}", y, U, "tiles")
    # streams the encoder never emits, at the listed edges
    for k in dec_edges(form):
        overlong = k in exempt
        fams = {}
        for p in F.around(k * DEC_TILE):
            fams[p] = [] if overlong else [c for c in F.family(p) if len(c.stream) <= clim and c.U <= Umax]
        two_sided = any(c.serial for f in fams.values() for c in f) and \
            any(not c.serial for f in fams.values() for c in f)
        own = not two_sided or any(len(f) < 8 for f in fams.values())
        for p, fam in fams.items():
            for i, c in enumerate(fam):
                out.append(DecCase(f"fam-k{k}-p{p}-{i}", c.stream, c.U, c.cap, c.serial, "edge", edge=k, p=p))
            if own:
                out += _own_edge_cases(form, k, p, overlong)
    # A by-value launch selects its form from the stream's own C and U, and some forms' own range
    # holds few of the cases above or none: (4, 32768, 1) is at most 4 tiles with U past 16384, more
    # than 4 tiles decode to.  So up to 64 (the multi-round forms: 16) of the edge streams in the
    # form's range of C again, with U spread over the form's range of U (a U past the decoded
    # length: SHORT, or the last token's byte filling up to U).
    (_, _), (lo_in, lo_out) = DEC_HINTS[form]
    seen, src = set(), []
    for c in out:
        if c.group == "edge" and lo_in <= len(c.stream) <= clim and id(c.stream) not in seen:
            seen.add(id(c.stream))
            src.append(c)
    take = 64 if clim <= ROUND * DEC_TILE else 16   # (needs_serial walks in pure Python)
    for j, c in enumerate(src[::max(1, len(src) // take)][:take]):
        U = lo_out + j * 977 % (Umax - lo_out + 1)
        cap = U if j % 4 == 3 else U + len(c.stream) + 16
        out.append(DecCase(f"ownsize-{j}-k{c.edge}-p{c.p}-U{U}-cap{cap}", c.stream, U, cap,
                           F.needs_serial(c.stream, U), "ownsize"))
    # one-tile streams with U = Umax (SHORT): wave 0 alone through the fill loop and its barriers
    for C in (1, 500, DEC_TILE):
        out.append(DecCase(f"short-C{C}", _car("lit")[:C], Umax, Umax, False, "short"))
    # past the form under its hints: the in-kernel one-wave fallback in this form's LDS layout
    C = clim + 500
    pairs = C // 3
    y = _car("x2")[:3 * pairs] + bytes(F._FILL[:C - 3 * pairs])
    out.append(DecCase("fallback-tiles", y, 2 * pairs + C - 3 * pairs, 2 * pairs + C - 3 * pairs, False, "fallback",
                       valid=True, fits=False))
    U = Umax + 1000
    out.append(DecCase("fallback-U", O.encode(bytes(U)), U, U, False, "fallback", valid=True, fits=False))
    _dec_cache[form] = out
    return out
