"""CPU pins of the decode stream family (tests/stream_family.py): the generator's invariants, its
routing rule against an independent brute-force walk, the oracle against the compiled reference
on every case (where oracle/_ref was built), and the committed sha256 pins (taken from the compiled
reference by tests/golden/make_golden.py) against the oracle's outputs -- the same pins the GPU
tests check their device outputs against."""
import json
import os
import re

import pytest

import rle_oracle as O
import stream_family as F
from conftest import GOLDEN

HAVE_REF = os.path.exists(O.REF_SO)
_TOKEN = re.compile(rb"(.)\1(.)?|.", re.S)
_PAIR = re.compile(rb"(.)\1(.)?", re.S)


def _pins():
    with open(os.path.join(GOLDEN, "stream_family.json")) as f:
        return json.load(f)


def _brute_serial(y, us):
    """Independent of stream_family.walk: the pair tokens by regular expression (the leftmost match
    from a token boundary is the next pair token in phase; the bytes before it are literals, and a
    last lone 0x00's fill writes zeros over zeros), the decoded length by the reference's own capped
    loop (a count clipped at U, or an output index past U, is N > U), for every U of `us` in one
    pass over the stream.  Returns one flag per U."""
    os_ = [0] * len(us)
    clipped = [False] * len(us)
    bad = False
    prev = 0
    for m in _PAIR.finditer(y):
        lit = m.start() - prev + 1   # the literals before the pair, and the pair's first byte
        prev = m.end()
        d = m.group(2)
        if d is None or not b"2" <= d <= b"9":
            bad = True
        x = (d[0] if d else 0)
        occ = (x - 256 if x >= 128 else x) - 48
        extra = (1 << 62) if occ < 0 else max(occ - 1, 0)
        for k, U in enumerate(us):
            o = os_[k] + lit
            room = max(U - o, 0)
            if extra > room:
                clipped[k] = True
            os_[k] = o + min(extra, room)
    tail = len(y) - prev
    return [bad or c or o + tail > U for c, o, U in zip(clipped, os_, us)]


_walked, _overflowed = set(), set()


def _sample(p):
    """The cases of position p that the pure-Python walks (needs_serial, _overflows) visit: all of
    them for short streams, every 7th or 13th (every U variant of the 3- and 4-case streams in turn)
    for longer ones.  The regex walk _brute_serial visits every case."""
    fam = F.family(p)
    return fam if p < 1100 else fam[::7] if p < 60000 else fam[::13]


def _groups():
    g = {("wave", k): v for k, v in F.WAVE_GROUPS.items()}
    g.update({("coop", k): v for k, v in F.COOP_GROUPS.items()})
    g[("seg", "four-launch")] = F.seg_positions(F.SEG)
    g[("seg", "resident")] = F.seg_positions(F.SEG_RES)
    for w in (4, 8, 16):
        g[("round", str(w))] = F.round_positions(w)
    for m in F.SEG_TILES_BETWEEN:
        g[("seg", "%02d-tiles" % m)] = F.seg_length_positions(m)
    return g


def test_generator_invariants():
    for p in F.all_positions():
        fam = F.family(p)
        assert fam, p
        for c in fam:
            pb = F.probe(c.probe, c.value)
            assert c.stream[p:p + len(pb)] == pb, c
            assert p == 0 or c.stream[p - 1] != c.value, c
            assert c.cap in (c.U, c.U + len(c.stream) + 16) and c.U >= 0, c
            rest = c.stream[p + len(pb):]
            assert not rest or (len(rest) > F.TILE and rest[0] != pb[-1]), c
    # the prefixes are valid canonical streams of exactly p bytes: the oracle's encoder reproduces them
    for kind in range(F.NKINDS):
        for p in (0, 1, 2, 17, 1007, 1008, F.SEG_RES + 1, F.SEG - 1, 2 * F.SEG + 2):
            for v in F.VALUES:
                pre, n = F.prefix(kind, p, v)
                x, st = O.decode(pre, n, n)
                assert len(pre) == p and st == 0 and O.encode(x) == pre and F.walk(pre) == (n, False), (kind, p, v)
    assert F.family(1008) is F.family(1008)
    h = F.pin(F.family(13), [bytes(c.cap) for c in F.family(13)])
    assert h == "%s" % h and len(h) == 64


def test_family_is_stable():
    """The generator is pinned: a change to it shows up here before it shows up as a pin mismatch."""
    fam = F.family(1008)
    import hashlib
    h = hashlib.sha256()
    for c in fam:
        h.update(c.stream + c.U.to_bytes(8, "little") + c.cap.to_bytes(8, "little"))
    assert h.hexdigest() == _pins()["family_1008"], h.hexdigest()


@pytest.mark.parametrize("group", sorted(_groups()), ids=lambda g: "-".join(g))
def test_routing_rule_and_mix(group):
    """needs_serial against the brute-force walk and the generator's own classification; at least
    20 % of every group is tiled-class (so a decoder that declined everything cannot pass the GPU
    tests' routing condition vacuously, and a generator edit cannot drift to all-serial)."""
    positions = _groups()[group]
    cs = F.cases(positions)
    for p in positions:
        if p in _walked:
            continue   # (the groups share positions)
        _walked.add(p)
        fam, i = F.family(p), 0
        while i < len(fam):     # every case against the brute-force walk, a stream's U variants together
            j = i
            while j < len(fam) and fam[j].stream is fam[i].stream:
                j += 1
            assert [c.serial for c in fam[i:j]] == _brute_serial(fam[i].stream, [c.U for c in fam[i:j]]), fam[i]
            i = j
        for c in _sample(p):    # needs_serial itself walks in pure Python
            assert F.needs_serial(c.stream, c.U) == c.serial, c
    tiled = sum(not c.serial for c in cs)
    assert 5 * tiled >= len(cs), (group, tiled, len(cs))
    for p in positions:   # and no position is one-sided
        fam = F.family(p)
        assert any(c.serial for c in fam) and any(not c.serial for c in fam), p


def test_lone_final_zero_is_tiled():
    assert not F.needs_serial(b"ab\0", 3) and not F.needs_serial(b"ab\0", 9) and F.needs_serial(b"ab\0", 2)
    assert F.needs_serial(b"ab\0\0", 9) and F.needs_serial(b"aa", 9) and not F.needs_serial(b"aa2a", 3)
    assert F.needs_serial(b"aa1", 9) and F.needs_serial(b"aa:", 99) and F.needs_serial(b"aa\xb5", 99)
    assert F.walk(b"aa\x7f") == (79, True) and F.walk(b"aa0b") == (2, True) and F.walk(b"aa/")[0] is None


def _windows():
    """Every -4..+2 (or -2..+1) window of consecutive positions of every group."""
    out = set()
    for positions in _groups().values():
        run = [positions[0]]
        for p in positions[1:] + [None]:
            if p is not None and p == run[-1] + 1:
                run.append(p)
            else:
                out.add(tuple(run))
                run = [p]
    return sorted(out)


@pytest.mark.parametrize("window", _windows(), ids=lambda w: f"{w[0]}-{w[-1]}")
def test_every_window_sees_every_class(window):
    """Across each edge's window of positions: all 16 probes, every value, every prefix kind, both
    suffix settings -- and every non-cut probe with a suffix and without one, so that at every edge
    every class of token is followed both by the stream's end and by another tile."""
    seen = set()
    for p in window:
        for c in F.family(p):
            seen.add((c.probe, c.value, c.kind, len(c.stream) > p + len(F.probe(c.probe, c.value))))
    assert {s[0] for s in seen} == set(range(F.NPROBES)), window
    assert {s[1] for s in seen} == set(F.VALUES) and {s[2] for s in seen} == set(range(F.NKINDS)), window
    for pi in range(14):
        assert {s[3] for s in seen if s[0] == pi} == {False, True}, (window, pi)
    assert not any(s[3] for s in seen if s[0] >= 14)


@pytest.mark.parametrize("group", sorted(_groups()), ids=lambda g: "-".join(g))
def test_oracle_equals_reference_and_pins(group):
    """The oracle's decode of every case equals the compiled reference's (where it was built; the
    reference runs with E = C + 16 -- with E = 0 it would write outside its block -- and a cap = U
    case compares its first U bytes), and the committed pins, taken from the compiled reference,
    match the oracle's outputs."""
    pins = _pins()["positions"]
    for p in _groups()[group]:
        fam = F.family(p)
        outs = []
        for c in fam:
            out, st = O.decode(c.stream, c.U, c.cap)
            outs.append(out)
            if HAVE_REF:
                ref = O.ref_decompress(c.stream, c.U, len(c.stream) + 16)
                assert out == ref[:c.cap], c
            # (cap = U + C + 16 holds every write: only the cap = U cases can overflow)
            assert st == 0 or c.cap == c.U, c
        if p not in _overflowed:
            _overflowed.add(p)
            for c in _sample(p):
                assert O.decode(c.stream, c.U, c.cap)[1] == (1 if c.cap == c.U and _overflows(c) else 0), c
        assert F.pin(fam, outs) == pins[str(p)], p


def _overflows(c):
    """The reference's loop reaches an output index >= cap with stream bytes left (independent of
    the oracle: tokens by regular expression)."""
    o = 0
    for m in _TOKEN.finditer(c.stream):
        if o >= c.cap:
            return True
        o += 1
        if m.group(1) is not None:
            d = m.group(2)
            x = d[0] if d else 0
            occ = (x - 256 if x >= 128 else x) - 48
            o += min((1 << 62) if occ < 0 else max(occ - 1, 0), max(c.U - o, 0))
    return False
