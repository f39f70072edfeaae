"""CPU self-checks of the cooperative forms' case builders (tests/coop_forms.py): every case fits
its form, the library's selector picks the form for the hints the GPU test passes, every listed edge
has its cases and both routing classes (or a counted exemption), and every valid case round-trips
through the oracle -- so a builder change cannot silently empty tests/test_gpu_coop_forms.py."""
import pytest

import coop_forms as CF
import rle_mi355x as R
import rle_oracle as O
import stream_family as F

_id = lambda f: "x".join(str(v) for v in f)


def test_form_lists_are_the_selectors():
    import test_coop_form as T
    assert CF.ENC_FORMS == T.ENC_FORMS and CF.DEC_FORMS == T.DEC_FORMS
    assert sorted(CF.DEC_HINTS) == sorted(CF.DEC_FORMS)


# ------------------------------------------------------------------ encode
@pytest.mark.parametrize("form", CF.ENC_FORMS, ids=_id)
def test_encode_cases(form):
    W, Rr = form
    lim, nt = 1024 * W * Rr, W * Rr
    cases = CF.enc_cases(form)
    assert cases is CF.enc_cases(form)
    hi, lo = CF.enc_hints(form)
    assert hi == lim and R.coop_enc_form(hi) == form and R.coop_enc_form(lo) == form
    assert R.coop_enc_form(lo - 1) != form and R.coop_enc_form(hi + 1) != form
    assert len({c.label for c in cases}) == len(cases)
    by = {}
    for c in cases:
        by.setdefault(c.group, []).append(c)
        assert c.fits == (len(c.data) <= lim), c
        y = O.encode(c.data)
        x, st = O.decode(y, len(c.data))
        assert x == c.data and st == 0, c
    assert [len(c.data) for c in by["fallback"]] == [lim + 1500]
    # sizes
    want = {0, 1} | {min(lim, 1024 * k + d) for k in range(1, nt + 1) for d in (-1, 0, 1)}
    assert {len(c.data) for c in by["sizes"]} == want and len(by["sizes"]) == len(want)
    # edges: every wave edge, the cross product at 1, W - 1 and the round edges
    edges = list(range(1, nt))
    full = sorted({1, W - 1} | {16 * r for r in range(1, Rr)})
    assert CF.enc_wave_edges(form) == edges and CF.enc_full_edges(form) == full
    assert len(CF.RUN_LENGTHS) == 12 and {8, 9, 10, 17, 18, 19, 27, 28} <= set(CF.RUN_LENGTHS)
    for k in edges:
        cs = [c for c in by["edge"] if c.edge == k]
        assert len(cs) == (36 if k in full else 12), (k, len(cs))
        assert {c.label.split("-")[3] for c in cs} == set(CF.SIDES), k
        e, bytes_seen = 1024 * k, set()
        for c in cs:
            L, side = int(c.label.split("-")[2][1:]), c.label.split("-")[3]
            lo_, hi_ = CF._run_span(e, L, side)
            hi_ = min(hi_, len(c.data))
            run = c.data[lo_:hi_]
            assert lo_ <= e <= hi_ and len(set(run)) == 1 and run[0] in (0x37, 0), c
            assert (side == "ends") == (hi_ == e) and (side == "starts") == (lo_ == e), c
            bytes_seen.add(run[0])
        assert bytes_seen == {0x37, 0}, k
    # carried starts
    carry = by.get("carry", [])
    assert len(carry) == 9 * (Rr - 1)
    for c in carry:
        r, ph = int(c.label.split("-")[1][1:]), int(c.label.split("-")[2][2:])
        e = 16384 * r
        assert len(set(c.data[e - ph:])) == 1 and len(c.data) > e, c
    assert any(len(c.data) == lim for c in carry) or Rr == 1
    rounds = by.get("round", [])
    assert len(rounds) == (9 if Rr == 4 else 0)
    for c in rounds:
        ph = int(c.label.split("ph")[1])
        assert len(set(c.data[16384 - ph:32768 + 3 + ph])) == 1 and len(c.data) > 32768 + 3 + ph + 1000, c
    spans = by["span"]
    assert len(spans) == Rr * (2 if W >= 4 else 1)
    for c in spans:   # a run from mid-tile over whole tiles: two where the round has four tiles
        r = int(c.label.split("-")[1][1:])
        base = 16384 * r
        runs, i = [], base
        while i < len(c.data):
            j = i
            while j < len(c.data) and c.data[j] == c.data[i]:
                j += 1
            runs.append((i, j))
            i = j
        lo_, hi_ = max(runs, key=lambda t: t[1] - t[0])
        whole = hi_ // 1024 - (lo_ + 1023) // 1024
        assert lo_ % 1024 != 0 and whole >= (2 if W >= 4 else W - 1), (c, lo_, hi_)
    # staging extremes
    st = {c.label: c.data for c in by["staging"]}
    assert len(O.encode(st["staging-exact-pairs-U"])) == lim * 3 // 2
    assert len(O.encode(st["staging-exact-pairs-U-1"])) == (lim - 2) * 3 // 2 + 1
    assert len(st["staging-pairs-U"]) == lim and len(st["staging-pairs-U-1"]) == lim - 1
    assert len(O.encode(st["staging-pairs-U"])) > lim
    assert len(st["staging-literals"]) == lim and len(O.encode(st["staging-literals"])) == lim
    assert st["staging-zero"] == bytes(lim)
    assert len(by["digits"]) == 24 and max(len(c.data) for c in by["digits"]) == lim
    # the by-value launches select a form from the buffer's own size: enough cases of this form's own
    own = [c for c in cases if R.coop_enc_form(len(c.data)) == form]
    assert len(own) >= 40 and len({c.group for c in own}) >= 4, len(own)
    sample = CF.rotating_sample(own, lambda c: c.group, 40, CF.ENC_FORMS.index(form))
    assert len(sample) == 40 and len(set(map(id, sample))) == 40, len(sample)
    assert {c.group for c in sample} == {c.group for c in own}
    print(f"encode form {form}: {len(cases)} cases, {len(own)} in the form's own size range, "
          f"{sum(len(c.data) for c in cases)} bytes")


# ------------------------------------------------------------------ decode
def _expected_dec_edges(form):
    W, _, Rr = form
    return sorted({1, W - 1, W * Rr - 1} | {16 * r for r in range(1, Rr)})


@pytest.mark.parametrize("form", CF.DEC_FORMS, ids=_id)
def test_decode_cases(form):
    W, Umax, Rr = form
    clim, nt = 1008 * W * Rr, W * Rr
    cases = CF.dec_cases(form)
    assert cases is CF.dec_cases(form)
    (hi_in, hi_out), (lo_in, lo_out) = CF.dec_hints(form)
    assert (hi_in, hi_out) == (clim, Umax)
    assert R.coop_dec_form(hi_in, hi_out) == form and R.coop_dec_form(lo_in, lo_out) == form
    assert R.coop_dec_form(lo_in - 1, lo_out) != form or lo_in == 1009
    assert R.coop_dec_form(lo_in, lo_out - 1) != form or lo_out == 1
    assert len({c.label for c in cases}) == len(cases)
    exempt = CF.EXEMPT.get(form, {})
    by = {}
    for i, c in enumerate(cases):
        by.setdefault(c.group, []).append(c)
        C = len(c.stream)
        assert c.fits == (C <= clim and c.U <= Umax), c
        assert c.cap >= c.U >= 0, c
        out, st = O.decode(c.stream, c.U, c.cap)
        assert st == 0 or c.cap == c.U, c
        if c.valid:
            assert not c.serial and st == 0 and c.cap == c.U and O.encode(out) == c.stream, c
        if c.group != "edge" or i % 13 == 0:   # (the walk is pure Python)
            assert F.needs_serial(c.stream, c.U) == c.serial, c
    # the limits
    vs = {c.label: c for c in by["valid"]}
    top = max(c.U for c in by["valid"])
    assert top == Umax or top == clim // 3 * 9 < Umax
    assert {c.U for c in by["valid"] if c.label.startswith("valid-zero")} == {top, top - 1}
    for name, e in [(f"round{r}", 16128 * r) for r in range(1, Rr)] + [("limit", clim)]:
        got = sorted(len(c.stream) for l, c in vs.items() if l.startswith(f"valid-{name}-") or
                     l.startswith(f"valid-{name}+"))
        if e > Umax + Umax // 2:
            assert name in exempt and not got, (name, got)
        else:
            assert name not in exempt and got == [C for C in (e - 1, e, e + 1) if C <= clim], (name, got)
    reach = min(nt, (Umax + Umax // 2 + 1007) // 1008)
    assert sorted((len(c.stream) + 1007) // 1008 for c in by["tiles"]) == list(range(1, reach + 1))
    assert reach == nt or "limit" in exempt
    # the edges
    assert CF.dec_edges(form) == _expected_dec_edges(form)
    for k in _expected_dec_edges(form):
        cs = [c for c in by["edge"] if c.edge == k]
        for p in range(1008 * k - 4, 1008 * k + 3):
            at = [c for c in cs if c.p == p]
            assert len(at) >= 8, (k, p, len(at))
            for c in at[::5]:
                pb = c.stream[p:p + 2]
                assert p + 1 <= len(c.stream) and c.stream[p - 1] != pb[0], c
        assert any(c.serial for c in cs), k
        if k in exempt:
            assert 672 * k > Umax and not any(not c.serial for c in cs), k
        else:
            assert any(not c.serial for c in cs), k
        # all 16 probes at the edge (the byte at p is a probe value)
        assert {c.stream[c.p] for c in cs} <= set(F.VALUES), k
    assert sorted(k for k in exempt if k != "limit" and not str(k).startswith("round")) == \
        [k for k in _expected_dec_edges(form) if 672 * k > Umax]
    # short streams and the fallback
    assert sorted(len(c.stream) for c in by["short"]) == [1, 500, 1008] and all(c.U == Umax for c in by["short"])
    fb = {c.label: c for c in by["fallback"]}
    assert (len(fb["fallback-tiles"].stream) + 1007) // 1008 > nt
    assert fb["fallback-U"].U > Umax   # (within the form's tiles where 9 W R tiles of runs pass Umax)
    assert len(fb["fallback-U"].stream) <= clim or 3 * clim < Umax + 1000
    assert [c for c in cases if not c.fits] == by["fallback"]
    # the by-value launches select a form from the stream's own sizes: enough cases, both classes
    own = [c for c in cases if R.coop_dec_form(len(c.stream), c.U) == form]
    assert len(own) >= 40 and any(c.serial for c in own) and any(not c.serial for c in own), len(own)
    sample = CF.rotating_sample(own, lambda c: (c.group, c.serial), 40, CF.DEC_FORMS.index(form))
    assert len(sample) == 40 and len(set(map(id, sample))) == 40
    assert {(c.group, c.serial) for c in sample} == {(c.group, c.serial) for c in own}
    nser = sum(c.serial for c in cases)
    print(f"decode form {form}: {len(cases)} cases ({nser} serial-class), {sum(len(c.stream) for c in cases)} "
          f"stream bytes, own-prefix {sum(c.label.startswith('own-') for c in cases)}, {len(own)} in the form's own "
          f"size range")


def test_exemptions_are_counted():
    """Three forms have places no stream reaches within Umax (coop_forms.EXEMPT): one tile edge and
    the stream limit each."""
    assert sorted(CF.EXEMPT) == [(8, 4096, 1), (16, 16384, 2), (16, 32768, 4)]
    assert sum(len(v) for v in CF.EXEMPT.values()) == 6
    assert {k for v in CF.EXEMPT.values() for k in v if k != "limit"} == {7, 31, 63}


def test_family_is_unchanged_by_the_builders():
    a = [(c.stream, c.U, c.cap) for c in F.family(16 * F.TILE)]
    CF.dec_cases((16, 16384, 2))
    assert [(c.stream, c.U, c.cap) for c in F.family(16 * F.TILE)] == a
