"""CPU tests of the segmented packed decode's store model (tests/readn_pack_seg_model.py): for every
destination phase, every phase of the first segment boundary and segment outputs of 0..48 bytes, no
wide store leaves its segment, the writes cover the file exactly, and nothing is written twice with
files abutting on both sides.  No GPU."""
import readn_pack_model as M
import readn_pack_seg_model as S

SIZES = range(49)
LAST = (0, 1, 2, 15, 16, 17, 31, 33, 48)   # the third segment's output (the first two take every size)
NEIGHBOUR = (1, 15, 16, 17, 40)            # lengths of the files in front and behind


def _files():
    """(p, offs, U): head = p % 16 over 0..15, three segments whose first two outputs take every size
    0..48, so that the first inner boundary lands on every phase for every head."""
    for head in range(16):
        p = 64 + head
        for s0 in SIZES:
            for s1 in SIZES:
                for s2 in LAST:
                    yield p, [0, s0, s0 + s1], s0 + s1 + s2


def test_entry_state():
    """A segment enters at head + off: its first stored chunk starts at that position rounded down,
    and the bytes below it in that chunk are the previous segment's (or another file's)."""
    for head in range(16):
        assert S.entry(head, 0) == (head, 0)   # the packed decode's own entry
        for off in range(100):
            sh, fl = S.entry(head, off)
            assert fl % 16 == 0 and 0 <= sh < 16 and fl + sh == head + off


def test_every_head_and_boundary_phase_is_visited():
    seen = {(p % 16, (p + offs[1]) % 16) for p, offs, _ in _files()}
    assert seen == {(h, b) for h in range(16) for b in range(16)}
    assert any(offs[1] == offs[2] for _, offs, _ in _files())   # segments that decode to nothing
    assert any(offs[1] == 0 for _, offs, _ in _files())


def test_no_wide_store_leaves_its_segment():
    for p, offs, U in _files():
        ends = offs[1:] + [U]
        for (head, chunks, tail), off, end in zip(S.segment_stores(p, offs, U), offs, ends):
            assert all(c % 16 == 0 and p + off <= c and c + 16 <= p + end for c in chunks), (p, offs, U)
            assert len(head) < 16 and len(tail) < 16
            assert all(p + off <= b < p + end for b in head + tail), (p, offs, U)


def test_writes_cover_the_file_exactly_once():
    for p, offs, U in _files():
        count = {}
        for head, chunks, tail in S.segment_stores(p, offs, U):
            for b in head + tail + [c + j for c in chunks for j in range(16)]:
                count[b] = count.get(b, 0) + 1
        assert sorted(count) == list(range(p, p + U)), (p, offs, U)
        assert set(count.values()) <= {1}, (p, offs, U)


def test_abutting_files_on_both_sides():
    """A file in front that ends at p and one behind that starts at p + U, segmented themselves: over
    the three files every byte is written once, and no wide store of one file holds a byte of
    another."""
    for p, offs, U in _files():
        if offs[1] % 7 or (offs[2] - offs[1]) % 5:   # (a sixteenth of the files: every head, 8 x 10 sizes)
            continue
        for n0 in NEIGHBOUR:
            for n1 in NEIGHBOUR:
                files = [(p - n0, [0, n0 // 2], n0), (p, offs, U), (p + U, [0, n1 // 3, n1 // 3], n1)]
                count = {}
                for q, o, u in files:
                    for head, chunks, tail in S.segment_stores(q, o, u):
                        wide = [c + j for c in chunks for j in range(16)]
                        assert all(q <= b < q + u for b in wide), (files,)
                        for b in head + tail + wide:
                            count[b] = count.get(b, 0) + 1
                assert sorted(count) == list(range(p - n0, p + U + n1)), (files,)
                assert set(count.values()) == {1}, (files,)


def test_one_segment_is_the_file_model():
    for p in range(32, 48):
        for U in range(49):
            assert S.segment_stores(p, [0], U) == [M.stores(p, U)]
