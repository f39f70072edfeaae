"""GPU test: a device-resident store (tests/store_gpu.py) through twelve rounds of removals, creations,
write batches with evictions and read-N replies, every round run on the state the round before left
behind, against the host model (tests/store_model.py: the oracle codec and evict_model.loop_model).

After every round, byte for byte and word for word: every live row's stream, d_len, d_ulen, d_tail and
d_cap; every dead row's zeroed words (the dead-row duty of include/rle_mi355x.h); d_need, every status
word, the selection's summary, the whole victim buffer and d_keep; the eviction reply and the read-N
reply over their poison; currStorageSize; and the bytes no call may write: the source arena of a
compaction, the destination at and past *d_total, under grow everything but the slots written and
[dst_base, *d_total), and after a NOFIT round both arenas, every table and d_victims.  Every second
round both tail scans are run afresh over the current arena and held to the carried words.

The conditions on the inputs (rounds with evictions, NOFIT rounds, revived rows written, both forms,
partial relocations and forced compactions) are asserted on the CPU in tests/test_store_model.py."""
import numpy as np
import pytest
import torch

import readn_reply_gpu as G
import readn_reply_model as RM
import rle_mi355x as R
import store_gpu as D
import store_model as SM
from append_fit_gpu import POISON
from append_tail_model import word_of

pytestmark = pytest.mark.gpu
N = SM.N
FORM = RM.READN | RM.END


def host(t):
    return t.cpu().tolist()


def check_reply(label, got, reply, names, ulens):
    """One reply call's image, places, total and status words against the model's bytes."""
    d_out, place, total, st = got
    want_place, want_total = RM.layout(ulens, [len(p) for p in names], FORM)
    assert want_total == len(reply) and int(total.item()) == len(reply), label
    assert host(place) == want_place and host(st) == [0] * len(names), label
    img = d_out.cpu().numpy()
    assert img.size == len(reply) + G.SLACK
    bad = np.flatnonzero(img != G.image_of(reply, img.size))
    assert not len(bad), (label, f"{len(bad)} bytes differ, the first at {int(bad[0])} of {len(reply)}")


class Run:
    """One store on the device beside its model, with what the test carries from round to round: the
    victim buffer as it must stand and each arena's high-water mark."""

    def __init__(self, scenario):
        self.sc, self.s = scenario, scenario.store
        self.ds = D.DeviceStore(self.s)
        self.victims = [D.PAT32] * N
        self.high = [self.ds.used_hi, 0]
        self.seen = dict(evict=0, nofit=0, compacted=0, partial=0, created_evict=0)
        assert self.s.names == G.names(N)
        assert R.seg_segment_bytes(D.HINT) == G.SB     # the shortest segment: the large row is cut many times

    def snapshot(self):
        ds = self.ds
        return [a.clone() for a in ds.arenas], [t.clone() for t in ds.tables()], ds.cur

    def selection(self, label, summary, victims, want):
        assert summary == want.summary, label
        self.victims[:len(want.victims)] = want.victims
        assert victims == self.victims, label

    def round(self):
        ds, s, k = self.ds, self.s, self.s.k
        arenas0, tables0, cur0 = self.snapshot()
        rnd, om = SM.step(self.sc)          # the model goes first: s is now the state after the round
        label = (s.policy, self.sc.seed, k)
        ds.remove(rnd.removals)
        for row, want in om.created:
            got = ds.create(row)
            assert (got is None) == (want is None), label
            if want is not None:
                self.selection(label, got[0], got[1], want)
                self.seen["created_evict"] += 1
        if om.dropped:
            arenas0, tables0, cur0 = self.snapshot()   # (after the removals and creations)
        od = ds.write(rnd.writes, rnd.seg)
        torch.cuda.synchronize()
        # the size query and the selection
        assert host(od.need) == om.need and host(od.st_size) == [0] * N, label
        self.selection(label, od.summary, od.victims, om.sel)
        assert host(od.keep) == om.sel.keep and od.dropped == om.dropped, label
        if om.dropped:
            # nothing of a refused batch is stored: both arenas and every table are as they were
            self.seen["nofit"] += 1
            assert od.summary[0] == R.RLE_STATUS_NOFIT and ds.cur == cur0, label
            assert all(torch.equal(a, b) for a, b in zip(ds.arenas, arenas0)), label
            assert all(torch.equal(a, b) for a, b in zip(ds.tables(), tables0)), label
        else:
            self.written(label, rnd, om, od, arenas0, tables0)
        self.state(label)
        # the read-N reply of the round's subset
        names = [s.names[i] for i in rnd.reads]
        check_reply(label + ("read",), ds.read(rnd.reads, rnd.seg), om.read_reply, names,
                    [len(s.content[i]) for i in rnd.reads])
        if k % 2:
            self.rescans(label)

    def written(self, label, rnd, om, od, arenas0, tables0):
        ds, s = self.ds, self.s
        need, m = om.need, len(om.sel.victims)
        self.seen["evict"] += m > 0
        if m:
            check_reply(label + ("evicted",), od.reply, om.reply, [s.names[v] for v in om.reply_rows], om.reply_ulen)
        else:
            assert od.reply is None
        assert od.compacted == om.compacted and od.bound == om.bound, label
        assert host(od.st_reloc) == [0] * N and host(od.st_fit2) == [0] * N, label
        # (the second append asks nothing of a file that is done: A = 0 reports the length it has)
        assert host(od.need_fit2) == [c if lv else 0 for c, lv in zip(need, s.live)], label
        total = int(od.total.item())
        src, dst = ds.arenas[od.src], ds.arenas[od.dst]
        if om.compacted:
            self.seen["compacted"] += 1
            assert od.src != od.dst and total == sum(SM.r16(c) for c, lv in zip(need, s.live) if lv) <= od.bound, label
            assert torch.equal(src, arenas0[od.src]), label                   # the source arena is as it was
            assert torch.equal(dst[total:], arenas0[od.dst][total:]), label  # nothing at or past *d_total
        else:
            self.seen["partial"] += bool(om.moved)
            moved = [i for i in range(N) if i in om.moved]
            assert [i for i, x in enumerate(host(od.moved)) if x] == moved and od.base == om.dst_base, label
            assert host(od.st_fit) == [R.RLE_STATUS_NOFIT if i in moved else 0 for i in range(N)], label
            assert host(od.need_fit) == [c if lv else 0 for c, lv in zip(need, s.live)], label
            assert total == od.base + sum(SM.r16(need[i]) for i in moved) <= od.base + od.bound, label
            # only the slots written in place (up to their new length) and [dst_base, *d_total) may change
            may = np.zeros(dst.numel(), bool)
            may[od.base:total] = True
            off0 = host(tables0[0])
            for i, a in rnd.writes.items():
                if a and i not in moved:
                    may[off0[i]:off0[i] + need[i]] = True
            diff = (dst != arenas0[od.dst]).cpu().numpy() & ~may
            assert not diff.any(), (label, int(np.flatnonzero(diff)[0]))
            off, cap, cap0 = host(ds.d_off), host(ds.d_cap), host(tables0[2])
            for i in s.live_rows():
                if i not in moved:
                    assert off[i] == off0[i] and cap[i] == cap0[i], (label, i)
        # bytes no call has ever reached are still poison
        self.high[od.dst] = max(self.high[od.dst], total)
        assert bool((dst[self.high[od.dst]:] == POISON).all().item()), label

    def state(self, label):
        """Every row of the device tables, and every live stream, against the model's store."""
        ds, s = self.ds, self.s
        img = ds.arena.cpu().numpy()
        off, ln, cap, ul, tl, key, live = (host(t) for t in ds.tables())
        assert live == s.live and key == s.key, label
        for i in range(N):
            if not s.live[i]:
                assert (ln[i], ul[i], tl[i]) == (0, 0, 0), (label, i)   # the dead-row duty
                continue
            y = SM.enc(s.content[i])
            assert ln[i] == len(y) and ul[i] == len(s.content[i]) and tl[i] == word_of(y), (label, i)
            assert img[off[i]:off[i] + ln[i]].tobytes() == y, (label, i)
            assert cap[i] == s.cap[i] >= ln[i] and off[i] % 16 == 0 and off[i] + cap[i] <= ds.used_hi, (label, i)
            if s.policy == "compact":
                assert cap[i] == SM.r16(ln[i]), (label, i)
        curr = sum(ln[i] for i in range(N) if s.live[i])
        assert curr == s.curr() <= s.max_bytes and ds.count == sum(s.live) and ds.used_hi == s.used_hi, label
        if not self.sc.last.dropped:
            assert curr == self.sc.last.sel.summary[3], label               # currStorageSize

    def rescans(self, label):
        """Both tail scans, fresh, over the arena as it stands: the carried words of the live rows,
        and for a dead row what its zero length gives."""
        ds = self.ds
        for seg in (False, True):
            tail, ulen, st = ds.rescan(seg)
            torch.cuda.synchronize()
            assert host(st) == [0] * N, (label, seg)
            assert torch.equal(tail, ds.d_tail) and torch.equal(ulen, ds.d_ulen), (label, seg)


def lifetime(scenario):
    run = Run(scenario)
    for _ in range(SM.ROUNDS):
        run.round()
    return run


@pytest.mark.parametrize("seed", SM.SEEDS)
@pytest.mark.parametrize("policy", SM.POLICIES)
def test_random_rounds(policy, seed):
    lifetime(SM.Scenario(seed, policy))


@pytest.mark.parametrize("policy", SM.POLICIES)
def test_scripted_scenario(policy):
    """store_model.Scripted: evictions of m >= 2, a victim revived and written, A = 0 everywhere, every
    file written, a NOFIT round, a creation at max_files, all but one file removed, and writes to the
    store the evictions have emptied of all but the spared file."""
    run = lifetime(SM.Scripted(policy))
    assert run.seen["nofit"] >= 1 and run.seen["created_evict"] == 1 and run.seen["evict"] >= 2
    assert run.s.live_rows() == [SM.BIG]
