"""Host model of a device-resident store over its lifetime (tests/test_store_model.py,
tests/test_gpu_store_lifetime.py; the device side is tests/store_gpu.py).  Plain Python, no GPU.

A store of N rows, each with a name, a plain content, a live flag and a policy key.  The model is the
batched contract as include/rle_mi355x.h states it, put together from the oracle codec and
evict_model.loop_model; it derives nothing from the kernels.

One round (Round) is, in this order: removals, creations (a dead row revived as an empty file; when the
file count is at max_files the reference's openFileHandler evicts one victim first,
src/filesystemApi.c:477-480: the selection with max_files - 1 and no bytes limit), a write batch
{row: new bytes} (A = 0 allowed) and a read-N subset.  For the write batch, in this order:
  need_i = len(encode(x_i ‖ new_i)) for a live row, 0 for a dead one;
  the selection with want = need, spare = (A_i > 0), live, max_bytes and max_files;
  RLE_STATUS_NOFIT drops the whole batch and nothing changes (the reference's E2BIG);
  else the victims in eviction order, the eviction reply (READN | END, the victims last evicted
  first), the new contents and currStorageSize = summary[3].
For a round that writes exactly one file this is the reference's writeToFileHandler loop
(src/filesystemApi.c:772-814): newCompressedSize > maxStorageSize is E2BIG (no victim set can make it
fit, so the selection answers NOFIT), and otherwise getVictim(store, fptr) is called while
currStorageSize - contentSize + newCompressedSize > maxStorageSize.  tests/test_store_model.py holds the
model to a literal write-by-write restatement there.

Keys are last-write times: every file written (A > 0) or created in round k gets CLOCK + 60 * (k + 1), so
files of one round tie and the index decides among them.

The model also mirrors the two slot policies of the device driver, from host-side values alone (the
sizes stay on the device there): compact (every write round relocates all survivors to slots of
r16(need) in the other arena) and grow (fit into the current slots, the NOFIT files moved to the used
end, a full compaction when the arena's room would be exceeded).  grow_bound / compact_bound are the
upper bounds a host can know for the bytes a relocation takes: the selection's bytes-after word and the
bytes it has itself sent to each file.

Scenario: the seeded random round generator; Scripted: the one scripted scenario."""
import functools
from collections import namedtuple

import numpy as np

import evict_model as M
import readn_reply_model as RM
import rle_oracle as O
from append_tail_model import tail_of

N = 48
ROUNDS = 12
SIZES = (0, 1, 9, 100, 1500, 4096, 12000)   # new bytes per write
SEEDS = (1, 2, 3)
POLICIES = ("compact", "grow")
BIG = 39                                     # the row that starts past 64 KiB of content
CLOCK = 0x6530010000

Round = namedtuple("Round", "removals creations writes reads seg")


def r16(v):
    return (v + 15) & ~15


@functools.lru_cache(maxsize=16384)
def enc(x):
    return O.encode(x)


def max_compressed(u):
    """No stream of u content bytes is longer (a pair costs three bytes)."""
    return u + (u + 1) // 2


def compact_bound(summary):
    """The end of the slots of a full compaction, at most: r16 of every survivor's size."""
    return r16(summary[3] + 16 * summary[5])


def grow_bound(summary, sent):
    """The bytes the NOFIT files of a grow round take at most: `sent` holds, per file written with
    A > 0, the content bytes the host has sent to it so far, this write included."""
    return r16(min(summary[3] + 16 * len(sent), sum(r16(max_compressed(u)) for u in sent)))


def extends(x, new):
    """Whether an append of `new` to content x goes on with the stream's final token (the kernel's
    e > 0): the run continues and the token's count is below 9."""
    if not x or not new or new[0] != x[-1]:
        return False
    return tail_of(enc(x))[1] < 9


class Outcome:
    """What one round gave: created [(row, selection Result or None)], need, sel (the write batch's
    Result), reply (None without victims; reply_rows and reply_ulen: its files), dropped (NOFIT),
    read_reply, and the slot policy's
    decisions: compacted, moved (the rows of a partial relocation), dst_base, bound; the coverage
    counters extended / not_extended / revived_writes."""


class Store:
    def __init__(self, names, contents, live, keys, max_bytes, max_files=0, policy="compact", room=None):
        n = self.n = len(names)
        self.names, self.content, self.live, self.key = list(names), list(contents), list(live), list(keys)
        self.max_bytes, self.max_files, self.policy = max_bytes, max_files, policy
        assert all(lv or not c for lv, c in zip(live, contents))
        self.k = 0
        self.by_eviction = [False] * n     # the row's last death was an eviction
        self.revived = [False] * n         # a live row revived after an eviction
        # the slots, as far as the host knows them
        self.sent = [len(c) for c in contents]
        self.cap = [r16(c) for c in self.sizes()]
        self.used_hi = sum(self.cap)
        self.room = room if room is not None else 2 * r16(max_bytes + 16 * n) + 4096

    def sizes(self):
        return [len(enc(c)) if lv else 0 for c, lv in zip(self.content, self.live)]

    def curr(self):
        return sum(self.sizes())

    def live_rows(self):
        return [i for i in range(self.n) if self.live[i]]

    def dead_rows(self):
        return [i for i in range(self.n) if not self.live[i]]

    def _kill(self, i, evicted):
        assert self.live[i]
        self.live[i], self.content[i], self.by_eviction[i], self.revived[i] = 0, b"", evicted, False

    def apply(self, rnd):
        out = Outcome()
        n, now = self.n, CLOCK + 60 * (self.k + 1)
        for i in rnd.removals:
            self._kill(i, False)
        out.created = []
        for i in rnd.creations:
            assert not self.live[i]
            res = None
            if self.max_files and sum(self.live) == self.max_files:      # src/filesystemApi.c:477-480
                res = M.loop_model(self.key, self.sizes(), None, self.live, None, M.M64, self.max_files - 1)
                assert res.status == M.OK and len(res.victims) == 1
                self._kill(res.victims[0], True)
            self.live[i], self.key[i], self.sent[i] = 1, now, 0
            self.revived[i] = self.by_eviction[i]
            out.created.append((i, res))
        # the write batch
        new = [bytes(rnd.writes.get(i, b"")) for i in range(n)]
        assert all(self.live[i] for i in rnd.writes)
        lens = self.sizes()
        out.need = [len(enc(x + a)) if lv else 0 for x, a, lv in zip(self.content, new, self.live)]
        spare = [int(bool(a)) for a in new]
        out.sel = sel = M.loop_model(self.key, lens, out.need, self.live, spare, self.max_bytes, self.max_files)
        out.dropped = sel.status != M.OK
        out.reply, out.compacted, out.moved, out.dst_base, out.bound = None, False, [], 0, 0
        out.extended = out.not_extended = out.revived_writes = 0
        assert sel.status in (M.OK, M.NOFIT)
        if not out.dropped:
            sent = sel.victims[::-1]                                     # last evicted first
            out.reply_rows, out.reply_ulen = sent, [len(self.content[v]) for v in sent]
            if sent:
                out.reply = RM.reply([self.names[v] for v in sent], [self.content[v] for v in sent], RM.READN | RM.END)
            for v in sel.victims:
                self._kill(v, True)
            assert self.live == sel.keep
            written = [i for i in range(n) if new[i]]
            for i in written:
                if extends(self.content[i], new[i]):
                    out.extended += 1
                else:
                    out.not_extended += 1
                out.revived_writes += self.revived[i]
                self.content[i] += new[i]
                self.sent[i] += len(new[i])
                self.key[i] = now
            assert self.sizes() == [c if lv else 0 for c, lv in zip(out.need, self.live)]
            assert self.curr() == sel.summary[3] <= self.max_bytes
            self._slots(out, written)
        out.read_reply = RM.reply([self.names[i] for i in rnd.reads], [self.content[i] for i in rnd.reads],
                                  RM.READN | RM.END)
        assert all(self.live[i] for i in rnd.reads)
        self.k += 1
        return out

    def _slots(self, out, written):
        """The slot policy's step after a write batch that was not dropped."""
        need, summary = out.need, out.sel.summary
        if self.policy == "grow":
            out.bound = grow_bound(summary, [self.sent[i] for i in written])
            if self.used_hi + out.bound <= self.room:
                out.dst_base = self.used_hi
                out.moved = [i for i in written if need[i] > self.cap[i]]
                for i in out.moved:
                    self.cap[i] = r16(need[i])
                self.used_hi += out.bound
                return
        out.compacted = True
        out.bound = compact_bound(summary)
        assert out.bound <= self.room
        self.cap = [r16(c) if lv else 0 for c, lv in zip(need, self.live)]
        self.used_hi = out.bound


# ---------------------------------------------------------------- the stores and their rounds
def names(n):
    """n names of 1..40 bytes or so, every fifth a single byte: readn_reply_gpu.names, which this module
    cannot import without the GPU helpers (the GPU test holds the two to each other)."""
    out = []
    for i in range(n):
        if i % 5 == 0:
            out.append(bytes([0x41 + i % 26]))
        else:
            out.append(b"/srv/" + b"d%d/" % (i % 7) * (i % 4) + b"f%d" % (i * 2654435761 % 10 ** (1 + i % 9)))
    return out


def initial(seed, policy, live_rows=40, slack=None, max_files=42):
    """The store every run starts from: N rows of which the first live_rows are live, contents of 100
    to 3000 bytes of the kinds 0-4 and one row past 64 KiB, lastRef-like keys with ties, and max_bytes
    = the initial bytes plus `slack` (default: by seed, a few writes' worth)."""
    contents = []
    for i in range(N):
        if i >= live_rows:
            contents.append(b"")
        elif i == BIG:
            contents.append(O.gen(2, 7000 + seed, 70000 + seed))
        else:
            x = O.gen((i + seed) % 5, 300 + 50 * seed + i, 100 + (i * 1237 + seed * 311) % 2901)
            contents.append(x + bytes([0x61 + i % 3]) * (i % 11))
    live = [int(i < live_rows) for i in range(N)]
    keys = [0x6530000000 + (i * 29 + seed) % 17 * 60 for i in range(N)]
    keys[BIG] = CLOCK
    total = sum(len(enc(c)) for c in contents)
    slack = 36000 + 6000 * seed if slack is None else slack
    return Store(names(N), contents, live, keys, total + slack, max_files, policy)


class Scenario:
    """The seeded random rounds of one run: next(store) gives round store.k from the store's state."""

    def __init__(self, seed, policy):
        self.seed = seed
        self.rng = np.random.default_rng(1000 * seed + 17)
        self.store = initial(seed, policy)

    def new_bytes(self, row, k):
        j = row + k + self.seed
        return O.gen(j % 5, 900 + 31 * k + row + 1000 * self.seed, SIZES[(row + 2 * k + self.seed) % len(SIZES)])

    def next(self, s):
        rng, k = self.rng, s.k

        def pick(rows, c):
            return sorted(int(x) for x in rng.choice(rows, size=min(c, len(rows)), replace=False))

        live = [i for i in s.live_rows() if i != BIG]
        removals = pick(live, int(rng.integers(1, 3))) if rng.integers(0, 10) < 3 and len(live) > 8 else []
        # a victim of an eviction comes back before a row that was removed or never lived
        first = [i for i in s.dead_rows() if s.by_eviction[i]]
        rest = [i for i in s.dead_rows() if not s.by_eviction[i]]
        count = int(rng.integers(0, 3))
        # (below max_files: the scripted scenario has the creation that evicts)
        count = min(count, s.max_files - sum(s.live) + len(removals))
        creations = ((pick(first, count) if first else []) + (pick(rest, count) if rest else []))[:count]
        live = [i for i in range(N) if (s.live[i] and i not in removals) or i in creations]
        rows = pick(live, int(rng.integers(0, 8))) if k != 7 else list(live)   # round 7: nothing is eligible
        rows += [i for i in live if s.revived[i] and not s.content[i] and i not in rows]   # an empty revived file
        if k % 4 == 1 and s.live[BIG]:
            rows.append(BIG)
        writes = {i: self.new_bytes(i, k) for i in sorted(set(rows)) if i not in creations}
        if k % 4 == 1 and BIG in writes:
            writes[BIG] = O.gen(2, 40 + k + self.seed, 12000)
        return Round(removals, creations, writes, None, k % 2 == 1)

    def reads(self, s, rnd):
        """The read-N subset, drawn once the writes are known to have left these rows live."""
        live = s.live_rows()
        c = int(self.rng.integers(1, 9))
        rows = [int(x) for x in self.rng.choice(live, size=min(c, len(live)), replace=False)]
        if s.k % 3 == 2 and s.live[BIG] and BIG not in rows:
            rows.append(BIG)
        return rows


def run(scenario, rounds=ROUNDS):
    """Every round of a scenario on its own store: [(Round, Outcome)].  The read subset is drawn after
    the write batch (a victim cannot be read), so each round is applied in two steps."""
    out = []
    for _ in range(rounds):
        out.append(step(scenario))
    return out


def step(scenario):
    """One round: (Round, Outcome); the store moves on."""
    s = scenario.store
    rnd = scenario.next(s)
    o = scenario.last = s.apply(rnd._replace(reads=[]))
    reads = scenario.reads(s, rnd)
    rnd = rnd._replace(reads=reads)
    o.read_reply = RM.reply([s.names[i] for i in reads], [s.content[i] for i in reads], RM.READN | RM.END)
    assert all(s.live[i] for i in reads)
    return rnd, o


class Scripted:
    """The scripted scenario, twelve rounds; what each round must contain is asserted in
    tests/test_store_model.py from the outcomes:
      0  a write that evicts m >= 2 files
      1  the first victim revived as an empty file
      2  that row written
      3  A = 0 for every file
      4  every live file written (9 bytes): nothing is eligible, the model says NOFIT or fits
      5  every live file written (1500 incompressible bytes): NOFIT
      6  creations up to max_files and one more: exactly one file evicted
      7  every file but BIG removed
      8  three files created
      9  those three written
      10 BIG written until only it fits: every other file evicted
      11 a write to the store that holds the spared file alone"""

    seed = 0

    def __init__(self, policy):
        self.store = initial(0, policy, slack=3000, max_files=40)
        self.victim = None

    def next(self, s):
        k = s.k
        e = lambda: Round([], [], {}, None, k % 2 == 1)  # noqa: E731
        live = s.live_rows()
        if k == 0:
            return e()._replace(writes={5: O.gen(1, 11, 12000), 9: O.gen(1, 12, 4096)})
        if k == 1:
            self.victim = self.last.sel.victims[0]
            return e()._replace(creations=[self.victim], writes={9: O.gen(3, 13, 100)})
        if k == 2:
            return e()._replace(writes={self.victim: O.gen(2, 14, 1500), 9: O.gen(0, 15, 9)})
        if k == 3:
            return e()._replace(writes={5: b"", 9: b"", BIG: b""})
        if k == 4:
            return e()._replace(writes={i: O.gen(4, 100 + i, 9) for i in live})
        if k == 5:
            return e()._replace(writes={i: O.gen(1, 200 + i, 1500) for i in live})
        if k == 6:
            dead = s.dead_rows()
            return e()._replace(creations=dead[:s.max_files - len(live) + 1])
        if k == 7:
            return e()._replace(removals=[i for i in live if i != BIG])
        if k == 8:
            return e()._replace(creations=s.dead_rows()[:3])
        if k == 9:
            return e()._replace(writes={i: O.gen(1 + i % 4, 300 + i, 1500) for i in live if i != BIG})
        if k == 10:
            # the largest incompressible write after which BIG alone still fits
            gap = s.max_bytes - len(enc(s.content[BIG]))
            a = gap - 64
            while len(enc(s.content[BIG] + O.gen(1, 77, a))) > s.max_bytes:
                a -= 64
            return e()._replace(writes={BIG: O.gen(1, 77, a)})
        return e()._replace(writes={BIG: O.gen(0, 78, 9)})

    def reads(self, s, rnd):
        live = s.live_rows()
        return live[::5] + ([BIG] if s.k % 2 and BIG not in live[::5] else [])
