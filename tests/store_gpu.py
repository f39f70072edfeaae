"""The device driver of the store lifetime test (tests/test_gpu_store_lifetime.py): a store whose
streams stay compressed in one of two device arenas, driven round after round through the documented
call sequences of include/rle_mi355x.h.  Its host model is tests/store_model.py.

On the device: the arenas, the row tables d_off, d_len, d_cap, d_ulen, d_tail, d_key, d_live, and the
path table.  Sizes, offsets, tail words and decoded lengths never go to the host between rounds; the
one copy is the selection's summary and victim list, which the header prescribes.  What the host
keeps is what a server has anyway: the names (so which rows are live, and how many), the bytes it has
itself sent to each file (so the length of a reply, and an upper bound for a stream), and an upper
bound for the used end of the arena (store_model.grow_bound / compact_bound).  Removals, revivals, key
updates and masks are torch operations on the device tables.

Slot policies:
  compact  size -> select -> gather -> eviction reply -> relocate all survivors into the other arena
           (d_want = d_need, d_sel = d_keep) -> fit append with d_cap = d_new_cap
  grow     size -> select -> gather -> eviction reply -> fit append into the current slots -> relocate
           the NOFIT files to dst_base = the used end of the same arena -> second fit append; a full
           compaction (the sequence above) when the arena's room would be exceeded.  Victims' slots
           are abandoned until then.
seg=True takes the _seg entries for the tail rescan, the size query, the fit appends and the replies,
with one workspace of each kind allocated once.

Dead rows (the caller's duty, include/rle_mi355x.h, the eviction section): _kill sets d_len, d_ulen and
d_tail of every row that is not kept to 0 on the device, and a dead row gets no new bytes.  Nothing
else of a dead row is touched: its d_off and d_cap stay whatever they were."""
import types

import torch

import readn_reply_gpu as G
import rle_mi355x as R
import rle_oracle as O
import store_model as SM
from append_fit_gpu import DEV, POISON, Arena, i64

HINT = G.HINT   # total bytes of every _seg call: the shortest segment (4 tiles)
PAT32, PAT64 = 0x7777, -7
NOFIT = R.RLE_STATUS_NOFIT


def z64(k):
    return torch.full((k,), PAT64, dtype=torch.int64, device=DEV)


def z32(k):
    return torch.full((k,), PAT32, dtype=torch.int32, device=DEV)


class DeviceStore:
    def __init__(self, s):
        """From the model store `s` as it starts: the live streams packed into arena 0 in slots of
        r16(len), the tail words and decoded lengths from one scan on the device."""
        n = self.n = s.n
        self.policy, self.max_bytes, self.max_files, self.room = s.policy, s.max_bytes, s.max_files, s.room
        self.names, self.h_live, self.sent, self.k = list(s.names), list(s.live), list(s.sent), 0
        self.count = sum(s.live)
        ys = [O.encode(c) if lv else b"" for c, lv in zip(s.content, s.live)]
        offs, pos = [], 0
        self.arenas = [torch.full((self.room + 64,), POISON, dtype=torch.uint8, device=DEV) for _ in range(2)]
        for y in ys:
            offs.append(pos)
            if y:
                self.arenas[0][pos:pos + len(y)] = torch.frombuffer(bytearray(y), dtype=torch.uint8).to(DEV)
            pos += SM.r16(len(y))
        assert pos == s.used_hi <= self.room
        self.cur, self.used_hi = 0, pos
        self.d_off, self.d_len, self.d_cap = i64(offs), i64([len(y) for y in ys]), i64([SM.r16(len(y)) for y in ys])
        self.d_key = i64(s.key)
        self.d_live = torch.tensor(s.live, dtype=torch.int32, device=DEV)
        self.d_tail, self.d_ulen = z64(n), z64(n)
        R.tail_batch(self.arenas[0], self.d_off, self.d_len, self.d_tail, self.d_ulen)
        self.table = G.PathTable(self.names)
        self.keep, self.d_victims, self.summary = z32(n), z32(n), z64(R.RLE_EVICT_SUMMARY_WORDS)
        self.ws_app = R.append_seg_workspace(n, HINT, DEV)
        self.ws_tail = R.tail_seg_workspace(n, HINT, DEV)
        self.ws_dec = R.decode_packed_seg_workspace(n, HINT, DEV)

    @property
    def arena(self):
        return self.arenas[self.cur]

    def tables(self):
        return (self.d_off, self.d_len, self.d_cap, self.d_ulen, self.d_tail, self.d_key, self.d_live)

    # ---------------------------------------------------------------- rows that die and come back
    def _kill(self, keep):
        """The dead-row duty: every row with keep == 0 gets d_len = d_ulen = 0 and d_tail =
        RLE_TAIL_EMPTY; d_live = keep."""
        mask = keep.to(torch.int64)
        self.d_len.mul_(mask)
        self.d_ulen.mul_(mask)
        self.d_tail.mul_(mask)
        self.d_live.copy_(keep)

    def remove(self, rows):
        if not rows:
            return
        keep = self.d_live.clone()
        keep[torch.tensor(rows, device=DEV)] = 0
        self._kill(keep)
        for i in rows:
            assert self.h_live[i]
            self.h_live[i] = 0
        self.count -= len(rows)

    def create(self, row):
        """A dead row revived as an empty file; with the file count at max_files, openFileHandler's one
        victim first.  Returns (summary, victims) of that selection as the host read them, or None."""
        assert not self.h_live[row]
        got = None
        if self.max_files and self.count == self.max_files:
            R.evict_select(self.d_key, self.d_len, self.keep, self.d_victims, self.summary, live=self.d_live,
                           max_files=self.max_files - 1)
            got = self.summary.cpu().tolist(), self.d_victims.cpu().tolist()   # the one copy
            assert got[0][0] == R.RLE_STATUS_OK
            self._kill(self.keep)
            for v in got[1][:got[0][1]]:
                self.h_live[v] = 0
            self.count = got[0][5]
        self.d_live[row] = 1
        self.d_key[row] = SM.CLOCK + 60 * (self.k + 1)
        self.h_live[row], self.sent[row] = 1, 0
        self.count += 1
        return got

    # ---------------------------------------------------------------- replies and scans
    def _reply(self, d_s, off, clen, ulen, poff, plen, rows, seg):
        """The READN | END reply of `rows` (host row numbers: names and sent bytes) from the gathered
        device tables: (image, place, total, status) as the call left them."""
        cap = sum(20 + len(self.names[i]) + self.sent[i] for i in rows) + 10
        d_out = torch.full((cap + G.SLACK,), G.POISON, dtype=torch.uint8, device=DEV)
        place, total, st = z64(len(rows)), z64(1), z32(len(rows))
        form = R.RLE_REPLY_READN | R.RLE_REPLY_END
        if seg:
            R.readn_reply_seg(d_s, off, clen, ulen, self.table.d_paths, poff, plen, d_out, place, total, st, form=form,
                              out_cap=cap, total_in_bytes=HINT, ws=self.ws_dec)
        else:
            R.readn_reply(d_s, off, clen, ulen, self.table.d_paths, poff, plen, d_out, place, total, st, form=form,
                          out_cap=cap)
        return d_out, place, total, st

    def read(self, rows, seg):
        """The read-N reply of the live rows `rows`, their table rows picked on the device."""
        assert rows and all(self.h_live[i] for i in rows)
        idx = torch.tensor(rows, device=DEV)
        pick = lambda t: t.index_select(0, idx)   # noqa: E731
        return self._reply(self.arena, pick(self.d_off), pick(self.d_len), pick(self.d_ulen), pick(self.table.off),
                           pick(self.table.len), rows, seg)

    def rescan(self, seg):
        """A fresh tail scan of every row over the current arena: (tail, ulen, status)."""
        tail, ulen, st = z64(self.n), z64(self.n), z32(self.n)
        if seg:
            R.tail_batch_seg(self.arena, self.d_off, self.d_len, tail, ulen, st, total_in_bytes=HINT, ws=self.ws_tail)
        else:
            R.tail_batch(self.arena, self.d_off, self.d_len, tail, ulen, st)
        return tail, ulen, st

    # ---------------------------------------------------------------- one write batch
    def _size(self, d_s, nw, need, st, seg):
        a = (d_s, self.d_off, self.d_len, self.d_tail, nw.d_n, nw.d_noff, nw.d_nlen, need, st)
        if seg:
            R.append_size_seg(*a, total_new_bytes=HINT, workspace=self.ws_app)
        else:
            R.append_size(*a)

    def _fit(self, d_s, nw, nlen, need, st, seg):
        a = (d_s, self.d_off, self.d_len, self.d_cap, self.d_ulen, nw.d_n, nw.d_noff, nlen, need, st)
        if seg:
            R.append_fit_seg(*a, total_new_bytes=HINT, workspace=self.ws_app, tail=self.d_tail)
        else:
            R.append_fit(*a, tail=self.d_tail)

    def write(self, writes, seg):
        """The write batch {row: new bytes} of round self.k.  Returns what the calls left, for the test
        to compare: need, st_size, summary and victims (as the host read them), keep, dropped, reply
        (or None), compacted, and the statuses and needs of the relocation and the fit appends."""
        n = self.n
        news = [bytes(writes.get(i, b"")) for i in range(n)]
        assert all(self.h_live[i] for i in writes) and sum(map(len, news)) <= HINT
        nw = Arena([b""] * n, news, [0] * n, [0] * n, [0] * n)   # (the new bytes' arena only)
        src = self.arena
        o = types.SimpleNamespace(need=z64(n), st_size=z32(n), reply=None, dropped=False, compacted=False,
                                  src=self.cur, dst=self.cur, base=0, total=z64(1), st_reloc=z32(n),
                                  st_fit=None, need_fit=None, st_fit2=z32(n), need_fit2=z64(n), nw=nw)
        self._size(src, nw, o.need, o.st_size, seg)
        spare = (nw.d_nlen != 0).to(torch.int32)
        R.evict_select(self.d_key, self.d_len, self.keep, self.d_victims, self.summary, want=o.need, live=self.d_live,
                       spare=spare, max_bytes=self.max_bytes, max_files=self.max_files)
        o.summary, o.victims = self.summary.cpu().tolist(), self.d_victims.cpu().tolist()   # the one copy
        o.keep = self.keep.clone()
        if o.summary[0] != R.RLE_STATUS_OK:
            o.dropped = True      # the reference's E2BIG: nothing of the batch is stored
            self.k += 1
            return o
        m = o.summary[1]
        gone = o.victims[:m]
        if m:
            rows = [z64(m) for _ in range(5)]
            R.evict_gather(self.d_victims, self.summary,
                           [self.d_off, self.d_len, self.d_ulen, self.table.off, self.table.len], rows,
                           order=R.RLE_EVICT_ORDER_REPLY)
            o.reply = self._reply(src, *rows, gone[::-1], seg)
        self._kill(self.keep)
        for v in gone:
            self.h_live[v] = 0
        self.count = o.summary[5]
        written = [i for i in range(n) if news[i]]
        for i in written:
            self.sent[i] += len(news[i])
        new_off, new_cap = z64(n), z64(n)
        compacting = self.policy == "compact"
        if not compacting:
            bound = SM.grow_bound(o.summary, [self.sent[i] for i in written])
            compacting = self.used_hi + bound > self.room
        if compacting:
            bound = SM.compact_bound(o.summary)
            assert bound <= self.room
            dst = self.arenas[self.cur ^ 1]
            R.relocate_batch(src, self.d_off, self.d_len, dst, new_off, new_cap, o.total, want=o.need, sel=self.keep,
                             status=o.st_reloc, dst_base=0, dst_cap=bound)
            self.d_off.copy_(new_off)
            self.d_cap.copy_(new_cap)
            self._fit(dst, nw, nw.d_nlen, o.need_fit2, o.st_fit2, seg)
            self.cur ^= 1
            self.used_hi, o.compacted, o.dst = bound, True, self.cur
        else:
            o.st_fit, o.need_fit, o.base = z32(n), z64(n), self.used_hi
            assert self.used_hi % 16 == 0 and self.used_hi + bound <= self.room
            self._fit(src, nw, nw.d_nlen, o.need_fit, o.st_fit, seg)
            sel = (o.st_fit == NOFIT).to(torch.int32)
            R.relocate_batch(src, self.d_off, self.d_len, src, new_off, new_cap, o.total, want=o.need_fit, sel=sel,
                             status=o.st_reloc, dst_base=self.used_hi, dst_cap=self.used_hi + bound)
            moved = sel != 0
            self.d_off.copy_(torch.where(moved, new_off, self.d_off))
            self.d_cap.copy_(torch.where(moved, new_cap, self.d_cap))
            nlen2 = torch.where(moved, nw.d_nlen, torch.zeros_like(nw.d_nlen))   # (the others are done: A = 0)
            self._fit(src, nw, nlen2, o.need_fit2, o.st_fit2, seg)
            self.used_hi += bound
            o.moved = moved
        o.bound = bound
        now = torch.full_like(self.d_key, SM.CLOCK + 60 * (self.k + 1))
        self.d_key.copy_(torch.where(nw.d_nlen != 0, now, self.d_key))
        self.k += 1
        return o
