"""Launch helper of the GPU tests of the append's size and fit entries (tests/test_gpu_append_fit*.py).

The arenas differ from append_tail_gpu.Files in what the fit forms are about: slots are laid out by
the capacity GIVEN for each file, packed 16-byte aligned with nothing between them, so the bytes
right behind a slot's capacity are the next file's stream or poison; every byte outside a stream is
0xEE, the bytes between a capacity and the next slot included; the new-content arena has 16 bytes of
the stored stream's final byte in front of every buffer (the virtual buffer's head positions, never
read) and repeats each file's last new byte behind it.  The whole image is compared after every
launch, with d_len, d_ulen, d_tail, d_need and the statuses."""
import numpy as np
import torch

import append_fit_model as F
import append_tail_model as M
import rle_mi355x as R
import rle_oracle as O

DEV = "cuda:0"
POISON = 0xEE
HEAD = 16
FORMS = ("size", "fit", "plain", "size_seg", "fit_seg")
NEED_POISON, STATUS_POISON = 0x4444444444, 0x7777


def i64(v):
    return torch.tensor(np.asarray(v, dtype=np.uint64).astype(np.int64), device=DEV)


def r16(v):
    return (v + 15) & ~15


class Arena:
    """The device state of one set of files, and one launch of any form over it."""

    def __init__(self, ys, news, words, caps, ulens, shifts=None, sshifts=None):
        n = len(ys)
        self.n, self.ys, self.news, self.words, self.caps, self.ulens = n, ys, news, words, caps, ulens
        shifts, sshifts = shifts or [0] * n, sshifts or [0] * n
        self.soffs, pos = [], 0
        for y, cap, sh in zip(ys, caps, sshifts):
            self.soffs.append(pos + sh)
            pos = r16(pos + sh + max(cap, len(y)))
        self.img = np.full(pos + 64, POISON, np.uint8)
        for y, o in zip(ys, self.soffs):
            self.img[o:o + len(y)] = np.frombuffer(y, np.uint8)
        noffs, ntotal = R.layout([HEAD + len(a) for a in news], pad=32)
        self.nimg = np.zeros(ntotal + 64, np.uint8)
        self.noffs = []
        for i, (a, o) in enumerate(zip(news, noffs)):
            t = words[i] & 0xFFFFFFFF
            self.nimg[o:o + HEAD] = ys[i][t] if t < len(ys[i]) else 0xAA
            o += HEAD + shifts[i]
            self.noffs.append(o)
            self.nimg[o:o + len(a)] = np.frombuffer(a, np.uint8)
            if a:
                self.nimg[o + len(a):o + len(a) + 24] = a[-1]
        self.upload()

    def upload(self):
        self.d_s = torch.from_numpy(self.img.copy()).to(DEV)
        self.d_n = torch.from_numpy(self.nimg).to(DEV)
        self.d_off, self.d_noff = i64(self.soffs), i64(self.noffs)
        self.d_nlen, self.d_cap = i64([len(a) for a in self.news]), i64(self.caps)
        self.d_len, self.d_ulen, self.d_tail = i64([len(y) for y in self.ys]), i64(self.ulens), i64(self.words)
        self.d_need = torch.full((self.n,), NEED_POISON, dtype=torch.int64, device=DEV)
        self.d_status = torch.full((self.n,), STATUS_POISON, dtype=torch.int32, device=DEV)

    def launch(self, form, hint=None, ws=None):
        a = self
        if form == "size":
            R.append_size(a.d_s, a.d_off, a.d_len, a.d_tail, a.d_n, a.d_noff, a.d_nlen, a.d_need, a.d_status)
        elif form == "fit":
            got = R.append_fit(a.d_s, a.d_off, a.d_len, a.d_cap, a.d_ulen, a.d_n, a.d_noff, a.d_nlen, a.d_need,
                               a.d_status, tail=a.d_tail)
            assert got is a.d_tail
        elif form == "plain":
            R.append_batch(a.d_s, a.d_off, a.d_len, a.d_cap, a.d_ulen, a.d_n, a.d_noff, a.d_nlen, a.d_status,
                           tail=a.d_tail)
        elif form == "size_seg":
            ws = ws if ws is not None else R.append_seg_workspace(a.n, hint, DEV)
            R.append_size_seg(a.d_s, a.d_off, a.d_len, a.d_tail, a.d_n, a.d_noff, a.d_nlen, a.d_need, a.d_status,
                              total_new_bytes=hint, workspace=ws)
        elif form == "fit_seg":
            ws = ws if ws is not None else R.append_seg_workspace(a.n, hint, DEV)
            got = R.append_fit_seg(a.d_s, a.d_off, a.d_len, a.d_cap, a.d_ulen, a.d_n, a.d_noff, a.d_nlen, a.d_need,
                                   a.d_status, total_new_bytes=hint, workspace=ws, tail=a.d_tail)
            assert got is a.d_tail
        else:
            raise ValueError(form)

    def fetch(self):
        """(image, len, ulen, tail, need, status) as numpy arrays."""
        torch.cuda.synchronize()
        u = lambda t: t.cpu().numpy().astype(np.uint64)
        return (self.d_s.cpu().numpy(), u(self.d_len), u(self.d_ulen), u(self.d_tail), u(self.d_need),
                self.d_status.cpu().numpy().astype(np.uint32))


class FitFiles:
    """One launch.  Each file: its content x (the stream is oracle.encode(x)) or a stream y given as
    it is, the new bytes, the capacity -- "exact" (C'), "short" (C' - 1), "plus1", "round16" (C'
    rounded up to 16), "slot" (rle_append_slot_bytes) or a number -- and optionally the tail word
    given, a shift of the new-content offset or of the stream offset, and the decoded length so far."""

    def __init__(self, form="fit", hint=None):
        assert form in FORMS
        self.form, self.hint = form, hint
        self.x, self.y, self.new, self.word, self.cap, self.shift, self.sshift, self.ulen = ([] for _ in range(8))

    def add(self, x, new, cap="exact", word=None, shift=0, sshift=0, ulen=None, y=None):
        y = O.encode(bytes(x)) if y is None else bytes(y)
        new = bytes(new)
        tw = M.word_of(y) if y else 0
        cn = len(O.encode(bytes(x) + new)) if x is not None else F.need(y, tw, new)
        slot = R.append_slot_bytes(len(y), len(new))
        cap = {"exact": cn, "short": max(cn - 1, 0), "plus1": cn + 1, "round16": r16(cn), "slot": slot}.get(cap, cap)
        self.x.append(None if x is None else bytes(x))
        self.y.append(y)
        self.new.append(new)
        self.word.append(tw if word is None else word)
        self.cap.append(int(cap))
        self.shift.append(shift)
        self.sshift.append(sshift)
        self.ulen.append(1000 + len(self.y) if ulen is None else ulen)
        return len(self.y) - 1

    def __len__(self):
        return len(self.y)

    def arena(self):
        return Arena(self.y, self.new, self.word, self.cap, self.ulen, self.shift, self.sshift)

    def expected(self, arena, form=None, status=None):
        """(image, len, ulen, tail, need, status) the launch must leave.  status: {index: status} of
        files refused for a reason the model does not see (past the segment tables)."""
        form = form or self.form
        img = arena.img.copy()
        ln, ul, tl, nd, st = [], [], [], [], []
        for i, (x, y, new) in enumerate(zip(self.x, self.y, self.new)):
            ok_addr = self.shift[i] % 16 == 0 and arena.soffs[i] % 16 == 0
            if form == "plain":
                s, c = F.decide(y, self.word[i], new, None, ok_addr)
                if not s & M.TOOLARGE and self.cap[i] < M.slot_bytes(len(y), len(new)):
                    s = M.MISALIGNED
            else:
                s, c = F.decide(y, self.word[i], new, None if form.startswith("size") else self.cap[i], ok_addr)
            if status and i in status:
                s, c = status[i], 0
            commit = s == 0 and new and not form.startswith("size")
            if commit:
                out = O.encode(x + new) if x is not None else M.append_carried(y, self.word[i], new)[0]
                assert len(out) == c and out == M.append_carried(y, self.word[i], new)[0], i
                img[arena.soffs[i]:arena.soffs[i] + len(out)] = np.frombuffer(out, np.uint8)
                ln.append(len(out))
                ul.append(self.ulen[i] + len(new))
                tl.append(M.word_of(out))
            else:
                ln.append(len(y))
                ul.append(self.ulen[i])
                tl.append(self.word[i])
            nd.append(NEED_POISON if form == "plain" else c)
            st.append(s)
        return img, ln, ul, tl, nd, st

    def compare(self, label, arena, got, exp):
        img, ln, ul, tl, nd, st = got
        eimg, eln, eul, etl, end, est = exp
        for i in range(len(self.y)):
            ctx = (label, i, len(self.y[i]), len(self.new[i]), self.cap[i], self.y[i][-6:], self.new[i][:12])
            assert st[i] == est[i], ("status", hex(st[i]), hex(est[i])) + ctx
            assert nd[i] == end[i], ("need", int(nd[i]), end[i]) + ctx
            assert ln[i] == eln[i], ("len", int(ln[i]), eln[i]) + ctx
            assert ul[i] == eul[i], ("ulen", int(ul[i]), eul[i]) + ctx
            assert tl[i] == etl[i], ("tail", hex(int(tl[i])), hex(etl[i])) + ctx
        diff = np.nonzero(img != eimg)[0]
        if diff.size:
            p = int(diff[0])
            b = max(i for i, o in enumerate(arena.soffs) if o <= p)
            raise AssertionError(f"{label}: slot of file {b}, byte +{p - arena.soffs[b]} is {img[p]:#x}, expected "
                                 f"{eimg[p]:#x} (old C {len(self.y[b])}, A {len(self.new[b])}, cap {self.cap[b]}, "
                                 f"status {est[b]:#x}); {diff.size} bytes differ")

    def check(self, label, status=None):
        """Builds the arenas, launches the form, compares everything; returns what the launch left."""
        arena = self.arena()
        arena.launch(self.form, self.hint)
        got = arena.fetch()
        self.compare(label, arena, got, self.expected(arena, status=status))
        return got
