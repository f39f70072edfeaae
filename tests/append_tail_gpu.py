"""Launch helpers of the tail-scan and append GPU tests (tests/test_gpu_tail_scan.py,
tests/test_gpu_append_batch.py): arenas built on the host, one launch through the C ABI, results
back as numpy arrays."""
import numpy as np
import torch

import append_tail_model as M
import rle_mi355x as R

DEV = "cuda:0"
POISON = 0xEE
PAD = 32   # spare bytes after every slot, so that a shifted or overrun buffer stays inside its own


def i64(v):
    return torch.tensor(np.asarray(v, dtype=np.uint64).astype(np.int64), device=DEV)


def scan(streams, padding=None, shift=None, length=None):
    """rle_tail_batch_device over `streams` packed 16-byte aligned.  padding: {index: bytes written
    right behind the stream}; shift: {index: bytes added to the offset}; length: {index: the length
    passed instead of the true one}.  Returns (status, tail, ulen) as numpy uint64/uint32 arrays."""
    n = len(streams)
    lens = [len(s) for s in streams]
    offs, total = R.layout(lens, pad=PAD)
    host = np.zeros(total + 64, np.uint8)
    for i, (s, o) in enumerate(zip(streams, offs)):
        host[o:o + len(s)] = np.frombuffer(s, np.uint8)
        fill = (padding or {}).get(i, b"")
        host[o + len(s):o + len(s) + len(fill)] = np.frombuffer(fill, np.uint8)
    offs, lens = list(offs), list(lens)
    for i, d in (shift or {}).items():
        offs[i] += d
    for i, v in (length or {}).items():
        lens[i] = v
    d_in = torch.from_numpy(host).to(DEV)
    tail = torch.full((n,), 0x5555555555, dtype=torch.int64, device=DEV)
    ulen = torch.full((n,), 0x6666666666, dtype=torch.int64, device=DEV)
    status = torch.full((n,), 0x7777, dtype=torch.int32, device=DEV)
    R.tail_batch(d_in, i64(offs), i64(lens), tail, ulen, status)
    torch.cuda.synchronize()
    return (status.cpu().numpy().astype(np.uint32), tail.cpu().numpy().astype(np.uint64),
            ulen.cpu().numpy().astype(np.uint64))


def scan_expected(stream):
    """(status, tail word, ulen) the scan must give for a stream."""
    tl = M.tail_of(stream)
    if tl is None:
        return M.NOTCANON, 0, 0
    return 0, M.tail_word(tl[0], tl[1]), tl[2]


class Files:
    """One append launch.  Each file: its stream y, the new bytes, and optionally the tail word given
    (default: the model's), the capacity passed (default: rle_append_slot_bytes), a shift of its
    new-content offset, and its decoded length so far."""

    def __init__(self):
        self.y, self.new, self.word, self.cap, self.shift, self.ulen = [], [], [], [], [], []

    def add(self, y, new, word=None, cap=None, shift=0, ulen=None):
        self.y.append(bytes(y))
        self.new.append(bytes(new))
        self.word.append(M.word_of(y) if word is None else word)
        self.cap.append(cap)
        self.shift.append(shift)
        self.ulen.append(1000 + len(self.y) if ulen is None else ulen)
        return len(self.y) - 1

    def __len__(self):
        return len(self.y)

    def run(self):
        """Launches the append; returns (slots image, slot offsets, len, ulen, tail, status, the image before).  Slots
        are poisoned (0xEE) outside the stream; the new-content arena's padding repeats each file's
        last new byte (hostile: it would extend the final run if it were read as content)."""
        n = len(self.y)
        need = [R.append_slot_bytes(len(y), len(a)) for y, a in zip(self.y, self.new)]
        assert all(need)
        soffs, stotal = R.layout(need, pad=PAD)
        img = np.full(stotal + 64, POISON, np.uint8)
        for y, o in zip(self.y, soffs):
            img[o:o + len(y)] = np.frombuffer(y, np.uint8)
        noffs, ntotal = R.layout([len(a) for a in self.new], pad=PAD)
        nimg = np.zeros(ntotal + 64, np.uint8)
        noffs = list(noffs)
        for i, (a, o) in enumerate(zip(self.new, noffs)):
            o += self.shift[i]
            noffs[i] = o
            nimg[o:o + len(a)] = np.frombuffer(a, np.uint8)
            if a:
                nimg[o + len(a):o + len(a) + 24] = a[-1]
        caps = [c if c is not None else nd for c, nd in zip(self.cap, need)]
        d_s = torch.from_numpy(img.copy()).to(DEV)
        d_n = torch.from_numpy(nimg).to(DEV)
        d_len, d_ulen, d_tail = i64([len(y) for y in self.y]), i64(self.ulen), i64(self.word)
        status = torch.full((n,), 0x7777, dtype=torch.int32, device=DEV)
        R.append_batch(d_s, i64(soffs), d_len, i64(caps), d_ulen, d_n, i64(noffs), i64([len(a) for a in self.new]),
                       status, tail=d_tail)
        torch.cuda.synchronize()
        return (d_s.cpu().numpy(), list(soffs), d_len.cpu().numpy().astype(np.uint64),
                d_ulen.cpu().numpy().astype(np.uint64), d_tail.cpu().numpy().astype(np.uint64),
                status.cpu().numpy().astype(np.uint32), img)

    def check(self, label, refused=None, want=None):
        """Runs the launch and compares everything: refused = {index: status bit} files must come
        back untouched; every other file must hold want[i] (default: the model's composition) with
        its length, decoded length and tail word (want[i], where given, must be what the model composes),
        and nothing else in the image may change."""
        refused = refused or {}
        got, soffs, ln, ul, tl, st, before = self.run()
        exp = before.copy()
        for i, (y, a) in enumerate(zip(self.y, self.new)):
            if i in refused:
                assert st[i] == refused[i], (label, i, hex(st[i]), hex(refused[i]))
                assert ln[i] == len(y) and ul[i] == self.ulen[i] and tl[i] == self.word[i], (label, i, "refused file changed")
                continue
            # (the tail from the final run of c^r ‖ new, not from a parse of the whole result:
            # tests/test_append_tail.py pins the two as equal)
            out, word = M.append_carried(y, self.word[i], a)
            if want is not None and want[i] is not None:
                assert out == want[i], (label, i, "the model's composition is not the expected stream")
            assert st[i] == 0, (label, i, hex(st[i]), y[-12:], a[:12])
            assert ln[i] == len(out), (label, i, int(ln[i]), len(out), y[-12:], a[:12])
            assert ul[i] == self.ulen[i] + len(a), (label, i, "ulen")
            assert tl[i] == word, (label, i, hex(int(tl[i])), hex(word), y[-12:], a[:12])
            exp[soffs[i]:soffs[i] + len(out)] = np.frombuffer(out, np.uint8)
        diff = np.nonzero(got != exp)[0]
        if diff.size:
            p = int(diff[0])
            b = max(i for i, o in enumerate(soffs) if o <= p)
            raise AssertionError(f"{label}: slot of file {b}, byte +{p - soffs[b]} is {got[p]:#x}, expected {exp[p]:#x} "
                                 f"(old C {len(self.y[b])}, A {len(self.new[b])}, tail {self.word[b]:#x}); "
                                 f"{diff.size} bytes differ")
        return got, soffs, ln, ul, tl
