"""Launch helper of the segmented append's GPU tests (tests/test_gpu_append_seg.py):
append_tail_gpu.Files with the launch replaced.  The arenas are those of Files.run -- slots poisoned
outside the stream, the new-content padding repeating each file's last new byte -- and, in front of
every new buffer, 16 bytes holding the stored stream's final byte c: the head positions of the
virtual buffer are never read, and a read of them would lengthen the entering run."""
import numpy as np
import torch

import append_tail_gpu as G
import rle_mi355x as R

HEAD = 16


class SegFiles(G.Files):
    """form: "seg" (rle_append_batch_device_seg with total_new_bytes = hint) or "wave" (the one-wave
    rle_append_batch_device on the same arenas).  short_ws: pass a workspace one byte short and
    expect RLE_E_INVAL from the host, nothing launched."""

    def __init__(self, hint, form="seg", short_ws=False):
        super().__init__()
        self.hint, self.form, self.short_ws = int(hint), form, short_ws

    def launch(self, d_s, soffs, d_len, caps, d_ulen, d_n, noffs, nlens, status, d_tail):
        if self.form == "wave":
            R.append_batch(d_s, soffs, d_len, caps, d_ulen, d_n, noffs, nlens, status, tail=d_tail)
            return
        n = len(self.y)
        if not self.short_ws:
            ws = R.append_seg_workspace(n, self.hint, G.DEV)
            got = R.append_batch_seg(d_s, soffs, d_len, caps, d_ulen, d_n, noffs, nlens, status,
                                     total_new_bytes=self.hint, workspace=ws, tail=d_tail)
            assert got is d_tail
            return
        need = int(R.lib().rle_append_seg_workspace_bytes(n, self.hint))
        ws = torch.zeros(need + 256, dtype=torch.uint8, device=G.DEV)
        wp, _ = R._ws_ptr(ws)
        p = R._ptr
        rc = R.lib().rle_append_batch_device_seg(p(d_s), p(soffs), p(d_len), p(caps), p(d_ulen), p(d_tail), p(d_n),
                                                 p(noffs), p(nlens), p(status), n, self.hint, wp, need - 1,
                                                 R._stream_ptr(None))
        assert rc == R.RLE_E_INVAL, rc
        torch.cuda.synchronize()
        assert int(ws.sum().item()) == 0, "a refused call wrote to its workspace"

    def run(self):
        n = len(self.y)
        need = [R.append_slot_bytes(len(y), len(a)) for y, a in zip(self.y, self.new)]
        assert all(need)
        soffs, stotal = R.layout(need, pad=G.PAD)
        img = np.full(stotal + 64, G.POISON, np.uint8)
        for y, o in zip(self.y, soffs):
            img[o:o + len(y)] = np.frombuffer(y, np.uint8)
        noffs, ntotal = R.layout([HEAD + len(a) for a in self.new], pad=G.PAD)
        nimg = np.zeros(ntotal + 64, np.uint8)
        noffs = [o + HEAD for o in noffs]
        for i, (a, o) in enumerate(zip(self.new, noffs)):
            t = self.word[i] & 0xFFFFFFFF
            nimg[o - HEAD:o] = self.y[i][t] if t < len(self.y[i]) else 0xAA
            o += self.shift[i]
            noffs[i] = o
            nimg[o:o + len(a)] = np.frombuffer(a, np.uint8)
            if a:
                nimg[o + len(a):o + len(a) + 24] = a[-1]
        caps = [c if c is not None else nd for c, nd in zip(self.cap, need)]
        d_s = torch.from_numpy(img.copy()).to(G.DEV)
        d_n = torch.from_numpy(nimg).to(G.DEV)
        d_len, d_ulen, d_tail = G.i64([len(y) for y in self.y]), G.i64(self.ulen), G.i64(self.word)
        status = torch.full((n,), 0x7777, dtype=torch.int32, device=G.DEV)
        self.launch(d_s, G.i64(soffs), d_len, G.i64(caps), d_ulen, d_n, G.i64(noffs), G.i64([len(a) for a in self.new]),
                    status, d_tail)
        torch.cuda.synchronize()
        return (d_s.cpu().numpy(), list(soffs), d_len.cpu().numpy().astype(np.uint64),
                d_ulen.cpu().numpy().astype(np.uint64), d_tail.cpu().numpy().astype(np.uint64),
                status.cpu().numpy().astype(np.uint32), img)
