"""The optional outputs of the append and tail entries on the GPU: d_ulen and d_status may be NULL,
and leaving them out changes nothing else.  Every entry runs twice over one small batch, once with
both tensors and once with both None: the whole poisoned stream arena and len, tail and need are
identical between the runs and equal the models' (append_fit_gpu.FitFiles.expected: append_fit_model
decides, append_tail_model appends).  The segmented forms run at the smallest segment length."""
import numpy as np
import pytest
import torch

import append_fit_gpu as FG
import append_fit_model as F
import append_tail_model as M
import rle_mi355x as R
from test_gpu_append_seg import hint4

pytestmark = pytest.mark.gpu
ENTRIES = ("plain", "size", "fit", "plain_seg", "size_seg", "fit_seg")


def batch():
    """An empty stream; final tokens of count 1 and 9; new bytes that extend the final token (e = 2);
    A = 0, 1 and 1100 (two tiles); a stream refused for its tail word (C > 0, word 0); a slot one
    byte short of the new length (NOFIT in the fit forms, MISALIGNED in the plain ones)."""
    f = FG.FitFiles()
    f.add(b"", F.new_of("runs50", 300, 0x62, 1), cap="slot", word=R.RLE_TAIL_EMPTY)
    f.add(F.stored_token(1)[0], F.new_of("random", 77, 0x61, 2), cap="slot")
    f.add(F.stored_token(9, 39)[0], b"a" * 5 + F.new_of("random", 40, 0x61, 3), cap="slot")
    f.add(F.stored_token(3, 41)[0], b"aa" + F.new_of("random", 50, 0x61, 4), cap="slot")
    f.add(F.stored_token(4)[0], b"", cap="slot")
    f.add(F.stored_token(5, 47)[0], b"k", cap="slot")
    f.add(F.stored_token(2, 33)[0], F.new_of("runs50", 1100, 0x61, 5), cap="slot")
    f.add(F.stored_token(6)[0], F.new_of("random", 64, 0x61, 6), cap="slot", word=0)
    f.add(F.stored_token(7, 45)[0], F.new_of("runs50", 200, 0x61, 7), cap="short")
    assert M.tail_of(f.y[1])[1] == 1 and M.tail_of(f.y[2])[1] == 9
    return f


def launch(entry, a, ulen, status):
    s = (a.d_s, a.d_off, a.d_len)
    new = (a.d_n, a.d_noff, a.d_nlen)
    seg = dict(total_new_bytes=hint4()) if entry.endswith("_seg") else {}
    if entry.startswith("size"):
        (R.append_size_seg if seg else R.append_size)(*s, a.d_tail, *new, a.d_need, status, **seg)
    elif entry.startswith("fit"):
        (R.append_fit_seg if seg else R.append_fit)(*s, a.d_cap, ulen, *new, a.d_need, status, tail=a.d_tail, **seg)
    else:
        (R.append_batch_seg if seg else R.append_batch)(*s, a.d_cap, ulen, *new, status, tail=a.d_tail, **seg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_append_without_ulen_and_status(entry):
    f = batch()
    form = entry[:-4] if entry.endswith("_seg") else entry
    runs = []
    for given in (True, False):
        a = f.arena()
        launch(entry, a, a.d_ulen if given else None, a.d_status if given else None)
        runs.append((a, a.fetch()))
    (a, with_), (_, without) = runs
    exp = f.expected(a, form=form)
    f.compare(f"{entry}, ulen and status given", a, with_, exp)
    assert {int(s) for s in with_[5]} >= {0, M.NOTCANON, F.NOFIT if form == "fit" else 0}
    for k, name in ((0, "image"), (1, "len"), (3, "tail"), (4, "need")):
        assert np.array_equal(with_[k], without[k]), (entry, name)
    # the tensors that were not passed keep what they were uploaded with
    assert [int(v) for v in without[2]] == f.ulen and (without[5] == FG.STATUS_POISON).all()


@pytest.mark.parametrize("seg", [False, True])
def test_tail_without_ulen_and_status(seg):
    f = batch()
    a = f.arena()
    n, tails = len(f), []
    for given in (True, False):
        tail = torch.full((n,), 0x5555, dtype=torch.int64, device=FG.DEV)
        ulen, status = (a.d_ulen, a.d_status) if given else (None, None)
        if seg:
            R.tail_batch_seg(a.d_s, a.d_off, a.d_len, tail, ulen, status, total_in_bytes=hint4())
        else:
            R.tail_batch(a.d_s, a.d_off, a.d_len, tail, ulen, status)
        tails.append(tail.cpu().numpy().astype(np.uint64))
    img, _, ulen, _, _, status = a.fetch()
    assert np.array_equal(img, a.img)
    assert [int(w) for w in tails[0]] == [M.word_of(y) if y else 0 for y in f.y]
    assert np.array_equal(tails[0], tails[1])
    assert [int(u) for u in ulen] == [len(x) for x in f.x] and not status.any()
