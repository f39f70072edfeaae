"""GPU test: the reference's write with evictions (src/filesystemApi.c:772-814, the reply of
src/server.c:314-323) on the device, at 48 stored files with 3 appends: tail scan, size query, victim
selection with d_want = d_need and the written files spared, one copy of the summary and the list to
the host, the victims' rows gathered in reply order, the eviction reply, the survivors relocated with
d_sel = d_keep, and the appends into the new slots.  Expected results come from a store model run
write by write (the oracle codec plus evict_model.loop_model)."""
import numpy as np
import pytest
import torch

import evict_model as M
import readn_reply_gpu as G
import readn_reply_model as RM
import rle_mi355x as R
import rle_oracle as O
from append_fit_gpu import DEV, Arena, i64, r16

pytestmark = pytest.mark.gpu
N = 48
WRITES = {7: 2000, 21: 5000, 40: 800}   # file: appended bytes


def the_store():
    xs = [O.gen(1 + i % 4, 300 + i, 100 + (i * 1237) % 2901) for i in range(N)]
    news = [O.gen(1 + (i + 1) % 4, 900 + i, WRITES.get(i, 0)) for i in range(N)]
    # lastRef-like keys with ties; the files being written were used last
    keys = [0x6530000000 + (i * 29) % 17 * 60 for i in range(N)]
    for k, i in enumerate(WRITES):
        keys[i] = 0x6530010000 + k
    return xs, news, keys


def write_by_write(xs, news, keys, max_bytes):
    """The reference's writes in batch order: (contents, sizes, live, evicted in order, currStorageSize)."""
    content, size, live, evicted = list(xs), [len(O.encode(x)) for x in xs], [1] * N, []
    curr = sum(size)
    for w, new in enumerate(news):
        if not new:
            continue
        x2 = content[w] + new
        c2 = len(O.encode(x2))
        assert c2 >= size[w] and live[w]
        r = M.loop_model(keys, size, [c2 if i == w else 0 for i in range(N)], live, [int(i == w) for i in range(N)],
                         max_bytes)                                  # :784-798, getVictim(store, fptr)
        assert r.status == M.OK
        for v in r.victims:
            live[v] = 0
        evicted += r.victims
        content[w], size[w], curr = x2, c2, r.summary[3]             # :807-814
    return content, size, live, evicted, curr


def test_write_with_evictions_on_the_device():
    xs, news, keys = the_store()
    paths = G.names(N)
    ys = [O.encode(x) for x in xs]
    need_m = [len(O.encode(x + a)) for x, a in zip(xs, news)]
    written = [int(bool(a)) for a in news]
    # the limit: what the store takes after the writes less the first six files of the order, exactly
    batch = M.store(keys, [len(y) for y in ys], need_m, None, written)
    max_bytes = M.totals(batch)[0] - M.prefix_bytes(batch, 6)
    batch["max_bytes"] = max_bytes
    # the model first: batch order and write-by-write order give the same victims
    content, size, live, evicted, curr = write_by_write(xs, news, keys, max_bytes)
    want = M.loop_model(**batch)
    assert want.status == M.OK and want.victims == evicted and 5 <= len(evicted) <= 7
    assert want.summary[3] == curr == sum(s for s, lv in zip(size, live) if lv) <= max_bytes
    assert want.keep == live

    a = Arena(ys, news, [0] * N, [r16(len(y)) for y in ys], [len(x) for x in xs])
    table = G.PathTable(paths)
    z64 = lambda k=N: torch.full((k,), -7, dtype=torch.int64, device=DEV)       # noqa: E731
    z32 = lambda k=N: torch.full((k,), 0x7777, dtype=torch.int32, device=DEV)   # noqa: E731
    d_key, d_tail, need, st = i64(keys), z64(), z64(), torch.full((4, N), 0x7777, dtype=torch.int32, device=DEV)
    keep, victims, summary = z32(), z32(), z64(R.RLE_EVICT_SUMMARY_WORDS)
    # 1-3: tail scan, size query, selection
    R.tail_batch(a.d_s, a.d_off, a.d_len, d_tail, None, st[0])
    R.append_size(a.d_s, a.d_off, a.d_len, d_tail, a.d_n, a.d_noff, a.d_nlen, need, st[1])
    spare = (a.d_nlen != 0).to(torch.int32)
    R.evict_select(d_key, a.d_len, keep, victims, summary, want=need, spare=spare, max_bytes=max_bytes)
    # 4: the one copy to the host
    h_summary, h_victims = summary.cpu().tolist(), victims.cpu().tolist()
    m = h_summary[1]
    assert h_summary == want.summary and h_victims[:m] == want.victims and h_victims[m:] == [0x7777] * (N - m)
    assert keep.cpu().tolist() == want.keep and need.cpu().tolist() == need_m
    # 5-6: the victims' rows in reply order, and the eviction reply
    rows = [z64(m) for _ in range(5)]
    R.evict_gather(victims, summary, [a.d_off, a.d_len, a.d_ulen, table.off, table.len], rows, order=R.RLE_EVICT_ORDER_REPLY)
    sent = want.victims[::-1]
    reply = RM.reply([paths[v] for v in sent], [xs[v] for v in sent], RM.READN | RM.END)
    size_out = len(reply) + G.SLACK
    d_out = torch.full((size_out,), G.POISON, dtype=torch.uint8, device=DEV)
    place, total, rst = z64(m), z64(1), z32(m)
    R.readn_reply(a.d_s, rows[0], rows[1], rows[2], table.d_paths, rows[3], rows[4], d_out, place, total, rst,
                  form=R.RLE_REPLY_READN | R.RLE_REPLY_END, out_cap=len(reply))
    # 7-8: the survivors to their new slots, and the appends into them
    dst = torch.full((sum(r16(c) for c in need_m) + 64,), 0xEE, dtype=torch.uint8, device=DEV)
    new_off, new_cap, rtotal, need2 = z64(), z64(), z64(1), z64()
    R.relocate_batch(a.d_s, a.d_off, a.d_len, dst, new_off, new_cap, rtotal, want=need, sel=keep, status=st[2])
    R.append_fit(dst, new_off, a.d_len, new_cap, a.d_ulen, a.d_n, a.d_noff, a.d_nlen, need2, st[3], tail=d_tail)
    torch.cuda.synchronize()

    assert st[:3].cpu().tolist() == [[0] * N] * 3 and rst.cpu().tolist() == [0] * m
    # (a victim's row is dead: it has no slot for the append to look at, and its status word says nothing)
    assert [s for s, lv in zip(st[3].cpu().tolist(), live) if lv] == [0] * sum(live)
    assert bool((dst[int(rtotal.item()):] == 0xEE).all().item())
    assert int(total.item()) == len(reply)
    assert (d_out.cpu().numpy() == G.image_of(reply, size_out)).all()           # byte-identical eviction reply
    img, off, ln, ul = dst.cpu().numpy(), new_off.cpu().tolist(), a.d_len.cpu().tolist(), a.d_ulen.cpu().tolist()
    assert new_cap.cpu().tolist() == [r16(c) if lv else 0 for c, lv in zip(need_m, live)]
    assert int(rtotal.item()) == sum(r16(c) for c, lv in zip(need_m, live) if lv)
    for i in range(N):
        if live[i]:
            y = img[off[i]:off[i] + ln[i]].tobytes()
            assert ln[i] == size[i] and ul[i] == len(content[i]) and y == O.encode(content[i]), i
            assert O.decode(y, ul[i]) == (content[i], 0), i
    assert sum(ln[i] for i in range(N) if live[i]) == h_summary[3] == curr       # currStorageSize
    assert np.array_equal(a.d_s.cpu().numpy(), a.img)                            # the old arena is as it was
