"""CPU tests of the store lifetime model (tests/store_model.py): the model against a literal
write-by-write restatement of the reference's writeToFileHandler on single-write rounds, the seeded
generator's determinism, the conditions the GPU test's inputs must meet (they are conditions on the
inputs: nothing here is measured), and what each round of the scripted scenario must contain."""
import numpy as np
import pytest

import evict_model as M
import rle_oracle as O
import store_model as SM


def write_by_write(content, live, key, w, new, max_bytes):
    """src/filesystemApi.c:772-814 for one write of `new` to file w, on copies: None for E2BIG, else
    (contents, live, evicted in order, currStorageSize)."""
    content, live = list(content), list(live)
    size = [len(O.encode(c)) if lv else 0 for c, lv in zip(content, live)]
    curr = sum(size)
    c2 = len(O.encode(content[w] + new))
    if c2 > max_bytes:                                       # :777-783
        return None
    evicted = []
    while curr - size[w] + c2 > max_bytes:                   # :784
        victim = None
        for i in range(len(content)):                        # getVictim(store, fptr): list order, strict <
            if live[i] and i != w and (victim is None or key[i] < key[victim]):
                victim = i
        assert victim is not None                            # :787
        live[victim], content[victim] = 0, b""               # :789 destroyFile
        curr -= size[victim]
        evicted.append(victim)
    curr = curr - size[w] + c2                               # :807
    content[w] += new                                        # :811-814
    return content, live, evicted, curr


@pytest.mark.parametrize("seed", [1, 2])
def test_single_write_rounds_are_the_reference_loop(seed):
    s = SM.initial(seed, "compact", slack=2500)
    rng = np.random.default_rng(seed)
    refused = evicting = 0
    for k in range(40):
        w = int(rng.choice(s.live_rows()))
        size = 140000 if k % 13 == 5 else SM.SIZES[1 + int(rng.integers(0, 6))]
        kind = int(rng.integers(0, 5))
        new = O.gen(1 if size > 12000 else kind, 5000 + k, size)   # (the large write is incompressible: E2BIG)
        want = write_by_write(s.content, s.live, s.key, w, new, s.max_bytes)
        before = list(s.content), list(s.live), list(s.key)
        o = s.apply(SM.Round([], [], {w: new}, [], False))
        if want is None:
            refused += 1
            assert o.dropped and o.sel.status == M.NOFIT and (list(s.content), list(s.live), list(s.key)) == before
            continue
        content, live, evicted, curr = want
        assert not o.dropped and o.sel.victims == evicted and s.content == content and s.live == live
        assert s.curr() == curr == o.sel.summary[3] <= s.max_bytes
        assert s.key[w] == SM.CLOCK + 60 * (k + 1)
        evicting += bool(evicted)
    assert refused >= 2 and evicting >= 5


def history(scenario):
    out = []
    for rnd, o in SM.run(scenario):
        out.append((rnd, o.need, o.sel, o.reply, o.read_reply, o.moved, o.compacted, o.bound))
    return out


@pytest.mark.parametrize("policy", SM.POLICIES)
def test_generator_is_deterministic(policy):
    assert history(SM.Scenario(SM.SEEDS[0], policy)) == history(SM.Scenario(SM.SEEDS[0], policy))
    assert history(SM.Scenario(SM.SEEDS[0], policy)) != history(SM.Scenario(SM.SEEDS[1], policy))
    assert history(SM.Scripted(policy)) == history(SM.Scripted(policy))


@pytest.mark.parametrize("policy", SM.POLICIES)
def test_coverage_conditions_of_the_seeded_runs(policy):
    """Over the seeded runs of one policy together."""
    c = dict(evict=0, m3=0, nofit=0, revived=0, ext=0, notext=0, seg=0, one=0, partial=0, compacted=0, writes=0)
    past_64k = False
    for seed in SM.SEEDS:
        sc = SM.Scenario(seed, policy)
        assert sc.store.curr() <= sc.store.max_bytes
        for _ in range(SM.ROUNDS):
            rnd, o = SM.step(sc)
            m = len(o.sel.victims)
            c["writes"] += any(rnd.writes.values())
            c["evict"] += m > 0
            c["m3"] += m >= 3
            c["nofit"] += o.dropped
            c["revived"] += o.revived_writes
            c["ext"] += o.extended > 0
            c["notext"] += o.not_extended > 0
            c["seg" if rnd.seg else "one"] += 1
            c["partial"] += bool(o.moved) and not o.compacted
            c["compacted"] += o.compacted
            s = sc.store
            assert rnd.reads and all(s.live[i] for i in rnd.reads)
            assert all(len(a) in SM.SIZES for a in rnd.writes.values())
            # the segmented forms cut real segments: the large row's stream is many segments long
            past_64k |= bool(rnd.seg and s.live[SM.BIG] and len(s.content[SM.BIG]) > 65536
                             and len(SM.enc(s.content[SM.BIG])) > 4 * 4032)
    assert c["evict"] >= 8 and c["m3"] >= 2 and c["nofit"] >= 1 and c["revived"] >= 2, c
    assert c["ext"] >= 1 and c["notext"] >= 1 and c["seg"] >= 5 and c["one"] >= 5 and past_64k, c
    assert c["writes"] / 4 <= c["evict"] <= c["writes"] / 2, c      # roughly a third of the write rounds evict
    if policy == "grow":
        assert c["partial"] >= 3 and c["compacted"] >= 1, c


@pytest.mark.parametrize("policy", SM.POLICIES)
def test_scripted_scenario_contains_its_rounds(policy):
    sc = SM.Scripted(policy)
    s = sc.store
    h = SM.run(sc)
    assert len(h) == SM.ROUNDS
    rnd, o = zip(*h)
    victims = o[0].sel.victims
    assert len(victims) >= 2 and not o[0].dropped                                   # 1: m >= 2
    assert rnd[1].creations == [victims[0]] and victims[0] not in rnd[1].writes     # 2: revived, empty
    assert rnd[2].writes[victims[0]] and o[2].revived_writes == 1 and not o[2].dropped   # 3: written
    assert rnd[3].writes and not any(rnd[3].writes.values()) and not o[3].dropped   # 4: A = 0 everywhere
    assert o[3].sel.victims == [] and o[3].need == o[2].need
    for k in (4, 5):                                                                # 5: every live file written
        assert all(rnd[k].writes.values()) and len(rnd[k].writes) == o[k].sel.summary[4]
        assert o[k].sel.victims == []
    assert o[5].dropped and o[5].sel.status == M.NOFIT                              # 6: NOFIT
    evictions = [res for _, res in o[6].created if res is not None]                 # 7: at max_files
    assert len(evictions) == 1 and len(evictions[0].victims) == 1 and o[6].created[-1][1] is evictions[0]
    assert evictions[0].summary[4] == s.max_files
    assert o[7].sel.summary[4] == 1 and len(rnd[7].removals) == s.max_files - 1     # 8: all but one removed
    assert len(o[10].sel.victims) == 3 and o[10].sel.keep == [int(i == SM.BIG) for i in range(SM.N)]
    assert not o[11].dropped and rnd[11].writes[SM.BIG] and o[11].sel.summary[4] == 1   # 9: the spared file alone
    assert s.live_rows() == [SM.BIG] and s.curr() <= s.max_bytes
    assert {r.seg for r in rnd} == {False, True}
