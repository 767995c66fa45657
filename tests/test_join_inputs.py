"""CPU checks of tests/join_cases.py: every case has the properties the GPU suite (tests/test_gpu_db_join.py) relies on, and the numpy
restatement of the join does what the definition says on them."""
import numpy as np

from oracle import ipk_oracle as co
from tests import join_cases as J
from tests import union_cases as U


def holders(c):
    """{key: the number of shards that hold it}"""
    n = {}
    for s in c["shards"]:
        for k in s["keys"]:
            n[int(k)] = n.get(int(k), 0) + 1
    return n


def joined(c, key):
    w = c["want"]
    i = int(np.searchsorted(w["keys"], key))
    assert w["keys"][i] == key
    a, b = int(w["off"][i]), int(w["off"][i + 1])
    return w["br"][a:b], w["sc"][a:b], w["pos"][a:b]


def concatenated(c, key):
    return [e for s in c["shards"] for e in J.lists_of(s).get(key, [])]


def test_every_case_is_listed_and_well_formed():
    assert [c["name"] for c in J.all_cases()] == J.CASE_NAMES
    for c in J.all_cases():
        w = c["want"]
        assert np.all(w["keys"][1:] > w["keys"][:-1]) and len(w["off"]) == len(w["keys"]) + 1 and w["off"][-1] == len(w["br"])
        assert sum(len(s["br"]) for s in c["shards"]) - w["dropped"] == len(w["br"])
        assert np.all(w["pos"] < 65536)                                     # (a file's positions are 16-bit)
        off = w["off"].astype(np.int64)
        for i in range(len(w["keys"])):                                     # a joined list's branches are distinct
            assert len(np.unique(w["br"][off[i]:off[i + 1]])) == off[i + 1] - off[i]
        for s in c["shards"]:                                               # and so are a source's own (the join's precondition)
            so = s["off"].astype(np.int64)
            for i in range(len(s["keys"])):
                assert len(np.unique(s["br"][so[i]:so[i + 1]])) == so[i + 1] - so[i]
        n = holders(c)
        assert w["shared_keys"] == sum(v > 1 for v in n.values())


def test_branch_ranges():
    c = J.case("branch_ranges")
    by = np.bincount(list(holders(c).values()), minlength=4)
    assert by[1] > 10 and by[2] > 10 and by[3] > 10, by
    assert c["want"]["dropped"] == 0 and c["want"]["route"] == 0
    seen = [set(s["br"].tolist()) for s in c["shards"]]
    assert not (seen[0] & seen[1]) and not (seen[0] & seen[2]) and not (seen[1] & seen[2])


def test_duplicates_winners():
    c = J.case("duplicates")
    assert c["want"]["route"] == 1
    n2 = n3 = 0
    for i, (what, scores, winner) in enumerate(J.DUP_ROWS):
        br, sc, pos = joined(c, J.DUP_KEY + i)
        first = next(s for s in range(3) if scores[s] is not None)
        held = sum(x is not None for x in scores)
        n2 += held == 2; n3 += held == 3
        # branch 7 stands where its first holder put it: behind that shard's first entry, and behind the full lists of the shards before
        assert list(br[:3 * first + 2]) == [x for s in range(first) for x in (20 + s, 30 + s)] + [20 + first, 7], what
        at = int(np.flatnonzero(br == 7)[0])
        assert np.count_nonzero(br == 7) == 1
        assert sc[at].view(np.uint32) == np.float32(scores[winner]).view(np.uint32), what
        assert pos[at] == 100 * winner + i, what                            # the position that belonged to the kept score
        assert len(br) == sum(2 + (x is not None) for x in scores) - (held - 1)
    assert n2 >= 7 and n3 >= 3
    assert J.ULP > np.float32(-1.5) and np.float32(J.ULP).view(np.uint32) + 1 == np.float32(-1.5).view(np.uint32)
    assert c["want"]["dropped"] == sum(sum(x is not None for x in r[1]) - 1 for r in J.DUP_ROWS)


def test_first_place():
    c = J.case("first_place")
    br, sc, pos = joined(c, 500)
    assert list(br) == [9, 4, 6, 2, 1, 8]
    assert sc[1] == np.float32(-2.0) and pos[1] == 5                      # shard 1's score and position at shard 0's place
    assert list(br) != sorted(br) and [e[0] for e in concatenated(c, 500)].index(4) == 1
    assert c["want"]["dropped"] == 1


def test_wave_edges():
    c = J.case("wave_edges")
    lengths = {}
    for key in holders(c):
        cat = [e[0] for e in concatenated(c, key)]
        lengths.setdefault(len(cat), []).append(cat)
    assert sorted(lengths) == J.WAVE_LENGTHS
    for n, cats in lengths.items():
        pairs = set()
        for cat in cats:
            dup = [i for i, b in enumerate(cat) if cat.count(b) > 1]
            if n > 1:
                assert len(dup) == 2
                pairs.add(tuple(dup))
        assert pairs == (set() if n == 1 else {(0, n - 1)} if n < 65 else {(0, n - 1), (63, 64)}), (n, pairs)
    assert c["want"]["dropped"] == 9


def test_long_lists():
    c = J.case("long_lists")
    want = {40: (6000, 50, 3), 41: (20000, 1, 2), 42: (J.LDS_LIST, 30, 2), 43: (J.LDS_LIST + 1, 30, 2)}
    n = holders(c)
    for key, (length, dups, shards) in want.items():
        cat = concatenated(c, key)
        assert len(cat) == length and n[key] == shards
        assert length - len(joined(c, key)[0]) == dups
    assert max(int(c["shards"][0]["br"].max()), 0) < 100000 and max(e[0] for e in concatenated(c, 40)) < 6000
    assert 6000 > J.LDS_LIST > J.WAVE_LIST                                 # they leave a wavefront and leave LDS
    # some duplicate's later score wins and some earlier one's does
    br, sc, _ = joined(c, 40)
    first = {}
    later_wins = earlier_wins = 0
    for b, s, _ in concatenated(c, 40):
        if b in first:
            later_wins += np.float32(s) > np.float32(first[b]); earlier_wins += not np.float32(s) > np.float32(first[b])
        else:
            first[b] = s
    assert later_wins > 5 and earlier_wins > 5


def test_tiles():
    c = J.case("tiles")
    w = c["want"]
    cnt = (w["off"][1:] - w["off"][:-1]).astype(np.int64)
    n = holders(c)
    assert cnt[0] == J.TILE and w["off"][1] % J.TILE == 0 and cnt[1] == 5000
    assert n[int(w["keys"][0])] == 2 and n[int(w["keys"][1])] == 2
    run = np.arange(4, 4 + U.TILES_RUN)
    assert np.all(cnt[run] == 1)
    owner = [0 if int(k) in set(c["shards"][0]["keys"].tolist()) else 1 for k in w["keys"][run]]
    assert all(owner[i] != owner[i + 1] for i in range(len(owner) - 1))
    assert w["off"][-1] % J.TILE != 0 and w["dropped"] == 0


def test_many_sources():
    c = J.case("many_sources")
    n = holders(c)
    assert len(c["shards"]) == 66 and n[77] == 65 and sum(len(s["keys"]) == 0 for s in c["shards"]) == 1
    br, sc, pos = joined(c, 77)
    assert len(br) == 64 and br[0] == 0 and sc[0] == np.float32(-1.0) and pos[0] == 65


def test_entryless():
    c = J.case("entryless")
    assert len(joined(c, 10)[0]) == 3 and len(joined(c, 20)[0]) == 0 and len(joined(c, 30)[0]) == 3
    assert list(c["want"]["keys"]) == [10, 20, 30]
    assert [len(J.lists_of(s)[10]) for s in c["shards"]] == [0, 3] and [len(J.lists_of(s)[20]) for s in c["shards"]] == [0, 0]


def test_disjoint_is_the_union():
    c = J.case("disjoint")
    u = U.restate(c["shards"])
    w = c["want"]
    assert w["shared_keys"] == 0 and w["dropped"] == 0 and w["route"] == 0
    assert np.array_equal(w["keys"], u["keys"]) and np.array_equal(w["off"], u["off"]) and np.array_equal(w["br"], u["br"])
    assert np.array_equal(w["sc"].view(np.uint32), u["sc"].view(np.uint32)) and np.array_equal(w["pos"], u["pos"])


def test_restatement_then_host_mif0_is_self_consistent():
    """Joining in two steps -- (shard 0, shard 1) first, then shard 2 -- is the join of all three, and the host MIF0 of the joined
    lists, which sums in entry order, gives the same values either way; joined in another order the lists, and with them possibly the
    sums' last bits, differ while the key set does not."""
    for name in ("branch_ranges", "duplicates", "first_place"):
        c = J.case(name)
        s = c["shards"]
        w = c["want"]
        step = J.restate(s[:2])
        step_db = J.shard(step["keys"], [list(zip(*joined(dict(want=step), int(k)))) for k in step["keys"]])
        two = J.restate([step_db, s[2]])
        for f in ("keys", "off", "br", "pos"):
            assert np.array_equal(two[f], w[f]), (name, f)
        assert np.array_equal(two["sc"].view(np.uint32), w["sc"].view(np.uint32))
        off = w["off"].astype(np.int64)
        thr = co.score_threshold(1.5, 4, 8) if hasattr(co, "score_threshold") else (1.5 / 4) ** 8
        a = [co.mif0(w["sc"][off[i]:off[i + 1]], 6001, thr) for i in range(len(w["keys"]))]
        b = [co.mif0(two["sc"][off[i]:off[i + 1]], 6001, thr) for i in range(len(w["keys"]))]
        assert np.array_equal(np.array(a, np.float64).view(np.uint64), np.array(b, np.float64).view(np.uint64))
        back = J.restate(s[::-1])
        assert np.array_equal(back["keys"], w["keys"]) and np.array_equal(back["off"][-1:], w["off"][-1:])
        assert not np.array_equal(back["br"], w["br"])
