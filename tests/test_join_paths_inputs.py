"""CPU checks of tests/join_paths.py: every case has the properties the GPU suite (tests/test_gpu_join_paths.py) relies on, the
restatement (tests/join_cases.restate) keeps what the chain table says, and three wrong walkers -- the mistakes a duplicate resolver
can make without failing tests/join_cases.py -- differ from it on named rows."""
import numpy as np
import pytest

from tests import join_cases as J
from tests import join_paths as P

KEY_INDEX = {key: i for i, (key, _) in enumerate(P.CHAIN_KEYS)}
LENGTH = dict(P.CHAIN_KEYS)


def bits(x):
    return int(np.float32(x).view(np.uint32))


def test_every_case_is_listed_and_well_formed():
    assert [c["name"] for c in P.all_cases()] == P.CASE_NAMES
    for c in P.all_cases():
        w = c["want"]
        assert np.all(w["keys"][1:] > w["keys"][:-1]) and len(w["off"]) == len(w["keys"]) + 1 and w["off"][-1] == len(w["br"])
        assert sum(len(s["br"]) for s in c["shards"]) - w["dropped"] == len(w["br"])
        assert np.all(w["pos"] < 65536)                                     # (a file's positions are 16-bit)
        for s in c["shards"]:                                               # a source's own branches are distinct (the join's precondition)
            so = s["off"].astype(np.int64)
            for i in range(len(s["keys"])):
                assert len(np.unique(s["br"][so[i]:so[i + 1]])) == so[i + 1] - so[i], (c["name"], int(s["keys"][i]))
        held = {}
        for s in c["shards"]:
            for k in s["keys"]:
                held[int(k)] = held.get(int(k), 0) + 1
        assert w["shared_keys"] == sum(v > 1 for v in held.values())


def test_chain_table_is_the_issue_s():
    """The scores are the float32 values meant, bit for bit, also inside the shards' arrays (a NaN's sign and payload survive)."""
    rows = dict((what, scores) for what, scores, _ in P.CHAIN_ROWS)
    assert len(P.CHAIN_ROWS) == 14 and P.N_OCCURRENCES == 50 and len(set(P.CHAIN_BRANCHES)) == 14
    assert P.CHAIN_BRANCHES[:4] == [0xFFFFFFFF, 0, 1 << 31, (1 << 18) + 5] and all(b < 1000 for b in P.CHAIN_BRANCHES[4:])
    assert [bits(s) for s in rows["zeros a"]] == [0x80000000, 0, 0x80000000, 0]
    assert [bits(rows["zeros b"][s]) for s in (0, 1, 3)] == [0, 0x80000000, 0x80000000] and rows["zeros b"][2] is None
    x = bits(-1.5)
    assert [bits(s) for s in rows["ulp up"]] == [x, x - 1, x - 1, x - 2] and [bits(s) for s in rows["ulp down"]] == [x - 2, x - 1, x, x - 1]
    assert P.up(P.X, 2) > P.up(P.X, 1) > P.X
    assert bits(rows["NaN first"][0]) == 0x7FC00000 and [bits(rows["NaN between"][s]) for s in (1, 3)] == [0x7FC00000] * 2
    assert bits(rows["negative NaN"][1]) == 0xFFC00000 and rows["negative NaN"][3] is None
    assert [bits(s) for s in rows["infinities"]] == [0xFF800000, bits(-1.0), 0x7F800000, bits(5.0)]
    c = P.case("chains")
    for s, shard in enumerate(c["shards"]):
        for r, b in enumerate(P.CHAIN_BRANCHES):
            got = shard["sc"][shard["br"] == np.uint32(b)]
            want = P.CHAIN_ROWS[r][1][s]
            assert len(got) == (0 if want is None else len(P.CHAIN_KEYS))
            assert all(bits(g) == bits(want) for g in got), (s, P.ROW_NAMES[r])


def test_chains_lengths_holders_and_rows():
    c = P.case("chains")
    assert len(c["shards"]) == P.N_SHARDS == 4 and c["header"] is P.K8
    assert sorted(LENGTH.values()) == [64, 65, 129, 257, 600, 1500, 4096, 4097, 4097, 6000]
    assert sum(LENGTH.values()) - 4097 > 16000
    for key, n in P.CHAIN_KEYS:
        per = [J.lists_of(s).get(key) for s in c["shards"]]
        assert all(p is not None and len(p) > 0 for p in per), key           # all four shards hold it
        cat = P.concatenated(c, key)
        assert len(cat) == n == sum(len(p) for p in per)
        br = [e[0] for e in cat]
        assert [br.count(b) for b in P.CHAIN_BRANCHES] == [sum(s is not None for s in r[1]) for r in P.CHAIN_ROWS]
        assert sum(br.count(b) for b in P.CHAIN_BRANCHES) == 50
        fill = [b for b in br if b not in P.CHAIN_BRANCHES]
        assert len(set(fill)) == len(fill) == n - 50                          # the fillers are distinct: the rows hold every duplicate
        assert len(P.joined(c["want"], key)[0]) == n - 36
        # a position per occurrence, which says (shard, row)
        pos = [e[2] for e in cat]
        assert len(set(pos)) == len(pos) and max(pos) < 65536
        for s, p in enumerate(per):
            for b, _, w in p:
                if b in P.CHAIN_BRANCHES:
                    assert w == P.chain_pos(KEY_INDEX[key], s, P.CHAIN_BRANCHES.index(b))
    assert len(LENGTH) == len(P.CHAIN_KEYS)
    all_pos = {P.chain_pos(k, s, r) for k in range(len(P.CHAIN_KEYS)) for s in range(4) for r in range(14)}
    assert len(all_pos) == len(P.CHAIN_KEYS) * 4 * 14 and max(all_pos) < 1024
    assert c["want"]["dropped"] == 36 * len(P.CHAIN_KEYS) and c["want"]["route"] == 1 and c["want"]["shared_keys"] == len(P.CHAIN_KEYS)
    # the wavefront's key: sixteen entries per shard, so a row's occurrences lie in both 32-lane halves
    assert [len(J.lists_of(s)[200]) for s in c["shards"]] == [16] * 4


def test_chains_fillers_and_places():
    c = P.case("chains")
    slot = lambda b: b % J.BRANCH_SLOTS
    row_slots = {slot(b) for b in P.CHAIN_BRANCHES}
    assert len(set(P.FILLERS)) == len(P.FILLERS) and not set(P.FILLERS) & set(P.CHAIN_BRANCHES)
    assert not {slot(b) for b in P.FILLERS} & row_slots                      # none aliases a row's branch
    first, last, inside = set(), set(), set()
    for key, n in P.CHAIN_KEYS:
        fill = [e[0] for e in P.concatenated(c, key) if e[0] not in P.CHAIN_BRANCHES]
        assert fill == P.FILLERS[:n - 50]                                    # every key takes a prefix of the same fillers
        high = sum(b >= J.BRANCH_SLOTS for b in fill)
        assert 0.4 * len(fill) <= high <= 0.6 * len(fill), (key, high, len(fill))
        f = l = i = 0
        for s in c["shards"]:
            br = [e[0] for e in J.lists_of(s)[key]]
            for r, b in enumerate(P.CHAIN_BRANCHES):
                if b in br:
                    at = br.index(b)
                    (first if at == 0 else last if at == len(br) - 1 else inside).add(r)
                    f += at == 0; l += at == len(br) - 1; i += 0 < at < len(br) - 1
        assert f == 4 and l == 4 and i == 42                                 # in every shard's list a row is first and a row is last
    assert first == last == inside == set(range(14))                         # every row is somewhere first, somewhere last, somewhere inside


def test_chains_resolvers_and_padded_sizes():
    by = {}
    for key, n in P.CHAIN_KEYS:
        by.setdefault(P.resolver(n), []).append(n)
    assert by == {"wave": [J.WAVE_LIST], "lds": [65, 129, 257, 600, 1500, J.LDS_LIST], "sorted": [J.LDS_LIST + 1, J.LDS_LIST + 1, 6000]}
    assert J.WAVE_LIST == 64 and J.LDS_LIST == 4096
    assert [P.padded(n) for n in by["lds"]] == [128, 256, 512, 1024, 2048, 4096]
    sizes, p = [], 2 * J.WAVE_LIST
    while p <= J.LDS_LIST:
        sizes.append(p); p *= 2
    assert sorted({P.padded(n) for n in by["lds"]}) == sizes                  # every size the sort can run at
    assert P.padded(J.LDS_LIST) == J.LDS_LIST                                # the longest list has no pad


def test_chains_far_keys():
    c = P.case("chains")
    keys = [k for k, _ in P.CHAIN_KEYS]
    far = [k for k, n in P.CHAIN_KEYS if P.resolver(n) == "sorted"]
    assert keys == sorted(keys) and list(c["want"]["keys"]) == keys
    assert far[0] == keys[0] and LENGTH[far[0]] == J.LDS_LIST + 1             # a far key is J-key 0
    a, b = far[1], far[2]
    assert b == a + 1 and keys.index(b) == keys.index(a) + 1 and 0 < keys.index(a) and keys.index(b) < len(keys) - 1
    assert {LENGTH[a], LENGTH[b]} == {J.LDS_LIST + 1, 6000}
    mid = keys[keys.index(b) + 1]
    assert LENGTH[mid] == 600 and keys.index(mid) < len(keys) - 1             # not far, between other keys
    fill = lambda k: {e[0] for e in P.concatenated(c, k) if e[0] not in P.CHAIN_BRANCHES}
    assert fill(a) <= fill(b) and fill(mid) <= fill(a) and fill(far[0]) == fill(a) and len(fill(mid)) == 550


@pytest.mark.parametrize("reverse", [False, True], ids=["in_order", "reversed"])
def test_chains_winners(reverse):
    """The restatement keeps the table's shard in every row at every length, by score bits and by position, at the branch's first
    place; reversed, the first place moves and other shards win."""
    c = P.case("chains")
    want = c["want_reversed" if reverse else "want"]
    changed = set()
    for ki, (key, n) in enumerate(P.CHAIN_KEYS):
        br, sc, pos = P.joined(want, key)
        cat = P.concatenated(c if not reverse else dict(shards=c["shards"][::-1]), key)
        seen, firsts = set(), []
        for b, _, _ in cat:
            if b not in seen:
                seen.add(b); firsts.append(b)
        assert list(br) == firsts                                            # every branch once, at its first place
        got = P.kept_rows(br, sc, pos)
        if not reverse:
            assert got == P.table_rows(ki), [(P.ROW_NAMES[r], n) for r in range(14) if got[r] != P.table_rows(ki)[r]]
            rows = dict(zip(P.ROW_NAMES, got))
            assert rows["NaN first"][0] == 0x7FC00000 and rows["NaN between"][0] == bits(-2.0) and rows["negative NaN"][0] == bits(-2.0)
            assert rows["zeros a"][0] == 0x80000000 and rows["zeros b"][0] == 0 and rows["infinities"][0] == 0x7F800000
            # `late`: first held by shard 2, so it stands in shard 2's stretch of the concatenated list, with shard 3's score
            sizes = [len(J.lists_of(s)[key]) for s in c["shards"]]
            at = [e[0] for e in cat].index(P.CHAIN_BRANCHES[P.ROW_NAMES.index("late")])
            assert sizes[0] + sizes[1] <= at < sizes[0] + sizes[1] + sizes[2]
            assert rows["late"] == (bits(-1.0), P.chain_pos(ki, 3, 13))
        else:
            assert all(g is not None for g in got)
            changed |= {P.ROW_NAMES[r] for r in range(14) if got[r] != P.table_rows(ki)[r]}
    if reverse:
        # the walk 3, 2, 1, 0: ties go to shard 3 now, the NaN that stands first in `NaN between` is kept, and `NaN first`'s comes last
        assert changed == {"peak", "equal", "zeros a", "zeros b", "NaN first", "NaN between"}, changed


def test_slot_alias():
    c = P.case("slot_alias")
    a, b = c["shards"]
    assert a["br"].max() < 1000 and b["br"].min() >= 1 << 18
    assert not set(a["br"].tolist()) & set(b["br"].tolist())                  # no equal branch anywhere
    assert {x % J.BRANCH_SLOTS for x in b["br"].tolist()} <= set(a["br"].tolist())     # every branch of shard 1 shares a slot with one of shard 0
    shared = set(a["keys"].tolist()) & set(b["keys"].tolist())
    assert len(shared) == P.SLOT_KEYS == 40 and len(set(a["keys"].tolist()) ^ set(b["keys"].tolist())) == 8
    for k in shared:
        la, lb = J.lists_of(a)[k], J.lists_of(b)[k]
        assert len(la) == len(lb) == 3 and [e[0] + (1 << 18) for e in la] == [e[0] for e in lb]
    w = c["want"]
    assert w["route"] == 1 and w["dropped"] == 0 and w["shared_keys"] == 40
    for k in w["keys"]:                                                      # the plain concatenation
        assert [e[0] for e in P.concatenated(c, int(k))] == list(P.joined(w, int(k))[0])
    assert len(w["br"]) == len(a["br"]) + len(b["br"])


def test_high_keys():
    c = P.case("high_keys")
    assert c["header"]["kmer_size"] == 16
    w = c["want"]
    for key in (0, 2 ** 31 - 1, 2 ** 31, 0xFFFFFFFF):
        per = [J.lists_of(s).get(key) for s in c["shards"]]
        assert all(p for p in per), key
        cat = [e[0] for e in P.concatenated(c, key)]
        assert len(cat) - len(set(cat)) == 1 == len(cat) - len(P.joined(w, key)[0])   # one duplicated branch each
    assert len(P.concatenated(c, 2 ** 31)) == 70 > J.WAVE_LIST
    assert w["dropped"] == 4 and w["shared_keys"] == 4 and w["route"] == 1
    for s in c["shards"]:                                                    # keys of its own on both sides of 2^31
        own = [int(k) for k in s["keys"] if int(k) not in P.HIGH_KEYS]
        assert sum(k < 2 ** 31 for k in own) >= 2 and sum(k > 2 ** 31 for k in own) >= 2
    # the later score wins in some keys and the earlier one in others
    later = 0
    for key in P.HIGH_KEYS:
        cat = P.concatenated(c, key)
        dup = [e for e in cat if [x[0] for x in cat].count(e[0]) == 2]
        br, sc, pos = P.joined(w, key)
        at = int(np.flatnonzero(br == np.uint32(dup[0][0]))[0])
        assert pos[at] == (dup[1][2] if dup[1][1] > dup[0][1] else dup[0][2]) and dup[0][1] != dup[1][1]
        later += bool(dup[1][1] > dup[0][1])
    assert later == 2


def test_locate():
    c = P.case("locate")
    lists = [J.lists_of(s) for s in c["shards"]]
    assert [len(p[300]) for p in lists] == [0, 40, 40, 10]
    assert lists[1][300][5][0] == 9 and lists[3][300][-1][0] == 9 and 9 not in [e[0] for e in lists[2][300]]
    assert [e[0] for e in lists[0][400]].count(3) == 1 and [e[0] for e in lists[1][400]].count(3) == 1
    assert len(P.concatenated(c, 300)) == 90 > J.WAVE_LIST
    # the concatenated layout: keys ascending, per key the shards' lists; the dropped entries' indices
    keys = [int(k) for k in c["want"]["keys"]]
    assert keys[0] < 300                                                     # key 300 is not the first: its runs' offsets are not 0
    dropped, at = [], 0
    for k in keys:
        seen = set()
        for b, _, _ in P.concatenated(c, k):
            if b in seen:
                dropped.append((at, k, b))
            seen.add(b); at += 1
    assert len(dropped) == c["want"]["dropped"] == 2
    assert min(dropped) == (len(P.concatenated(c, 100)) + 89, 300, 9)        # the smallest lies in key 300: its last entry


# ---- the cases discriminate: three wrong walkers ------------------------------------------------------------------------------------------

def code(s):
    """the order-preserving integer code of a score (enc_score_bits, dcla_device.hpp)"""
    u = bits(s)
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else u | 0x80000000


def walk(c, replaces, against_first=False):
    """{key index: per chain row (score bits, position)} of a per-key walk with the rule `replaces(later, reference)`; the reference is
    the kept score, or (against_first) the first occurrence's"""
    per = [J.lists_of(s) for s in c["shards"]]
    out = {}
    for ki, (key, _) in enumerate(P.CHAIN_KEYS):
        kept = {}
        for p in per:
            for b, s, w in p[key]:
                if b not in kept:
                    kept[b] = [s, s, w]
                elif replaces(s, kept[b][0] if against_first else kept[b][1]):
                    kept[b][1:] = [s, w]
        out[ki] = [(bits(kept[b][1]), kept[b][2]) for b in P.CHAIN_BRANCHES]
    return out


def rows_that_differ(got, positioned):
    """the rows a walk differs from the table on -- the same rows in every key"""
    per_key = []
    for ki in range(len(P.CHAIN_KEYS)):
        want = P.table_rows(ki)
        per_key.append({P.ROW_NAMES[r] for r in range(14) if (got[ki][r] if positioned else got[ki][r][0]) != (want[r] if positioned else want[r][0])})
    assert all(d == per_key[0] for d in per_key)
    return per_key[0]


WRONG = {
    # compares with the first occurrence's score: keeps the LAST score greater than the first
    "first_score": (dict(replaces=lambda s, ref: np.float32(s) > np.float32(ref), against_first=True), {"infinities"}, {"peak", "infinities"}),
    # >= : a tie goes to the later occurrence
    "greater_or_equal": (dict(replaces=lambda s, ref: np.float32(s) >= np.float32(ref)), {"zeros a", "zeros b"}, {"peak", "equal", "zeros a", "zeros b"}),
    # integer codes: +0.0 above -0.0, a positive NaN above everything
    "integer_codes": (dict(replaces=lambda s, ref: code(s) > code(ref)), {"zeros a", "NaN between"}, {"zeros a", "NaN between"}),
}


def test_the_right_walker_is_the_table():
    got = walk(P.case("chains"), lambda s, ref: np.float32(s) > np.float32(ref))
    assert rows_that_differ(got, False) == set() and rows_that_differ(got, True) == set()


@pytest.mark.parametrize("name", sorted(WRONG))
def test_wrong_walkers_differ_on_named_rows(name):
    args, plain, positioned = WRONG[name]
    got = walk(P.case("chains"), **args)
    assert rows_that_differ(got, False) == plain and plain
    assert rows_that_differ(got, True) == positioned
