"""Cases for the join of databases that share k-mers (ipkgpu_db_join, Engine.join_dbs, `ipk.py merge --shared-keys`) and a numpy
restatement of the join's definition (include/ipkgpu.h): the set union of the keys; per key the sources' lists concatenated in source
order; a branch that occurs again kept once, at its first place, with `put`'s maximum (a later score replaces the kept one only if it
is strictly greater as a float; the position goes with the kept score).  The restatement is a direct per-key walk.

A case is a dict: name, header, shards -- each a database in host arrays as tests/db_files.synthetic makes them (keys, off, br, sc, pos,
fv, order), written as files by write_shards -- and want, the restatement's result with the counts the join reports: shared_keys (keys
held by more than one shard), dropped (entries dropped as duplicates), route (1 where some key lies in two shards and some branch, taken
modulo BRANCH_SLOTS, lies in two shards: the device then resolves duplicates; 0: it only concatenates).  Every case serves plain and positioned."""
import functools

import numpy as np

from ipk_amd import dbfile
from tests import db_files as F
from tests import union_cases as U

TILE = U.TILE
K8 = U.K8
BRANCH_SLOTS = 1 << 18                                 # DB_JOIN_BRANCH_SLOTS (kernels_dbjoin.hpp)
WAVE_LIST, LDS_LIST = 64, 4096                         # DB_JOIN_WAVE_LIST, DB_JOIN_LDS_LIST: the list lengths at which the duplicate stage changes kernels


def shard(keys, lists, seed=0):
    """A shard from ascending keys and per key a list of (branch, score, position); filter values are random (the join ignores them)."""
    keys = np.asarray(keys, np.uint32)
    assert len(keys) == len(lists) and np.all(keys[1:] > keys[:-1])
    cnt = np.array([len(x) for x in lists], np.int64)
    flat = [e for x in lists for e in x]
    rng = np.random.default_rng(1000 + seed)
    fv = (rng.random(len(keys)) * 4.0 - 2.0).astype(np.float32)
    return dict(keys=keys, off=np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64), br=np.array([e[0] for e in flat], np.uint32),
                sc=np.array([e[1] for e in flat], np.float32), pos=np.array([e[2] for e in flat], np.uint32), fv=fv,
                order=np.argsort(dbfile.filter_sort_code(fv, keys), kind="stable").astype(np.uint32))


def lists_of(db):
    """{key: [(branch, score, position), ...]} of a database in host arrays."""
    off = db["off"].astype(np.int64)
    return {int(k): [(int(db["br"][e]), db["sc"][e], int(db["pos"][e])) for e in range(off[i], off[i + 1])] for i, k in enumerate(db["keys"])}


def restate(shards):
    """The join of the shards by the definition: a plain walk, key by key and occurrence by occurrence."""
    per = [lists_of(s) for s in shards]
    keys = sorted(set().union(*[set(p) for p in per])) if per else []
    out, shared, dropped = [], 0, 0
    for k in keys:
        holders = [p for p in per if k in p]
        shared += len(holders) > 1
        kept, at = [], {}
        for p in holders:
            for b, s, w in p[k]:
                if b not in at:
                    at[b] = len(kept)
                    kept.append([b, s, w])
                else:
                    dropped += 1
                    if np.float32(s) > np.float32(kept[at[b]][1]):
                        kept[at[b]][1], kept[at[b]][2] = s, w
        out.append(kept)
    cnt = np.array([len(x) for x in out], np.int64)
    flat = [e for x in out for e in x]
    seen, route = {}, 0
    for i, s in enumerate(shards):
        for b in np.unique(s["br"] % BRANCH_SLOTS):
            if seen.setdefault(int(b), i) != i:
                route = 1
    route = route if shared else 0                                   # no key in two shards: nothing to resolve
    return dict(keys=np.array(keys, np.uint32), off=np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64),
                br=np.array([e[0] for e in flat], np.uint32), sc=np.array([e[1] for e in flat], np.float32), pos=np.array([e[2] for e in flat], np.uint32),
                shared_keys=int(shared), dropped=int(dropped), route=route)


def with_filter(want, fv):
    """want with filter values and the order that goes with them (what a written file needs)."""
    fv = np.asarray(fv, np.float32)
    return dict(want, fv=fv, order=np.argsort(dbfile.filter_sort_code(fv, want["keys"]), kind="stable").astype(np.uint32))


def split_entries(db, owner_of_entry, n_owners, keep_empty=False):
    """One shard per owner: owner_of_entry[e] is the owner of entry e; a key goes to every owner that holds one of its entries
    (keep_empty: and, entry-less, to owner 0 if it has no entries at all)."""
    off = db["off"].astype(np.int64)
    all_lists = lists_of(db)
    out = []
    for o in range(n_owners):
        keys, lists = [], []
        for i, k in enumerate(db["keys"]):
            mine = [e for e, j in zip(all_lists[int(k)], range(off[i], off[i + 1])) if owner_of_entry[j] == o]
            if mine or (keep_empty and o == 0 and off[i] == off[i + 1]):
                keys.append(int(k)); lists.append(mine)
        out.append(shard(keys, lists, seed=o))
    return out


def branch_ranges():
    """One synthetic database split by branch into 3 shards (branch < 1300, < 2700, the rest): keys held by one, two and all three
    shards, no branch in two shards of a key -- and none in two shards at all, for a key's branches are a range's."""
    db = F.synthetic(300, seed=31, k=8)
    owner = np.where(db["br"] < 1300, 0, np.where(db["br"] < 2700, 1, 2))
    return dict(name="branch_ranges", header=K8, shards=split_entries(db, owner, 3))


DUP_KEY = 1000                                         # the keys of `duplicates`: DUP_KEY + i for the i-th row of DUP_ROWS
ULP = np.nextafter(np.float32(-1.5), np.float32(0))
# (what the row shows, the scores of branch 7 in shards 0, 1, 2 -- None: the shard does not hold it --, the shard whose score wins)
DUP_ROWS = [
    ("later greater", [-3.0, -2.0, None], 1),
    ("earlier greater", [-2.0, -3.0, None], 0),
    ("equal bits", [-2.5, -2.5, None], 0),
    ("-0.0 before +0.0", [-0.0, 0.0, None], 0),
    ("+0.0 before -0.0", [0.0, -0.0, None], 0),
    ("one ulp up", [-1.5, ULP, None], 1),
    ("one ulp down", [ULP, -1.5, None], 0),
    ("three shards, the last greatest", [-3.0, -2.0, -1.0], 2),
    ("three shards, the middle greatest", [-3.0, -1.0, -2.0], 1),
    ("three shards, equal", [-1.0, -1.0, -1.0], 0),
    ("first and third only", [-4.0, None, -3.5], 2),
]


def duplicates():
    """The same (key, branch 7) in two and in three shards, one key per row of DUP_ROWS; every position is different
    (100 * shard + row), and every shard holds other branches around the shared one."""
    shards = []
    for s in range(3):
        keys, lists = [], []
        for i, (_, scores, _) in enumerate(DUP_ROWS):
            lst = [(20 + s, np.float32(-5.0), 1000 + 10 * s + i)]
            if scores[s] is not None:
                lst.append((7, np.float32(scores[s]), 100 * s + i))
            lst.append((30 + s, np.float32(-5.5), 2000 + 10 * s + i))
            keys.append(DUP_KEY + i); lists.append(lst)
        shards.append(shard(keys, lists, seed=s))
    return dict(name="duplicates", header=K8, shards=shards)


def first_place():
    """Key 500: shard 0 holds branches (9, 4, 6), shard 1 (2, 4, 1) with the greater score of 4, shard 2 (8): the joined list is
    9 4 6 2 1 8 -- branch 4 at its FIRST place (index 1, with shard 1's score), not at the winner's (index 4) and not in branch order."""
    s0 = shard([500], [[(9, np.float32(-1.0), 1), (4, np.float32(-3.0), 2), (6, np.float32(-1.5), 3)]], 0)
    s1 = shard([500], [[(2, np.float32(-2.0), 4), (4, np.float32(-2.0), 5), (1, np.float32(-2.5), 6)]], 1)
    s2 = shard([500], [[(8, np.float32(-0.5), 7)]], 2)
    return dict(name="first_place", header=K8, shards=[s0, s1, s2])


WAVE_LENGTHS = [1, 2, 63, 64, 65, 128, 129]


def _pair_list(n, lanes, rng, cut):
    """Two lists whose concatenation has n entries of distinct branches except that the entries at the two lanes are one branch;
    the first list has `cut` entries."""
    br = rng.permutation(3000)[:n] + 10
    a, b = lanes
    br[b] = br[a]
    sc = (-6.0 * rng.random(n)).astype(np.float32)
    full = [(int(br[i]), sc[i], 7 * i + 1) for i in range(n)]
    return full[:cut], full[cut:]


def wave_edges():
    """Joined lists of 1, 2, 63, 64, 65, 128 and 129 entries; from 2 on with a duplicate pair at lanes (0, last), and from 65 on a
    second key with the pair at lanes (63, 64).  Key 100 + 2 i: pair (0, last); key 101 + 2 i: pair (63, 64)."""
    rng = np.random.default_rng(33)
    k0, l0, k1, l1 = [], [], [], []
    for i, n in enumerate(WAVE_LENGTHS):
        if n == 1:
            k0.append(100); l0.append([(5, np.float32(-1.0), 3)])
            continue
        cut = max(1, n // 2)
        a, b = _pair_list(n, (0, n - 1), rng, cut)
        k0.append(100 + 2 * i); l0.append(a); k1.append(100 + 2 * i); l1.append(b)
        if n >= 65:
            a, b = _pair_list(n, (63, 64), rng, 64)
            k0.append(101 + 2 * i); l0.append(a); k1.append(101 + 2 * i); l1.append(b)
    return dict(name="wave_edges", header=K8, shards=[shard(k0, l0, 0), shard(k1, l1, 1)])


def long_lists():
    """Key 40: 6000 entries from 3 shards (2000 each, branches below 6000) with 50 duplicates; key 41: 20000 entries from 2 shards
    with 1 duplicate (the first shard's first branch is the second shard's last).  These leave a wavefront and leave LDS."""
    rng = np.random.default_rng(34)
    br = rng.permutation(6000)[:5950]
    parts = [list(br[:2000]), list(br[2000:4000]), list(br[4000:5950])]
    parts[2] += list(rng.choice(br[:2000], size=25, replace=False)) + list(rng.choice(br[2000:4000], size=25, replace=False))
    big = rng.permutation(100000)[:19999]
    big_parts = [list(big[:10000]), list(big[10000:]) + [big[0]]]
    # keys 42, 43: 4096 and 4097 entries from 2 shards with 30 duplicates each -- the last list LDS holds and the first it does not
    edge = {}
    for key, n in ((42, LDS_LIST), (43, LDS_LIST + 1)):
        e = rng.permutation(50000)[:n - 30]
        edge[key] = [list(e[:n // 2]), list(e[n // 2:]) + list(rng.choice(e[:n // 2], size=30, replace=False))]
    entry = lambda b: (int(b), np.float32(-6.0 * rng.random()), int(rng.integers(0, 65536)))
    shards = []
    for s in range(3):
        keys, lists = [40], [[entry(b) for b in parts[s]]]
        if s < 2:
            keys.append(41); lists.append([entry(b) for b in big_parts[s]])
            for key in (42, 43):
                keys.append(key); lists.append([entry(b) for b in edge[key][s]])
        shards.append(shard(keys, lists, s))
    return dict(name="long_lists", header=K8, shards=shards)


def tiles():
    """The union's `tiles` counts, each such key split over two shards: a key whose joined list has exactly TILE entries, one with
    5000, and a run of 1100 one-entry keys that alternate between the shards."""
    counts = [TILE, 5000, 3, 7] + [1] * U.TILES_RUN + [2, 65, 300]
    rng = np.random.default_rng(35)
    keys = np.sort(rng.choice(4 ** 8, size=len(counts), replace=False))
    db = F.synthetic(seed=35, k=8, keys=keys, counts=counts, n_branches=6000)
    off = db["off"].astype(np.int64)
    owner = np.zeros(len(db["br"]), np.int64)
    for i, c in enumerate(counts):
        if c == 1:
            owner[off[i]] = i % 2
        else:
            owner[off[i] + c // 2:off[i + 1]] = 1                  # the second half of the list goes to shard 1
    return dict(name="tiles", header=K8, shards=split_entries(db, owner, 2))


def many_sources():
    """66 shards: 65 that all hold key 77, each with a branch of its own and a few keys of its own, and shard 40, which is empty;
    the last shard repeats shard 0's branch of key 77 with a greater score."""
    rng = np.random.default_rng(36)
    shards = []
    for s in range(66):
        if s == 40:
            shards.append(shard([], [], s))
            continue
        b = 0 if s == 65 else s
        keys = [77] + [1000 + 10 * s + j for j in range(1 + s % 3)]
        lists = [[(b, np.float32(-1.0 if s == 65 else -2.0 - s / 100), s)]] + [[(int(x), np.float32(-3.0), 5) for x in rng.permutation(500)[:2]] for _ in keys[1:]]
        shards.append(shard(keys, lists, s))
    return dict(name="many_sources", header=K8, shards=shards)


def entryless():
    """Key 10: entry-less in shard 0, three entries in shard 1; key 20: entry-less in both; key 30: entries in both."""
    s0 = shard([10, 20, 30], [[], [], [(1, np.float32(-1.0), 1), (2, np.float32(-2.0), 2)]], 0)
    s1 = shard([10, 20, 30], [[(3, np.float32(-1.0), 3), (4, np.float32(-2.0), 4), (5, np.float32(-2.0), 5)], [], [(6, np.float32(-3.0), 6)]], 1)
    return dict(name="entryless", header=K8, shards=[s0, s1])


def disjoint():
    """A key-disjoint split (union_cases.split): the join is the union."""
    db = F.synthetic(300, seed=37, k=8)
    return dict(name="disjoint", header=K8, shards=U.split(db, db["keys"] % 3, 3))


CASE_NAMES = ["branch_ranges", "duplicates", "first_place", "wave_edges", "long_lists", "tiles", "many_sources", "entryless", "disjoint"]


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every case, built once; the arrays are shared by the tests and must not be changed."""
    cs = [branch_ranges(), duplicates(), first_place(), wave_edges(), long_lists(), tiles(), many_sources(), entryless(), disjoint()]
    for c in cs:
        c["want"] = restate(c["shards"])
    return tuple(cs)


def case(name):
    return next(c for c in all_cases() if c["name"] == name)


def write_shards(directory, c, positioned):
    return [str(F.write(directory / f"{c['name']}_{int(positioned)}_shard{i}.ipk", s, positioned, c["header"])) for i, s in enumerate(c["shards"])]
