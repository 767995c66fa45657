"""Cases for the duplicate stage of the join (ipkgpu_db_join; kernels_dbjoin.hpp), written against its branch points; the expectation is
tests/join_cases.restate, unchanged.  Shared by tests/test_join_paths_inputs.py (CPU: the cases are what they claim) and
tests/test_gpu_join_paths.py (GPU: every resolver against the restatement, bit for bit).  Not a test file.

`chains`       the same 14 chain rows (CHAIN_ROWS: one branch, a score per shard, the shard whose score and position are kept) in one
               key per concatenated length of CHAIN_KEYS, every key held by four shards: a branch that occurs three and four times,
               ties, -0.0 against +0.0, one-ulp steps, NaN of either sign and both infinities meet the wavefront kernel (64), the LDS
               kernel at every padded size (65 .. 4096) and the sorted pass (4097, 6000, with the same filler branches in neighbouring
               keys); the rows' branches are the values the kernels use as sentinels (0xFFFFFFFF, 0) and ids at and above 2^18.
`slot_alias`   two shards whose branches differ by 2^18 exactly: every slot of the hashed branch table is shared, no branch is.
`high_keys`    keys 0, 2^31 - 1, 2^31 and 0xFFFFFFFF in both shards, a duplicate in each.
`locate`       the first dropped entry lies in a 90-entry list whose first run has no entries; first held by source 1, again by source 3."""
import functools

import numpy as np

from tests import join_cases as J
from tests import union_cases as U

K8, K16 = U.K8, U.K16
N_SHARDS = 4
X = np.float32(-1.5)


def up(x, n):
    """x moved n ulps towards 0"""
    for _ in range(n):
        x = np.nextafter(np.float32(x), np.float32(0))
    return np.float32(x)


NAN = np.uint32(0x7FC00000).view(np.float32)
NEG_NAN = np.uint32(0xFFC00000).view(np.float32)
INF = np.float32(np.inf)
# (the row, its scores in shards 0, 1, 2, 3 -- None: the shard does not hold the branch --, the shard whose score and position are kept)
CHAIN_ROWS = [
    ("rising", [-4.0, -3.0, -2.0, -1.0], 3),
    ("falling", [-1.0, -2.0, -3.0, -4.0], 0),
    ("peak", [-3.0, -1.0, -2.0, -1.0], 1),
    ("equal", [-1.0, -1.0, -1.0, -1.0], 0),
    ("zeros a", [-0.0, 0.0, -0.0, 0.0], 0),
    ("zeros b", [0.0, -0.0, None, -0.0], 0),
    ("ulp up", [X, up(X, 1), up(X, 1), up(X, 2)], 3),
    ("ulp down", [up(X, 2), up(X, 1), X, up(X, 1)], 0),
    ("NaN first", [NAN, -1.0, -2.0, -0.5], 0),
    ("NaN between", [-3.0, NAN, -2.0, NAN], 2),
    ("negative NaN", [-3.0, NEG_NAN, -2.0, None], 2),
    ("infinities", [-INF, -1.0, INF, 5.0], 2),
    ("sparse", [-4.0, None, None, -3.5], 3),
    ("late", [None, None, -2.0, -1.0], 3),
]
CHAIN_ROWS = [(what, [None if s is None else np.float32(s) for s in scores], kept) for what, scores, kept in CHAIN_ROWS]
ROW_NAMES = [r[0] for r in CHAIN_ROWS]
CHAIN_BRANCHES = [0xFFFFFFFF, 0, 1 << 31, (1 << 18) + 5] + list(range(11, 21))     # the branch of row r
N_OCCURRENCES = sum(s is not None for r in CHAIN_ROWS for s in r[1])                # 50
# (key, concatenated length): a far key (beyond LDS_LIST) first, two more at adjacent keys neither first nor last, the 600-entry key behind them
CHAIN_KEYS = [(100, 4097), (200, 64), (210, 65), (220, 129), (230, 257), (300, 4097), (301, 6000), (310, 600), (320, 1500), (330, 4096)]
# the filler branches, the same in every key (a key takes a prefix): first the neighbours of the rows' branches in sorted order, then
# ids below and at or above 2^18 in turn; none shares a slot of the branch table with a row's branch
FILLERS = [0xFFFFFFFE, 1, 0x80000001, (1 << 18) + 4, (1 << 18) + 6, 2] + \
          [1000 + i if i % 2 == 0 else ((i % 5) + 1 << 18) + 5000 + i for i in range(6000)]


def chain_pos(key_index, shard, row):
    """the position of a row's occurrence: different for every (key, shard, row)"""
    return 1 + row + 16 * shard + 64 * key_index


def resolver(length):
    """the kernel that resolves a list of this concatenated length"""
    return "wave" if length <= J.WAVE_LIST else "lds" if length <= J.LDS_LIST else "sorted"


def padded(length):
    """the size the LDS kernel's bitonic sort runs at"""
    p = 2 * J.WAVE_LIST
    while p < length:
        p *= 2
    return p


def chains():
    rng = np.random.default_rng(41)
    lists = [[] for _ in range(N_SHARDS)]
    for ki, (key, n) in enumerate(CHAIN_KEYS):
        fill_at = 0
        for s in range(N_SHARDS):
            n_s = n // N_SHARDS + (s < n % N_SHARDS)
            rows = [r for r in range(len(CHAIN_ROWS)) if CHAIN_ROWS[r][1][s] is not None]
            rot = (ki + 3 * s) % len(rows)
            rows = rows[rot:] + rows[:rot]                                  # the rows in the order of their places: the first and the last vary
            inner = np.sort(rng.choice(np.arange(1, n_s - 1), size=len(rows) - 2, replace=False))
            row_at = dict(zip([0] + [int(i) for i in inner] + [n_s - 1], rows))
            lst = []
            for i in range(n_s):
                if i in row_at:
                    r = row_at[i]
                    lst.append((CHAIN_BRANCHES[r], CHAIN_ROWS[r][1][s], chain_pos(ki, s, r)))
                else:
                    lst.append((FILLERS[fill_at], np.float32(-6.0 * rng.random()), 1024 + (7 * fill_at + ki) % 64000))
                    fill_at += 1
            lists[s].append(lst)
    keys = [k for k, _ in CHAIN_KEYS]
    return dict(name="chains", header=K8, shards=[J.shard(keys, lists[s], 40 + s) for s in range(N_SHARDS)])


SLOT_KEYS = 40


def slot_alias():
    rng = np.random.default_rng(42)
    keys = [[], []]
    lists = [[], []]
    used = []
    for i in range(SLOT_KEYS):
        br = rng.permutation(1000)[:3]
        used += [int(b) for b in br]
        for s in range(2):
            keys[s].append(1000 + 3 * i)
            lists[s].append([(int(b) + (s << 18), np.float32(-6.0 * rng.random()), 100 * i + 10 * s + j) for j, b in enumerate(br)])
    for i in range(8):                                                      # keys that one shard holds alone, among and behind the shared ones
        s = i % 2
        keys[s].append(1001 + 15 * i)
        lists[s].append([(int(b) + (s << 18), np.float32(-3.0), 5000 + i) for b in rng.choice(sorted(set(used)), size=2, replace=False)])
    out = []
    for s in range(2):
        order = np.argsort(keys[s])
        out.append(J.shard([keys[s][i] for i in order], [lists[s][i] for i in order], 50 + s))
    return dict(name="slot_alias", header=K8, shards=out)


HIGH_KEYS = [0, 2 ** 31 - 1, 2 ** 31, 0xFFFFFFFF]
HIGH_LDS_KEY, HIGH_LDS_LEN = 2 ** 31, 70


def high_keys():
    rng = np.random.default_rng(43)
    alone = [[5, 2 ** 31 - 7, 2 ** 31 + 9, 0xFFFFFFF0], [77, 2 ** 31 - 3, 2 ** 31 + 2, 0xFFFFFFFE]]
    keys = [list(HIGH_KEYS) + alone[s] for s in range(2)]
    lists = [[], []]
    for i, key in enumerate(HIGH_KEYS):
        n = HIGH_LDS_LEN if key == HIGH_LDS_KEY else 7
        br = rng.permutation(5000)[:n - 1] + 10
        cut = n // 2
        a = [int(b) for b in br[:cut]]
        b = [int(x) for x in br[cut:]] + [a[i % cut]]                      # shard 1's last branch is one of shard 0's
        greater = i % 2                                                    # the later score is the greater one in every other key
        sc = lambda s, last: np.float32(-2.0 if (s == greater and last) else -3.0 if last else -6.0 * rng.random())
        lists[0].append([(x, sc(0, x == b[-1]), 100 * i + j) for j, x in enumerate(a)])
        lists[1].append([(x, sc(1, j == len(b) - 1), 100 * i + 50 + j) for j, x in enumerate(b)])
    for s in range(2):
        for j, key in enumerate(alone[s]):
            lists[s].append([(int(x), np.float32(-4.0), 1000 + 10 * s + j) for x in rng.permutation(5000)[:3]])
    out = []
    for s in range(2):
        order = np.argsort(np.array(keys[s], np.uint64))
        out.append(J.shard([keys[s][i] for i in order], [lists[s][i] for i in order], 60 + s))
    return dict(name="high_keys", header=K16, shards=out)


LOCATE_KEY, LOCATE_BRANCH = 300, 9


def locate():
    rng = np.random.default_rng(44)
    other = [int(b) for b in rng.permutation(3000)[:200] + 20]
    e = lambda b, i: (b, np.float32(-6.0 * rng.random()), i + 1)
    s1 = [e(b, i) for i, b in enumerate(other[:40])]
    s1[5] = e(LOCATE_BRANCH, 5)
    s2 = [e(b, 100 + i) for i, b in enumerate(other[40:80])]
    s3 = [e(b, 200 + i) for i, b in enumerate(other[80:89])] + [e(LOCATE_BRANCH, 209)]
    shards = [
        J.shard([LOCATE_KEY, 400], [[], [e(3, 300), e(4, 301)]], 70),
        J.shard([LOCATE_KEY, 400], [s1, [e(5, 310), e(3, 311)]], 71),
        J.shard([100, LOCATE_KEY], [[e(b, 400 + i) for i, b in enumerate(other[100:105])], s2], 72),
        J.shard([100, LOCATE_KEY], [[e(b, 500 + i) for i, b in enumerate(other[110:113])], s3], 73),
    ]
    return dict(name="locate", header=K8, shards=shards)


CASE_NAMES = ["chains", "slot_alias", "high_keys", "locate"]


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every case, built once, with the restatement's result (and that of `chains` in reversed shard order); the arrays are shared by
    the tests and must not be changed."""
    cs = [chains(), slot_alias(), high_keys(), locate()]
    for c in cs:
        c["want"] = J.restate(c["shards"])
    cs[0]["want_reversed"] = J.restate(cs[0]["shards"][::-1])
    return tuple(cs)


def case(name):
    return next(c for c in all_cases() if c["name"] == name)


def joined(want, key):
    """(branches, scores, positions) of the key's joined list"""
    i = int(np.searchsorted(want["keys"], key))
    assert want["keys"][i] == key
    a, b = int(want["off"][i]), int(want["off"][i + 1])
    return want["br"][a:b], want["sc"][a:b], want["pos"][a:b]


def concatenated(c, key):
    return [e for s in c["shards"] for e in J.lists_of(s).get(key, [])]


def kept_rows(br, sc, pos):
    """per chain row: (score bits, position) of the row's branch in a joined list, None where the branch is absent or not unique"""
    out = []
    for b in CHAIN_BRANCHES:
        at = np.flatnonzero(br == np.uint32(b))
        out.append((int(sc[at[0]].view(np.uint32)), int(pos[at[0]])) if len(at) == 1 else None)
    return out


def table_rows(key_index):
    """per chain row: (score bits, position) the table asks for in key CHAIN_KEYS[key_index]"""
    return [(int(scores[kept].view(np.uint32)), chain_pos(key_index, kept, r)) for r, (_, scores, kept) in enumerate(CHAIN_ROWS)]
