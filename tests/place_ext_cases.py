"""Fabricated databases and queries of the tests of ipkgpu_db_place_opts (tests/test_place_ext_inputs.py on the host,
tests/test_gpu_place_ext.py on the device): built once per process from fixed seeds, never changed afterwards.  The queries are
written first; the keys of a database are then drawn from the resolutions of their windows, and planted groups of keys give the
ambiguous windows whose resolutions, entry counts and shared branches the tests name."""
import functools

import numpy as np

from tests import place_cases as pc
from tests import place_ext_oracle as xo
from tests import place_oracle as po

LOG_EPS = pc.LOG_EPS
K = 8


class ExtCase(pc.Case):
    """A Case placed with options: expected(keep, ambiguity, strands) is the oracle's, computed once."""

    @functools.lru_cache(maxsize=None)
    def expected(self, keep, ambiguity=True, strands="given", variant=None):
        return xo.place(self.view, self.queries, self.sigma, self.k, LOG_EPS, keep, ambiguity, strands, variant)


def _rand(rng, n, letters="ACGT"):
    return "".join(rng.choice(list(letters), n))


def _assemble(rng, lists, n_branches):
    """The database arrays of {key: (branches, scores) or a count}: a count draws that many distinct random branches (make_db)."""
    keys = sorted(lists)
    counts = [lists[c] if isinstance(lists[c], int) else len(lists[c][0]) for c in keys]
    kk, off, br, sc = pc.make_db(rng, keys, n_branches, counts)
    for i, c in enumerate(keys):
        if not isinstance(lists[c], int):
            a, b = int(off[i]), int(off[i + 1])
            br[a:b], sc[a:b] = lists[c][0], lists[c][1]
    return kk, off, br, sc


def _codes(window, sigma):
    """The resolution codes of one k-long string with at most one ambiguous symbol."""
    (_, codes), = xo.windows(window, sigma, len(window))
    return codes


def _group(rng, lists, window, counts, shares, n_branches, sigma=4):
    """Plants the resolutions of `window` as keys: resolution r with counts[r] entries (0: no key); shares = {branch: resolutions that
    name it}; the other entries name random branches outside `shares`."""
    codes = _codes(window, sigma)
    pool = np.setdiff1d(np.arange(n_branches), list(shares))
    for r, code in enumerate(codes):
        lists.pop(code, None)
        if counts[r] == 0:
            continue
        mine = [b for b, rs in shares.items() if r in rs]
        br = np.concatenate([rng.choice(pool, counts[r] - len(mine), replace=False), mine]).astype(np.uint32)
        br = br[rng.permutation(len(br))]
        lists[code] = (br, pc.mixed_scores(rng, len(br)))


# planted windows of main_ext_case (k = 8), by name: (window, entries per resolution, {branch: resolutions naming it})
GROUPS = {
    "all4": ("ACGTNACG", [63, 64, 65, 129], {7: [2], 8: [0, 3], 9: [0, 1, 2], 10: [0, 1, 2, 3]}),
    "all3": ("TTGBCAGT", [20, 31, 9], {7: [1], 8: [0, 2], 9: [0, 1, 2]}),
    "all2": ("GGATCRTA", [12, 40], {7: [0], 8: [0, 1]}),
    "one": ("CATGANCC", [0, 0, 17, 0], {}),
    "none": ("TGNCATCA", [0, 0, 0, 0], {}),
}


@functools.lru_cache(maxsize=None)
def main_ext_case():
    """DNA k = 8, branches below 300.  Queries (numbered in the list below): an ambiguous symbol at every position of a window, at query
    positions 0, 63, 64, 70 and in the last symbol, two of them 8 and 4 apart, NN, every DNA code, lower case, -, *, ? and X, the
    planted GROUPS alone and between exact windows, long queries of several tiles."""
    rng = np.random.default_rng(8801)
    r = lambda n: _rand(rng, n)
    g = {n: w for n, (w, _, _) in GROUPS.items()}
    every = "".join(r(8) + c for c in "RYSWKMBDHVN") + r(8)
    q = [
        r(7) + "N" + r(7),                                                   # 0: 8 consecutive ambiguous windows, N at positions 7 .. 0
        "N" + r(80),                                                         # 1: query position 0
        r(63) + "R" + r(40),                                                 # 2: 63
        r(64) + "Y" + r(40),                                                 # 3: 64
        r(70) + "B" + r(40),                                                 # 4: 64 + k - 2
        r(50) + "N",                                                         # 5: the last symbol
        r(20) + "N" + r(7) + "S" + r(20),                                    # 6: two, k apart
        r(20) + "W" + r(3) + "K" + r(20),                                    # 7: two, 4 apart
        r(20) + "NN" + r(20),                                                # 8: a run
        every,                                                               # 9: R = 2, 3 and 4
        every.lower(),                                                       # 10
        r(12) + "X" + r(12) + "N" + r(12) + "*" + r(10) + "?" + r(10) + "-" + r(10) + "n" + r(9),   # 11: invalid bytes stay invalid
        g["all4"], g["all3"], g["all2"], g["one"], g["none"],                # 12 .. 16: one window each
        r(30) + g["all4"] + r(30) + g["all3"] + r(9) + g["one"] + r(30),     # 17: the groups between exact windows
        g["all2"] + r(40),                                                   # 18: an ambiguous window first
        "".join(r(int(n)) + c for n, c in zip(rng.integers(9, 40, 12), "NRYNBDNHVNSW")) + r(30),     # 19: several tiles
        "".join(r(int(n)) + c for n, c in zip(rng.integers(1, 12, 30), "NRYKMBDHVNSWNNNRYKMBDHVNSWNNAC")) + r(5),   # 20: close together
        r(7) + "N", "N" + r(7), r(6) + "N", "N" * 8, r(200),                 # 21 .. 25
    ]
    # keys: the resolutions of the queries' windows, three in five of them; 600 random others; then the planted groups
    lists = {}
    for s in q:
        for _, codes in xo.windows(s, 4, K):
            for c in codes:
                if c not in lists and rng.random() < 0.6:
                    lists[c] = int(rng.integers(1, 41))
    for _, codes in xo.windows(q[0], 4, K):                                  # query 0: every resolution a key of 100 .. 150 entries
        for c in codes:
            lists[c] = int(rng.integers(100, 151))
    for c in rng.choice(4 ** K, 600, replace=False).tolist():
        lists.setdefault(c, int(rng.integers(1, 41)))
    for name, (w, counts, shares) in GROUPS.items():
        _group(rng, lists, w, counts, shares, 300)
    return ExtCase(4, K, _assemble(rng, lists, 300), q)


@functools.lru_cache(maxsize=None)
def aa_ext_case(k):
    """Amino acids, k = 3 or 6: B, Z, J and X (20 resolutions), alone and together, either case."""
    rng = np.random.default_rng(2000 + k)
    letters = po.ALPHABET[20][0]
    r = lambda n: _rand(rng, n, letters)
    q = [r(k - 1) + "X", "X" + r(k - 1), r(10) + "B" + r(10) + "Z" + r(10) + "J" + r(10) + "X" + r(10), (r(12) + "x" + r(7) + "b" + r(9)).lower(),
         r(5) + "XX" + r(5), r(4) + "J" + r(k - 2) + "Z" + r(4), r(70) + "X" + r(20), r(9) + "*" + r(3) + "B" + r(9) + "O" + r(9) + "U" + r(3) + "Z" + r(8)]
    lists = {}
    for s in q:
        for _, codes in xo.windows(s, 20, k):
            for c in codes:
                if c not in lists and rng.random() < 0.6:
                    lists[c] = int(rng.integers(1, 31))
    for c in _codes(q[0], 20):                                               # query 0: all 20 resolutions keys
        lists.setdefault(c, int(rng.integers(5, 31)))
    for _ in range(300):
        lists.setdefault(po.encode_kmer(r(k), 20), int(rng.integers(1, 31)))
    return ExtCase(20, k, _assemble(rng, lists, 90), q)


# queries of strand_case by name -> index
STRAND = {"reverse_wins": 0, "given_wins": 1, "palindrome": 2, "neither": 3, "only_reverse": 4, "codes": 5, "len_first": 6}
STRAND_LENGTHS = [K - 1, K, K + 63, K + 64, K + 65]


@functools.lru_cache(maxsize=None)
def strand_case():
    """DNA k = 8: texts T whose every window is a key; a query is T (the given strand wins) or rc(T) (the reverse wins).  "codes":
    rc of a text with Y, M, V, H at every 8th position (every window ambiguous), whose keys are resolutions that R, K, B, D in
    the same places do not have -- the reverse strand is placed only if the codes are complemented; the given strand has one poor key."""
    rng = np.random.default_rng(5150)
    r = lambda n: _rand(rng, n)
    rc = xo.revcomp
    texts = [r(60), r(60), r(24)]
    coded = "".join(r(7) + c for c in "YMVHYMVH") + r(7)
    # the resolution planted per code: one that the uncomplemented code (R, K, B, D) does not have
    right = {"Y": "C", "M": "A", "V": "A", "H": "C"}
    lens = [r(n) for n in STRAND_LENGTHS]
    lists = {}
    for t in texts + lens:
        for _, codes in xo.windows(t, 4, K):
            lists.setdefault(codes[0], int(rng.integers(5, 41)))
    for st in range(len(coded) - K + 1):
        w = coded[st:st + K]
        amb = [i for i, ch in enumerate(w) if ch in right]
        lists.setdefault(po.encode_kmer(w[:amb[0]] + right[w[amb[0]]] + w[amb[0] + 1:], 4), int(rng.integers(5, 41)))
    poor = _codes(rc(coded)[:K], 4)[0]                                       # the given strand of "codes": its first window's first resolution
    lists[poor] = (np.array([3], np.uint32), np.array([-7.5], np.float32))
    no_key = lambda s: all(c[0] not in lists for _, c in xo.windows(s, 4, K))
    while True:                                                              # "neither": no window of either strand is a key
        neither = r(50)
        if no_key(neither) and no_key(rc(neither)):
            break
    while True:                                                              # "only_reverse": rc(T), no window of which is a key
        only = r(40)
        if no_key(rc(only)) and not set(c[0] for _, c in xo.windows(only, 4, K)) & set(c[0] for _, c in xo.windows(rc(only), 4, K)):
            break
    for _, codes in xo.windows(only, 4, K):
        lists.setdefault(codes[0], int(rng.integers(5, 41)))
    q = [rc(texts[0]), texts[1], texts[2] + rc(texts[2]), neither, rc(only), rc(coded)] + [rc(t) for t in lens] + [lens[2], lens[4]]
    q += [rc(texts[0])[:30] + "N" + rc(texts[0])[31:], r(3) + "-" + rc(texts[1])]
    return ExtCase(4, K, _assemble(rng, lists, 120), q)


@functools.lru_cache(maxsize=None)
def big_branch_ext_case():
    """A branch id of 70 000 under ambiguous windows: the global tables of sums and of the window."""
    rng = np.random.default_rng(70001)
    r = lambda n: _rand(rng, n)
    q = [r(7) + "N" + r(7), r(20) + "R" + r(20) + "B" + r(12), r(30), "N" + r(7)]
    pool = np.concatenate([rng.choice(70000, 120, replace=False), [70000, 0, 4095, 4096, 65535, 65536]])
    lists = {}
    for s in q:
        for _, codes in xo.windows(s, 4, K):
            for c in codes:
                if c not in lists and rng.random() < 0.8:
                    n = int(rng.integers(1, 80))
                    br = rng.choice(pool, n, replace=False).astype(np.uint32)
                    lists[c] = (br, pc.mixed_scores(rng, n))
    first = _codes(q[0][:K], 4)[1]
    if 70000 not in lists.get(first, (np.zeros(0),))[0]:
        br = np.concatenate([rng.choice(pool[:120], 30, replace=False), [70000]]).astype(np.uint32)
        lists[first] = (br, pc.mixed_scores(rng, len(br)))
    return ExtCase(4, K, _assemble(rng, lists, 70001), q)


def reuse_ext_draw(G):
    """Members of main_ext_case() + strand_case() queries (one pool over main_ext_case's database) for 2 G + 37 short queries: a
    workgroup of a grid G wide places queries i, i + G and i + 2 G."""
    return np.random.default_rng(4243).integers(0, len(reuse_ext_pool().queries), 2 * G + 37)


@functools.lru_cache(maxsize=None)
def reuse_ext_pool():
    m = main_ext_case()
    short = [s for s in m.queries if len(s) <= 130]
    return ExtCase(4, K, m.db, short + [xo.revcomp(s) for s in short[:8]] + [""])


ALL_CASES = {"main_ext_case": main_ext_case, "aa3_ext_case": lambda: aa_ext_case(3), "aa6_ext_case": lambda: aa_ext_case(6),
             "strand_case": strand_case, "big_branch_ext_case": big_branch_ext_case}
# (ambiguity, strands) each case is placed with
MODES = {"main_ext_case": [(True, "given"), (True, "both"), (False, "both")], "aa3_ext_case": [(True, "given")], "aa6_ext_case": [(True, "given")],
         "strand_case": [(False, "both"), (True, "both")], "big_branch_ext_case": [(True, "given"), (True, "both")]}
