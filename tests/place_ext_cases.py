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


# ---- the cases of tests/test_place_ext_paths_inputs.py (host) and tests/test_gpu_place_ext_paths.py (device) ---------------------------
# Appended after the cases above, which keep their seeds: nothing here draws from their generators.

import decimal          # noqa: E402


def exact_contribution(xs, R, log_eps):
    """(y, right, d) of an ambiguous window's contribution to a branch that the resolutions with the scores `xs` name, of R resolutions:
    y = log10((sum 10^x + (R - c) 10^log_eps) / R) at 60 digits, `right` the binary32 nearest to it and d the distance of y from the
    nearer of the two binary32 rounding midpoints around `right`."""
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        e32 = float(np.float32(log_eps))
        P = sum((D(10) ** D(float(x)) for x in xs), D(0)) + (R - len(xs)) * D(10) ** D(e32)
        y = (P / R).log10()
        f = np.float32(float(y))
        cand = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        right = min(cand, key=lambda v: abs(D(float(v)) - y))
        d = min(abs(y - (D(float(cand[0])) + D(float(cand[1]))) / 2), abs(y - (D(float(cand[1])) + D(float(cand[2]))) / 2))
    return y, np.float32(right), d

_EXT_AT = {}


def expected_ext_at(case, log_eps, keep, ambiguity, strands):
    """xo.place of the case's queries with a threshold of the caller's (ExtCase.expected has LOG_EPS), computed once."""
    key = (id(case), float(log_eps), keep, ambiguity, strands)
    if key not in _EXT_AT:
        _EXT_AT[key] = (case, xo.place(case.view, case.queries, case.sigma, case.k, log_eps, keep, ambiguity, strands))
    return _EXT_AT[key][1]


# -- the lookup of an ambiguous window's resolutions: DNA k = 9, 12, 13, 15, 16 and AA k = 3, 4, 5, 6

LOOKUP_EXT_SHAPES = pc.LOOKUP_SHAPES + [(4, 16), (20, 6)]
# the letters a planted window is written with, by alphabet: DNA R = 2, 3, 4; amino acids R = 2 where the symbol has a two-way code, and X
DNA_LETTERS = {"A": "RDN", "C": "YBN", "G": "SVN", "T": "KHN"}
AA_LETTERS = {"D": "BX", "N": "BX", "E": "ZX", "Q": "ZX", "I": "JX", "L": "JX"}


def straddle_position(sigma, k):
    """The window position whose symbol's bits lie on both sides of the prefix table's shift, or None."""
    bits, shift = po.ALPHABET[sigma][1], pc.lookup_shift(sigma, k)
    return k - 1 - shift // bits if shift % bits else None


def lookup_positions(sigma, k):
    """name -> window position of the ambiguous symbol in the planted windows of lookup_ext_case."""
    pos = {"first": 0, "last": k - 1}
    if straddle_position(sigma, k) is not None:
        pos["straddle"] = straddle_position(sigma, k)
    return pos


def resolution_kind(keys, table, shift, code):
    """What place_lookup meets for `code`: "key"; "empty_slot"; "after_last" / "before_first" / "between" (absent in a slot with keys);
    "above_last" (absent above the database's last key, whatever its slot: the search ends at n_keys)."""
    j = code >> shift
    a, b = int(table[j]), int(table[j + 1])
    i = a + int(np.searchsorted(keys[a:b], code))
    if i < b and int(keys[i]) == code:
        return "key"
    if code > int(keys[-1]):
        return "above_last"
    if a == b:
        return "empty_slot"
    return "after_last" if i == b else "before_first" if i == a else "between"


def lookup_table(case):
    """(keys i64, the prefix table restated with np.searchsorted, shift) of a lookup case."""
    keys = case.db[0].astype(np.int64)
    bits = po.ALPHABET[case.sigma][1] * case.k
    shift = pc.lookup_shift(case.sigma, case.k)
    return keys, np.searchsorted(keys, np.arange((1 << min(bits, 16)) + 1, dtype=np.int64) << shift), shift


@functools.lru_cache(maxsize=None)
def lookup_ext_case(sigma, k, tail=False):
    """pc.lookup_case(sigma, k, tail)'s database.  A planted window is a code of a chosen kind (a key; absent in an empty slot, after a
    slot's last key, before its first key, with `tail` above the database's last key) written with an ambiguity letter in place of its
    symbol at window position 0, k - 1 or the position whose bits straddle the shift: that resolution is of the kind, its siblings are
    what they are.  `planted`: [(position name, kind, letter, window)].  Queries: every planted window alone, then the windows in runs
    between keys; at DNA k = 16 also T...TN and NT...T (0xFFFFFFFF is a key without `tail` and above the last key with it)."""
    base = pc.lookup_case(sigma, k, tail)
    rng = np.random.default_rng(31000 + 100 * sigma + 2 * k + int(tail))
    keys, table, shift = lookup_table(base)
    letters = DNA_LETTERS if sigma == 4 else AA_LETTERS
    targets = {"key": [c for v in base.planted.values() for c in (v[0], v[len(v) // 2], v[-1])] + rng.choice(keys, 6).tolist(),
               "empty_slot": list(base.absent["empty_slot"])}
    if shift:
        first = pc.slot_codes(base.R + 5, sigma, k)                           # its first code is the slot's only key
        targets["after_last"] = [first[1], first[len(first) // 2], first[-1]]
    if shift and not tail:
        last = pc.slot_codes(base.R + 7, sigma, k)                            # its last code is the slot's only key
        targets["before_first"] = [last[0], last[len(last) // 2], last[-2]]
    if tail:
        targets["above_last"] = list(base.absent["above_last"])
        if shift:                                                            # (the slots of R + 7 lie above the last key)
            low = [j for j in range(1, base.R) if table[j + 1] - table[j] == 1 and len(pc.slot_codes(j, sigma, k)) > 2]
            j = low[len(low) // 2]
            cs = pc.slot_codes(j, sigma, k)
            targets["before_first"] = [c for c in (cs[0], cs[1]) if c < keys[table[j]]]
            targets["after_last"] += [c for c in (cs[-1], cs[-2]) if c > keys[table[j]]]
    planted = []
    for pname, pos in lookup_positions(sigma, k).items():
        for kind, codes in targets.items():
            for n, code in enumerate(codes):
                text = pc.decode(int(code), sigma, k)
                choice = letters.get(text[pos], "X")
                for letter in (choice if n == 0 else choice[n % len(choice)]):
                    planted.append((pname, kind, letter, text[:pos] + letter + text[pos + 1:]))
    q = [w for _, _, _, w in planted]
    names = [pc.decode(int(c), sigma, k) for c in rng.choice(keys, 40)]
    order = rng.permutation(len(planted))
    per_run = max(7, 90 // k)
    for a in range(0, len(order), per_run):                                   # runs: a key, a planted window, a key, ... (several tiles long)
        q.append("".join(names[(a + i) % 40] + planted[j][3] for i, j in enumerate(order[a:a + per_run])) + names[a % 40])
    if (sigma, k) == (4, 16):
        q += ["T" * 15 + "N", "N" + "T" * 15, "T" * 15 + "K", "G" + "T" * 14 + "N" + "T" * 15]
    c = ExtCase(sigma, k, base.db, q)
    c.base, c.planted = base, planted
    return c


# -- the bounds of the LDS tables under ambiguous windows

@functools.lru_cache(maxsize=None)
def bound_ext_case(top):
    """pc.bound_case(top)'s database; queries with one ambiguous symbol each over the keys that name branch `top` (every third key), the
    symbol at a position and with a letter that change from key to key: alone, in runs, between exact windows."""
    base = pc.bound_case(top)
    names = [pc.decode(int(c), 4, 8) for c in base.db[0]]
    ws = []
    for i in range(0, len(names), 3):
        pos, text = (i // 3) % 8, names[i]
        letter = DNA_LETTERS[text[pos]][(i // 3) % 3]
        ws.append(text[:pos] + letter + text[pos + 1:])
    q = ws[:6] + ["".join(ws), "".join(ws[:9]), names[0] + ws[1] + names[6], ws[2] + "".join(names[9:40:3]), "".join(names[1:30]) + ws[3] + names[12].lower(),
                  ws[4].lower() + names[3] * 9]
    c = ExtCase(4, 8, base.db, q)
    c.windows = ws
    return c


# -- a long query on both strands

LONG_EXT_INVALID = "-*?.X#"


@functools.lru_cache(maxsize=None)
def long_ext_case():
    """One DNA query of 70 000 symbols made of the database's 400 k-mers (every 8th window a key before the substitutions): an
    ambiguity code that holds the symbol it replaces every 40 .. 60 symbols, two codes 5 apart at 20 places, an invalid byte every
    3000 .. 5000 symbols -- and the same text reverse-complemented.  Branches below 60, 1 .. 6 entries per key."""
    rng = np.random.default_rng(70070)
    keys = sorted(set(rng.choice(4 ** K, 400, replace=False).tolist()))
    db = pc.make_db(rng, keys, 60, rng.integers(1, 7, len(keys)))
    names = [pc.decode(c, 4, K) for c in keys]
    s = list("".join(rng.choice(names, 70000 // K)))
    assert len(s) == 70000
    codes = {"A": "RWMDHVN", "C": "YSMBHVN", "G": "RSKBDVN", "T": "YWKBDHN"}
    at = int(rng.integers(0, 50))
    n_codes = 0
    while at < len(s):
        s[at] = str(rng.choice(list(codes[s[at]])))
        if n_codes % 70 == 3 and at + 5 < len(s):                             # two codes fewer than k apart
            s[at + 5] = str(rng.choice(list(codes[s[at + 5]])))
        n_codes += 1
        at += int(rng.integers(40, 61))
    at = int(rng.integers(1000, 3000))
    while at < len(s):
        s[at] = LONG_EXT_INVALID[(at // 7) % len(LONG_EXT_INVALID)]
        at += int(rng.integers(3000, 5001))
    s = "".join(s)
    return ExtCase(4, K, db, [s, xo.revcomp(s)])


# -- bytes whose low five bits are an ambiguous letter's

ALIAS_LETTERS = "RYSWKMBDHVN"


def alias_bytes():
    """Every byte that is no letter and equals an ambiguous DNA letter in its low five bits, ascending."""
    low = {ord(ch) & 31 for ch in ALIAS_LETTERS}
    return [b for b in range(256) if b & 31 in low and not (b < 128 and chr(b).isalpha())]


@functools.lru_cache(maxsize=None)
def alias_case():
    """main_ext_case's database.  Queries are Latin-1 strings (one character a byte: .encode("latin-1") is what the device gets): runs of
    keys with an alias byte, 0x00, 0x80 or 0xFF between them, the same runs with the letter the byte aliases, runs with U and u."""
    m = main_ext_case()
    rng = np.random.default_rng(3131)
    names = [pc.decode(int(c), 4, K) for c in m.db[0]]
    run = lambda n: "".join(rng.choice(names, n))
    odd = alias_bytes() + [0x00, 0x80, 0xFF]
    q = []
    for a in range(0, len(odd), 6):                                           # six bytes a query, each between two runs
        q.append("".join(run(2) + chr(b) for b in odd[a:a + 6]) + run(2))
    q.append("".join(chr(b) for b in odd))                                    # nothing but such bytes
    q.append(run(1) + "".join(chr(b) + "ACGTACG" for b in odd[:40]))          # no window between them: 7 valid symbols, then a byte
    real = run(3) + "N" + run(2) + "\x0e" + run(2) + "\xce" + run(1) + "n" + run(2)      # N and n expanded, 0x0E and 0xCE not
    q += [real, real.replace("N", "\x2e").replace("n", "\xee")]
    t_rich = [s for s in names if s.count("T") >= 3][:12]
    q += ["".join(t_rich).replace("T", "U"), "".join(t_rich[:6]).replace("T", "u") + "N" + "".join(t_rich[6:]).replace("T", "U"),
          xo.revcomp("".join(t_rich)).replace("T", "U")]
    return ExtCase(4, K, m.db, q)


# -- a strand tie between different branches

TIE_WINDOWS = 24


@functools.lru_cache(maxsize=None)
def tie_case():
    """Texts T and U of TIE_WINDOWS windows each: T's keys name branch 3 alone and U's branch 9 alone, with the same multiples of -0.5
    in another order (both sums exact and equal); no window of rc(T) or rc(U) is a key.  Queries: T + "-" + rc(U) (the given strand
    places branch 3, the reverse strand branch 9, equal scores: strand 0, branch 3), rc(T) + "-" + U (strand 0, branch 9), and the
    parts alone and with a symbol less on one side (no tie there)."""
    rng = np.random.default_rng(3939)
    rc = xo.revcomp
    codes = lambda s: [c[0] for _, c in xo.windows(s, 4, K)]
    while True:
        T, U = _rand(rng, TIE_WINDOWS + K - 1), _rand(rng, TIE_WINDOWS + K - 1)
        own = codes(T) + codes(U)
        if len(set(own)) == 2 * TIE_WINDOWS and not set(own) & set(codes(rc(T)) + codes(rc(U))):
            break
    mult = rng.integers(1, 9, TIE_WINDOWS)
    lists = {}
    for c, m in zip(codes(T), mult):
        lists[c] = (np.array([3], np.uint32), np.array([-0.5 * m], np.float32))
    for c, m in zip(codes(U), mult[rng.permutation(TIE_WINDOWS)]):
        lists[c] = (np.array([9], np.uint32), np.array([-0.5 * m], np.float32))
    for c in rng.choice(4 ** K, 200, replace=False).tolist():
        if c not in lists and c not in codes(rc(T)) + codes(rc(U)):
            lists[c] = int(rng.integers(1, 21))
    q = [T + "-" + rc(U), rc(T) + "-" + U, T, rc(U), T + "-" + rc(U)[:-1], T[1:] + "-" + rc(U)]
    c = ExtCase(4, K, _assemble(rng, lists, 40), q)
    c.T, c.U = T, U
    return c


# -- three queries a workgroup, batches narrower than the grid; batches under a budget

def reuse_ext_draw3(G):
    """Members of reuse_ext_pool() for N = 2 G + G / 2 + 37 queries: half of the workgroups of a grid G wide place a third query."""
    return np.random.default_rng(4244).integers(0, len(reuse_ext_pool().queries), 2 * G + G // 2 + 37)


def budget_ext_draw():
    """pc.budget_draw()'s 1500 members mapped onto reuse_ext_pool()."""
    return pc.budget_draw() % len(reuse_ext_pool().queries)


def big_branch_ext_draw():
    """200 members of big_branch_ext_case()."""
    return np.random.default_rng(201).integers(0, len(big_branch_ext_case().queries), 200)


PLACE_EXT_QUERY_BYTES_7 = pc.PLACE_QUERY_BYTES_7 + 2 * 4       # strand and n_ambiguous as well


# -- the rounding ladder (tools/place_ladder_search.py): binary32 x (hex bits) whose y = log10((10^x + (R - 1) 10^-4.5) / R) lies at a
# distance d, 2^rung <= d < 2^(rung + 1), from a binary32 rounding midpoint; {R: {rung: [bits of x]}}, up to eight a rung
LADDER = {
    # R = 2: 5985 prescreened; inputs per rung: -36: 2953, -37: 1484, -38: 790, -39: 361, -40: 183, -41: 103, -42: 44, -43: 26, -44: 23, -45: 6, -48: 3, -49: 1
    # finest d = 2^-48.4
    2: {
        -36: [0xBF800324, 0xBF9919EA, 0xBFB44B21, 0xBFCF2EBE, 0xBFF76D25, 0xC02F9748, 0xC063AF0D, 0xC0BFED39],
        -37: [0xBF800F7E, 0xBF9B7A50, 0xBFB32699, 0xBFCC290A, 0xBFF0AA1D, 0xC02C794A, 0xC067CE37, 0xC0BF19DD],
        -38: [0xBF801BD4, 0xBF9D8080, 0xBFB78D37, 0xBFD5CE8B, 0xC00BFFF0, 0xC03EA223, 0xC06A63FE, 0xC0BD61B7],
        -39: [0xBF8071E5, 0xBF9BDBFC, 0xBFB74435, 0xBFD4DEB3, 0xC00967A1, 0xC03DEA9E, 0xC0715D8A, 0xC0BF2860],
        -40: [0xBF80BB41, 0xBF993180, 0xBFB4FC93, 0xBFD0A6BD, 0xC0000E61, 0xC039421B, 0xC0678394, 0xC0BF6AD3],
        -41: [0xBF81AD17, 0xBFA0002D, 0xBFC1F2CC, 0xBFDC524B, 0xC00BDAC3, 0xC0347F49, 0xC0680D34, 0xC0BC2853],
        -42: [0xBF8327AE, 0xBF9A8EAA, 0xBFAC7937, 0xBFC6964D, 0xBFD8B3FF, 0xBFF9B314, 0xC05B1750, 0xC0AC3C8D],
        -43: [0xBF82A6AC, 0xBF99E508, 0xBFBE7EDE, 0xC004AAD9, 0xC0206D7F, 0xC036A706, 0xC062D950, 0xC09D8285],
        -44: [0xBF87B4DE, 0xBFA51523, 0xBFD444AF, 0xC01B8BC9, 0xC0679335, 0xC08220CF, 0xC0900001, 0xC0A62330],
        -45: [0xBF879F56, 0xBF9FE459, 0xBFA3033E, 0xBFA3F4C9, 0xBFBBBECA, 0xC04C8F34],
        -48: [0xC0194138, 0xC087DFF4, 0xC098200C],
        -49: [0xC045CE9B],
    },
    # R = 4: 5117 prescreened; inputs per rung: -36: 2644, -37: 1209, -38: 621, -39: 320, -40: 178, -41: 67, -42: 43, -43: 18, -44: 11, -45: 2, -46: 1, -48: 1
    # finest d = 2^-47.0
    4: {
        -36: [0xBF800D49, 0xBF96E7D3, 0xBFABDC33, 0xBFD50454, 0xC00563DB, 0xC035923C, 0xC068ABC2, 0xC0BFFE95],
        -37: [0xBF80324C, 0xBF96EA8E, 0xBFB10B5F, 0xBFD9854A, 0xC0078F45, 0xC0336351, 0xC0610438, 0xC0BECCA9],
        -38: [0xBF803A82, 0xBF9A49FA, 0xBFAF1DE0, 0xBFD77DEF, 0xC009BD5D, 0xC0344FF8, 0xC067DBE2, 0xC0BFBEC4],
        -39: [0xBF805736, 0xBF997074, 0xBFB763FF, 0xBFD5BC9F, 0xBFFA6A77, 0xC0248A61, 0xC052FF52, 0xC0BECB49],
        -40: [0xBF8042B7, 0xBF97D0C5, 0xBFA61418, 0xBFC897F6, 0xBFF75285, 0xC02A606A, 0xC05AC855, 0xC0BF96E7],
        -41: [0xBF80092B, 0xBF92037F, 0xBFAC9A21, 0xBFD2C638, 0xBFF0D6CF, 0xC018BBB0, 0xC05CB810, 0xC0BDB967],
        -42: [0xBF8046D1, 0xBFA252DA, 0xBFB4AB85, 0xBFCDBE9E, 0xBFEE0765, 0xC0221875, 0xC04E370F, 0xC0BE1B8E],
        -43: [0xBF93AA88, 0xBFAA37CC, 0xC009C2A7, 0xC01BB637, 0xC08FFFFE, 0xC0910CF1, 0xC09D7916, 0xC0BF0D89],
        -44: [0xBF843F9C, 0xBFA7DC73, 0xC0041652, 0xC00CF642, 0xC02F16E4, 0xC03E8319, 0xC08A7490, 0xC0A7143E],
        -45: [0xC022AF7A, 0xC041EB6F],
        -46: [0xC00AA036],
        -48: [0xBF994942],
    },
}
LADDER_ASSERTED_FROM = -44       # rungs -36 .. -44 (d >= 2^-44, the suite's own margin) are asserted, the finer ones reported


def ladder_inputs():
    """[(R, rung, x f32)] of LADDER in a fixed order."""
    return [(R, rung, np.uint32(b).view(np.float32)) for R in sorted(LADDER) for rung in sorted(LADDER[R], reverse=True) for b in LADDER[R][rung]]


@functools.lru_cache(maxsize=None)
def ladder_case():
    """Input i of ladder_inputs(): key = (the 7 symbols that spell i in base 4) + A with the one entry (branch i mod 50, x); query i is
    the 7 symbols + R (R = 2: A or G) or + N (R = 4) -- one window, one resolution a key, W = C = 1 and no penalty: the placement's
    score is y itself.  `want_bits`: the 60-digit y rounded to binary32, per query."""
    inputs = ladder_inputs()
    lists, q, want = {}, [], []
    for i, (R, rung, x) in enumerate(inputs):
        stem = pc.decode(i, 4, K - 1)
        lists[po.encode_kmer(stem + "A", 4)] = (np.array([i % 50], np.uint32), np.array([x], np.float32))
        q.append(stem + ("R" if R == 2 else "N"))
        want.append(int(exact_contribution((float(x),), R, LOG_EPS)[1].view(np.uint32)))
    c = ExtCase(4, K, _assemble(np.random.default_rng(0), lists, 50), q)
    c.want_bits = np.array(want, np.uint32)
    return c


NEW_CASES = {f"lookup_ext_{s}_{k}_{'tail' if t else 'top'}": (lambda s=s, k=k, t=t: lookup_ext_case(s, k, t)) for s, k in LOOKUP_EXT_SHAPES for t in (False, True)}
NEW_CASES.update({f"bound_ext_{top}": (lambda top=top: bound_ext_case(top)) for top in (4095, 4096, 63, 64)})
NEW_CASES.update({"long_ext_case": long_ext_case, "tie_case": tie_case, "alias_case": alias_case, "ladder_case": ladder_case})
NEW_MODES = {n: ([(True, "given"), (True, "both")] if n.startswith("lookup_ext_4_") or n.startswith("bound_ext_") else [(True, "given")]) for n in NEW_CASES}
NEW_MODES.update({"long_ext_case": [(True, "both")], "tie_case": [(False, "both"), (True, "both")], "alias_case": [(True, "both")]})
