"""Fabricated databases and queries of the placement tests (tests/test_place_inputs.py on the host, tests/test_gpu_place.py on the
device): built once per process from fixed seeds, never changed afterwards."""
import functools

import numpy as np

from tests import place_oracle as po

LOG_EPS = -4.5            # a threshold of the builds' magnitude (log_threshold(1.5, 4, 8) = -3.4, k = 10: -4.3)


def decode(code, sigma, k):
    letters, bits = po.ALPHABET[sigma]
    return "".join(letters[(code >> (bits * (k - 1 - i))) & ((1 << bits) - 1)] for i in range(k))


def mixed_scores(rng, n):
    """f32 scores of three magnitudes (about -7, -0.1, -1e-3): sums of them depend on the order of the additions."""
    mag = rng.choice(np.array([-7.0, -0.1, -1e-3]), n)
    return (mag * rng.uniform(0.5, 1.5, n)).astype(np.float32)


def make_db(rng, keys, n_branches, counts):
    """(keys asc, key_offsets, branches, scores): key i with counts[i] distinct random branches below n_branches, in random order."""
    keys = np.asarray(sorted(keys), np.uint32)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    br = np.concatenate([rng.choice(n_branches, c, replace=False) for c in counts] or [np.zeros(0, np.int64)]).astype(np.uint32)
    return keys, off, br, mixed_scores(rng, len(br))


class Case:
    def __init__(self, sigma, k, db, queries):
        self.sigma, self.k, self.db, self.queries = sigma, k, db, queries
        self.view = po.DbView(*db)

    @functools.lru_cache(maxsize=None)
    def expected(self, keep):
        return po.place(self.view, self.queries, self.sigma, self.k, LOG_EPS, keep)


@functools.lru_cache(maxsize=None)
def main_case():
    """DNA k = 8: about 3000 keys with key 0 and key 4^8 - 1, branches below 300, 1..200 entries per key (63, 64, 65 and 129 among
    them), 64 queries of the lengths that give 0, 1, 2, 63, 64, 65 and more windows."""
    rng = np.random.default_rng(20240)
    sigma, k = 4, 8
    keys = set(rng.choice(4 ** k, 3000, replace=False).tolist()) | {0, 4 ** k - 1}
    keys = sorted(keys)
    counts = rng.integers(1, 201, len(keys))
    counts[[0, 5, 6, 7, len(keys) - 1]] = [64, 63, 65, 129, 65]        # key 0: 64 entries; the last key: 65
    db = make_db(rng, keys, 300, counts)
    present = np.array(keys)
    lengths = [k - 1, k, k + 1, k + 62, k + 63, k + 64, k + 65, 300, 1000]

    def from_kmers(n, pick):
        """n symbols: k-mers of the database one behind the other (every k-th window a key for sure)."""
        s = "".join(decode(int(c), sigma, k) for c in pick(n // k + 1))
        return s[:n]
    rand_keys = lambda m: rng.choice(present, m)
    q = [from_kmers(n, rand_keys) for n in lengths]                                    # 0 .. 8: every length
    q += [from_kmers(n, rand_keys).lower() for n in (k, k + 63, 300)]                  # lower case
    q += [from_kmers(n, rand_keys).replace("T", "U") for n in (k + 1, k + 64, 300)]    # U = T
    q += [from_kmers(300, rand_keys).replace("T", "u")]
    s = from_kmers(300, rand_keys)
    q += [s[:100] + "N" * 30 + s[130:], "N" * 20 + s[20:], s[:280] + "NNNNNNNNNNNNNNNNNNNN"]   # runs of N
    q += ["".join(ch if (i + 1) % k else "N" for i, ch in enumerate(from_kmers(n, rand_keys))) for n in (k, k + 64, 300)]  # W = 0
    q += [s[:150].replace("A", "X", 3), s[:150] + "*" + s[150:], "-" + s[:80] + "." + s[80:200]]     # other invalid bytes
    one = decode(int(present[17]), sigma, k)
    q += [one * 10, one * 40, (one + decode(int(present[40]), sigma, k)) * 20]         # repeated k-mers
    absent = [c for c in rng.choice(4 ** k, 400, replace=False).tolist() if c not in set(keys)]
    ab = lambda n: "".join(decode(c, sigma, k) for c in absent)[:n]
    only_absent = [s_ for s_ in (ab(k), ab(k + 5), ab(40)) if all(po.DbView(*db).entries(c) is None for _, c in po.window_codes(s_, sigma, k))]
    q += only_absent                                                                    # only absent k-mers
    q += ["A" * k, "T" * k, "A" * (k + 70), "T" * 200, "A" * k + "T" * k, "a" * 100 + "U" * 100]   # the first and the last key
    while len(q) < 64:
        n = lengths[len(q) % len(lengths)]
        q.append(from_kmers(n, rand_keys) if len(q) % 2 else "".join(rng.choice(list("ACGT"), n)))
    return Case(sigma, k, db, q[:64])


@functools.lru_cache(maxsize=None)
def order_case():
    """The order-sensitivity case: the main database, long queries made of its k-mers -- every branch is scored many times, by
    scores of three magnitudes."""
    m = main_case()
    rng = np.random.default_rng(777)
    keys = m.db[0]
    q = ["".join(decode(int(c), m.sigma, m.k) for c in rng.choice(keys, 60)) for _ in range(8)]
    return Case(m.sigma, m.k, m.db, q)


@functools.lru_cache(maxsize=None)
def aa_case():
    """AA k = 6: 30-bit codes, one key the last letter throughout."""
    rng = np.random.default_rng(606)
    sigma, k = 20, 6
    letters = po.ALPHABET[20][0]
    kmers = {"".join(rng.choice(list(letters), k)) for _ in range(400)} | {"V" * k, "R" * k, "RHKDES"}
    keys = sorted(po.encode_kmer(s, sigma) for s in kmers)
    db = make_db(rng, keys, 90, rng.integers(1, 70, len(keys)))
    names = [decode(c, sigma, k) for c in keys]
    pick = lambda m: "".join(rng.choice(names, m))
    q = ["V" * k, "V" * 30, "v" * 7 + "R" * 9, "RHKDES", pick(12), pick(12).lower(), pick(5) + "X" + pick(5), pick(4) + "*" + pick(3) + "B" + pick(2),
         "".join(rng.choice(list(letters), 200)), pick(3)[:k - 1], pick(11)[:k + 64]]
    return Case(sigma, k, db, q)


@functools.lru_cache(maxsize=None)
def k16_case():
    """DNA k = 16: 32-bit codes, keys 0, 0x80000000 and 0xFFFFFFFF among them."""
    rng = np.random.default_rng(1616)
    sigma, k = 4, 16
    keys = sorted(set(rng.integers(0, 2 ** 32, 300).tolist()) | {0, 0x80000000, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000001, 0x0000FFFF, 0x00010000})
    db = make_db(rng, keys, 50, rng.integers(1, 40, len(keys)))
    names = [decode(c, sigma, k) for c in keys]
    pick = lambda m: "".join(rng.choice(names, m))
    q = ["A" * 16, "T" * 16, "G" + "A" * 15, "A" * 40 + "T" * 40, decode(0x7FFFFFFF, 4, 16) + "T", pick(6), pick(6).lower().replace("t", "u"),
         pick(2) + "N" + pick(2), "".join(rng.choice(list("ACGT"), 300)), "ACGT" * 3 + "ACG", pick(5)[:16 + 63]]
    return Case(sigma, k, db, q)


@functools.lru_cache(maxsize=None)
def k2_case():
    """DNA k = 2: all 16 keys present (a code is its own place in the prefix table)."""
    rng = np.random.default_rng(22)
    db = make_db(rng, range(16), 20, rng.integers(1, 21, 16))
    q = ["A", "AC", "ACG", "".join(rng.choice(list("ACGT"), 66)), "".join(rng.choice(list("ACGTN"), 200)), "acgu" * 16 + "a", "NN", ""]
    return Case(4, 2, db, q)


@functools.lru_cache(maxsize=None)
def one_key_case():
    rng = np.random.default_rng(1)
    key = po.encode_kmer("ACGTACGT", 4)
    db = make_db(rng, [key], 10, [4])
    return Case(4, 8, db, ["ACGTACGT", "ACGTACGTACGTACGT", "TTTTTTTTTT", "ACGTACG", "acgtacgu" * 9])


@functools.lru_cache(maxsize=None)
def empty_case():
    db = (np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32))
    return Case(4, 8, db, ["ACGTACGT", "A" * 100, "ACG", ""])


@functools.lru_cache(maxsize=None)
def big_branch_case():
    """A branch id of 70 000: 12 x 70 001 bytes of sums, counts and touched list, more than any LDS table."""
    rng = np.random.default_rng(70000)
    sigma, k = 4, 8
    keys = sorted(set(rng.choice(4 ** k, 200, replace=False).tolist()))
    counts = rng.integers(1, 120, len(keys))
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    pool = np.concatenate([rng.choice(70000, 150, replace=False), [70000, 0, 4095, 4096, 65535, 65536]])
    br = np.concatenate([rng.choice(pool, c, replace=False) for c in counts]).astype(np.uint32)
    br[0] = 70000 if 70000 not in br[:counts[0]] else br[0]
    db = (np.asarray(keys, np.uint32), off, br, mixed_scores(rng, len(br)))
    names = [decode(c, sigma, k) for c in keys]
    q = ["".join(rng.choice(names, m)) for m in (1, 2, 9, 25, 40)] + [names[0], names[0] * 3, "ACGTN" * 10]
    return Case(sigma, k, db, q)


@functools.lru_cache(maxsize=None)
def topn_case():
    """One query touching about 100 branches, two of them (11 and 57) with identical entries -- equal scores, the lower id first."""
    rng = np.random.default_rng(64)
    sigma, k = 4, 8
    keys = sorted(set(rng.choice(4 ** k, 60, replace=False).tolist()))
    kk, off, br, sc = make_db(rng, keys, 100, rng.integers(20, 60, len(keys)))
    br, sc, off = br.tolist(), sc.tolist(), off.tolist()
    nb, ns, noff = [], [], [0]
    for i in range(len(kk)):                                  # take 11 and 57 out, then put both back with one score
        e = [(b, x) for b, x in zip(br[off[i]:off[i + 1]], sc[off[i]:off[i + 1]]) if b not in (11, 57)]
        if i % 2 == 0:
            x = float(mixed_scores(rng, 1)[0])
            e += [(57, x), (11, x)]
        nb += [b for b, _ in e]; ns += [x for _, x in e]; noff.append(len(nb))
    db = (kk, np.asarray(noff, np.uint64), np.asarray(nb, np.uint32), np.asarray(ns, np.float32))
    names = [decode(int(c), sigma, k) for c in kk]
    return Case(sigma, k, db, ["".join(names), "".join(names[:3]), names[1]])


def write_case_db(path, case):
    """The case's database as a file of this library (dbfile.write_db: the host serialiser), keys in ascending order."""
    from ipk_amd import dbfile
    keys, off, br, sc = case.db
    dbfile.write_db(path, "DNA" if case.sigma == 4 else "AA", [(1, 0.0)], "(a:1,b:1)r;", case.k, 1.5, keys, off, br, sc,
                    np.zeros(len(keys), np.float32), np.arange(len(keys), dtype=np.uint32))
    return path


# ---- the cases of tests/test_place_paths_inputs.py (host) and tests/test_gpu_place_paths.py (device) ---------------------------------
# Appended after the cases above, which keep their seeds: nothing here draws from their generators.

EPS_INEXACT = np.float32(8 * np.log10(1.5 / 4))      # -3.40775: (float)(W - C) * log_eps rounds, and so does the sum with S

_AT = {}


def expected_at(case, log_eps, keep):
    """po.place of the case's queries with a threshold of the caller's (Case.expected has LOG_EPS), computed once."""
    key = (id(case), float(log_eps), keep)
    if key not in _AT:
        _AT[key] = (case, po.place(case.view, case.queries, case.sigma, case.k, log_eps, keep))
    return _AT[key][1]


# -- many queries per workgroup

REUSE_SEED = 4242


@functools.lru_cache(maxsize=None)
def reuse_pool():
    """D: the 72 distinct queries of main_case() and order_case(), then "" (a query without a byte) -- on the main database."""
    m = main_case()
    d = list(dict.fromkeys(m.queries + order_case().queries))
    assert "" not in d
    return Case(m.sigma, m.k, m.db, d + [""])


def reuse_draw(G):
    """Members of reuse_pool() for N = 2 G + G / 2 + 37 queries: a workgroup of a grid G wide places queries i, i + G, i + 2 G."""
    return np.random.default_rng(REUSE_SEED).integers(0, len(reuse_pool().queries), 2 * G + G // 2 + 37)


@functools.lru_cache(maxsize=None)
def reuse_branch_sets():
    """The branches each member of reuse_pool() scores (the oracle's C > 0)."""
    c = reuse_pool()
    return [frozenset(np.nonzero(po.accumulate(c.view, q, c.sigma, c.k)[3])[0].tolist()) for q in c.queries]


# -- the bounds of the LDS tables

@functools.lru_cache(maxsize=None)
def bound_case(top):
    """DNA k = 8, about 100 keys of 1..150 entries, branch ids up to `top` (B = top + 1); `top` itself under every third key with a
    score next to 0, so that a query made of those keys has it among its best."""
    rng = np.random.default_rng(50000 + top)
    sigma, k = 4, 8
    keys = sorted(set(rng.choice(4 ** k, 100, replace=False).tolist()))
    keys, off, br, sc = make_db(rng, keys, top + 1, rng.integers(1, min(150, top + 1) + 1, len(keys)))
    for i in range(0, len(keys), 3):
        a, b = int(off[i]), int(off[i + 1])
        at = np.nonzero(br[a:b] == top)[0]
        j = a + (int(at[0]) if len(at) else int(rng.integers(0, b - a)))
        br[j], sc[j] = top, np.float32(-1e-3 * (1 + i % 7))
    names = [decode(int(c), sigma, k) for c in keys]
    pick = lambda m: "".join(rng.choice(names, m))
    q = ["".join(names[::3]), "".join(names[::3][:9]), names[0], names[3] * 9, pick(8), pick(20), pick(40), pick(125), "".join(names)]
    return Case(sigma, k, (keys, off, br, sc), q)


# -- the lookup: DNA k = 9, 12, 13, 15 and AA k = 3, 4, 5

LOOKUP_SHAPES = [(4, 9), (4, 12), (4, 13), (4, 15), (20, 3), (20, 4), (20, 5)]
LOOKUP_RESERVED = 12          # slots R .. R + 11 hold the planted keys of lookup_case and nothing else


def code_of_rank(r, sigma, k):
    """The r-th valid code in ascending order (DNA: r itself; AA: the base-20 digits of r, 5 bits each)."""
    bits, code = po.ALPHABET[sigma][1], 0
    for i in range(k):
        code |= (r % sigma) << (bits * i)
        r //= sigma
    return code


def rank_of_code(code, sigma, k):
    """The inverse of code_of_rank; None for a code with a symbol outside the alphabet."""
    bits, r = po.ALPHABET[sigma][1], 0
    for i in range(k - 1, -1, -1):
        s = (code >> (bits * i)) & ((1 << bits) - 1)
        if s >= sigma:
            return None
        r = r * sigma + s
    return r


def lookup_shift(sigma, k):
    bits = po.ALPHABET[sigma][1] * k
    return bits - min(bits, 16)


def slot_codes(j, sigma, k):
    """The valid codes of slot j of the prefix table, ascending."""
    shift = lookup_shift(sigma, k)
    r = range(j << shift, (j + 1) << shift)
    return r if sigma == 4 else [c for c in r if rank_of_code(c, sigma, k) is not None]


class LookupCase(Case):
    """A Case with what the host file needs to prove its properties: R (the first reserved slot), `absent` (kind -> codes that are no
    keys) and `planted` (name -> codes)."""


@functools.lru_cache(maxsize=None)
def lookup_case(sigma, k, tail=False):
    """Keys: code 0 and the largest valid code; slot R + 2 filled from its first code (min(2^shift, 1024) consecutive valid codes, and its
    last); slot R + 5 with its first code only, R + 7 with its last only, R + 9 with both; the other slots of R .. R + 11 empty; 300
    random keys elsewhere.  At shift 0 a slot is a code: R + 5 and R + 7 hold a key, R + 2 and R + 9 stay empty.
    tail: the keys below slot R + 11 and the first code of slot R + 11 as the LAST key -- every code above it is absent (`above_last`).
    Branches below 200, 1..40 entries per key.  Queries: present and absent codes of every kind one behind the other after a prefix of
    0 .. k - 1 symbols, cut to 63, 64, 65, 66, 127 and 129 windows or left several tiles long."""
    rng = np.random.default_rng(1000 * sigma + k)
    shift, n_valid = lookup_shift(sigma, k), sigma ** k
    slot = lambda c: c >> shift
    code = lambda r: code_of_rank(int(r), sigma, k)
    top = code(n_valid - 1)
    while True:                                        # R: an even slot, R .. R + 11 each with valid codes (at shift 0: R + 5, R + 7, R + 11)
        R = slot(code(rng.integers(n_valid // 4, n_valid // 2))) & ~1
        need = range(R, R + LOOKUP_RESERVED) if shift else (R + 5, R + 7, R + 11)
        if all(len(slot_codes(j, sigma, k)) for j in need):
            break
    planted = {"zero": [0], "top": [top], "first_only": [slot_codes(R + 5, sigma, k)[0]], "last_only": [slot_codes(R + 7, sigma, k)[-1]]}
    if shift:
        full = slot_codes(R + 2, sigma, k)
        planted["full"] = sorted(set(list(full[:min(1 << shift, 1024)]) + [full[-1]]))
        pair = slot_codes(R + 9, sigma, k)
        planted["pair"] = [pair[0], pair[-1]]
    keys = {c for v in planted.values() for c in v}
    while len(keys) < sum(len(v) for v in planted.values()) + 300:
        c = code(rng.integers(0, n_valid))
        if not R <= slot(c) < R + LOOKUP_RESERVED:
            keys.add(c)
    if tail:
        last = slot_codes(R + 11, sigma, k)[0]
        keys = {c for c in keys if c < last} | {last}
        planted = {n: [c for c in v if c < last] for n, v in planted.items() if v[0] < last}
        planted["last"] = [last]
    keys = sorted(keys)
    kset = set(keys)
    db = make_db(rng, keys, 200, rng.integers(1, 41, len(keys)))

    def valid_near(c, step):
        r = rank_of_code(c, sigma, k) + step
        return code(r) if 0 <= r < n_valid else None
    absent = {"neighbour": [], "empty_slot": []}
    for c in rng.choice(keys, 40).tolist() + [c for v in planted.values() for c in (v[0], v[-1])]:
        absent["neighbour"] += [n for n in (valid_near(c, -1), valid_near(c, 1)) if n is not None and n not in kset]
    for j in (R, R + 1, R + 3, R + 4, R + 6, R + 8, R + 10):
        cs = slot_codes(j, sigma, k)
        absent["empty_slot"] += [cs[0], cs[len(cs) // 2], cs[-1]] if len(cs) else []
    if shift and not tail:
        # the next valid code after the full slot's last key: the first code of the empty slot R + 3, so a search like `empty_slot`'s
        # (a code above the run INSIDE the full slot is `gap_in_full`, which only DNA k = 15 has room for)
        absent["above_full"] = [slot_codes(R + 3, sigma, k)[0]]
        gap = [c for c in slot_codes(R + 2, sigma, k) if c not in kset]
        if gap:
            absent["gap_in_full"] = [gap[0], gap[len(gap) // 2], gap[-1]]      # inside the full slot: above its run, below its last key
        absent["beside_single"] = [slot_codes(R + 5, sigma, k)[1], slot_codes(R + 7, sigma, k)[-2], slot_codes(R + 9, sigma, k)[1]]
    if tail:
        above = [valid_near(keys[-1], 1), valid_near(keys[-1], 2), top] + [code(r) for r in rng.integers(rank_of_code(keys[-1], sigma, k) + 1, n_valid, 12)]
        absent["above_last"] = above
    absent = {n: sorted(set(v) - kset) for n, v in absent.items()}
    present = rng.choice(keys, 80).tolist() + [c for v in planted.values() for c in (v[0], v[len(v) // 2], v[-1])]
    pool = present + [c for v in absent.values() for c in v]
    pool = [pool[i] for i in rng.permutation(len(pool))]
    at = [0]

    def take(m):
        out = [pool[(at[0] + i) % len(pool)] for i in range(m)]
        at[0] += m
        return out
    q = []
    for windows in (63, 64, 65, 66, 127, 129, None, None, None, None, None, None):
        lead = decode(present[len(q)], sigma, k)[:int(rng.integers(0, k))]
        n = max(60, 300 // k) if windows is None else (windows + k - 1) // k + 2
        s = lead + "".join(decode(c, sigma, k) for c in take(n))
        q.append(s if windows is None else s[:windows + k - 1])
    c = LookupCase(sigma, k, db, q)
    c.R, c.absent, c.planted = R, absent, planted
    return c


# -- the duplicate check beyond its first pass of 32 768 branches

def dup_db(which):
    """(keys, key_offsets, branches, scores, key at fault or None).  Four keys, branch ids up to 70 000 (three passes of the check).
    "tile": key 500 names 40 000 at places 3 and 50 of 64; "apart": at places 20 and 220 of 300; "last": the last key names 70 000 at
    places 10 and 90 of 100; "control": no key names a branch twice -- 32 767, 32 768, 65 535, 65 536 and 40 000 under key 11,
    40 000 under key 500 as well."""
    rng = np.random.default_rng(4040)
    others = np.setdiff1d(np.arange(70000), [40000, 32767, 32768, 65535, 65536])
    n = {"tile": [40, 64, 130, 100], "apart": [40, 300, 130, 100], "last": [40, 64, 130, 100], "control": [40, 64, 130, 100]}[which]
    keys = np.array([11, 500, 4000, 60000], np.uint32)
    lists = [rng.choice(others, m, replace=False) for m in n]
    lists[2][7] = 70000
    bad = None
    if which == "tile":
        lists[1][[3, 50]] = 40000; bad = 500
    elif which == "apart":
        lists[1][[20, 220]] = 40000; bad = 500
    elif which == "last":
        lists[3][[10, 90]] = 70000; bad = 60000
    else:
        lists[0][[1, 5, 9, 13, 30]] = [32767, 32768, 65535, 65536, 40000]
        lists[1][50] = 40000
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
    br = np.concatenate(lists).astype(np.uint32)
    return keys, off, br, mixed_scores(rng, len(br)), bad


@functools.lru_cache(maxsize=None)
def dup_control_case():
    keys, off, br, sc, _ = dup_db("control")
    names = [decode(int(c), 4, 8) for c in keys]
    return Case(4, 8, (keys, off, br, sc), [names[0], names[1], names[0] + names[1], "".join(names), "".join(names) * 3, names[3] + "N" + names[2]])


# -- a long query under EPS_INEXACT

@functools.lru_cache(maxsize=None)
def long_case():
    """One query of 70 000 symbols made of the main database's k-mers: W = 69 993, every 8th window a key for sure."""
    m = main_case()
    rng = np.random.default_rng(70)
    s = "".join(decode(int(c), m.sigma, m.k) for c in rng.choice(m.db[0], 70000 // m.k))
    assert len(s) == 70000
    return Case(m.sigma, m.k, m.db, [s])


# -- batches under a device budget

BUDGET_ROOM = 256 << 10            # what the budget leaves above the loaded database
PLACE_QUERY_BYTES_7 = 8 + 7 * (8 + 4 + 4 + 4) + 3 * 4      # device bytes of a query's offset and results at keep_at_most = 7


def budget_draw():
    """Members of reuse_pool() for 1500 queries: their sequence and result bytes are more than twice BUDGET_ROOM."""
    return np.random.default_rng(600).integers(0, len(reuse_pool().queries), 1500)


def fused_penalty_changes(case, log_eps, keep):
    """(changed, pairs, changed among the best `keep` of a query): the scored (query, branch) pairs of the case whose score bits differ
    between the definition (the product rounded, then the sum) and a penalty added with ONE rounding,
    float32(float64(S) + float64(W - C) * float64(log_eps))."""
    changed = pairs = in_top = 0
    eps = np.float32(log_eps)
    for q in case.queries:
        W, _, S, Cn = po.accumulate(case.view, q, case.sigma, case.k)
        hit = np.nonzero(Cn)[0]
        two = S[hit] + (W - Cn[hit]).astype(np.float32) * eps
        one = (S[hit].astype(np.float64) + (W - Cn[hit]).astype(np.float64) * np.float64(eps)).astype(np.float32)
        diff = two.view(np.uint32) != one.view(np.uint32)
        best = sorted(range(len(hit)), key=lambda i: (-float(two[i]), int(hit[i])))[:keep]
        pairs += len(hit); changed += int(diff.sum()); in_top += int(diff[best].sum())
    return changed, pairs, in_top
