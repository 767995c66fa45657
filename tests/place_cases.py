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
