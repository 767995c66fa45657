"""The cases of tests/test_select_inputs.py (host) and tests/test_gpu_db_select.py / test_gpu_cli_select.py (device), and the selection's
definition (ipkgpu_db_select in include/ipkgpu.h) restated in numpy over the dictionaries of tests/db_files.synthetic.
Test infrastructure only: nothing under ipk_amd/ imports it."""
import numpy as np

from ipk_amd import dbfile
from tests import db_files as F

TILE = 1024                      # entries per workgroup of the selection's per-entry kernels (DB_UNPACK_TILE)
M_GRID = [0, 1, 2, 199, 200, 201, 1 << 40]
NEG_INF, POS_INF = np.float32(-np.inf), np.float32(np.inf)


def restate(db, keep_kmers, t, positioned=True):
    """The selection V of `db` (keys, off, br, sc, pos, fv, order) at (keep_kmers, t), step by step as the header states it."""
    keys, off, order = np.asarray(db["keys"], np.uint32), np.asarray(db["off"], np.uint64), np.asarray(db["order"], np.uint32)
    sc = np.asarray(db["sc"], np.float32)
    n = len(keys)
    m = min(int(keep_kmers), n)
    cand = np.zeros(n, bool)
    cand[order[:m]] = True                                                     # 1. the first M records of the order
    cnt = (off[1:] - off[:-1]).astype(np.int64)
    key_of = np.repeat(np.arange(n), cnt)
    with np.errstate(invalid="ignore"):
        above = sc > np.float32(t)                                             # 2. binary32, strict; NaN fails
    keep = (cand[key_of] & above) if n else np.zeros(0, bool)
    new_cnt = np.bincount(key_of[keep], minlength=n).astype(np.int64) if n else np.zeros(0, np.int64)
    stays = new_cnt > 0                                                        # 3. a key without an entry is dropped
    new_index = np.cumsum(stays) - 1
    survivors = [int(j) for j in order[:m] if stays[j]]                        # 4. the surviving records, in D's order
    out = dict(keys=keys[stays], off=np.concatenate([[0], np.cumsum(new_cnt[stays])]).astype(np.uint64), br=np.asarray(db["br"], np.uint32)[keep],
               sc=sc[keep], fv=np.asarray(db["fv"], np.float32)[stays], order=new_index[survivors].astype(np.uint32))
    if positioned:
        out["pos"] = np.asarray(db["pos"], np.uint32)[keep]
    return out


def same_arrays(a, b, positioned=True):
    """Two database dictionaries, array for array and bit for bit."""
    names = ["keys", "off", "br", "fv", "order", "sc"] + (["pos"] if positioned else [])
    return all(np.array_equal(np.asarray(a[x]).view(np.uint32) if np.asarray(a[x]).dtype == np.float32 else np.asarray(a[x]),
                              np.asarray(b[x]).view(np.uint32) if np.asarray(b[x]).dtype == np.float32 else np.asarray(b[x])) for x in names)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------

SANDWICH = 100                   # key index: all entries of keys SANDWICH - 1 and SANDWICH + 1 pass t = T_MID, all of SANDWICH fail
T_LOW, T_MID = np.float32(-7.0), np.float32(-3.0)


def edges():
    """synthetic(n_keys=200) with EDGE_COUNTS, plus: an all-fail key between two all-pass keys at T_MID, and inside the 3000-entry list
    an entry whose score bits are t_exact() beside one a single step above it."""
    db = F.synthetic(200, seed=5)
    off, sc = db["off"], db["sc"]
    for j, value in ((SANDWICH - 1, -1.0), (SANDWICH, -5.0), (SANDWICH + 1, -2.0)):
        sc[int(off[j]):int(off[j + 1])] = np.float32(value)
    a = exact_entry(db)
    sc[a] = np.float32(-2.75)
    sc[a + 1] = np.nextafter(np.float32(-2.75), np.float32(0))
    return db


def long_key(db):
    cnt = (db["off"][1:] - db["off"][:-1]).astype(np.int64)
    return int(np.argmax(cnt))


def exact_entry(db):
    """Index of the entry whose bits t_exact() takes: the 100th of the longest list (its neighbour passes by one step)."""
    return int(db["off"][long_key(db)]) + 100


def t_exact(db):
    return np.float32(db["sc"][exact_entry(db)])


def t_grid(db):
    return [NEG_INF, T_LOW, T_MID, t_exact(db), POS_INF]


def heavy():
    """One key of 5000 entries among 3000 keys of one entry each (DNA k = 8); the threshold is the median score."""
    rng = np.random.default_rng(21)
    keys = np.sort(rng.choice(4 ** 8, size=3001, replace=False)).astype(np.uint32)
    counts = np.ones(3001, np.int64)
    counts[1700] = 5000
    db = F.synthetic(keys=keys, counts=counts, seed=22, n_branches=6000)
    return db, np.float32(np.median(db["sc"]))


def single():
    return F.synthetic(keys=[201], counts=[3], seed=6)


def equal_fv():
    """50 k-mers in five runs of equal filter values: the order inside a run is by ascending key."""
    db = F.synthetic(50, seed=31)
    db["fv"] = np.repeat(np.array([0.5, -1.25, 0.5, 0.0, -1.25], np.float32), 10)
    db["order"] = np.argsort(dbfile.filter_sort_code(db["fv"], db["keys"]), kind="stable").astype(np.uint32)
    return db


HEAVY_HEADER = dict(F.HEADER, kmer_size=8)


# ---- build equivalence: the smallest scoring input of the GPU parity tests (tests/test_gpu_parity.py::test_dna_all_k at k = 8) ----------

BUILD_K, BUILD_SIGMA, BUILD_GROUPS, BUILD_OMEGAS = 8, 4, [5, 5, 9, 9], (1.5, 1.8)


def build_mats():
    from ipk_amd.synth import synth_matrices
    return synth_matrices(4, 48, 4, 0.1, 200 + BUILD_K)


def oracle_db(mats, log_eps):
    """The CPU oracle's key-major database of the build input at a threshold, as a dictionary restate() takes."""
    from oracle import db_oracle, ipk_oracle as co
    groups = np.asarray(BUILD_GROUPS)
    res = []
    for g in dict.fromkeys(BUILD_GROUPS):
        keys, scores, _ = co.explore_group(mats[groups == g], BUILD_K, log_eps)
        res.append((g, keys, scores))
    keys, off, br, bits = db_oracle.db_shard_arrays(db_oracle.build_db(res), BUILD_SIGMA, BUILD_K, 0, 1)
    n = len(keys)
    return dict(keys=keys, off=off, br=br, sc=bits.view(np.float32), fv=np.zeros(n, np.float32), order=np.arange(n, dtype=np.uint32))


def entry_sets(db):
    """key -> the set of its (branch, score bits)."""
    off, bits = db["off"], np.asarray(db["sc"], np.float32).view(np.uint32)
    return {int(k): set(zip(db["br"][int(off[i]):int(off[i + 1])].tolist(), bits[int(off[i]):int(off[i + 1])].tolist())) for i, k in enumerate(db["keys"])}


def queries_of(db, k, n_queries=6, seed=3):
    """Query strings made of the database's own k-mers (and a stretch of N), so that placements exist."""
    from ipk_amd.cli import decode_kmer
    rng = np.random.default_rng(seed)
    out = []
    for q in range(n_queries):
        picks = rng.choice(len(db["keys"]), size=min(len(db["keys"]), 3 + 5 * q), replace=False)
        out.append("NN".join(decode_kmer(db["keys"][i], k, "DNA") for i in picks))
    return out + ["", "ACGTNACG"]
