"""The cases of tests/test_stream_inputs.py (host) and tests/test_gpu_stream.py / test_gpu_cli_stream.py (device), and the definitions of
include/ipkgpu.h restated in numpy: the k-mer set K of a batch of queries (ipkgpu_kmer_set_of_queries) from place_ext_oracle's windows,
the restriction R(D, K) (ipkgpu_db_select_keys) by select_cases.restate's array rules, and the window cuts of ipkgpu_db_load_wanted.
Test infrastructure only: nothing under ipk_amd/ imports it."""
import functools

import numpy as np

from tests import db_files as F
from tests import place_cases as pc
from tests import place_ext_oracle as xo
from tests import place_oracle as po
from tests import select_cases as S


# ---- the definitions ---------------------------------------------------------------------------------------------------------------------

def kmer_codes(seqs, sigma, k, ambiguity=False, strands="given"):
    """K: every code the placement of `seqs` with these options passes to its lookup."""
    out = set()
    for q in seqs:
        q = q.decode("latin-1") if isinstance(q, bytes) else q
        for strand in ([q, xo.revcomp(q)] if strands == "both" else [q]):
            for _, codes in xo.windows(strand, sigma, k):
                if len(codes) == 1 or ambiguity:                              # (without the option an ambiguous symbol is an invalid byte)
                    out.update(codes)
    return out


def n_words(sigma, k):
    return max(2, (1 << (po.ALPHABET[sigma][1] * k)) // 32)


def words_of(codes, sigma, k):
    """The bitmap: bit `code` of 32-bit word code >> 5."""
    w = np.zeros(n_words(sigma, k), np.uint32)
    c = np.fromiter(codes, np.int64, len(codes))
    np.bitwise_or.at(w, c >> 5, (np.uint32(1) << (c & 31).astype(np.uint32)))
    return w


def restrict(db, codes, positioned=True):
    """R(D, K): the keys of D in K, each with all its entries; arrays by rule 4 of the selection (the surviving records in D's order,
    renumbered; filter values bit for bit)."""
    keys, off, order = np.asarray(db["keys"], np.uint32), np.asarray(db["off"], np.uint64), np.asarray(db["order"], np.uint32)
    n = len(keys)
    stays = np.fromiter((int(x) in codes for x in keys), bool, n)
    cnt = (off[1:] - off[:-1]).astype(np.int64)
    keep = np.repeat(stays, cnt)
    new_index = np.cumsum(stays) - 1
    survivors = [int(j) for j in order if stays[j]]
    out = dict(keys=keys[stays], off=np.concatenate([[0], np.cumsum(cnt[stays])]).astype(np.uint64), br=np.asarray(db["br"], np.uint32)[keep],
               sc=np.asarray(db["sc"], np.float32)[keep], fv=np.asarray(db["fv"], np.float32)[stays], order=new_index[survivors].astype(np.uint32))
    if positioned:
        out["pos"] = np.asarray(db["pos"], np.uint32)[keep]
    return out


def expected(db, codes, keep_kmers, t, positioned=True):
    """ipkgpu_db_load_wanted's contract: select_keys(load_select(path, M, t), set)."""
    return restrict(S.restate(db, keep_kmers, t, positioned), codes, positioned)


def record_sizes(db, positioned):
    cnt = (db["off"][1:] - db["off"][:-1]).astype(np.int64)[db["order"]]
    return (16 + (10 if positioned else 8) * cnt).tolist()


def windows_of(sizes, cap):
    """The window cuts of the streamed load as [(first record, one past the last)]: a window is closed at the start of the first record
    that would end beyond `cap` bytes; a record longer than `cap` is a window of its own (the device block grows, the cuts do not)."""
    out, first, used = [], 0, 0
    for r, size in enumerate(sizes):
        if used + size > cap and r > first:
            out.append((first, r))
            first, used = r, 0
        used += size
    if len(sizes) > first:
        out.append((first, len(sizes)))
    return out


def queries_naming(codes, sigma, k, per_query=7):
    """Queries whose k-mer set is exactly `codes`: the k-mers one behind the other with an invalid byte between them."""
    names = [pc.decode(int(c), sigma, k) for c in sorted(codes)]
    return ["-".join(names[i:i + per_query]) for i in range(0, len(names), per_query)] or [""]


# ---- the streamed file: DNA k = 4 (F.HEADER), 200 records, its hard spots -------------------------------------------------------------------

K4 = F.HEADER["kmer_size"]
OUTSIDE = 4 ** K4                 # the first value outside the code space: a fabricated record carries it as its key
FIRST_WINDOW = 5                  # records of the first window at STREAM cap: it is exactly full
CHUNK = 64                        # "db_load_chunk_bytes" of the streamed tests: heads straddle chunks, most records are longer than one
ABSENT = 77                       # a code the queries name and the file does not hold


@functools.lru_cache(maxsize=None)
def stream_db():
    """199 keys of the code space with 31, 32 and 4^k - 1 among them, and the key 4^k; EDGE_COUNTS (one record of 3000 entries) as in
    tests/db_files.synthetic."""
    rng = np.random.default_rng(77)
    rest = [c for c in range(4 ** K4) if c not in (31, 32, 4 ** K4 - 1, ABSENT)]
    keys = sorted(rng.choice(rest, 196, replace=False).tolist() + [31, 32, 4 ** K4 - 1, OUTSIDE])
    return F.synthetic(keys=keys, seed=78)


def window_cap(positioned, which="several"):
    """The three window sizes: "longest" -- the smallest that holds the longest record; "several" -- the first FIRST_WINDOW records' bytes
    (the first window is exactly full, the 3000-entry record is longer than the window); "default" -- 0, the library's."""
    sizes = record_sizes(stream_db(), positioned)
    return {"longest": max(sizes), "several": sum(sizes[:FIRST_WINDOW]), "default": 0}[which]


@functools.lru_cache(maxsize=None)
def stream_wanted(positioned):
    """The wanted codes at window_cap(positioned, "several"): the first window's first and last records, none of one later window,
    all of another, the file's last record, 31, 32 and 4^k - 1, every third record of the rest -- and a code the file does not hold."""
    db = stream_db()
    keys_in_file_order = db["keys"][db["order"]].tolist()
    wins = windows_of(record_sizes(db, positioned), window_cap(positioned))
    must = {31, 32, 4 ** K4 - 1, keys_in_file_order[0], keys_in_file_order[wins[0][1] - 1], keys_in_file_order[-1]}
    inside = lambda w: set(keys_in_file_order[w[0]:w[1]])
    none_w = next(w for w in wins[1:] if not inside(w) & must)
    all_w = next(w for w in wins[1:] if w != none_w and w[1] - w[0] > 1 and OUTSIDE not in inside(w))
    want = must | {ABSENT} | inside(all_w) | set(keys_in_file_order[::3])
    want -= inside(none_w) | {OUTSIDE}
    return frozenset(want)


def stream_queries(positioned):
    return queries_naming(stream_wanted(positioned), 4, K4)


# ---- placement: a case's database as a file with filter values and an order of its own ---------------------------------------------------

def case_db_dict(case, seed=5):
    """The case's database as the dictionary tests/db_files.write takes: random filter values, their order, positions."""
    keys, off, br, sc = case.db
    rng = np.random.default_rng(seed)
    fv = (rng.random(len(keys)) * 4.0 - 2.0).astype(np.float32)
    from ipk_amd import dbfile
    order = np.argsort(dbfile.filter_sort_code(fv, np.asarray(keys, np.uint32)), kind="stable").astype(np.uint32)
    return dict(keys=np.asarray(keys, np.uint32), off=np.asarray(off, np.uint64), br=np.asarray(br, np.uint32), sc=np.asarray(sc, np.float32),
                pos=rng.integers(0, 65536, size=len(br)).astype(np.uint32), fv=fv, order=order)


def case_header(case):
    return dict(F.HEADER, sequence_type="DNA" if case.sigma == 4 else "AA", kmer_size=case.k)


def view_of(d):
    return po.DbView(d["keys"], d["off"], d["br"], d["sc"])
