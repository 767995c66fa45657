"""Cases for the union of databases with disjoint key sets (ipkgpu_db_union, Engine.union_dbs, `ipk.py merge`) and a numpy
restatement of the union: concatenate the shards' keys, sort by key, gather counts, entries, positions and filter values, and order
the keys by dbfile.filter_sort_code.

A case is a dict: name, header (tests/db_files.HEADER's fields), shards -- each a database in host arrays as db_files.synthetic makes
them (keys, off, br, sc, pos, fv, order), in its own filter order, so that a file written from it is what a build writes.  Every case
serves plain and positioned (db_files.write(..., positioned)).  The hosts' files are a few hundred keys each.

Case 7 of the list this suite was planned with, keys WITHOUT entries, is included: dbfile.write_db -> read_db round-trips such a record
on the CPU (checked by tests/test_union_inputs.py::test_entryless_records_round_trip_on_the_host, which the case depends on)."""
import functools

import numpy as np

from ipk_amd import dbfile
from tests import db_files as F

TILE = 1024                                         # DB_UNPACK_TILE: entries per workgroup of the copy kernel
K8 = dict(F.HEADER, kmer_size=8)
K16 = dict(F.HEADER, kmer_size=16)
F32_MAX = np.float32(3.4028235e38)


def take(db, idx):
    """The shard of `db` that holds its keys at the (ascending) positions idx, in its own filter order."""
    idx = np.asarray(idx, np.int64)
    off = db["off"].astype(np.int64)
    cnt = (off[1:] - off[:-1])[idx]
    ent = np.concatenate([np.arange(off[i], off[i + 1]) for i in idx] + [np.zeros(0, np.int64)]).astype(np.int64)
    keys, fv = db["keys"][idx], db["fv"][idx]
    return dict(keys=keys, off=np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64), br=db["br"][ent], sc=db["sc"][ent], pos=db["pos"][ent],
                fv=fv, order=np.argsort(dbfile.filter_sort_code(fv, keys), kind="stable").astype(np.uint32))


def split(db, owner, n_owners):
    """One shard per owner: owner[i] is the owner of the key at position i."""
    owner = np.asarray(owner)
    return [take(db, np.nonzero(owner == o)[0]) for o in range(n_owners)]


def restate(shards):
    """The union of the shards in host arrays (fv64: the float32 values widened, as a loaded file's are)."""
    keys = np.concatenate([s["keys"] for s in shards]).astype(np.uint32)
    cnt = np.concatenate([(s["off"][1:] - s["off"][:-1]).astype(np.int64) for s in shards] + [np.zeros(0, np.int64)])
    fv = np.concatenate([s["fv"] for s in shards]).astype(np.float32)
    e_base = np.concatenate([[0], np.cumsum([len(s["br"]) for s in shards])]).astype(np.int64)
    start = np.concatenate([s["off"][:-1].astype(np.int64) + e_base[i] for i, s in enumerate(shards)] + [np.zeros(0, np.int64)])
    br = np.concatenate([s["br"] for s in shards]); sc = np.concatenate([s["sc"] for s in shards]); pos = np.concatenate([s["pos"] for s in shards])
    perm = np.argsort(keys, kind="stable")
    assert len(np.unique(keys)) == len(keys), "the shards' key sets are not disjoint"
    keys, cnt, fv, start = keys[perm], cnt[perm], fv[perm], start[perm]
    ent = np.concatenate([np.arange(a, a + c) for a, c in zip(start, cnt)] + [np.zeros(0, np.int64)]).astype(np.int64)
    return dict(keys=keys, off=np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64), br=br[ent].astype(np.uint32), sc=sc[ent].astype(np.float32),
                pos=pos[ent].astype(np.uint32), fv=fv, order=np.argsort(dbfile.filter_sort_code(fv, keys), kind="stable").astype(np.uint32))


def _owners_whole():
    return F.synthetic(600, seed=11, k=8)            # EDGE_COUNTS at random k-mers


def owners(p):
    db = _owners_whole()
    return dict(name=f"owners{p}", header=K8, shards=split(db, db["keys"] % p, p))


def owners_empty():
    """Five owners by key % 5, the keys chosen so that owner 4 has none."""
    rng = np.random.default_rng(12)
    pool = np.arange(4 ** 8)
    keys = np.sort(rng.choice(pool[pool % 5 != 4], size=300, replace=False))
    db = F.synthetic(seed=12, k=8, keys=keys)
    return dict(name="owners5_one_empty", header=K8, shards=split(db, db["keys"] % 5, 5))


def ranges():
    """Four contiguous key ranges, the third one empty."""
    db = F.synthetic(400, seed=13, k=8)
    owner = np.zeros(400, np.int64)
    owner[90:250] = 1
    owner[250:] = 3
    return dict(name="ranges", header=K8, shards=split(db, owner, 4))


TILES_RUN = 1100


def tiles():
    """Counts at the copy kernel's tile edges: the first key has exactly TILE entries (the next record starts at a tile boundary), one
    key has 5000 (whole tiles inside one record), a run of 1100 one-entry keys follows (more keys than lanes in one tile), the last
    tile is partial, and neighbouring keys come from different shards throughout (owner = position % 2)."""
    counts = [TILE, 5000, 3, 7] + [1] * TILES_RUN + [2, 65, 300]
    rng = np.random.default_rng(14)
    keys = np.sort(rng.choice(4 ** 8, size=len(counts), replace=False))
    db = F.synthetic(seed=14, k=8, keys=keys, counts=counts, n_branches=6000)
    return dict(name="tiles", header=K8, shards=split(db, np.arange(len(counts)) % 2, 2))


def many_sources():
    """64 shards of 1 to 3 keys each beside one of 400 keys."""
    db = F.synthetic(400 + 128, seed=15, k=8)
    rng = np.random.default_rng(15)
    owner = np.zeros(528, np.int64)
    small = rng.permutation(528)[:128]
    sizes = np.array([1, 2, 3] * 21 + [1], np.int64)           # 64 sizes, 127 keys
    at = 0
    for s, n in enumerate(sizes):
        owner[small[at:at + n]] = 1 + s
        at += n
    return dict(name="many_sources", header=K8, shards=split(db, owner, 65))


def filter_ties():
    """Equal float32 filter values in different shards (the tie is broken by key), -0.0 and +0.0, a negative and a positive value and
    the largest finite one."""
    db = F.synthetic(240, seed=16, k=8)
    vals = np.array([-0.0, 0.0, -1.5, 1.5, F32_MAX, 0.25, 0.25, 0.25], np.float32)
    db["fv"] = vals[np.arange(240) % len(vals)].copy()
    return dict(name="filter_ties", header=K8, shards=split(db, np.arange(240) % 3, 3))         # 8 and 3 are coprime: every value in every shard


def key_bounds():
    """A head with kmer_size 16 and the keys 0 and 0xFFFFFFFF in different shards."""
    rng = np.random.default_rng(17)
    keys = np.unique(np.concatenate([[0, 0xFFFFFFFF], rng.integers(1, 0xFFFFFFFF, size=198)])).astype(np.uint32)
    db = F.synthetic(seed=17, k=16, keys=keys)
    owner = np.arange(len(keys)) % 2
    owner[0], owner[-1] = 0, 1
    return dict(name="key_bounds", header=K16, shards=split(db, owner, 2))


def entryless():
    """Keys without entries at the first, a middle and the last position of the union, in different shards."""
    n = 150
    rng = np.random.default_rng(18)
    keys = np.sort(rng.choice(4 ** 8, size=n, replace=False))
    counts = rng.integers(1, 9, size=n)
    counts[[0, n // 2, n - 1]] = 0
    counts[5] = 2 * TILE + 5
    db = F.synthetic(seed=18, k=8, keys=keys, counts=counts)
    return dict(name="entryless", header=K8, shards=split(db, np.arange(n) % 3, 3))


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every case, built once; the arrays are shared by the tests and must not be changed."""
    cs = [owners(1), owners(2), owners(3), owners(8), owners_empty(), ranges(), tiles(), many_sources(), filter_ties(), key_bounds(), entryless()]
    for c in cs:
        c["want"] = restate(c["shards"])
    return tuple(cs)


CASE_NAMES = ["owners1", "owners2", "owners3", "owners8", "owners5_one_empty", "ranges", "tiles", "many_sources", "filter_ties", "key_bounds", "entryless"]


def case(name):
    return next(c for c in all_cases() if c["name"] == name)


def write_shards(directory, c, positioned):
    """The case's shards as files (shard<i>.ipk), each under the case's header with its own totals."""
    return [str(F.write(directory / f"{c['name']}_{int(positioned)}_shard{i}.ipk", s, positioned, c["header"])) for i, s in enumerate(c["shards"])]


def host_merged(directory, c, positioned):
    """The host merge of the case's shard files (dbfile.merge_shard_files, no GPU) -> (merged path, shard paths)."""
    paths = write_shards(directory, c, positioned)
    out = directory / f"{c['name']}_{int(positioned)}_merged.ipk"
    totals = dbfile.merge_shard_files(out, **dbfile.header_args(c["header"]), shard_paths=paths)
    assert totals == (len(c["want"]["keys"]), int(c["want"]["off"][-1]))
    return str(out), paths


def reads_of(want, k, n_reads=12, seed=5):
    """Query sequences that look up keys of the database: each read spells a few of its k-mers end to end."""
    from ipk_amd.cli import decode_kmer
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(n_reads):
        ks = rng.choice(want["keys"], size=4, replace=False)
        reads.append("".join(decode_kmer(int(x), k, "DNA") for x in ks))
    return reads
