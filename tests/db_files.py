"""Synthetic database files for the tests of the reading side (dbfile.file_info / check_file, Engine.load_db, Engine.diff_dbs):
small host arrays written with dbfile.write_db / write_db_positions, and the same files damaged in known places."""
import struct

import numpy as np

from ipk_amd import dbfile

# entries per k-mer at the edges of the unpack and diff kernels: one wavefront (64 lanes) and one workgroup row (256) minus one,
# exactly, plus one; and one list of several 1024-entry tiles
EDGE_COUNTS = [1, 2, 63, 64, 65, 255, 256, 257, 3000]
HEADER = dict(sequence_type="DNA", tree_index=[(5, 3.25), (1, 0.5), (3, 2.0), (1, 0.75), (1, 1.0)], newick="((a:0.5,(b:0.75,c:1)x:0.25)r:0);",
              kmer_size=4, omega=1.5)


def synthetic(n_keys=200, seed=1, k=4, counts=None, keys=None, n_branches=4000):
    """A database in host arrays: ascending keys, random filter values and the filter order, every k-mer's branches distinct.
    counts: the entries per k-mer (default: EDGE_COUNTS at random k-mers, 1..8 elsewhere)."""
    rng = np.random.default_rng(seed)
    if keys is None:
        keys = np.sort(rng.choice(4 ** k, size=n_keys, replace=False)).astype(np.uint32)
    keys = np.asarray(keys, np.uint32)
    n_keys = len(keys)
    if counts is None:
        counts = rng.integers(1, 9, size=n_keys)
        at = rng.permutation(n_keys)[:len(EDGE_COUNTS)]
        counts[at] = EDGE_COUNTS[:len(at)]
    counts = np.asarray(counts, np.int64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    br = np.concatenate([rng.permutation(n_branches)[:c] for c in counts] + [np.zeros(0, np.int64)]).astype(np.uint32)
    sc = (-6.0 * rng.random(len(br))).astype(np.float32)
    pos = rng.integers(0, 65536, size=len(br)).astype(np.uint32)
    if len(pos) >= 2:
        pos[0], pos[-1] = 0, 65535
    fv = (rng.random(n_keys) * 4.0 - 2.0).astype(np.float32)
    order = np.argsort(dbfile.filter_sort_code(fv, keys), kind="stable").astype(np.uint32)
    return dict(keys=keys, off=off, br=br, sc=sc, pos=pos, fv=fv, order=order)


def write(path, db, positioned=False, header=HEADER):
    h = dbfile.header_args(header)
    if positioned:
        dbfile.write_db_positions(path, h["sequence_type"], h["tree_index"], h["newick"], h["kmer_size"], h["omega"], db["keys"], db["off"],
                                  db["br"], db["sc"], db["pos"], db["fv"], db["order"])
    else:
        dbfile.write_db(path, h["sequence_type"], h["tree_index"], h["newick"], h["kmer_size"], h["omega"], db["keys"], db["off"], db["br"],
                        db["sc"], db["fv"], db["order"])
    return path


def record_starts(db, positioned=False):
    """Byte offset of every record inside the body, in file order, and the body's size."""
    cnt = (db["off"][1:] - db["off"][:-1]).astype(np.int64)[db["order"]]
    size = 16 + (10 if positioned else 8) * cnt
    ends = np.cumsum(size)
    return (ends - size), int(ends[-1]) if len(ends) else 0


def damaged(tmp_path, db, positioned=False):
    """{name: (path, record index the message must name or None)}: the file of `db` cut or edited in one place each."""
    good = write(tmp_path / ("good_pos.ipk" if positioned else "good.ipk"), db, positioned)
    raw = good.read_bytes()
    body_at = dbfile.file_info(good)["body_offset"]
    starts, body = record_starts(db, positioned)
    assert body_at + body == len(raw)
    tag = "pos_" if positioned else ""
    out = {}

    def put(name, data, rec):
        p = tmp_path / f"{tag}{name}.ipk"
        p.write_bytes(data)
        out[name] = (p, rec)

    r = len(starts) // 2
    cnt = struct.unpack_from("<Q", raw, body_at + int(starts[r]) + 8)[0]
    put("truncated", raw[:body_at + int(starts[r]) + 16 + 3], r)                       # in the middle of record r (its first entry)
    put("truncated_head", raw[:body_at + int(starts[-1]) + 9], len(starts) - 1)        # inside the last record's head

    def with_count(rec, value):
        b = bytearray(raw)
        struct.pack_into("<Q", b, body_at + int(starts[rec]) + 8, value)
        return bytes(b)

    put("count_plus_one", with_count(r, cnt + 1), None)              # (every later head is read from the wrong place: some record is refused)
    put("count_last_plus_one", with_count(len(starts) - 1, struct.unpack_from("<Q", raw, body_at + int(starts[-1]) + 8)[0] + 1), len(starts) - 1)
    put("count_2_40", with_count(r, 1 << 40), r)
    put("count_zeroed", with_count(r, 0), None)
    b = bytearray(raw)
    struct.pack_into("<Q", b, body_at - 16, len(starts) + 1)
    put("total_kmers", bytes(b), None)
    b = bytearray(raw)
    struct.pack_into("<Q", b, body_at - 8, int(db["off"][-1]) - 1)
    put("total_entries", bytes(b), None)
    return good, out
