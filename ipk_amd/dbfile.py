"""Database file: Python face of the C++ serialiser, plus a reader for the tests.

IPK streams its database through i2l::save_header / save_phylo_kmer over a Boost binary_oarchive
(ipk/src/db_builder.cpp:145-146,176-177,297-306,323-327).  The byte layout lives in ONE place,
ipk_amd/csrc/ipk_format.hpp (a reconstruction: i2l and Boost are un-vendored, so it is not pinned against a real .ipk);
it is written by ipkgpu_db_write (streamed from the device: every build path, filter_and_write_device) and ipkgpu_db_write_host
(host arrays: the C ABI's host serialiser and the tests' yardstick).  This module calls both and parses the layout back for the tests.
"""
import ctypes as C
import os
import struct

import numpy as np

from .engine import IpkGpuError, load_library

ABI_SYMBOLS = ["ipkgpu_db_write", "ipkgpu_db_write_host", "ipkgpu_db_write_host_positions", "ipkgpu_db_write_last_error", "ipkgpu_db_write_time_s",
               "ipkgpu_db_merge_files", "ipkgpu_db_merge_last_error", "ipkgpu_db_protocol_version",
               "ipkgpu_db_file_open", "ipkgpu_db_file_close", "ipkgpu_db_file_last_error", "ipkgpu_db_file_check", "ipkgpu_db_file_header",
               "ipkgpu_db_file_sequence_type", "ipkgpu_db_file_positions_loaded", "ipkgpu_db_file_protocol_version",
               "ipkgpu_db_file_library_version", "ipkgpu_db_file_tree_index_size", "ipkgpu_db_file_tree_num_nodes",
               "ipkgpu_db_file_tree_subtree_length", "ipkgpu_db_file_newick", "ipkgpu_db_file_kmer_size", "ipkgpu_db_file_omega",
               "ipkgpu_db_file_total_kmers", "ipkgpu_db_file_total_entries", "ipkgpu_db_file_bytes", "ipkgpu_db_file_body_offset"]
_bound = False


class _Header(C.Structure):
    _fields_ = [("sequence_type", C.c_char_p), ("tree_index_size", C.c_uint64), ("tree_num_nodes", C.POINTER(C.c_uint32)),
                ("tree_subtree_length", C.POINTER(C.c_double)), ("newick", C.c_char_p), ("kmer_size", C.c_uint64),
                ("omega", C.c_float)]


def _lib():
    global _bound
    L = load_library()
    if not _bound:
        L.ipkgpu_db_write.restype = C.c_int
        L.ipkgpu_db_write.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(_Header), C.c_char_p, C.POINTER(C.c_uint64)]
        L.ipkgpu_db_write_host.restype = C.c_int
        L.ipkgpu_db_write_host.argtypes = [C.POINTER(_Header), C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_char_p, C.POINTER(C.c_uint64)]
        L.ipkgpu_db_write_host_positions.restype = C.c_int
        L.ipkgpu_db_write_host_positions.argtypes = [C.POINTER(_Header), C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64)]
        L.ipkgpu_db_write_last_error.restype = C.c_char_p
        L.ipkgpu_db_write_last_error.argtypes = []
        L.ipkgpu_db_write_time_s.restype = C.c_double
        L.ipkgpu_db_write_time_s.argtypes = [C.c_void_p, C.c_int]
        L.ipkgpu_db_merge_files.restype = C.c_int
        L.ipkgpu_db_merge_files.argtypes = [C.POINTER(_Header), C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p, C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.ipkgpu_db_merge_last_error.restype = C.c_char_p
        L.ipkgpu_db_merge_last_error.argtypes = []
        L.ipkgpu_db_protocol_version.restype = C.c_uint32
        L.ipkgpu_db_protocol_version.argtypes = []
        L.ipkgpu_db_file_open.restype = C.c_int
        L.ipkgpu_db_file_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.ipkgpu_db_file_close.restype = None
        L.ipkgpu_db_file_close.argtypes = [C.c_void_p]
        L.ipkgpu_db_file_last_error.restype = C.c_char_p
        L.ipkgpu_db_file_last_error.argtypes = []
        L.ipkgpu_db_file_check.restype = C.c_int
        L.ipkgpu_db_file_check.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.ipkgpu_db_file_header.restype = C.c_int
        L.ipkgpu_db_file_header.argtypes = [C.c_void_p, C.POINTER(_Header)]
        for name, t in (("sequence_type", C.c_char_p), ("positions_loaded", C.c_int), ("protocol_version", C.c_uint32),
                        ("library_version", C.c_uint32), ("tree_index_size", C.c_uint64), ("tree_num_nodes", C.POINTER(C.c_uint32)),
                        ("tree_subtree_length", C.POINTER(C.c_double)), ("newick", C.c_char_p), ("kmer_size", C.c_uint64),
                        ("omega", C.c_float), ("total_kmers", C.c_uint64), ("total_entries", C.c_uint64), ("bytes", C.c_uint64),
                        ("body_offset", C.c_uint64)):
            fn = getattr(L, "ipkgpu_db_file_" + name)
            fn.restype = t
            fn.argtypes = [C.c_void_p]
        _bound = True
    return L


def _header(sequence_type, tree_index, newick, kmer_size, omega):
    """tree_index: (num_nodes u32 [n], subtree_branch_length f64 [n]) or a list of (num_nodes, length) pairs."""
    if isinstance(tree_index, tuple) and len(tree_index) == 2 and hasattr(tree_index[0], "dtype"):
        nn, sl = tree_index
    else:
        nn = np.array([t[0] for t in tree_index], dtype=np.uint32)
        sl = np.array([t[1] for t in tree_index], dtype=np.float64)
    nn, sl = np.ascontiguousarray(nn, np.uint32), np.ascontiguousarray(sl, np.float64)
    h = _Header(sequence_type.encode(), len(nn), nn.ctypes.data_as(C.POINTER(C.c_uint32)), sl.ctypes.data_as(C.POINTER(C.c_double)),
                newick.encode(), int(kmer_size), float(omega))
    h._keep = (nn, sl)
    return h


def write_db_device(engine, db, path, sequence_type, tree_index, newick, kmer_size, omega):
    """ipkgpu_db_write: the shard `db` (filter values computed) streamed from device memory. Returns bytes written."""
    L = _lib()
    h = _header(sequence_type, tree_index, newick, kmer_size, omega)
    n = C.c_uint64()
    rc = L.ipkgpu_db_write(engine._h, db._h, C.byref(h), str(path).encode(), C.byref(n))
    if rc != 0:
        raise engine._err(rc)
    return int(n.value)


def filter_and_write_device(engine, db, file, filter_, sequence_type, tree_index, newick, k, omega, n_nodes, threshold):
    """The one filter-and-write stage of every build path: the shard `db` filtered on the device (filter_ "mif0": n_nodes = MIF0's N,
    threshold = the score threshold, not its log; "random": neither is used) and streamed to `file` by the device writer.
    Returns (seconds in the filter, seconds in the write)."""
    import time
    t0 = time.time()
    if filter_ == "mif0":
        db.filter_mif0(engine, n_nodes, threshold)
    elif filter_ == "random":
        db.filter_random(engine)
    else:
        raise ValueError(f"unknown filter {filter_!r} (mif0, random)")
    t1 = time.time()
    write_db_device(engine, db, file, sequence_type, tree_index, newick, k, omega)
    return t1 - t0, time.time() - t1


def write_times(engine):
    L = _lib()
    return {k: float(L.ipkgpu_db_write_time_s(engine._h, i)) for i, k in enumerate(("total_s", "device_s", "file_s"))}


def write_db(path, sequence_type, tree_index, newick, kmer_size, omega, keys, key_offsets, branches, scores, filter_values, order):
    """ipkgpu_db_write_host over host arrays: a database shard (ascending keys); order = positions in filter order."""
    L = _lib()
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    off = np.ascontiguousarray(key_offsets, dtype=np.uint64)
    ent = np.empty((len(branches), 2), dtype=np.uint32)
    ent[:, 0] = np.asarray(branches, dtype=np.uint32)
    ent[:, 1] = np.asarray(scores, dtype=np.float32).view(np.uint32)
    fv = np.ascontiguousarray(filter_values, dtype=np.float32)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    if len(off) == 0:
        off = np.zeros(1, np.uint64)
    h = _header(sequence_type, tree_index, newick, kmer_size, omega)
    n = C.c_uint64()
    rc = L.ipkgpu_db_write_host(C.byref(h), len(keys), keys.ctypes.data, off.ctypes.data, ent.ctypes.data, fv.ctypes.data,
                                order.ctypes.data, str(path).encode(), C.byref(n))
    if rc != 0:
        raise IpkGpuError(rc, L.ipkgpu_db_write_last_error().decode())
    return int(n.value)


def write_db_positions(path, sequence_type, tree_index, newick, kmer_size, omega, keys, key_offsets, branches, scores, positions,
                       filter_values, order):
    """ipkgpu_db_write_host_positions: the positioned database of ipk-aa-pos -- as write_db, every entry with the window position of
    its kept score (db_builder.cpp:655-662,687-689)."""
    L = _lib()
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    off = np.ascontiguousarray(key_offsets, dtype=np.uint64)
    ent = np.empty((len(branches), 2), dtype=np.uint32)
    ent[:, 0] = np.asarray(branches, dtype=np.uint32)
    ent[:, 1] = np.asarray(scores, dtype=np.float32).view(np.uint32)
    pos = np.ascontiguousarray(positions, dtype=np.uint32)
    fv = np.ascontiguousarray(filter_values, dtype=np.float32)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    if len(off) == 0:
        off = np.zeros(1, np.uint64)
    h = _header(sequence_type, tree_index, newick, kmer_size, omega)
    n = C.c_uint64()
    rc = L.ipkgpu_db_write_host_positions(C.byref(h), len(keys), keys.ctypes.data, off.ctypes.data, ent.ctypes.data, pos.ctypes.data,
                                          fv.ctypes.data, order.ctypes.data, str(path).encode(), C.byref(n))
    if rc != 0:
        raise IpkGpuError(rc, L.ipkgpu_db_write_last_error().decode())
    return int(n.value)


def protocol_version():
    """What the writers put behind the archive preamble (0: no protocol word, no positions flag); ipk_format.hpp."""
    return int(_lib().ipkgpu_db_protocol_version())


def info_of_handle(h):
    """The head of an open ipkgpu_db_file as the dict read_db returns, plus file_bytes and body_offset."""
    L = _lib()
    n = int(L.ipkgpu_db_file_tree_index_size(h))
    nn, sl = L.ipkgpu_db_file_tree_num_nodes(h), L.ipkgpu_db_file_tree_subtree_length(h)
    return dict(sequence_type=L.ipkgpu_db_file_sequence_type(h).decode(), tree_index=[(int(nn[i]), float(sl[i])) for i in range(n)],
                newick=L.ipkgpu_db_file_newick(h).decode(), kmer_size=int(L.ipkgpu_db_file_kmer_size(h)),
                omega=float(L.ipkgpu_db_file_omega(h)), total_num_kmers=int(L.ipkgpu_db_file_total_kmers(h)),
                total_num_entries=int(L.ipkgpu_db_file_total_entries(h)), library_version=int(L.ipkgpu_db_file_library_version(h)),
                protocol_version=int(L.ipkgpu_db_file_protocol_version(h)), positions_loaded=bool(L.ipkgpu_db_file_positions_loaded(h)),
                file_bytes=int(L.ipkgpu_db_file_bytes(h)), body_offset=int(L.ipkgpu_db_file_body_offset(h)))


def header_args(info):
    """The writers' header arguments out of a file_info / Db.header dict."""
    return dict(sequence_type=info["sequence_type"], tree_index=info["tree_index"], newick=info["newick"], kmer_size=info["kmer_size"],
                omega=info["omega"])


def _open(path):
    L = _lib()
    h = C.c_void_p()
    rc = L.ipkgpu_db_file_open(os.fsencode(path), C.byref(h))
    if rc != 0:
        raise IpkGpuError(rc, L.ipkgpu_db_file_last_error().decode())
    return L, h


def file_info(path):
    """ipkgpu_db_file_open: every field of the file's head (host only, no walk over the records) -- the dict read_db returns."""
    L, h = _open(path)
    try:
        return info_of_handle(h)
    finally:
        L.ipkgpu_db_file_close(h)


def check_file(path):
    """ipkgpu_db_file_check: walks the records by their count fields; returns (records, entries) or raises IpkGpuError with the record
    index and byte offset where the file stops being one (truncated, a bad count, totals that differ from the header's)."""
    L, h = _open(path)
    try:
        nr, ne = C.c_uint64(0), C.c_uint64(0)
        rc = L.ipkgpu_db_file_check(h, C.byref(nr), C.byref(ne))
        if rc != 0:
            raise IpkGpuError(rc, L.ipkgpu_db_file_last_error().decode())
        return int(nr.value), int(ne.value)
    finally:
        L.ipkgpu_db_file_close(h)


def read_db(path, as_arrays=False, protocol=None):
    """Parses the layout of ipk_format.hpp.  Returns (header dict, records): records = list of (key, filter_value, branches,
    scores) in file order, or with as_arrays the arrays (keys, filter_values, counts, entry_offsets, branches, scores).
    protocol: the protocol version the file was written with (None: this process' -- IPKGPU_IPK_PROTOCOL_VERSION or the default)."""
    if protocol is None:
        protocol = protocol_version()
    raw = np.fromfile(path, dtype=np.uint8)
    buf = raw.tobytes()
    p = 0

    def take(fmt):
        nonlocal p
        v = struct.unpack_from("<" + fmt, buf, p)
        p += struct.calcsize("<" + fmt)
        return v[0] if len(v) == 1 else v

    def take_string():
        nonlocal p
        n = take("Q")
        s = buf[p:p + n].decode()
        p += n
        return s

    assert take_string() == "serialization::archive", "not a Boost binary archive preamble"
    lib_version = take("H")
    sizes = take("BBBB")
    assert sizes == (4, 8, 4, 8) and take("i") == 1
    proto = take("I") if protocol else 0
    assert proto == protocol, f"protocol word {proto}, expected {protocol}"
    st = take_string()
    positions = bool(take("B")) if protocol else False
    ni = take("Q")
    ti = np.frombuffer(buf, dtype=[("n", "<u8"), ("l", "<f8")], count=ni, offset=p)
    p += ni * 16
    newick = take_string()
    k = take("Q"); omega = take("f"); nk = take("Q"); ne = take("Q")
    hdr = dict(sequence_type=st, tree_index=[(int(a), float(b)) for a, b in ti], newick=newick, kmer_size=k, omega=omega,
               total_num_kmers=nk, total_num_entries=ne, library_version=lib_version, protocol_version=proto,
               positions_loaded=positions)
    if positions:
        # records of 16 + 10 n bytes: key, filter value, n, then n x (u32 branch, f32 score, u16 position)
        recs, q = [], p
        ent_t = np.dtype([("b", "<u4"), ("s", "<f4"), ("p", "<u2")])
        for _ in range(nk):
            key, fvb, cnt = struct.unpack_from("<IfQ", buf, q)
            e = np.frombuffer(buf, dtype=ent_t, count=cnt, offset=q + 16)
            recs.append((key, fvb, e["b"].copy(), e["s"].copy(), e["p"].astype(np.uint32)))
            q += 16 + 10 * cnt
        assert q == len(buf) and sum(len(r[2]) for r in recs) == ne, "body size does not match the header's totals"
        return hdr, recs
    body = np.frombuffer(buf[p:], dtype="<u4") if (len(buf) - p) % 4 == 0 else None
    assert body is not None and len(body) == 4 * nk + 2 * ne, "body size does not match the header's totals"
    # record starts: head of 4 words, then 2 words per entry -- walk the counts
    keys = np.empty(nk, np.uint32); fvs = np.empty(nk, np.float32); counts = np.empty(nk, np.uint64)
    starts = np.empty(nk, np.int64)
    q = 0
    for i in range(nk):
        starts[i] = q
        c = int(body[q + 2]) | (int(body[q + 3]) << 32)
        counts[i] = c
        q += 4 + 2 * c
    assert q == len(body)
    keys[:] = body[starts]; fvs[:] = body[starts + 1].view(np.float32)
    eoff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    mask = np.ones(len(body), bool)
    for d in range(4):
        mask[starts + d] = False
    ent = body[mask].reshape(-1, 2)
    br, sc = ent[:, 0].copy(), ent[:, 1].copy().view(np.float32)
    if as_arrays:
        return hdr, (keys, fvs, counts, eoff, br, sc)
    recs = [(int(keys[i]), float(fvs[i]), br[eoff[i]:eoff[i + 1]], sc[eoff[i]:eoff[i + 1]]) for i in range(nk)]
    return hdr, recs


# ---- several GPUs: every rank owns the k-mers with code % P == rank ---------------------------------
# Filter values are per k-mer, so each rank computes them on its own shard and writes the shard, in its own filter order, as a
# database file; the final file is the streaming merge of the P shard files by filter value (ipkgpu_db_merge_files) -- the
# role merge_stage2 plays for the reference's on-disk batches (db_builder.cpp:392-458).

def filter_sort_code(filter_values, keys):
    """The engine's filter order as one integer per k-mer: order-preserving code of the float32 filter value, ties by
    ascending key (ipk_amd/csrc/kernels_filter.hpp, filter_sortkey_kernel)."""
    u = np.asarray(filter_values, dtype=np.float32).view(np.uint32).astype(np.uint64)
    code = np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    return (code << np.uint64(32)) | np.asarray(keys, dtype=np.uint64)


def splitmix_unit(keys):
    """A reproducible value in [0, 1) per k-mer code (the `random` filter): independent of the sharding.  The host form of
    random_filter_kernel (ipk_amd/csrc/kernels_filter.hpp), which the builds use (Db.filter_random)."""
    x = np.asarray(keys, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(40)).astype(np.float64) / float(1 << 24)


def merge_shard_files(path, sequence_type, tree_index, newick, kmer_size, omega, shard_paths):
    """ipkgpu_db_merge_files: streaming P-way merge of the ranks' shard files (each a database file in its own filter order)
    by (filter value, key) -- merge_stage2's role (db_builder.cpp:392-458).  Returns (total k-mers, total entries).
    Positioned shards (write_db_positions / a positioned Db through write_db_device: the positions flag in their headers) give a
    positioned file; a mixture of positioned and plain shards is refused."""
    L = _lib()
    h = _header(sequence_type, tree_index, newick, kmer_size, omega)
    arr = (C.c_char_p * len(shard_paths))(*[str(p).encode() for p in shard_paths])
    nk, ne, nb = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = L.ipkgpu_db_merge_files(C.byref(h), arr, len(shard_paths), str(path).encode(), C.byref(nk), C.byref(ne), C.byref(nb))
    if rc != 0:
        raise IpkGpuError(rc, L.ipkgpu_db_merge_last_error().decode())
    return int(nk.value), int(ne.value)


def union_shard_files(engine, path, sequence_type, tree_index, newick, kmer_size, omega, shard_paths):
    """ipkgpu_db_union_files: merge_shard_files on the device -- every shard loaded, the databases united (ipkgpu_db_union), the union
    written by the streamed device writer.  The same file byte for byte for shards that are each in filter order, and the same return
    value (total k-mers, total entries).  All shards and the union are on the device together: IpkGpuError with code 3
    (IPKGPU_ERR_NOMEM) when they do not fit -- the caller decides whether merge_shard_files takes over."""
    L = _lib()
    if not getattr(L, "_union_files_bound", False):
        L.ipkgpu_db_union_files.restype = C.c_int
        L.ipkgpu_db_union_files.argtypes = [C.c_void_p, C.POINTER(_Header), C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p, C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L._union_files_bound = True
    h = _header(sequence_type, tree_index, newick, kmer_size, omega)
    arr = (C.c_char_p * max(len(shard_paths), 1))(*[os.fsencode(p) for p in shard_paths])
    nk, ne, nb = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = L.ipkgpu_db_union_files(engine._h, C.byref(h), arr, len(shard_paths), os.fsencode(path), C.byref(nk), C.byref(ne), C.byref(nb))
    if rc != 0:
        raise engine._err(rc)
    return int(nk.value), int(ne.value)


def join_shard_files(engine, output, sequence_type, tree_index, newick, k, omega, paths, filter_, n_nodes):
    """Database files whose k-mer sets may overlap (branch shards: builds over different branch groups of one tree) joined into one
    file: every shard loaded, the databases joined in the order given (Engine.join_dbs: `put`'s maximum per branch), the sources freed,
    the join filtered anew (filter_and_write_device's stage; n_nodes = MIF0's N of the WHOLE tree, the threshold score_threshold of
    the head's omega and k) and written by the streamed device writer.  Returns (k-mers, entries, entries dropped as duplicates).
    All shards and the join are on the device together: IpkGpuError with code 3 (IPKGPU_ERR_NOMEM) when they do not fit -- there
    is no host route for shared keys."""
    from .engine import score_threshold
    sigma = {"DNA": 4, "AA": 20}[sequence_type]
    srcs = []
    try:
        for p in paths:
            srcs.append(engine.load_db(os.fspath(p)))
        db = engine.join_dbs(srcs)
    finally:
        for d in srcs:
            d.free()
    try:
        dropped = int(engine.join_stats()["entries_dropped"])
        filter_and_write_device(engine, db, output, filter_, sequence_type, tree_index, newick, k, omega, n_nodes, score_threshold(omega, sigma, k))
        return db.num_keys, db.num_entries, dropped
    finally:
        db.free()


def join_shard_files_streamed(engine, output, sequence_type, tree_index, newick, k, omega, paths, filter_, n_nodes, tmp_dir=None):
    """join_shard_files for shards that do not fit device memory together (Engine.join_files, ipkgpu_db_join_files): the same file byte
    for byte and the same return value, joined by key ranges that each fit "device_budget_bytes" (or the device's free memory) -- no
    shard and no whole join is ever resident.  The range files live in tmp_dir (default: output + ".ranges") until the host merge has
    made `output` of them.  IpkGpuError with code 3 when one key bin alone does not fit."""
    from .engine import score_threshold
    sigma = {"DNA": 4, "AA": 20}[sequence_type]
    return engine.join_files(paths, output, sequence_type, tree_index, newick, k, omega, filter_, n_nodes, score_threshold(omega, sigma, k), tmp_dir=tmp_dir)
