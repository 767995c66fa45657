"""Measurements of Engine.place on one GPU, on the database of tools/db_load_probe.py: the 125-group share of the benchmark config
cfg2, built in memory (or a file of it, loaded).

  python tools/place_probe.py [--db FILE.ipk] [--reads 100000 1000000] [--out profiles/place_probe.txt] [--expand-ambiguous] [--strands both]

Synthetic reads of 150 symbols: half cut from the most probable sequence of a group's first matrix, half uniformly random.  Written:
the index build of the database's first call, and per read count the minimum over five calls after a warm-up of the call's wall time
and of the placement kernels' time, as reads per second and looked-up (valid) windows per second.  Beside them, as the comparison
figure, the time the tests' host oracle (tests/place_oracle.py, one core) takes for the first 1000 of the reads -- whose placements
the device's are checked against on the way.
--expand-ambiguous: one symbol of every fourth read becomes N and the reads are placed with ambiguity=True; --strands both: every third
read is reverse-complemented and the reads are placed on both strands (the oracle is then tests/place_ext_oracle.py)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ipk_amd                                                           # noqa: E402
from ipk_amd import distributed as D                                     # noqa: E402
from tests import place_ext_oracle as xo                                 # noqa: E402
from tests import place_oracle as po                                     # noqa: E402
from tools.ondisk_probe import share                                     # noqa: E402

READ = 150


def make_reads(mats, mpg, n, seed, ambiguity=False, strands="given"):
    """uint8 [n, READ]: even reads cut from a group's most probable sequence, odd reads random; ambiguity: an N at a random place of
    every fourth read; strands "both": every third read reverse-complemented."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    best = letters[mats[::mpg].argmax(axis=2)]                           # [groups, sites]
    g = rng.integers(0, best.shape[0], n)
    s = rng.integers(0, best.shape[1] - READ + 1, n)
    reads = best[g[:, None], s[:, None] + np.arange(READ)[None, :]]
    odd = np.arange(n) % 2 == 1
    reads[odd] = letters[rng.integers(0, 4, (int(odd.sum()), READ))]
    if strands == "both":
        comp = np.zeros(256, np.uint8)
        comp[letters] = letters[::-1]
        reads[::3] = comp[reads[::3, ::-1]]
    if ambiguity:
        rows = np.arange(0, n, 4)
        reads[rows, rng.integers(0, READ, len(rows))] = ord("N")
    return np.ascontiguousarray(reads)


def probe(out_path, n_groups, db_file, read_counts, ambiguity=False, strands="given"):
    import torch
    cfg, mats, groups = share("cfg2", n_groups)
    k, sigma = cfg["k"], cfg["sigma"]
    eps = ipk_amd.log_threshold(cfg["omega"], sigma, k)
    eng = ipk_amd.Engine(0)
    parts = None
    if db_file:
        db = eng.load_db(db_file)
    else:
        db, parts = D.build_db_shard(eng, torch.from_numpy(mats).cuda(), groups, k, eps, sigma)
    lines = [f"cfg2 share: {n_groups} groups, sigma={sigma} k={k} sites={cfg['sites']}: {db.num_keys} k-mers, {db.num_entries} entries"
             + (f" (loaded from {os.path.basename(db_file)})" if db_file else " (built in memory)") + f"; reads of {READ} symbols, keep_at_most 7"
             + ("; an N in every fourth read, expanded" if ambiguity else "") + ("; every third read reverse-complemented, both strands placed" if strands == "both" else "")]
    first = True
    check = None
    for n in read_counts:
        reads = make_reads(mats, cfg["mats_per_group"], n, 1000 + n, ambiguity, strands)
        off = np.arange(n + 1, dtype=np.uint64) * READ
        walls, kernels = [], []
        for rep in range(6):                                             # one warm-up, five timed
            t0 = time.time()
            res = eng.place_packed(db, reads.reshape(-1), off, keep_at_most=7, sigma=sigma, k=k, log_eps=eps, ambiguity=ambiguity, strands=strands)
            wall = time.time() - t0
            if first:
                lines.append(f"first call on the database: index build (prefix table, branch count, duplicate check) {res.time_ms['index']:.3f} ms; "
                             f"{int(res.n_branches.max())} branches at most per read")
                first = False
            if rep:
                walls.append(wall); kernels.append(res.time_ms["place"] / 1e3)
        windows = int(res.n_kmers.sum())
        lines.append(f"{n} reads ({windows} valid windows, {int(res.n_ambiguous.sum())} of them expanded, {int(res.n_found.sum())} of them keys, "
                     f"{int(res.strand.sum())} reads placed on the reverse strand; {int((res.branches[:, 0] != 0xFFFFFFFF).sum())} reads placed): "
                     f"call {min(walls):.4f} s = {n / min(walls) / 1e6:.3f} M reads/s, {windows / min(walls) / 1e6:.1f} M windows/s; placement kernels "
                     f"{min(kernels) * 1e3:.3f} ms = {n / min(kernels) / 1e6:.3f} M reads/s, {windows / min(kernels) / 1e6:.1f} M windows/s "
                     f"(minimum of 5 calls after a warm-up)")
        if check is None:
            check = (reads[:1000], res)
    # the comparison figure: the host oracle on 1000 of the reads, one core
    br, sc = db.entries()
    view = po.DbView(db.keys(), db.key_offsets(), br, sc)
    seqs = [bytes(r) for r in check[0]]
    t0 = time.time()
    ext = ambiguity or strands == "both"
    want = xo.place(view, seqs, sigma, k, eps, 7, ambiguity, strands) if ext else po.place(view, seqs, sigma, k, eps, 7)
    t = time.time() - t0
    sub = eng.place_packed(db, check[0].reshape(-1), np.arange(len(seqs) + 1, dtype=np.uint64) * READ, keep_at_most=7, sigma=sigma, k=k, log_eps=eps,
                           ambiguity=ambiguity, strands=strands)
    (xo.check if ext else po.check)(sub, want)
    lines.append(f"host oracle (tests/place{'_ext' if ext else ''}_oracle.py, one core), {len(seqs)} of the reads: {t:.3f} s = {len(seqs) / t:.0f} reads/s; the device's placements of them "
                 f"equal the oracle's (branches, score bits, counts; lwr within tolerance)")
    db.free()
    if parts is not None:
        parts.free()
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--groups", type=int, default=125)
    ap.add_argument("--db", default=None, help="a database file of the same share (tools/db_load_probe.py writes one) instead of building it")
    ap.add_argument("--reads", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--expand-ambiguous", action="store_true", help="an N in every fourth read; placed with ambiguity=True")
    ap.add_argument("--strands", choices=["given", "both"], default="given", help="both: every third read reverse-complemented; both strands placed")
    a = ap.parse_args()
    probe(a.out, a.groups, a.db, a.reads, a.expand_ambiguous, a.strands)
