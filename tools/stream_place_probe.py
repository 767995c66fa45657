"""Measurements of placing reads on a database FILE without holding it on the device (Engine.kmer_set + Engine.load_db(path, wanted=) +
Engine.place, the steps of Engine.place_file) against Engine.load_db + Engine.place, on the file of tools/db_load_probe.py: the
125-group share of the benchmark config cfg2 written as a database file of about 0.96 GB, and 10^5 random reads of 150 symbols.

  python tools/stream_place_probe.py [--out profiles/stream_place_probe.txt]

Written, per number of reads and per window size ("db_load_window_bytes"): the seconds of the k-mer set, of the streamed load -- split
into file read, host walk, waiting for the device and the host's time in the windows' device work -- and of the placement; the
windows, the records kept and the device memory's high-water mark; and whether the placements equal those on the loaded file.  No
gate: what is seen is recorded."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ipk_amd                                                           # noqa: E402
from tools.ondisk_probe import in_memory, share                          # noqa: E402

WINDOWS = [0, 64 << 20]                                                  # the default (256 MiB) and a quarter of it
READS = [100000, 1000]
READ_LENGTH = 150


def same(a, b):
    return all(np.array_equal(getattr(a, n), getattr(b, n)) for n in ("branches", "counts", "n_kmers", "n_found", "n_branches")) and \
        np.array_equal(a.scores.view(np.uint32), b.scores.view(np.uint32))


def probe(out_path, n_groups):
    tmp = tempfile.mkdtemp(prefix="stream_place_probe_", dir=os.environ.get("IPK_PROBE_DIR"))
    cfg, mats, groups = share("cfg2", n_groups)
    eng = ipk_amd.Engine(0)
    path = os.path.join(tmp, "cfg2.ipk")
    m = in_memory(eng, cfg, mats, groups, path)
    del mats
    eng.set_option("release_workspaces", 1)
    size = os.path.getsize(path)
    sigma, k = cfg["sigma"], cfg["k"]
    lines = [f"cfg2 share: {n_groups} groups, sigma={sigma} k={k}: {m['keys']} k-mers, {m['entries']} entries, file {size} bytes"]
    rng = np.random.default_rng(150)
    all_reads = ["".join(r) for r in rng.choice(list("ACGT"), (max(READS), READ_LENGTH))]
    for n_reads in READS:
        reads = all_reads[:n_reads]
        lines.append(f"-- {n_reads} reads of {READ_LENGTH}")
        want = None
        for rep in range(2):                                             # (the first run allocates the pinned buffers and the workspaces)
            eng.mem_stats(reset_peak=True)
            t0 = time.time()
            db = eng.load_db(path)
            t1 = time.time()
            t = eng.load_times()
            want = eng.place(db, reads)
            t2 = time.time()
            peak = eng.mem_stats()[1]
            db.free()
            eng.set_option("release_workspaces", 1)
            lines.append(f"load_db + place (run {rep + 1}): {t2 - t0:.3f} s = load {t1 - t0:.3f} s (file read {t['read_s']:.3f}, host walk {t['walk_s']:.3f}, "
                         f"waiting for the device {t['device_wait_s']:.3f}) + place {t2 - t1:.3f} s (kernels {want.time_ms['place']:.1f} ms, index "
                         f"{want.time_ms['index']:.1f} ms); device memory peak {peak / 2 ** 20:.0f} MiB")
        for window in WINDOWS:
            eng.set_option("db_load_window_bytes", window)
            for rep in range(2):
                eng.mem_stats(reset_peak=True)
                t0 = time.time()
                kset = eng.kmer_set(reads, sigma, k)
                t1 = time.time()
                db = eng.load_db(path, wanted=kset)
                t2 = time.time()
                t = eng.load_times()
                got = eng.place(db, reads)
                t3 = time.time()
                peak = eng.mem_stats()[1]
                lines.append(f"window {'default' if window == 0 else window >> 20} MiB, kmer_set + load_db(wanted=) + place (run {rep + 1}): {t3 - t0:.3f} s = set "
                             f"{t1 - t0:.3f} s ({kset.count} codes) + load {t2 - t1:.3f} s (file read {t['read_s']:.3f}, host walk {t['walk_s']:.3f}, waiting for "
                             f"the pinned buffers {t['device_wait_s']:.3f}, the windows' device work and the final sort and gather, waited for, "
                             f"{t['device_ms'] / 1e3:.3f}; {int(t['windows'])} windows, {int(t['records_kept'])} of {m['keys']} records kept, {db.num_entries} entries) "
                             f"+ place {t3 - t2:.3f} s (kernels {got.time_ms['place']:.1f} ms); device memory peak {peak / 2 ** 20:.0f} MiB; "
                             f"placements {'equal' if same(got, want) else 'DIFFER from'} those on the loaded file")
                db.free()
                kset.free()
                eng.set_option("release_workspaces", 1)
        eng.set_option("db_load_window_bytes", 0)
    eng.close()
    shutil.rmtree(tmp, ignore_errors=True)
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
    a = ap.parse_args()
    probe(a.out, a.groups)
