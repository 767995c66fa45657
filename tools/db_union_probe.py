"""Measurements of the union of databases on the device (ipkgpu_db_union) on one MI355X, files in the page cache (each is written
moments before it is read).  No test runs this.

  python tools/db_union_probe.py [--out profiles/db_union_probe.txt] [--parent DIR] [--only a,b,c]

(a) The 125-group share of cfg2 (the 961.7-MB file of tools/db_load_probe.py) as 8 owner shards by key % 8 -- scored with
    n_owners = 8, every owner's database filtered and written, as 8 ranks would: the host merge of the 8 files in seconds beside
    eight loads + union + write; the union's timers and the entry copy in GB/s (16 bytes moved per entry: 8 read, 8 written), and
    beside it db_unpack_entries_kernel over the same entries in the same run (the load of the whole file) -- the existing kernel that
    moves the same bytes; and the copy's 8-byte form (option "union_copy_bytes" = 8) against its 16-byte form, the default, by turns.
(b) tools/keyrange_probe.py's k = 14 shape (16 groups x 2 matrices x 10 000 sites) in 4 passes, the default route against
    union_on_device, end to end.
(c) with --parent DIR (a built checkout of the parent commit): `python bench.py --gpus 1` there and here, alternated three times each.
    The default path runs no new code; the figures show it."""
import argparse
import filecmp
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ipk_amd                                                           # noqa: E402
from ipk_amd import dbfile, keyrange                                     # noqa: E402
from ipk_amd.synth import synth_matrices                                 # noqa: E402
from tools.ondisk_probe import in_memory, share                          # noqa: E402

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def owner_shards(n_groups, owners=8):
    import torch
    tmp = tempfile.mkdtemp(prefix="db_union_probe_", dir=os.environ.get("IPK_PROBE_DIR"))
    cfg, mats, groups = share("cfg2", n_groups)
    k, sigma, omega = cfg["k"], cfg["sigma"], cfg["omega"]
    eng = ipk_amd.Engine(0)
    whole = os.path.join(tmp, "whole.ipk")
    m = in_memory(eng, cfg, mats, groups, whole)
    say(f"(a) cfg2 share: {n_groups} groups, k={k}, sites={cfg['sites']}: {m['keys']} k-mers, {m['entries']} entries, one file {m['file_bytes']} bytes "
        f"(built in memory: score {m['score_s']:.3f} s, filter {m['filter_s']:.3f} s, file {m['file_s']:.3f} s)")
    eps = ipk_amd.log_threshold(omega, sigma, k)
    thr = ipk_amd.score_threshold(omega, sigma, k)
    dev = torch.from_numpy(mats).cuda()
    parts = eng.score_groups_keymajor(dev, groups, k, eps, n_owners=owners)
    paths = []
    for o in range(owners):
        a, b = int(parts.owner_offsets[o]), int(parts.owner_offsets[o + 1])
        db = eng.merge_parts(sigma, k, o, owners, parts.counts_tensor()[o:o + 1].contiguous(), parts.entries_tensor()[a:b].contiguous(), np.zeros(1, np.uint64))
        db.filter_mif0(eng, 2 * n_groups, thr)
        paths.append(os.path.join(tmp, f"shard{o}.ipk"))
        dbfile.write_db_device(eng, db, paths[-1], "DNA", [], "", k, omega)
        db.free()
    parts.free()
    del dev
    head = ("DNA", [], "", k, omega)
    for rep in range(2):
        t0 = time.time()
        totals = dbfile.merge_shard_files(os.path.join(tmp, "host.ipk"), *head, paths)
        t_host = time.time() - t0
        t0 = time.time()
        dbfile.union_shard_files(eng, os.path.join(tmp, "device.ipk"), *head, paths)
        t_dev = time.time() - t0
        say(f"    run {rep + 1}: host merge of the {owners} shard files {t_host:.3f} s; {owners} loads + union + write (ipkgpu_db_union_files) {t_dev:.3f} s; "
            f"{totals[0]} k-mers, {totals[1]} entries")
    same = filecmp.cmp(os.path.join(tmp, "host.ipk"), whole, shallow=False), filecmp.cmp(os.path.join(tmp, "device.ipk"), whole, shallow=False)
    say(f"    host-merged file equals the one-owner file: {same[0]}; device-united file equals it: {same[1]}")
    # the same steps apart, the copy kernel in its 8-byte and its 16-byte form by turns
    for rep, form in enumerate((8, 16, 8, 16)):
        eng.set_option("union_copy_bytes", form)
        t0 = time.time()
        srcs, walk = [], 0.0
        for p in paths:
            srcs.append(eng.load_db(p))
            walk += eng.load_times()["walk_s"]
        t1 = time.time()
        u = eng.union_dbs(srcs)
        t2 = time.time()
        ut = eng.union_times()
        for d in srcs:
            d.free()
        dbfile.write_db_device(eng, u, os.path.join(tmp, "device.ipk"), *head)
        t3 = time.time()
        ne, n = u.num_entries, u.num_keys
        u.free()
        ok = filecmp.cmp(os.path.join(tmp, "device.ipk"), whole, shallow=False)
        say(f"    apart, run {rep + 1}, {form}-byte copy: {owners} loads {t1 - t0:.3f} s (host walk {walk:.3f} s), union {t2 - t1:.4f} s wall, write {t3 - t2:.3f} s, file equal "
            f"{ok}; union on the device {ut['total_ms']:.3f} ms: key sort {ut['key_sort_ms']:.3f}, entry copy {ut['entry_copy_ms']:.3f} = "
            f"{16 * ne / ut['entry_copy_ms'] / 1e6:.0f} GB/s of {16 * ne} bytes, order sort {ut['order_sort_ms']:.3f}; union_bytes {eng.union_bytes(n, ne, owners, False)}")
        d = eng.load_db(whole)
        lt = eng.load_times()
        d.free()
        say(f"        db_unpack_entries_kernel over the same {ne} entries (load of the one file): {lt['entries_ms']:.3f} ms = {16 * ne / lt['entries_ms'] / 1e6:.0f} GB/s; "
            f"that load {lt['total_s']:.3f} s, host walk {lt['walk_s']:.3f} s")
    eng.set_option("union_copy_bytes", 0)
    eng.close()
    shutil.rmtree(tmp, ignore_errors=True)


def key_passes(groups=16, sites=10000, k=14, n=4):
    import torch
    mats = synth_matrices(2 * groups, sites, 4, 0.05, 42)
    mg = np.repeat(np.arange(groups, dtype=np.uint32), 2)
    dev = torch.from_numpy(mats).cuda()
    eng = ipk_amd.Engine(0)
    work = tempfile.mkdtemp(prefix="db_union_probe_kr_", dir=os.environ.get("IPK_PROBE_DIR"))
    eps = ipk_amd.log_threshold(1.5, 4, k)
    say(f"(b) key-range build: {groups} groups x 2 matrices x {sites} sites, k = {k} in {n} passes, mif0, end to end (second of two runs each)")
    for on_device in (False, True, False, True):
        out = os.path.join(work, f"db{int(on_device)}.ipk")
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = keyrange.build_db_file(eng, dev, mg, k, eps, 4, out, work, "DNA", [(1, 0.0)] * (groups + 1), "a;", 1.5, "mif0", groups + 1, passes=n,
                                   union_on_device=on_device)
        wall = time.perf_counter() - t0
        say(f"    union_on_device={on_device}: route {r['route']}: {wall:.3f} s wall; scoring calls {r['score_s']:.3f} s, filter {r['filter_s']:.3f} s, files written "
            f"{r['write_s']:.3f} s, host merge {r['merge_s']:.3f} s, union + one write {r['union_s']:.3f} s; {r['totals'][0]} k-mers, {r['totals'][1]} entries, "
            f"file {os.path.getsize(out)} bytes")
    say(f"    the two routes' files are equal: {filecmp.cmp(os.path.join(work, 'db0.ipk'), os.path.join(work, 'db1.ipk'), shallow=False)}")
    eng.close()
    shutil.rmtree(work, ignore_errors=True)


def bench_pairs(parent):
    say(f"(c) python bench.py --gpus 1, parent and branch alternated three times each")
    for rep in range(3):
        for name, d in (("parent", parent), ("branch", ROOT)):
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1"], cwd=d, capture_output=True, text=True, timeout=600)
            res = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not res:
                say(f"    {name} run {rep + 1}: failed ({p.returncode}): {p.stderr[-300:]}")
                return
            j = json.loads(res[-1])
            say(f"    {name} run {rep + 1}: " + ", ".join(f"{key} {j[key]}" for key in ("value", "unit", "ms_per_step") if key in j))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--groups", type=int, default=125)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for (c)")
    ap.add_argument("--only", default="a,b,c")
    a = ap.parse_args()
    only = a.only.split(",")
    if "a" in only:
        owner_shards(a.groups)
    if "b" in only:
        key_passes()
    if "c" in only and a.parent:
        bench_pairs(a.parent)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if os.path.exists(a.out) and a.only != "a,b,c" else "w") as fh:
            fh.write("\n".join(lines) + "\n")
