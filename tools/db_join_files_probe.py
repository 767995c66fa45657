"""Measurements of the join of branch shards by key ranges (ipkgpu_db_join_files) on one MI355X.  No test runs this.

  python tools/db_join_files_probe.py [--out profiles/db_join_files_probe.txt] [--groups 125] [--dir DIR]

The 125-group share of cfg2 (the input of tools/db_join_probe.py) built as 4 BRANCH SHARDS -- contiguous ranges of the group order, each
scored on its own and written as a file.  The yardstick is the in-memory route on those files, dbfile.join_shard_files (what
`merge --shared-keys` runs): every shard loaded, joined, filtered with MIF0, written.  Against it the streamed route,
dbfile.join_shard_files_streamed: with room for one range (no budget), and under budgets meant to plan 2 and 4 ranges (a little more
than a half and than a quarter of what the formula gives for the whole set).  Per run: wall seconds, passes over a body, the host walk's
share, the final host merge, the device peak against the budget, and whether the file equals the yardstick's."""
import argparse
import hashlib
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ipk_amd                                                           # noqa: E402
from ipk_amd import dbfile                                               # noqa: E402
from ipk_amd import distributed as D                                     # noqa: E402
from ipk_amd import engine as E                                          # noqa: E402
from tools.ondisk_probe import share                                     # noqa: E402

lines = []
WAYS = 4


def say(s):
    print(s, flush=True)
    lines.append(s)


def digest(path):
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for block in iter(lambda: fh.read(1 << 24), b""):
            h.update(block)
    return h.hexdigest()


def whole_need(infos):
    """The formula's figure for one range of everything, from the heads, at the largest window."""
    fixed, longest_joined = 0, 16
    for i in infos:
        body = i["file_bytes"] - i["body_offset"]
        window = max(min(256 << 20, body), 16)
        longest = min(body, 16 + 8 * i["total_num_entries"])
        fixed = max(fixed, E.stream_window_bytes(window, min(i["total_num_kmers"], max(window // 16, 1)), longest))
        longest_joined += max(longest - 16, 0)
    return E.join_files_range_bytes(fixed, [i["total_num_kmers"] for i in infos], [i["total_num_entries"] for i in infos], False, 256 << 20, longest_joined)


def run(n_groups, directory):
    import torch
    cfg, mats, groups = share("cfg2", n_groups)
    k, sigma, omega = cfg["k"], cfg["sigma"], cfg["omega"]
    eps, thr = ipk_amd.log_threshold(omega, sigma, k), ipk_amd.score_threshold(omega, sigma, k)
    n_nodes = 2 * n_groups
    head = ("DNA", [], "", k, omega)
    eng = ipk_amd.Engine(0)
    dev = torch.from_numpy(mats).cuda()
    order = list(dict.fromkeys(groups.tolist()))
    paths = []
    for w in range(WAYS):
        lo, hi = D.shard_range(len(order), WAYS, w)
        sel = np.isin(groups, order[lo:hi])
        db, p = D.build_db_shard(eng, dev[torch.from_numpy(sel)], groups[sel], k, eps, sigma)
        p.free()
        paths.append(os.path.join(directory, f"shard{w}.ipk"))
        dbfile.filter_and_write_device(eng, db, paths[-1], "random", *head, n_nodes, thr)
        db.free()
    del dev
    torch.cuda.empty_cache()
    infos = [dbfile.file_info(p) for p in paths]
    bodies = sum(i["file_bytes"] - i["body_offset"] for i in infos)
    say(f"cfg2 share: {n_groups} groups, k={k}, as {WAYS} branch shards: {sum(i['total_num_kmers'] for i in infos)} k-mers and {sum(i['total_num_entries'] for i in infos)} "
        f"entries in all, {bodies} body bytes")
    eng.set_option("release_workspaces", 1)
    out = os.path.join(directory, "whole.ipk")
    held = eng.mem_stats(reset_peak=True)[0]
    t0 = time.time()
    nk, ne, dropped = dbfile.join_shard_files(eng, out, *head, paths, "mif0", n_nodes)
    wall = time.time() - t0
    want = digest(out)
    say(f"in memory (join_shard_files): {wall:.3f} s wall; {nk} k-mers, {ne} entries, {dropped} dropped; device peak {eng.mem_stats()[1] - held} bytes; "
        f"{os.path.getsize(out)} bytes written")
    need = whole_need(infos)
    say(f"the formula for one range of everything, from the heads: {need} bytes")
    for label, avail in (("room for one range (no budget)", None), ("budget 0.55 x that", int(0.55 * need)), ("budget 0.29 x that", int(0.29 * need))):
        eng.set_option("release_workspaces", 1)
        held = eng.mem_stats(reset_peak=True)[0]
        eng.set_option("device_budget_bytes", 0 if avail is None else held + avail)
        out = os.path.join(directory, "streamed.ipk")
        t0 = time.time()
        try:
            ret = dbfile.join_shard_files_streamed(eng, out, *head, paths, "mif0", n_nodes)
        finally:
            eng.set_option("device_budget_bytes", 0)
        wall = time.time() - t0
        st, ranges = eng.join_files_stats(), eng.join_files_ranges()
        say(f"streamed, {label}: {wall:.3f} s wall, {len(ranges)} ranges, {st['passes']} passes over a body ({st['body_bytes_read']} bytes read); histogram passes "
            f"{st['hist_s']:.3f} s, range loads {st['loads_s']:.3f} s, host walk {st['walk_s']:.3f} s ({100 * st['walk_s'] / st['total_s']:.0f} % of the call), joins "
            f"{st['join_ms']:.1f} ms on the device, filter and range writes {st['write_s']:.3f} s, final host merge {st['merge_s']:.3f} s; window {st['window_bytes']}; "
            f"device peak {eng.mem_stats()[1] - held} (ranges {st['range_peak_bytes']}) of {'no budget' if avail is None else avail}; returned {ret}; "
            f"equals the in-memory file {digest(out) == want}")
        os.remove(out)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--groups", type=int, default=125)
    ap.add_argument("--dir", default=None, help="where the shard files and the outputs go [a temporary directory]")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        run(a.groups, d)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
