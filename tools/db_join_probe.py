"""Measurements of the join of databases that share k-mers (ipkgpu_db_join) on one MI355X, everything in device memory.  No test
runs this.

  python tools/db_join_probe.py [--out profiles/db_join_probe.txt] [--groups 125]

(a) The 125-group share of cfg2 (the database of tools/db_union_probe.py) built as 2, 4 and 8 BRANCH SHARDS -- contiguous ranges of
    the group order, each scored on its own -- then joined and filtered with MIF0: the join's timers, the filter, and whether keys,
    entries and filter values equal the one-call build's bit for bit.  The shards' branches are disjoint, so "join_route" = 0 only
    concatenates; the same input with "join_route" = 1 shows what the duplicate stage costs when it finds nothing.
(b) The same database as 8 KEY-DISJOINT shards (owners by key % 8, as 8 ranks leave them): ipkgpu_db_union beside the join's
    concatenation route on the same sources.  The union is the yardstick for "the concatenation route costs no more than the union plus
    the count sum": the union also copies filter values and sorts the order, the join also scans the head flags and fills the branch table."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ipk_amd                                                           # noqa: E402
from ipk_amd import distributed as D                                     # noqa: E402
from tools.ondisk_probe import share                                     # noqa: E402

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def same(a, b, fv=True):
    ok = a.num_keys == b.num_keys and a.num_entries == b.num_entries and np.array_equal(a.keys(), b.keys()) and np.array_equal(a.key_offsets(), b.key_offsets())
    ok = ok and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a.entries(), b.entries()))
    if fv:
        ok = ok and np.array_equal(a.filter_values().view(np.uint32), b.filter_values().view(np.uint32)) and np.array_equal(a.filter_order(), b.filter_order())
    return bool(ok)


def stats_text(st):
    return (f"join on the device {st['total_ms']:.3f} ms: key stage {st['key_ms']:.3f}, entry copy {st['entry_copy_ms']:.3f}, duplicate stage "
            f"{st['duplicate_ms']:.3f}; {int(st['shared_keys'])} shared k-mers, {int(st['entries_dropped'])} dropped, route {int(st['route'])}")


def run(n_groups):
    import torch
    cfg, mats, groups = share("cfg2", n_groups)
    k, sigma, omega = cfg["k"], cfg["sigma"], cfg["omega"]
    eps, thr = ipk_amd.log_threshold(omega, sigma, k), ipk_amd.score_threshold(omega, sigma, k)
    n_nodes = 2 * n_groups
    eng = ipk_amd.Engine(0)
    dev = torch.from_numpy(mats).cuda()
    whole, parts = D.build_db_shard(eng, dev, groups, k, eps, sigma)
    parts.free()
    whole.filter_mif0(eng, n_nodes, thr)
    say(f"cfg2 share: {n_groups} groups, k={k}, sites={cfg['sites']}: {whole.num_keys} k-mers, {whole.num_entries} entries; MIF0 over the one-call build "
        f"{whole.filter_time_ms():.3f} ms on the device")
    say("(a) branch shards: contiguous group ranges, each scored on its own, joined in range order, MIF0 over the join")
    order = list(dict.fromkeys(groups.tolist()))
    for ways in (2, 4, 8):
        shards = []
        for w in range(ways):
            lo, hi = D.shard_range(len(order), ways, w)
            sel = np.isin(groups, order[lo:hi])
            db, p = D.build_db_shard(eng, dev[torch.from_numpy(sel)], groups[sel], k, eps, sigma)
            p.free()
            shards.append(db)
        keys_in, ent_in = sum(d.num_keys for d in shards), sum(d.num_entries for d in shards)
        for route in (0, 1, 0, 1):
            eng.set_option("join_route", route)
            t0 = time.time()
            j = eng.join_dbs(shards)
            t1 = time.time()
            st = eng.join_stats()
            j.filter_mif0(eng, n_nodes, thr)
            t2 = time.time()
            say(f"    {ways} shards ({keys_in} k-mers, {ent_in} entries in all), join_route {route}: join {t1 - t0:.4f} s wall, filter {t2 - t1:.4f} s wall ({j.filter_time_ms():.3f} ms on the device); "
                f"{stats_text(st)}; equals the one-call build {same(j, whole)}; join_bytes {eng.join_bytes(keys_in, ent_in, ways, False)}")
            j.free()
        eng.set_option("join_route", 0)
        for d in shards:
            d.free()
    say("(b) 8 key-disjoint shards (owners by key % 8) of the same database: ipkgpu_db_union beside the join's concatenation route")
    owners = 8
    parts = eng.score_groups_keymajor(dev, groups, k, eps, n_owners=owners)
    srcs = []
    for o in range(owners):
        a, b = int(parts.owner_offsets[o]), int(parts.owner_offsets[o + 1])
        db = eng.merge_parts(sigma, k, o, owners, parts.counts_tensor()[o:o + 1].contiguous(), parts.entries_tensor()[a:b].contiguous(), np.zeros(1, np.uint64))
        db.filter_mif0(eng, n_nodes, thr)
        srcs.append(db)
    parts.free()
    for rep in range(3):
        t0 = time.time()
        u = eng.union_dbs(srcs)
        t1 = time.time()
        ut = eng.union_times()
        j = eng.join_dbs(srcs)
        t2 = time.time()
        st = eng.join_stats()
        say(f"    run {rep + 1}: union {t1 - t0:.4f} s wall, on the device {ut['total_ms']:.3f} ms: key sort {ut['key_sort_ms']:.3f}, entry copy {ut['entry_copy_ms']:.3f}, "
            f"order sort {ut['order_sort_ms']:.3f}")
        say(f"           join  {t2 - t1:.4f} s wall, {stats_text(st)}; keys, offsets and entries equal the union's {same(j, u, fv=False)} and the one-call build's {same(j, whole, fv=False)}")
        u.free(); j.free()
    for d in srcs:
        d.free()
    whole.free()
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--groups", type=int, default=125)
    a = ap.parse_args()
    run(a.groups)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
