"""Times what the positioned database pays for several ranks: the owner split of the scoring call and the merge of positioned sources.
Usage: python tools/positions_ranks_probe.py CONFIG GROUPS [--owners P] [--once]
  (a) score_groups_keymajor_positions_owners at n_owners = P against n_owners = 1, beside the same two calls of the plain
      score_groups_keymajor: the owner split should cost the positioned call what it costs the plain one
  (b) merge_parts_positions_ptrs against merge_parts_ptrs over the SAME P sources (the share cut into P ranges of groups, each scored
      with n_owners = P; owner 0 merges block 0 of every range): 12 bytes moved per entry against 8 over the same metadata, so a
      ratio of at most 1.5 is expected.  The two merges alternate in one process; the spread of the plain one is printed beside it.
Minimum of 5 timed calls after a warm-up each, from the calls' own device events (IPKGPU_T_TOTAL, ipkgpu_db_time_ms).
--once: one plain and one positioned merge only (for a kernel trace)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import ipk_amd
from ipk_amd import distributed as D
from ipk_amd import engine as E
from ipk_amd.synth import CONFIGS, synth_matrices


def device_matrices(cfg, n_groups):
    mpg = cfg["mats_per_group"]
    d = torch.empty((n_groups * mpg, cfg["sites"], cfg["sigma"]), dtype=torch.float32, device="cuda")
    step = 64
    for m0 in range(0, n_groups * mpg, step):
        m1 = min(n_groups * mpg, m0 + step)
        d[m0:m1].copy_(torch.from_numpy(synth_matrices(m1 - m0, cfg["sites"], cfg["sigma"], cfg["alpha"], cfg["seed"], first_mat=m0)))
    torch.cuda.synchronize()
    return d, np.repeat(np.arange(n_groups, dtype=np.uint32), mpg)


def best_of(call, reps=5):
    """-> (minimum IPKGPU_T_TOTAL over `reps` calls after a warm-up, entries)"""
    best, entries = 1e30, 0
    for i in range(reps + 1):
        r = call()
        if i:
            best = min(best, r.time_ms(E.T_TOTAL))
        entries = r.num_entries
        r.free()
    return best, entries


def main():
    name, n_groups = sys.argv[1], int(sys.argv[2])
    P = int(sys.argv[sys.argv.index("--owners") + 1]) if "--owners" in sys.argv else 8
    once = "--once" in sys.argv
    cfg = CONFIGS[name]
    k, sigma, mpg = cfg["k"], cfg["sigma"], cfg["mats_per_group"]
    eps = ipk_amd.log_threshold(cfg["omega"], sigma, k)
    logp, groups = device_matrices(cfg, n_groups)
    eng = ipk_amd.Engine(0)
    if not once:
        print(f"== {name}: {n_groups} groups x {mpg} x {cfg['sites']} sites, sigma {sigma}, k {k}")
        t = {}
        for label, call in (("plain", eng.score_groups_keymajor), ("positioned", eng.score_groups_keymajor_positions_owners)):
            for owners in (1, P):
                t[label, owners], n = best_of(lambda: call(logp, groups, k, eps, n_owners=owners))
            print(f"(a) {label} call: n_owners = 1 {t[label, 1]:.2f} ms, n_owners = {P} {t[label, P]:.2f} ms, "
                  f"{P} owners / 1 owner = {t[label, P] / t[label, 1]:.3f} ({n} entries)")
    # (b) the share as P ranks' pieces, each split for P owners; owner 0's sources
    srcs = []
    for r in range(P):
        g0, g1 = D.shard_range(n_groups, P, r)
        srcs.append(eng.score_groups_keymajor_positions_owners(logp[g0 * mpg:g1 * mpg], groups[g0 * mpg:g1 * mpg], k, eps, n_owners=P))
    cps = [p.counts_ptr() for p in srcs]                                      # block 0: the parts' first counts row, entries from 0
    eps_ = [p.entries_ptr() for p in srcs]
    pps = [p.positions_ptr() for p in srcs]
    plain, pos = [], []
    for i in range(2 if once else 6):
        a = eng.merge_parts_ptrs(sigma, k, 0, P, cps, eps_)
        b = eng.merge_parts_positions_ptrs(sigma, k, 0, P, cps, eps_, pps)
        if i:
            plain.append(a.time_ms()); pos.append(b.time_ms())
        n = a.num_entries
        assert b.num_entries == n
        a.free(); b.free()
    if not once:
        spread = (max(plain) - min(plain)) / min(plain)
        print(f"(b) merge of {P} sources, owner 0, {n} entries: plain {min(plain):.3f} ms (5 repeats: {min(plain):.3f} .. {max(plain):.3f}, "
              f"spread {100 * spread:.1f} %), positioned {min(pos):.3f} ms ({min(pos):.3f} .. {max(pos):.3f})")
        print(f"    positioned / plain = {min(pos) / min(plain):.3f} (12 bytes per entry against 8: at most 1.5 expected, "
              f"{1.5 * (1 + spread):.3f} with the plain merge's spread)")
    for p in srcs:
        p.free()
    eng.close()


if __name__ == "__main__":
    main()
