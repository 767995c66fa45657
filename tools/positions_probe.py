"""Times the positioned key-major call against the plain step and against the earlier route to a positioned database.
Usage: python tools/positions_probe.py CONFIG GROUPS [--join-groups N] [--once]
  (a) score_groups_keymajor                      -- the plain step, the lower bound
  (b) score_groups_keymajor_positions            -- one scoring pass, positions riding along; per-kernel times (IPKGPU_T_*)
  (c) the earlier route: (a) + score_groups_positions (tiles kernel, a global 64-bit atomicMax per scored phylo-k-mer, dense
      8-byte tables) on the device, plus the host join of its per-branch result with the database, timed at --join-groups groups
Minimum of 5 timed calls after a warm-up each; device memory taken = drop of hipMemGetInfo's free bytes over the calls of a leg
(a fresh context per leg, so the workspaces a leg keeps are its own).  --once: one positioned call only (for a kernel trace)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import ipk_amd
from ipk_amd import engine as E
from ipk_amd.synth import CONFIGS, synth_matrices

NAMES = {E.T_TOTAL: "total", E.T_PREFIX: "prefix", E.T_XP_COUNT: "xp count", E.T_XP_WRITE: "xp write", E.T_SCORE_MAIN: "score main",
         E.T_SCORE_REDUCE: "reduce", E.T_KM_WRITE: "key-major writer", E.T_COMPACT: "count+scan+writer"}


def device_matrices(cfg, n_groups):
    mpg = cfg["mats_per_group"]
    d = torch.empty((n_groups * mpg, cfg["sites"], cfg["sigma"]), dtype=torch.float32, device="cuda")
    step = 64
    for m0 in range(0, n_groups * mpg, step):
        m1 = min(n_groups * mpg, m0 + step)
        d[m0:m1].copy_(torch.from_numpy(synth_matrices(m1 - m0, cfg["sites"], cfg["sigma"], cfg["alpha"], cfg["seed"], first_mat=m0)))
    torch.cuda.synchronize()
    return d, np.repeat(np.arange(n_groups, dtype=np.uint32), mpg)


def leg(call, reps=5):
    """-> (per-field minimum over `reps` calls after a warm-up, device bytes taken, entries)"""
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    eng = ipk_amd.Engine(0)
    best, low, entries = {}, free0, 0
    try:
        for i in range(reps + 1):
            r = call(eng)
            low = min(low, torch.cuda.mem_get_info()[0])
            if i:
                for w in NAMES:
                    best[w] = min(best.get(w, 1e30), r.time_ms(w))
            entries = r.num_entries
            r.free()
    finally:
        eng.close()
    return best, free0 - low, entries


def show(title, best, taken, entries):
    print(f"{title}: {best[E.T_TOTAL]:.2f} ms, {entries} entries, {taken / 2**30:.2f} GiB of device memory taken")
    print("    " + ", ".join(f"{NAMES[w]} {best[w]:.2f}" for w in NAMES if w != E.T_TOTAL and best.get(w, 0) > 0))


def host_join(eng, logp, groups, cfg, eps):
    """The join cli.py used to do: per branch group a flatnonzero over all entries plus a searchsorted. -> seconds"""
    k, sigma = cfg["k"], cfg["sigma"]
    parts = eng.score_groups_keymajor(logp, groups, k, eps)
    db = eng.db_from_parts(parts, sigma, k)
    res = eng.score_groups_positions(logp.cpu().numpy(), groups, k, eps)
    t0 = time.perf_counter()
    keys_db, off_db = db.keys(), db.key_offsets().astype(np.int64)
    br_db, _ = db.entries()
    entry_key = np.repeat(keys_db, np.diff(off_db))
    pos_db = np.empty(len(br_db), dtype=np.uint32)
    rk, rp = res.keys(), res.positions()
    for gi, gid in enumerate(res.group_ids.tolist()):
        a, b = int(res.offsets[gi]), int(res.offsets[gi + 1])
        sel = np.flatnonzero(br_db == gid)
        pos_db[sel] = rp[a:b][np.searchsorted(rk[a:b], entry_key[sel])]
    dt = time.perf_counter() - t0
    n = db.num_entries
    res.free(); db.free(); parts.free()
    return dt, n


def main():
    name, n_groups = sys.argv[1], int(sys.argv[2])
    join_groups = int(sys.argv[sys.argv.index("--join-groups") + 1]) if "--join-groups" in sys.argv else min(n_groups, 8)
    cfg = CONFIGS[name]
    k, sigma = cfg["k"], cfg["sigma"]
    eps = ipk_amd.log_threshold(cfg["omega"], sigma, k)
    logp, groups = device_matrices(cfg, n_groups)
    if "--once" in sys.argv:
        eng = ipk_amd.Engine(0)
        for _ in range(2):
            eng.score_groups_keymajor_positions(logp, groups, k, eps).free()
        eng.close()
        return
    print(f"== {name}: {n_groups} groups x {cfg['mats_per_group']} x {cfg['sites']} sites, sigma {sigma}, k {k}")
    a = leg(lambda e: e.score_groups_keymajor(logp, groups, k, eps))
    show("(a) plain key-major step", *a)
    b = leg(lambda e: e.score_groups_keymajor_positions(logp, groups, k, eps))
    show("(b) positioned key-major step", *b)
    host = logp.cpu().numpy()

    class Old:                                          # score_groups_positions' result behind the parts' timing interface
        def __init__(self, r): self.r, self.num_entries = r, r.num_entries
        def time_ms(self, w): return self.r.time_ms(w) if w in (E.T_TOTAL, E.T_PREFIX, E.T_SCORE_MAIN, E.T_COMPACT) else 0.0
        def free(self): self.r.free()
    c = leg(lambda e: Old(e.score_groups_positions(host, groups, k, eps)), reps=3)
    show("(c') score_groups_positions alone (3 calls)", *c)
    dev_c = a[0][E.T_TOTAL] + c[0][E.T_TOTAL]
    print(f"(c) earlier route, device time: (a) + (c') = {dev_c:.2f} ms; memory: the larger of both legs, {max(a[1], c[1]) / 2**30:.2f} GiB")
    print(f"(b) / (a) = {b[0][E.T_TOTAL] / a[0][E.T_TOTAL]:.3f};  (b) / (c) = {b[0][E.T_TOTAL] / dev_c:.3f}")
    for w in (E.T_XP_COUNT, E.T_XP_WRITE, E.T_SCORE_REDUCE, E.T_KM_WRITE):
        if a[0].get(w, 0) > 0:
            print(f"    {NAMES[w]}: (b) / (a) = {b[0][w] / a[0][w]:.2f}")
    eng = ipk_amd.Engine(0)
    jm = logp[:join_groups * cfg["mats_per_group"]].contiguous()
    dt, n = host_join(eng, jm, groups[:join_groups * cfg["mats_per_group"]], cfg, eps)
    eng.close()
    print(f"host join of the earlier route at {join_groups} groups ({n} entries): {dt:.2f} s wall "
          f"(its cost grows with groups x entries: x{(n_groups / join_groups) ** 2:.0f} at {n_groups} groups)")


if __name__ == "__main__":
    main()
