"""Measurements of the on-disk build (ipk_amd/ondisk.py) beside the in-memory build, on one GPU.

  python tools/ondisk_probe.py [--out profiles/ondisk_probe.txt]     a cfg2 share (125 groups) and a cfg4 share (64 groups): wall times of
        the in-memory build (score, filter, file) beside the on-disk build's three stages, bytes spilled beside the dense form's,
        spill write / block read rates, the held peaks of both builds
  python tools/ondisk_probe.py --floor                                the figures of tests/test_gpu_ondisk.py::test_the_valve: F, b and G
  python tools/ondisk_probe.py --kernels cfg2|cfg4                    one spill and one merge of the share, for a rocprofv3 --kernel-trace run

File rates are to be read beside tools/micro_filewrite.cpp on the same box in the same run."""
import argparse
import glob
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ipk_amd                                                           # noqa: E402
from ipk_amd import dbfile, ondisk                                        # noqa: E402
from ipk_amd import distributed as D                                      # noqa: E402
from ipk_amd.synth import CONFIGS, synth_matrices                         # noqa: E402

MIB = 1 << 20
SHARES = {"cfg2": 125, "cfg4": 64}


def share(name, n_groups, sites=None):
    cfg = CONFIGS[name]
    sites = sites or cfg["sites"]
    mpg = cfg["mats_per_group"]
    mats = np.concatenate([synth_matrices(mpg * min(25, n_groups - g), sites, cfg["sigma"], cfg["alpha"], cfg["seed"], first_mat=mpg * g)
                           for g in range(0, n_groups, 25)])
    groups = np.repeat(np.arange(1, n_groups + 1, dtype=np.uint32), mpg)
    return cfg, mats, groups


def in_memory(eng, cfg, mats, groups, path):
    import torch
    k, sigma = cfg["k"], cfg["sigma"]
    eps = ipk_amd.log_threshold(cfg["omega"], sigma, k)
    eng.mem_stats(reset_peak=True)
    t0 = time.time()
    dev = torch.from_numpy(mats).cuda()
    db, parts = D.build_db_shard(eng, dev, groups, k, eps, sigma)
    t1 = time.time()
    db.filter_mif0(eng, 2 * len(set(groups.tolist())), ipk_amd.score_threshold(cfg["omega"], sigma, k))
    t2 = time.time()
    dbfile.write_db_device(eng, db, path, "DNA" if sigma == 4 else "AA", [], "", k, cfg["omega"])
    t3 = time.time()
    out = {"score_s": t1 - t0, "filter_s": t2 - t1, "file_s": t3 - t2, "keys": db.num_keys, "entries": db.num_entries,
           "held_peak": eng.mem_stats()[1], "file_bytes": os.path.getsize(path)}
    db.free(); parts.free()
    return out


def on_disk(eng, cfg, mats, groups, path, work, **kw):
    k, sigma = cfg["k"], cfg["sigma"]
    eps = ipk_amd.log_threshold(cfg["omega"], sigma, k)
    return ondisk.build_db_file(eng, mats, groups, k, eps, sigma, path, work, "DNA" if sigma == 4 else "AA", [], "", cfg["omega"], "mif0",
                                2 * len(set(groups.tolist())), **kw)


def rates(eng, cfg, mats, groups, work, B=32):
    """One piece of the whole share spilled, then every batch read back: bytes and seconds of each direction alone."""
    k, sigma = cfg["k"], cfg["sigma"]
    eps = ipk_amd.log_threshold(cfg["omega"], sigma, k)
    os.makedirs(work, exist_ok=True)
    parts = eng.score_groups_keymajor(mats, groups, k, eps, n_owners=B)
    t0 = time.time()
    nbytes = eng.parts_spill(parts, work, 0)
    t_w = time.time() - t0
    parts.free()
    t_r = 0.0
    for b in range(B):
        t0 = time.time()
        db = eng.spill_merge(sigma, k, b, B, [ondisk.block_path(work, 0, b)])
        t_r += time.time() - t0
        db.free()
    shutil.rmtree(work, ignore_errors=True)
    return nbytes, t_w, t_r


def probe(out_path):
    lines = []
    tmp = tempfile.mkdtemp(prefix="ondisk_probe_", dir=os.environ.get("IPK_PROBE_DIR"))
    for name, n_groups in SHARES.items():
        cfg, mats, groups = share(name, n_groups)
        eng = ipk_amd.Engine(0)
        one, two = os.path.join(tmp, f"{name}_mem.ipk"), os.path.join(tmp, f"{name}_disk.ipk")
        in_memory(eng, cfg, mats, groups, one)                         # (warm-up: first-call allocations)
        m = in_memory(eng, cfg, mats, groups, one)
        eng.close()
        eng = ipk_amd.Engine(0)
        d = on_disk(eng, cfg, mats, groups, two, os.path.join(tmp, name + "_w"))
        same = open(one, "rb").read() == open(two, "rb").read()
        nbytes, t_w, t_r = rates(eng, cfg, mats, groups, os.path.join(tmp, name + "_r"))
        nbytes, t_w, t_r = rates(eng, cfg, mats, groups, os.path.join(tmp, name + "_r"))
        eng.close()
        lines += [
            f"{name} share: {n_groups} groups, sigma={cfg['sigma']} k={cfg['k']} sites={cfg['sites']}: {m['keys']} k-mers, {m['entries']} entries, "
            f"file {m['file_bytes']} bytes; on-disk file identical: {same}",
            f"  in-memory  score {m['score_s']:.3f} s  filter {m['filter_s']:.3f} s  file {m['file_s']:.3f} s  total {m['score_s'] + m['filter_s'] + m['file_s']:.3f} s"
            f"  held_peak {m['held_peak']} bytes",
            f"  on-disk    stage 1 {d['stage1_s']:.3f} s ({d['pieces']} pieces)  stage 2 {d['stage2_s']:.3f} s ({d['batches']} batches; filter {d['filter_s']:.3f} s)"
            f"  stage 3 {d['stage3_s']:.3f} s  total {d['stage1_s'] + d['stage2_s'] + d['stage3_s']:.3f} s  held_peak {d['held_peak']} bytes"
            f" (budget {d['budget_bytes']})",
            f"  spilled {d['spilled_bytes']} bytes packed; dense rows would have taken {d['dense_bytes']} bytes ({d['dense_bytes'] / max(1, d['spilled_bytes']):.2f} x)",
            f"  one piece of the whole share: {nbytes} bytes; spill (pack + copy + write) {t_w:.3f} s = {nbytes / t_w / 1e9:.2f} GB/s; "
            f"read + unpack + merge of its 32 blocks {t_r:.3f} s = {nbytes / t_r / 1e9:.2f} GB/s",
        ]
    shutil.rmtree(tmp, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)


def one_group_pieces(cfg, mats, groups, budget):
    """The on-disk build with one-group pieces under `budget`; None if it does not fit."""
    eng = ipk_amd.Engine(0)
    tmp = tempfile.mkdtemp(prefix="ondisk_floor_", dir=os.environ.get("IPK_PROBE_DIR"))
    try:
        return on_disk(eng, cfg, mats, groups, os.path.join(tmp, "db.ipk"), os.path.join(tmp, "w"), piece_sizes=[1], budget_bytes=budget)
    except ondisk.OnDiskError:
        return None
    except ipk_amd.IpkGpuError as e:
        if e.code != 3:
            raise
        return None
    finally:
        eng.close()
        shutil.rmtree(tmp, ignore_errors=True)


def floor(sites, G=16, rounds=4):
    """F, b, G of the valve test.  The engine sizes its pair pool by the memory it may count on, so a build that is given much holds
    much (6.1 GB for one cfg2 group on an empty device, nearly all of it spare chunks): the FLOOR is the held peak under the least
    budget (whole MiB, by bisection) with which the build with one-group pieces completes.  Iterated until G groups' entries
    exceed 2 b with b = 2 F from a G-group build."""
    for _ in range(rounds):
        cfg, mats, groups = share("cfg2", G, sites)
        t0 = time.time()
        free = one_group_pieces(cfg, mats, groups, 64 << 30)
        lo, hi, best = 8, 16 << 10, None                       # MiB: lo does not fit, hi does
        while hi - lo > 1:
            mid = (lo + hi) // 2
            d = one_group_pieces(cfg, mats, groups, mid * MIB)
            if d is None:
                lo = mid
            else:
                hi, best = mid, d
        if best is None:
            best = one_group_pieces(cfg, mats, groups, hi * MIB)
        F = best["held_peak"]
        b = (2 * F + MIB - 1) // MIB * MIB
        per_group = best["totals"][1] / G
        need = int(2 * b / (8 * per_group)) + 2
        print(f"sites {sites} G = {G}: least budget {hi} MiB, held peak under it F = {F} bytes (stage 1 {best['stage1_peak']}, stage 2 {best['stage2_peak']}); "
              f"given 64 GiB the same build holds {free['held_peak']} bytes; b = {b // MIB} MiB, {per_group:.0f} entries per group, "
              f"entries x 8 = {8 * best['totals'][1]} bytes, G needed {need}; {time.time() - t0:.1f} s", flush=True)
        if need <= G:
            print(f"VALVE_SITES = {sites}  VALVE_FLOOR_BYTES = {F}  VALVE_BUDGET = {b // MIB} * MIB  VALVE_GROUPS = {G}")
            return
        G = need


def kernels(name):
    cfg, mats, groups = share(name, SHARES[name])
    eng = ipk_amd.Engine(0)
    tmp = tempfile.mkdtemp(prefix="ondisk_kernels_", dir=os.environ.get("IPK_PROBE_DIR"))
    print(rates(eng, cfg, mats, groups, os.path.join(tmp, "r")))
    eng.close()
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--floor", action="store_true")
    ap.add_argument("--sites", type=int, default=10000)
    ap.add_argument("--groups", type=int, default=16, help="--floor: the group count to start from")
    ap.add_argument("--rounds", type=int, default=4, help="--floor: builds at most")
    ap.add_argument("--kernels", default=None, choices=sorted(SHARES))
    a = ap.parse_args()
    if a.floor:
        floor(a.sites, a.groups, a.rounds)
    elif a.kernels:
        kernels(a.kernels)
    else:
        probe(a.out)
