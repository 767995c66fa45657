"""Wall time of `ipk.py build --filter random` on a 125-group share of cfg2 (tools/ondisk_probe.py's shape, built in memory).

  python tools/random_filter_probe.py [--tree NAME=DIR ...] [--runs 3] [--out profiles/random_filter_probe.txt]

Writes the share as a `.raxml.ancestralProbs` text file (9 decimals, as RAxML-ng does) and a --mapping file once, then runs the
command of every tree (default: this checkout alone; several trees, e.g. a parent checkout beside this one, are run ALTERNATED) in a
fresh process `--runs` times each and records the wall time of the process and its "Filtering time" and "Merge time" lines.
With --filter mif0 the same for the default filter."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ipk_amd.synth import CONFIGS, synth_matrices                         # noqa: E402

N_GROUPS = 125


def write_share(d):
    cfg = CONFIGS["cfg2"]
    mpg, sites = cfg["mats_per_group"], cfg["sites"]
    os.makedirs(os.path.join(d, "AR"))
    site_txt = [f"\t{s + 1}\tA\t" for s in range(sites)]
    with open(os.path.join(d, "AR", "share.raxml.ancestralProbs"), "w") as fh, open(os.path.join(d, "map.tsv"), "w") as mp:
        fh.write("Node\tSite\tState\tp_A\tp_C\tp_G\tp_T\n")
        for g in range(N_GROUPS):
            p = np.power(10.0, synth_matrices(mpg, sites, cfg["sigma"], cfg["alpha"], cfg["seed"], first_mat=mpg * g).astype(np.float64))
            for j in range(mpg):
                lab = f"{g}_X{j}"
                mp.write(f"{lab}\t{g + 1}\n")
                fh.write("".join(lab + site_txt[s] + "%.9f\t%.9f\t%.9f\t%.9f\n" % tuple(row) for s, row in enumerate(p[j].tolist())))
    return cfg


def run(tree, d, cfg, filt, tag):
    out = os.path.join(d, f"{tag}.ipk")
    work = os.path.join(d, f"w_{tag}")
    cmd = [sys.executable, os.path.join(tree, "ipk.py"), "build", "-w", work, "--ar-dir", os.path.join(d, "AR"), "--mapping", os.path.join(d, "map.tsv"),
           "-k", str(cfg["k"]), "--omega", str(cfg["omega"]), "--filter", filt, "--num-tree-nodes", str(2 * N_GROUPS), "-o", out]
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tree, timeout=600)
    wall = time.time() - t0
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed:\n{r.stdout}\n{r.stderr}")
    ms = lambda name: float(re.search(name + r" time: (\d+) ms", r.stdout).group(1))
    totals = re.search(r"\((\d+) k-mers, (\d+) entries\)", r.stdout).groups()
    size = os.path.getsize(out)
    shutil.rmtree(work, ignore_errors=True)
    return wall, ms("Computation"), ms("Filtering"), ms("Merge"), totals, size, out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", action="append", default=[], help="NAME=DIR of a checkout whose ipk.py is run (built); default: this one")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--filter", default="random", choices=["mif0", "random"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    trees = [t.split("=", 1) for t in a.tree] or [["this", ROOT]]
    d = tempfile.mkdtemp(prefix="random_filter_probe_", dir=os.environ.get("IPK_PROBE_DIR"))
    try:
        t0 = time.time()
        cfg = write_share(d)
        lines = [f"cfg2 share: {N_GROUPS} groups, sigma={cfg['sigma']} k={cfg['k']} sites={cfg['sites']}, `ipk.py build --filter {a.filter}` in a fresh "
                 f"process per run, trees alternated (input written in {time.time() - t0:.1f} s)"]
        files = {}
        for i in range(a.runs):
            for name, tree in trees:
                wall, score, filt, merge, totals, size, out = run(os.path.abspath(tree), d, cfg, a.filter, name)
                files[name] = out
                lines.append(f"  {name:8s} run {i + 1}: wall {wall:.2f} s  Computation time {score:.0f} ms  Filtering time {filt:.0f} ms  Merge time {merge:.0f} ms"
                             f"  ({totals[0]} k-mers, {totals[1]} entries, file {size} bytes)")
                print(lines[-1], flush=True)
        if len(files) > 1:
            blobs = [open(f, "rb").read() for f in files.values()]
            lines.append(f"  files of {', '.join(files)} identical: {all(b == blobs[0] for b in blobs)}")
        text = "\n".join(lines) + "\n"
        print(text, end="")
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(text)
    finally:
        shutil.rmtree(d, ignore_errors=True)
