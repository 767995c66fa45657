"""Searches the rounded-bound cases of tests/rounded_paths.py on the CPU and prints table rows.

    python tools/rounded_cases_search.py dna_k8 [--family tenth|floor] [--seeds 0:6] [--eps 1.3:2.4] [--heavy 0] [--long-lists]

For every (seed, eps) of the sweep: the scored count (at most MAX_SCORED), the windows with a half list beyond and within the
family's capacity, the k-mers that D1 (inner joins keep `>=`) and D3 (prefix sum restarted at the window) change, in all and in
windows beyond the capacity, and the tied keys per group.  A row that meets every floor is marked `ok`.  `long` sweeps the long case
(D4, D5).  --record NAME... prints rounded_paths.describe of cases already in the table, as COUNTS holds it."""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import grid_paths as gp                     # noqa: E402
from tests import rounded_paths as rp                  # noqa: E402

SHAPES = {"dna_k6": (4, 6, 136), "dna_k7": (4, 7, 137), "dna_k8": (4, 8, 138), "dna_k9": (4, 9, 139), "dna_k10": (4, 10, 140),
          "dna_k11": (4, 11, 77), "dna_k12": (4, 12, 78), "dna_k13": (4, 13, 17), "dna_k14": (4, 14, 18), "dna_k15": (4, 15, 18),
          "dna_k16": (4, 16, 19), "aa_k4": (20, 4, 30), "aa_k5": (20, 5, 20), "aa_k6": (20, 6, 14), "long": (4, 10, 4200),
          "aa_long": (20, 4, 4200)}


def span(text, step):
    a, b = (float(x) for x in text.split(":"))
    return np.arange(round(a / step), round(b / step) + 1) * step


def clear():
    for f in (rp.load, gp.load, gp.oracle, rp.half_lists):
        f.cache_clear()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="?")
    ap.add_argument("--family", default="tenth")
    ap.add_argument("--seeds", default="0:5")
    ap.add_argument("--eps", default="1.5:2.0")
    ap.add_argument("--heavy", type=int, default=0)
    ap.add_argument("--sites", type=int, default=0)
    ap.add_argument("--long-lists", action="store_true", help="half lists beyond the big-list cap are wanted (slice_long_lists)")
    ap.add_argument("--record", nargs="*")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        ge = rp.inner_ge_library(tmp)
        if args.record is not None:
            for name in args.record or list(rp.CASES):
                print(f"    {name!r}: {rp.describe(name, ge)},", flush=True)
                clear()
            return
        sigma, k, sites = SHAPES[args.shape]
        sites = args.sites or sites
        long = args.shape.endswith("long")
        for seed in span(args.seeds, 1).astype(int):
            for e in span(args.eps, 0.1):
                eps = -float(np.float32(round(e * 10) / 10))
                case = rp._case("candidate", "long" if long else args.family, sigma, k, sites, eps, int(seed), args.heavy,
                                groups=rp.LONG_GROUPS if long else rp.GROUPS)
                rp.CASES["candidate"] = case
                clear()
                c = rp.cheap_counts("candidate")
                row = f"{args.shape} {case.family} sites {sites} heavy {args.heavy} seed {seed} eps {eps:.1f}: {c}"
                ok = 0 < c["scored"] <= rp.MAX_SCORED
                if ok and "over_cap" in c and not long:
                    if k >= 13:
                        ok = (c["over_cap"] >= 3) if args.long_lists else (c["over_cap"] == 0 and c["longest"] > gp.ROWS_CAP)
                    else:
                        ok = c["over_cap"] >= 5 and c["below_cap"] >= 5
                if ok:
                    d = rp.describe("candidate", ge)
                    row = f"{args.shape} {case.family} sites {sites} heavy {args.heavy} seed {seed} eps {eps:.1f}: {d}"
                    devs = [v for key, v in d.items() if key[0] == "D" and not key.endswith("over_cap")]
                    ok = min(devs) >= rp.DEVIATION_FLOOR and min(d["tied"]) >= rp.TIED_FLOOR
                print(("ok   " if ok else "     ") + row, flush=True)


if __name__ == "__main__":
    main()
