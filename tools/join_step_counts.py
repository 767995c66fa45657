#!/usr/bin/env python3
"""Steps of the final join of the DNA k <= 10 scoring kernel per window, counted on the CPU for cfg2's own matrices (DESIGN A.8).

usage: join_step_counts.py [--mats 3] [--windows 990] [--out profiles/childstep_join_steps.json]

Half lists by the oracle's definition (every h-mer of a half whose score exceeds eps minus the other half's best, float64 sums of
the float32 entries), eps = log10((omega / 4)^k).  Per window with both half lists non-empty:
  today       R in blocks of <= 64 entries, floor(64 / width) rows of L per step (kernels_quad.hpp);
  best_split  R cut into n blocks of equal width (the last one shorter), the n that gives the fewest steps, no block setup counted;
  floor       candidates / 64: what any candidate-per-lane join needs at least;
  staircase   both lists sorted by score: a row's passing pairs are a prefix of R, and only the prefix and the one pair that ends
              it are visited -- (sum over rows of min(prefix + 1, |R|)) / 64.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ipk_amd.synth import CONFIGS, synth_matrices  # noqa: E402


def all_sums(cols):
    s = np.zeros(1)
    for c in cols:
        s = (s[:, None] + c[None, :].astype(np.float64)).ravel()
    return s


def steps_today(n_l, n_r):
    steps = 0
    for jb in range(0, n_r, 64):
        w = min(64, n_r - jb)
        steps += math.ceil(n_l / (64 // w))
    return steps


def steps_best_split(n_l, n_r):
    best = None
    for n in range(math.ceil(n_r / 64), n_r + 1):
        w = math.ceil(n_r / n)
        widths = [w] * (n_r // w) + ([n_r % w] if n_r % w else [])
        s = sum(math.ceil(n_l / (64 // x)) for x in widths)
        best = s if best is None else min(best, s)
        if w == 1:
            break
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mats", type=int, default=3)
    ap.add_argument("--windows", type=int, default=990)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "childstep_join_steps.json"))
    a = ap.parse_args()
    cfg = CONFIGS["cfg2"]
    k, hl = cfg["k"], cfg["k"] // 2
    eps = float(np.float32(k * math.log10(cfg["omega"] / cfg["sigma"])))
    mats = synth_matrices(a.mats, a.windows + k - 1, cfg["sigma"], cfg["alpha"], cfg["seed"])
    acc = dict(windows=0, empty=0, single_step=0, candidates=0, passing=0, today=0, best_split=0, floor=0.0, staircase=0.0)
    for m in mats:
        cmax = m.max(axis=1).astype(np.float64)
        for w in range(a.windows):
            eps_l, eps_r = eps - cmax[w + hl:w + k].sum(), eps - cmax[w:w + hl].sum()
            left, right = all_sums(m[w:w + hl]), all_sums(m[w + hl:w + k])
            left, right = np.sort(left[left > eps_l])[::-1], np.sort(right[right > eps_r])[::-1]
            acc["windows"] += 1
            n_l, n_r = len(left), len(right)
            if n_l == 0 or n_r == 0:
                acc["empty"] += 1
                continue
            prefix = (left[:, None] + right[None, :] > eps).sum(axis=1)
            acc["candidates"] += n_l * n_r
            acc["passing"] += int(prefix.sum())
            acc["today"] += steps_today(n_l, n_r)
            acc["best_split"] += steps_best_split(n_l, n_r)
            acc["floor"] += n_l * n_r / 64
            acc["staircase"] += float(np.minimum(prefix + 1, n_r).sum()) / 64
    n = acc["windows"]
    out = dict(config="cfg2", k=k, eps=eps, matrices=a.mats, windows=n, windows_with_an_empty_half=acc["empty"],
               per_window={key: acc[key] / n for key in ("candidates", "passing", "today", "best_split", "floor", "staircase")})
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
