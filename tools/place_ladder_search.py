"""Searches the rounding ladder of tests/place_ext_cases.py (LADDER) on the CPU and prints it as the literal the case file holds.

    python tools/place_ladder_search.py [--per-rung 8]

A single-window query whose one ambiguous symbol (R resolutions) has exactly one resolution in the database, with one entry of score x,
places that branch with y = (float)log10((10^x + (R - 1) E) / R), E = 10^log_eps.  For every binary32 x in [-6, -1), R = 2 and R = 4,
log_eps = -4.5: y in binary64 as a prescreen, then the 60-digit value of those within 2^-35 of a binary32 rounding midpoint; d is the
60-digit distance to the nearer midpoint and the rung of an input is floor(log2 d): rung -44 holds 2^-44 <= d < 2^-43.  Up to
--per-rung inputs per rung and R are recorded from rung -36 down to the finest found, spread over the range of x.  About 21 M values
per R; never run by a test (tests/test_place_ext_paths_inputs.py checks each recorded d again)."""
import argparse
import decimal
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import place_ext_cases as xc                # noqa: E402

LO, HI = 0xBF800001, 0xC0C00000                        # the bits of the binary32 values in [-6, -1): -1 excluded, -6 included
COARSEST = -36


def prescreen(R, log_eps, chunk=1 << 21):
    """bits of the x whose binary64 y lies within 2^-35 (and a slack for the binary64 error) of a binary32 midpoint."""
    E = 10.0 ** float(np.float32(log_eps))
    keep = []
    for a in range(LO, HI + 1, chunk):
        bits = np.arange(a, min(a + chunk, HI + 1), dtype=np.uint32)
        x = bits.view(np.float32).astype(np.float64)
        y = np.log10((np.power(10.0, x) + (R - 1) * E) / R)
        f = y.astype(np.float32)
        up = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
        dn = np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
        f = f.astype(np.float64)
        d = np.minimum(np.abs(y - (f + up) / 2), np.abs(y - (f + dn) / 2))
        keep.append(bits[d < 2.0 ** (COARSEST + 1) + 2.0 ** -45])
    return np.concatenate(keep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-rung", type=int, default=8)
    args = ap.parse_args()
    print("LADDER = {")
    for R in (2, 4):
        rungs = {}
        cand = prescreen(R, xc.LOG_EPS)
        for b in cand.tolist():
            y, right, d = xc.exact_contribution((float(np.uint32(b).view(np.float32)),), R, xc.LOG_EPS)
            rung = math.floor(math.log2(float(d)))
            if rung <= COARSEST:
                rungs.setdefault(rung, []).append((b, float(d)))
        print(f"    # R = {R}: {len(cand)} prescreened; inputs per rung: " + ", ".join(f"{r}: {len(v)}" for r, v in sorted(rungs.items(), reverse=True)))
        finest = min(v[1] for vs in rungs.values() for v in vs)
        print(f"    # finest d = 2^{math.log2(finest):.1f}")
        print(f"    {R}: {{")
        for r in sorted(rungs, reverse=True):
            v = sorted(rungs[r])
            pick = sorted(set(np.linspace(0, len(v) - 1, min(args.per_rung, len(v))).round().astype(int).tolist()))
            print(f"        {r}: [" + ", ".join(f"0x{v[i][0]:08X}" for i in pick) + "],")
        print("    },")
    print("}")


if __name__ == "__main__":
    decimal.getcontext().prec = 60
    main()
