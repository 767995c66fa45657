"""The fixtures of tests/golden/ref/ (written by oracle/gen_ref_golden.py from the compiled reference) and the random inputs of
the live sweeps, shared by tests/test_ref_pin.py (CPU) and tests/test_gpu_ref_pin.py (GPU).  Not a test file."""
import functools
import os

import numpy as np

from ipk_amd.synth import synth_matrices
from oracle import gen_ref_golden as gen

REF_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref")
SCORE_NAMES = sorted(list(gen.SYNTH) + list(gen.GRID), key=lambda n: (n.split("_")[0], n.split("_")[1], int(n.split("_k")[1])))
GRID_NAMES = [n for n in SCORE_NAMES if n.startswith("grid_")]


class Fixture:
    """One scoring fixture: the input and, per group in first-seen order, what the reference gave."""

    def __init__(self, name):
        z = np.load(os.path.join(REF_DIR, name + ".npz"))
        self.name = name
        self.family = str(z["family"])
        self.mats = np.ascontiguousarray(z["logp"], dtype=np.float32)
        self.sigma, self.k = int(z["sigma"]), int(z["k"])
        self.eps = float(z["eps_bits"].reshape(1).view(np.float32)[0])
        self.mat_group = z["mat_group"].astype(np.uint32)
        self.group_ids = z["group_ids"].tolist()
        n = len(self.group_ids)
        self.keys = [z[f"keys_{g}"] for g in range(n)]
        self.score_bits = [z[f"score_bits_{g}"] for g in range(n)]
        self.positions = [z[f"positions_{g}"] for g in range(n)]
        self.emitted = [int(z[f"emitted_{g}"]) for g in range(n)]
        self.on_eps, self.above_eps, self.tied_keys = int(z["on_eps"]), int(z["above_eps"]), int(z["tied_keys"])

    def group_mats(self, gi):
        return self.mats[self.mat_group == self.group_ids[gi]]

    def db(self):
        """The key-major database of the fixture: (keys ascending, key_offsets, branches, score bits, positions), the entries of
        a key in group (first-seen) order."""
        keys = np.concatenate(self.keys)
        br = np.concatenate([np.full(len(k), g, dtype=np.uint32) for g, k in zip(self.group_ids, self.keys)])
        rank = np.concatenate([np.full(len(k), i, dtype=np.int64) for i, k in enumerate(self.keys)])
        order = np.lexsort((rank, keys))
        uk, counts = np.unique(keys, return_counts=True)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        return uk, off, br[order], np.concatenate(self.score_bits)[order], np.concatenate(self.positions)[order]


@functools.lru_cache(maxsize=None)
def load(name):
    return Fixture(name)


@functools.lru_cache(maxsize=None)
def load_mif0():
    z = np.load(os.path.join(REF_DIR, "mif0.npz"))
    off = z["offsets"]
    lists = [z["scores"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    thr = float(z["threshold_bits"].reshape(1).view(np.float32)[0])
    return lists, z["N"].tolist(), thr, z["fv_bits"]


def random_case(rng, max_k_dna=10, max_k_aa=4):
    """One small random input of either family: (family, mats, sigma, k, eps)."""
    sigma = 4 if rng.random() < 0.6 else 20
    k = int(rng.integers(2, max_k_dna + 1)) if sigma == 4 else int(rng.integers(2, max_k_aa + 1))
    sites = int(rng.integers(k, k + 7))
    n_mats = int(rng.integers(1, 5))
    if rng.random() < 0.5:
        family = "grid"
        mats = gen.grid_matrices(n_mats, sites, sigma, 0, float(rng.choice([0.0, 0.1])), rng=rng)
        best = mats.max(axis=2)                       # aim eps a few steps under the best window score of the case
        top = max(float(best[q, s:s + k].sum()) for q in range(n_mats) for s in range(sites - k + 1))
        eps = (top if np.isfinite(top) else -0.25 * k) - 0.25 * int(rng.integers(0, 5))
    else:
        family = "synth"
        alpha = float(rng.choice([0.03, 0.1, 0.3] if sigma == 4 else [0.03, 0.05]))
        mats = synth_matrices(n_mats, sites, sigma, alpha, int(rng.integers(1, 10 ** 6)))
        if rng.random() < 0.3:
            mats.reshape(-1)[rng.integers(0, mats.size, size=3)] = -np.inf
        eps = float(np.float32(k * np.log10(float(rng.choice([1.0, 1.5, 2.0])) / sigma))) + float(rng.choice([0.0, 0.5]))
    return family, mats, sigma, k, float(np.float32(eps))
