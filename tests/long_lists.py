"""Inputs whose windows have half lists beyond the big-list kernels' capped capacity (6144 entries a half list from DNA k = 13,
kernels_score.hpp BIG_CAP_ENTRIES), shared by tests/test_long_lists_inputs.py (CPU: the inputs are what they claim) and
tests/test_gpu_long_lists.py (GPU: the option "slice_long_lists" scores them).  Not a test file."""
import numpy as np

from oracle import ipk_oracle as co

CAP = 6144            # BIG_CAP_ENTRIES
LONG = 7000           # what a list must reach to count as beyond the cap: no ulp at a bound decides it

GRADES = (0.34, 0.28, 0.22, 0.16)
# (k, slack) of the graded recipe
GRADED_SLACK = {14: 1.2, 15: 1.0, 16: 1.0}


def graded(k, seed, sites=None):
    """Near-flat columns: the four grades permuted per site; log10 as float32.  sites = k + 1: two windows."""
    rng = np.random.default_rng(seed)
    sites = k + 1 if sites is None else sites
    p = np.stack([rng.permutation(GRADES) for _ in range(sites)])
    return np.log10(p).astype(np.float32)


def graded_eps(m, k, slack):
    """The threshold `slack` below the best score of window 0."""
    best = co.prefix_max(m)
    return float(np.float32(np.float32(best[k] - best[0]) - np.float32(slack)))


def graded_input(k, n_mats=1, seed=None):
    """n_mats graded matrices (seeds seed, seed + 1, ...; seed = k by default) and the threshold of the first one's window 0."""
    seed = k if seed is None else seed
    mats = np.stack([graded(k, seed + i) for i in range(n_mats)])
    return mats, graded_eps(mats[0], k, GRADED_SLACK[k])


def k13_input():
    """DNA k = 13, omega = 1.5: six peaked sites (0.97 / 0.01 x 3) then nine flat ones -- the 7-symbol right half of window 0
    is all 4^7 suffixes -- and the same matrix reversed.  Returns (mats [2, 15, 4], eps)."""
    sites = np.full((15, 4), 0.25, np.float64)
    for i in range(6):
        sites[i] = 0.01
        sites[i, 0] = 0.97
    a = np.log10(sites).astype(np.float32)
    mats = np.stack([a, a[::-1]]).astype(np.float32)
    return np.ascontiguousarray(mats), co.log_threshold(1.5, 4, 13)


def flat_input(k):
    """Worst case: flat columns, sites = k (one window a matrix), two matrices, a threshold below every score."""
    v = np.float32(np.log10(0.25))
    mats = np.full((2, k, 4), v, np.float32)
    return mats, float(np.float32(k * np.log10(0.25) - 0.5))


def split_sum_bits(v, k):
    """Score bits of k equal float32 terms added in the order of pk_compute.cpp:54-58,90: halves h / 2 and h - h / 2, recursively."""
    def rec(h):
        if h == 1:
            return np.float32(v)
        return np.float32(rec(h // 2) + rec(h - h // 2))
    return int(np.array([rec(k)], dtype=np.float32).view(np.uint32)[0])


def half_list_sizes(m, k, start, eps):
    """(|L|, |R|) of window `start`: the oracle's DC on the half's columns with the half's threshold (pk_compute.cpp:54-55)."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    best = co.prefix_max(m)
    hl = k // 2
    e = np.float32(eps)
    eps_l = np.float32(e - np.float32(best[start + k] - best[start + hl]))
    eps_r = np.float32(e - np.float32(best[start + hl] - best[start]))
    nl = len(co.window(m[start:start + hl], hl, 0, float(eps_l))[0])
    nr = len(co.window(m[start + hl:start + k], k - hl, 0, float(eps_r))[0])
    return nl, nr


def longest_half_lists(mats, k, eps):
    """Per window of every matrix: (matrix, start, |L|, |R|)."""
    out = []
    for i, m in enumerate(mats):
        for s in range(m.shape[0] - k + 1):
            out.append((i, s) + half_list_sizes(m, k, s, eps))
    return out


def ordinary_second_group(k, seed=7):
    """One ordinary (peaked) matrix of k + 1 sites: a second group beside a graded one."""
    from ipk_amd.synth import synth_matrices
    return synth_matrices(1, k + 1, 4, 0.1, seed)


def k14_input():
    """Two different graded matrices in group 5 (both halves of every window beyond the cap) and an ordinary matrix as group 9."""
    mats, eps = graded_input(14, 2)
    return np.concatenate([mats, ordinary_second_group(14)]), np.array([5, 5, 9], dtype=np.uint32), eps


def keyrange_input(k):
    """The key-range cases: k = 14 as k14_input; k = 15, 16: one graded matrix (group 5) and an ordinary one (group 9)."""
    if k == 14:
        return k14_input()
    mats, eps = graded_input(k, 1)
    return np.concatenate([mats, ordinary_second_group(k)]), np.array([5, 9], dtype=np.uint32), eps


CLI_LABELS = ("0_X0", "0_X1")
CLI_OMEGA = 1.5


def write_probs_file(path, labels, mats):
    """A .raxml.ancestralProbs file of the DNA matrices `mats` (log10 values; probabilities written with nine decimals)."""
    with open(path, "w") as fh:
        fh.write("Node\tSite\tState\t" + "\t".join("p_" + c for c in "ACGT") + "\n")
        for lab, m in zip(labels, mats):
            p = np.power(10.0, m.astype(np.float64))
            for s in range(p.shape[0]):
                fh.write(f"{lab}\t{s + 1}\t{'ACGT'[int(np.argmax(p[s]))]}\t" + "\t".join("%.9f" % v for v in p[s]) + "\n")
