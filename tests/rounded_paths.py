"""Inputs whose look-ahead bounds round, one per kernel family, shared by tests/test_rounded_paths_inputs.py (CPU: the cases decide
what they claim to decide, and the oracle is pinned on them) and tests/test_gpu_rounded_paths.py (GPU: every entry point against
the oracle).  Not a test file.

Every entry is float32(-0.1) * an integer and every threshold the float32 of a multiple of 0.1.  A tenth is no binary fraction:
the prefix sums of the column maxima (window.cpp:16-27) round at nearly every site, a node's bound is
fl(eps - fl(best[a + len] - best[a])) (window.cpp:69-72, pk_compute.cpp:54-55), and candidates sit within an ulp of these bounds
by the thousand.  Whether such a candidate is scored then depends on how the prefix sums and the bounds are associated and on
whether an inner join keeps `score > bound` or `score >= bound` -- which the exact-sum cases of tests/grid_paths.py cannot tell.
The deviations below restate such slips on the CPU; a case is in the table because they change its scored k-mers."""
import collections
import functools

import numpy as np

from oracle import gen_ref_golden as gen
from oracle import ipk_oracle as co
from tests import grid_paths as gp

GROUPS = gp.GROUPS
LONG_GROUPS = np.array([7, 3], dtype=np.uint32)       # the long case: one matrix a group, no twins
CHUNK = 2048                                          # sites a workgroup of the prefix kernel sums at a time
MAX_SCORED = gp.MAX_SCORED
DEVIATION_FLOOR = 20                                  # scored k-mers a deviation must change, at least
TIED_FLOOR = 50

Case = collections.namedtuple("Case", "name family sigma k sites heavy eps seed groups opts")


def _case(name, fam, sigma, k, sites, eps, seed, heavy=0, opts=(), groups=GROUPS):
    return Case(name, fam, sigma, k, sites, heavy, float(np.float32(eps)), seed, groups, dict(opts))


# Found by tools/rounded_cases_search.py on the CPU; recorded here, no test loops over seeds.  Families of inputs: `tenth`
# (gen_ref_golden.tenth_twin_matrices), `floor` (tenth_floor_matrices; `heavy` leading columns around -100 on top of `sites`),
# `long` (tenth_matrices, two matrices, no twins).  Window counts as in grid_paths.CASES.  profiles/rounded_bounds_inputs.txt
# has every count and names what the search could not satisfy.
#           name                   family  sigma k  sites  eps  seed
CASES = {c.name: c for c in (
    _case("dna_k6_floor",       "floor",  4,  6, 136, -1.6, 0),
    _case("dna_k7_floor",       "floor",  4,  7, 137, -1.6, 0),
    _case("dna_k8_tenth",       "tenth",  4,  8, 138, -1.6, 1),
    _case("dna_k9_tenth",       "tenth",  4,  9, 139, -1.6, 2),
    _case("dna_k11_tenth",      "tenth",  4, 11,  77, -2.2, 0),
    _case("dna_k12_tenth",      "tenth",  4, 12,  78, -2.2, 0),
    _case("dna_k13_mid_tenth",  "tenth",  4, 13,  17, -2.7, 0),
    _case("dna_k13_long_tenth", "tenth",  4, 13,  17, -3.2, 0, opts=gp.SLICE),
    _case("dna_k14_mid_tenth",  "tenth",  4, 14,  18, -2.9, 0),
    _case("dna_k14_long_tenth", "tenth",  4, 14,  18, -3.4, 0, opts=gp.SLICE),
    _case("dna_k15_mid_tenth",  "tenth",  4, 15,  18, -3.2, 0),
    _case("dna_k15_long_tenth", "tenth",  4, 15,  18, -3.5, 0, opts=gp.SLICE),
    _case("dna_k16_tenth",      "tenth",  4, 16,  19, -2.9, 0),
    _case("aa_k5_floor",        "floor", 20,  5,  20, -1.6, 4),
    _case("aa_k6_floor",        "floor", 20,  6,  10, -1.6, 4),
    _case("dna_k10_long",       "long",   4, 10, 4200, -1.6, 1, groups=LONG_GROUPS),
)}
LONG = "dna_k10_long"
# The cases for which the search found no input that meets both D1 and D3: the deviation they do not meet.
ONE_DEVIATION = {"dna_k15_long_tenth": ("D3",), "dna_k16_tenth": ("D3",)}
# The cases with half lists beyond their family's capacity in none of whose windows beyond it a deviation changes a k-mer.
NONE_BEYOND_CAP = ()

# describe() of every case, recorded: the GPU tests assert the cheap part (scored, entries, half lists) before they call the engine,
# tests/test_rounded_paths_inputs.py all of it.
COUNTS = {
    'dna_k6_floor': {'scored': 72270, 'entries': 8036, 'tied': [4028, 3874], 'cut': [0, 1], 'D1': 38, 'D3': 268},
    'dna_k7_floor': {'scored': 68490, 'entries': 20434, 'tied': [10187, 10204], 'cut': [5, 1], 'D1': 162, 'D3': 384},
    'dna_k8_tenth': {'scored': 418341, 'entries': 105896, 'over_cap': 40, 'below_cap': 484, 'longest': 256, 'tied': [48137, 57415], 'cut': [8, 2], 'D1': 574, 'D1_over_cap': 0, 'D3': 1144, 'D3_over_cap': 150},
    'dna_k9_tenth': {'scored': 341019, 'entries': 145648, 'over_cap': 57, 'below_cap': 467, 'longest': 662, 'tied': [47693, 90437], 'cut': [3, 5], 'D1': 279, 'D1_over_cap': 270, 'D3': 1710, 'D3_over_cap': 422},
    'dna_k11_tenth': {'scored': 1365720, 'entries': 669891, 'over_cap': 64, 'below_cap': 204, 'longest': 2265, 'tied': [363843, 291418], 'cut': [100, 5], 'D1': 3442, 'D1_over_cap': 1838, 'D3': 3420, 'D3_over_cap': 1346},
    'dna_k12_tenth': {'scored': 1365452, 'entries': 683586, 'over_cap': 63, 'below_cap': 205, 'longest': 1946, 'tied': [391239, 282881], 'cut': [588, 0], 'D1': 3928, 'D1_over_cap': 2252, 'D3': 3848, 'D3_over_cap': 2362},
    'dna_k13_mid_tenth': {'scored': 1073186, 'entries': 758045, 'over_cap': 0, 'below_cap': 20, 'longest': 2725, 'tied': [230090, 81277], 'cut': [0, 0], 'D1': 5690, 'D1_over_cap': 0, 'D3': 3990, 'D3_over_cap': 0},
    'dna_k13_long_tenth': {'scored': 8364939, 'entries': 5380792, 'over_cap': 3, 'below_cap': 17, 'longest': 6592, 'tied': [1794555, 951666], 'cut': [0, 9], 'D1': 27884, 'D1_over_cap': 9474, 'D3': 10286, 'D3_over_cap': 0},
    'dna_k14_mid_tenth': {'scored': 1002242, 'entries': 681043, 'over_cap': 0, 'below_cap': 20, 'longest': 3826, 'tied': [134167, 185831], 'cut': [0, 0], 'D1': 3524, 'D1_over_cap': 0, 'D3': 5256, 'D3_over_cap': 0},
    'dna_k14_long_tenth': {'scored': 10723112, 'entries': 6969075, 'over_cap': 8, 'below_cap': 12, 'longest': 9040, 'tied': [1653631, 1952082], 'cut': [0, 0], 'D1': 4244, 'D1_over_cap': 2780, 'D3': 7632, 'D3_over_cap': 6360},
    'dna_k15_mid_tenth': {'scored': 2083371, 'entries': 1337782, 'over_cap': 0, 'below_cap': 16, 'longest': 5054, 'tied': [219613, 521840], 'cut': [1302, 0], 'D1': 22522, 'D1_over_cap': 0, 'D3': 1350, 'D3_over_cap': 0},
    'dna_k15_long_tenth': {'scored': 8298953, 'entries': 5285486, 'over_cap': 9, 'below_cap': 7, 'longest': 8270, 'tied': [1028241, 1932124], 'cut': [0, 0], 'D1': 64, 'D1_over_cap': 64, 'D3': 0, 'D3_over_cap': 0},
    'dna_k16_tenth': {'scored': 229464, 'entries': 152125, 'over_cap': 0, 'below_cap': 16, 'longest': 3916, 'tied': [5739, 71600], 'cut': [0, 0], 'D1': 64, 'D1_over_cap': 0, 'D3': 0, 'D3_over_cap': 0},
    'aa_k5_floor': {'scored': 11309729, 'entries': 4186300, 'over_cap': 58, 'below_cap': 6, 'longest': 6540, 'tied': [1695936, 1455133], 'cut': [0, 127], 'D1': 12400, 'D1_over_cap': 12400, 'D3': 70740, 'D3_over_cap': 70740},
    'aa_k6_floor': {'scored': 5471944, 'entries': 3483572, 'over_cap': 13, 'below_cap': 7, 'longest': 3555, 'tied': [229282, 1626875], 'cut': [0, 0], 'D1': 2448, 'D1_over_cap': 2448, 'D3': 19728, 'D3_over_cap': 19728},
    'dna_k10_long': {'scored': 9221756, 'entries': 2068037, 'over_cap': 1282, 'below_cap': 7100, 'longest': 963, 'tied': [163874, 178601], 'cut': [-1, -1], 'D4': 18502, 'D5_beyond_2048': 19967, 'D5_beyond_4096': 299},
}


def matrices(case):
    if case.family == "floor":
        return gen.tenth_floor_matrices(len(case.groups), case.sites, case.sigma, case.seed, case.heavy)
    if case.family == "long":
        if case.sigma == 20:                             # (plain tenth columns of 20 states nearly all have maximum 0)
            return gen.tenth_floor_matrices(len(case.groups), case.sites, case.sigma, case.seed, twins=False)
        return gen.tenth_matrices(len(case.groups), case.sites, case.sigma, case.seed)
    assert case.family == "tenth" and case.heavy == 0
    return gen.tenth_twin_matrices(len(case.groups), case.sites, case.sigma, case.seed)


@functools.lru_cache(maxsize=None)
def load(name):
    case = CASES[name]
    return case, matrices(case)


def group_order(case):
    return list(dict.fromkeys(case.groups.tolist()))


def oracle(name):
    """grid_paths.oracle: per group in first-seen order (gid, keys, score bits, positions, scored count)."""
    return gp.oracle(name)


@functools.lru_cache(maxsize=None)
def half_lists(name):
    """int64 [windows, 2]: (|L|, |R|) of every window (matrices in order), from the oracle's own list building with the matrix-wide
    prefix sums (ipk_oracle.window_halves)."""
    case, mats = load(name)
    out = []
    for m in mats:
        best = co.prefix_max(m)
        out += [co.window_halves(m, case.k, w, case.eps, best) for w in range(m.shape[0] - case.k + 1)]
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def cheap_counts(name):
    """What a GPU test can afford to assert before it runs: scored k-mers, entries, windows with a half list beyond the family's
    capacity and within it."""
    case, _ = load(name)
    res = oracle(name)
    out = dict(scored=sum(r[4] for r in res), entries=sum(len(r[1]) for r in res))
    cap = gp.family(case.sigma, case.k)[1]
    if cap:
        longest = half_lists(name).max(axis=1)
        out.update(over_cap=int((longest > cap).sum()), below_cap=int((longest <= cap).sum()), longest=int(longest.max()))
    return out


# ---- the deviations -------------------------------------------------------------------------------------------------------------------

def prefix_f64(m):
    """D4: the prefix sums of the column maxima accumulated in float64 and rounded to float32 once."""
    return np.concatenate([[0.0], np.cumsum(m.max(axis=1).astype(np.float64))]).astype(np.float32)


def prefix_chunked(m, chunk=CHUNK):
    """D5: the float prefix sum restarted at every multiple of `chunk` sites, the chunk's base added to each of its sums."""
    best = np.zeros(m.shape[0] + 1, dtype=np.float32)
    for a in range(0, m.shape[0], chunk):
        local = co.prefix_max(m[a:a + chunk])
        best[a + 1:a + len(local)] = best[a] + local[1:]          # float32 + float32, one rounding each
    return best


def prefix_window(m, k, w):
    """D3: the prefix sum restarted at the window's first column (only best[w .. w + k] is meaningful)."""
    best = np.zeros(m.shape[0] + 1, dtype=np.float32)
    best[w:w + k + 1] = co.prefix_max(m[w:w + k])
    return best


def window_keys(m, k, eps, windows=None, prefix=None, L=None):
    """The key set of every window in `windows` (all by default) of one matrix; `prefix`: None (matrix::preprocess), a prefix array
    or "window" (D3); `L`: a deviating oracle library (D1)."""
    best = co.prefix_max(m) if prefix is None else prefix
    windows = range(m.shape[0] - k + 1) if windows is None else windows
    return [co.window(m, k, w, eps, prefix_window(m, k, w) if isinstance(best, str) else best, L=L)[0] for w in windows]


def changed(a, b):
    """Per window: the size of the symmetric difference of two key sets."""
    return np.array([len(np.setxor1d(x, y, assume_unique=True)) for x, y in zip(a, b)], dtype=np.int64)


def inner_ge_library(out_dir):
    """D1: the oracle compiled so that joins below the top level keep `score >= bound`, into `out_dir`."""
    return co.build_deviating(out_dir, "IPKO_DEVIATE_INNER_GE")


def deviations(name, inner_ge):
    """Per deviation the scored k-mers it changes, per window (matrices in order) -- D1, D3 for the table's cases, D4 and D5 for
    the long one, whose windows are those from CHUNK - k + 1 on only (no earlier one reads a prefix sum beyond the first chunk)."""
    case, mats = load(name)
    out = collections.defaultdict(list)
    for m in mats:
        if case.family == "long":
            wins = range(CHUNK - case.k + 1, m.shape[0] - case.k + 1)
            ref = window_keys(m, case.k, case.eps, wins)
            out["D4"].append(changed(ref, window_keys(m, case.k, case.eps, wins, prefix_f64(m))))
            out["D5"].append(changed(ref, window_keys(m, case.k, case.eps, wins, prefix_chunked(m))))
        else:
            ref = window_keys(m, case.k, case.eps)
            out["D1"].append(changed(ref, window_keys(m, case.k, case.eps, L=inner_ge)))
            out["D3"].append(changed(ref, window_keys(m, case.k, case.eps, prefix="window")))
    return {d: np.concatenate(v) for d, v in out.items()}


# ---- ties and cut candidates ----------------------------------------------------------------------------------------------------------

def dc_scores(m, k, w, keys, bits):
    """float32 scores of the k-mers `keys` in window w, added in the order of DCLA::DC (halves h // 2 and h - h // 2, recursively)."""
    def rec(j, h):
        if h == 1:
            return m[w + j][(keys >> np.uint32(bits * (k - 1 - j))) & np.uint32((1 << bits) - 1)]
        return rec(j, h // 2) + rec(j + h // 2, h - h // 2)
    return rec(0, k)


def ties_and_cuts(name):
    """Per group: (keys whose kept score two or more windows reach, keys whose kept position is not the first window in which the
    candidate itself scores the kept score -- there a rounded bound cut it, and a later window, the twin's, keeps the position)."""
    case, mats = load(name)
    bits = co.bits(case.sigma)
    out = []
    for gid, keys, sbits, pos, _ in oracle(name):
        gm = mats[case.groups == gid]
        tied = gp.tied_keys(gp.window_lists(gm, case.k, case.eps), keys, sbits)
        if case.family == "long":                        # (thousands of windows times a million keys: not counted)
            out.append((tied, -1))
            continue
        first = np.full(len(keys), -1, dtype=np.int64)
        kept = sbits.view(np.float32)
        for m in gm:
            for w in range(m.shape[0] - case.k + 1):
                hit = (first < 0) & (dc_scores(m, case.k, w, keys, bits) == kept)
                first[hit] = w
        assert (first >= 0).all()
        out.append((tied, int((first != pos).sum())))
    return out


def describe(name, inner_ge):
    """Everything tests/test_rounded_paths_inputs.py asserts of a case and profiles/rounded_bounds_inputs.txt records."""
    case, _ = load(name)
    out = cheap_counts(name)
    tc = ties_and_cuts(name)
    out.update(tied=[t for t, _ in tc], cut=[c for _, c in tc])
    cap = gp.family(case.sigma, case.k)[1]
    for d, per_window in deviations(name, inner_ge).items():
        if case.family == "long":
            start = np.concatenate([np.arange(CHUNK - case.k + 1, case.sites - case.k + 1)] * len(case.groups))
            if d == "D4":
                out[d] = int(per_window.sum())
            else:
                out[d + "_beyond_2048"] = int(per_window[(start > CHUNK) & (start <= 2 * CHUNK)].sum())
                out[d + "_beyond_4096"] = int(per_window[start > 2 * CHUNK].sum())
        else:
            out[d] = int(per_window.sum())
            if cap:
                out[d + "_over_cap"] = int(per_window[half_lists(name).max(axis=1) > cap].sum())
    return out
