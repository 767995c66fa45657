"""Exact-sum inputs that reach every list-size path of the scoring kernels, shared by tests/test_grid_paths_inputs.py (CPU: the cases
are what they claim, and the oracle is pinned on them) and tests/test_gpu_grid_paths.py (GPU: every entry point against the oracle).
Not a test file.

Every value is float32 -0.25 * an integer (or -inf) and every threshold a multiple of -0.25, so every sum is exact in float32 and in
float64: many candidates score exactly eps, many half-list entries sit exactly on their half's bound, equal scores in different
windows and matrices are common -- and the path counts of `path_counts` are exact, not estimates."""
import collections
import functools

import numpy as np

from oracle import gen_ref_golden as gen
from oracle import ipk_oracle as co

GROUPS = np.array([7, 3, 7, 3], dtype=np.uint32)      # interleaved, ids not ascending; matrix 2 + i is matrix i one site further down
PERIOD = 37                                           # coprime to the 32-, 40- and 128-window tiles
BIG_CAP = 6144                                        # capped big-list capacity from DNA k = 13 (BIG_CAP_ENTRIES)
ROWS_CAP = 384                                        # fast capacity of the row-per-lane join (DNA k >= 11)


# ---- the exact classifier -----------------------------------------------------------------------------------------------------------

def split(k):
    """(LA, LB, RA, RB): the window's halves (k // 2 | rest) and their children, each halved the same way."""
    hl = k // 2
    hr = k - hl
    return hl // 2, hl - hl // 2, hr // 2, hr - hr // 2


def all_sums(cols):
    """float64 scores of all sigma^h h-mers over the h columns `cols`, first symbol most significant."""
    s = np.zeros(1)
    for c in cols:
        s = (s[:, None] + c[None, :].astype(np.float64)).ravel()
    return s


def half(cols, ha, hb, eps_h):
    """One half of a window under its threshold eps_h: (first child's list length, second child's, half-list length)."""
    ma, mb = cols[:ha].max(axis=1).astype(np.float64).sum(), cols[ha:].max(axis=1).astype(np.float64).sum()
    a, b = all_sums(cols[:ha]), all_sums(cols[ha:])
    a, b = a[a > eps_h - mb], b[b > eps_h - ma]                      # child lists: s > e - M(rest)
    return len(a), len(b), int(((a[:, None] + b[None, :]) > eps_h).sum())


def classify(mats, k, eps, cap=160):
    """Counts of windows per path of the DNA k = 8..10 kernel, in float64 (exact on grid inputs, close enough for counting elsewhere)."""
    la, lb, ra, rb = split(k)
    hl = la + lb
    n = dict(single=0, one_long=0, both_long=0, one_row=0, over_cap=0, cap_lists=[])
    for m in mats:
        cmax = m.max(axis=1).astype(np.float64)
        for w in range(m.shape[0] - k + 1):
            win = m[w:w + k]
            eps_l, eps_r = eps - cmax[w + hl:w + k].sum(), eps - cmax[w:w + hl].sum()   # s > eps - M(other half)
            nla, nlb, nl = half(win[:hl], la, lb, eps_l)
            nra, nrb, nr = half(win[hl:], ra, rb, eps_r)
            long_l, long_r = nla * nlb > 64, nra * nrb > 64
            n["single" if not (long_l or long_r) else "both_long" if long_l and long_r else "one_long"] += 1
            n["one_row"] += (long_l and nlb > 32) or (long_r and nrb > 32)
            n["over_cap"] += nl > cap or nr > cap
            n["cap_lists"].append((nl, nr))
    return n


def family(sigma, k):
    """The kernel family that scores (sigma, k), and the fast capacity of its half lists (None: a half list cannot overflow)."""
    if sigma == 20:
        return ("aa_stream", 512) if k <= 5 else ("aa_exact", 512)
    if k <= 7:
        return "tiles", None
    if k <= 10:
        return "quad", 160
    if k <= 12:
        return "rows", ROWS_CAP
    return "exact", BIG_CAP


def half_lists(mats, k, eps):
    """Per window of every matrix (matrices in order, windows in order): (|L|, |R|, candidates of L exactly on L's bound, of R on R's),
    int64 [n, 4], by dense enumeration of both halves in float64."""
    hl = k // 2
    out = []
    for m in mats:
        cmax = m.max(axis=1).astype(np.float64)
        for w in range(m.shape[0] - k + 1):
            eps_l, eps_r = eps - cmax[w + hl:w + k].sum(), eps - cmax[w:w + hl].sum()
            left, right = all_sums(m[w:w + hl]), all_sums(m[w + hl:w + k])
            out.append((int((left > eps_l).sum()), int((right > eps_r).sum()), int((left == eps_l).sum()), int((right == eps_r).sum())))
    return np.array(out, dtype=np.int64).reshape(-1, 4)


def path_counts(mats, sigma, k, eps):
    """Exact per-window path counts of a grid input: `windows`; `over_cap` / `below_cap` against the family's capacity (`family`);
    `mid` (DNA k >= 11: a half list of 385..6144 entries, none longer); `on_bound` (half-list candidates exactly on their half's
    threshold); `longest`; and for DNA k = 8..10 `single`, `one_long`, `both_long`, `one_row` as `classify` defines them."""
    _, cap = family(sigma, k)
    hls = half_lists(mats, k, eps)
    longest = hls[:, :2].max(axis=1)
    n = dict(windows=len(hls), on_bound=int(hls[:, 2:].sum()), longest=int(longest.max()))
    n["over_cap"] = int((longest > cap).sum()) if cap else 0
    n["below_cap"] = n["windows"] - n["over_cap"]
    if sigma == 4 and k >= 11:
        n["mid"] = int(((longest > ROWS_CAP) & (longest <= BIG_CAP)).sum())
    if sigma == 4 and 8 <= k <= 10:
        c = classify(mats, k, eps)
        assert c["cap_lists"] == [tuple(r) for r in hls[:, :2].tolist()]        # (the child bounds lose no pair of an exact input)
        n.update({p: int(c[p]) for p in ("single", "one_long", "both_long", "one_row")})
    return n


# ---- the cases ----------------------------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "name family sigma k sites eps ninf seed groups opts floors")


def _case(name, fam, sigma, k, sites, eps, ninf, seed, opts=(), **floors):
    return Case(name, fam, sigma, k, sites, float(eps), float(ninf), seed, GROUPS, dict(opts), floors)


SLICE = (("slice_long_lists", 1),)

QUAD = dict(single=10, one_long=10, both_long=10, one_row=10, over_cap=5)

# Found by a search over seeds, thresholds and -inf fractions on the CPU; recorded here, no test loops over seeds.  Conditions
# (tests/test_grid_paths_inputs.py asserts them, so a case that drifts off its path fails instead of passing idly):
#   - every floor of the case's last column (windows per path, see path_counts; max_longest is a ceiling on the longest half list);
#   - on_bound >= 1000 half-list candidates exactly on their half's threshold;
#   - >= 1000 candidates exactly on eps, by dense enumeration, where sigma^k <= 4^10;
#   - >= 50 keys per group whose kept score two or more windows reach; `periodic`: >= 50 whose tying windows lie in different
#     32-window tiles;
#   - at most 2 * 10^7 scored k-mers.
# DNA k = 8..10: 131 windows a matrix = 3 tiles of 40 and a tail of 11, one tile of 128 and a tail of 3.  k = 8 has no `one_row`
# floor: its second children have 2 symbols, at most 16 entries, and a row per step needs more than 32.  DNA k = 11, 12: 67 windows
# a matrix = 2 tiles of 32 and a tail of 3.  DNA k >= 13: 3 or 4 windows a matrix keep the volume down; `*_long` have half lists
# beyond BIG_CAP (scored with slice_long_lists = 1, refused without), `*_mid` none beyond it but some beyond ROWS_CAP.  AA: the
# uniform grid puts nearly every half list beyond 512 at any threshold that emits, so three entries in ten are -inf.
#                 name             family      sigma k  sites  eps   -inf  seed
CASES = {c.name: c for c in (
    _case("dna_k6",          "grid",     4,  6, 136, -3.0, 0.0, 1, below_cap=524),
    _case("dna_k8",          "grid",     4,  8, 138, -4.0, 0.0, 1, **dict(QUAD, one_row=0)),
    _case("dna_k9",          "grid",     4,  9, 139, -4.0, 0.0, 0, **QUAD),
    _case("dna_k10",         "grid",     4, 10, 140, -4.5, 0.0, 0, **QUAD),
    _case("dna_k10_periodic", "periodic", 4, 10, 140, -4.5, 0.0, 0, **QUAD),
    _case("dna_k11",         "grid",     4, 11,  77, -4.5, 0.1, 1, mid=10, below_cap=10),
    _case("dna_k12",         "grid",     4, 12,  78, -5.5, 0.1, 0, mid=10, below_cap=10),
    _case("dna_k13_mid",     "grid",     4, 13,  17, -7.0, 0.0, 0, mid=10, max_longest=BIG_CAP),
    _case("dna_k13_long",    "grid",     4, 13,  16, -8.5, 0.0, 2, SLICE, over_cap=3),
    _case("dna_k14_mid",     "grid",     4, 14,  18, -7.0, 0.0, 0, mid=10, max_longest=BIG_CAP),
    _case("dna_k14_long",    "grid",     4, 14,  17, -8.5, 0.1, 1, SLICE, over_cap=3),
    _case("dna_k15_long",    "grid",     4, 15,  18, -9.0, 0.0, 10, SLICE, over_cap=3),
    _case("aa_k5",           "grid",    20,  5,  20, -2.0, 0.3, 1, over_cap=10, below_cap=10),
    _case("aa_k6",           "grid",    20,  6,  14, -2.0, 0.3, 0, over_cap=10, below_cap=10),
)}
TENTH = _case("dna_k10_tenth", "tenth", 4, 10, 140, np.float32(-1.6), 0.0, 5)     # entries -0.1 * an integer: rounded inner bounds decide
MAX_SCORED = 2 * 10 ** 7
TENTH_OVER_CAP = 5                    # windows of TENTH with a half list beyond 160, at least

# The exact path counts of every case (path_counts), recorded: the GPU tests assert them before they call the engine.
COUNTS = {
    'dna_k6': {'windows': 524, 'on_bound': 4009, 'longest': 64, 'over_cap': 0, 'below_cap': 524},
    'dna_k8': {'windows': 524, 'on_bound': 12265, 'longest': 256, 'over_cap': 30, 'below_cap': 494, 'single': 250, 'one_long': 107, 'both_long': 167, 'one_row': 0},
    'dna_k9': {'windows': 524, 'on_bound': 13104, 'longest': 429, 'over_cap': 38, 'below_cap': 486, 'single': 340, 'one_long': 89, 'both_long': 95, 'one_row': 40},
    'dna_k10': {'windows': 524, 'on_bound': 21160, 'longest': 567, 'over_cap': 54, 'below_cap': 470, 'single': 274, 'one_long': 85, 'both_long': 165, 'one_row': 74},
    'dna_k10_periodic': {'windows': 524, 'on_bound': 20090, 'longest': 567, 'over_cap': 86, 'below_cap': 438, 'single': 291, 'one_long': 74, 'both_long': 159, 'one_row': 101},
    'dna_k11': {'windows': 268, 'on_bound': 10271, 'longest': 2516, 'over_cap': 12, 'below_cap': 256, 'mid': 12},
    'dna_k12': {'windows': 268, 'on_bound': 13729, 'longest': 1386, 'over_cap': 22, 'below_cap': 246, 'mid': 22},
    'dna_k13_mid': {'windows': 20, 'on_bound': 10643, 'longest': 3100, 'over_cap': 0, 'below_cap': 20, 'mid': 18},
    'dna_k13_long': {'windows': 16, 'on_bound': 14472, 'longest': 8203, 'over_cap': 3, 'below_cap': 13, 'mid': 13},
    'dna_k14_mid': {'windows': 20, 'on_bound': 11506, 'longest': 2727, 'over_cap': 0, 'below_cap': 20, 'mid': 16},
    'dna_k14_long': {'windows': 16, 'on_bound': 12783, 'longest': 10223, 'over_cap': 3, 'below_cap': 13, 'mid': 13},
    'dna_k15_long': {'windows': 16, 'on_bound': 29031, 'longest': 8394, 'over_cap': 5, 'below_cap': 11, 'mid': 11},
    'aa_k5': {'windows': 64, 'on_bound': 12130, 'longest': 1248, 'over_cap': 21, 'below_cap': 43},
    'aa_k6': {'windows': 36, 'on_bound': 10638, 'longest': 913, 'over_cap': 13, 'below_cap': 23},
}


def matrices(case):
    """The case's matrices [4, sites, sigma]: `grid` as gen_ref_golden.grid_matrices gives them; `periodic` repeats the first PERIOD
    columns of such a matrix, so windows w and w + PERIOD of a matrix score the same k-mers alike; `tenth` is tenth_matrices."""
    if case.family == "tenth":
        return gen.tenth_matrices(4, case.sites, case.sigma, case.seed)
    if case.family == "periodic":
        base = gen.grid_matrices(4, PERIOD, case.sigma, case.seed, case.ninf)
        return np.ascontiguousarray(base[:, np.arange(case.sites) % PERIOD])
    return gen.grid_matrices(4, case.sites, case.sigma, case.seed, case.ninf)


@functools.lru_cache(maxsize=None)
def load(name):
    """(case, matrices, exact path counts), computed once; of a case of either table, this one (and TENTH) or tests/rounded_paths.py's
    (whose sums round: no exact path counts)."""
    case = CASES.get(name) or {TENTH.name: TENTH}.get(name)
    if case is None:
        from tests import rounded_paths
        return rounded_paths.load(name) + (None,)
    mats = matrices(case)
    return case, mats, (path_counts(mats, case.sigma, case.k, case.eps) if case.family != "tenth" else None)


def group_order(case):
    return list(dict.fromkeys(case.groups.tolist()))


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Per group in first-seen order: (gid, keys, score bits, positions, scored count) from oracle.ipk_oracle.explore_group_pos
    (tests/test_grid_paths_inputs.py pins it to explore_group, to dense enumeration and to the reference's compiled code)."""
    case, mats, _ = load(name)
    out = []
    for gid in group_order(case):
        keys, scores, pos, emitted = co.explore_group_pos(mats[case.groups == gid], case.k, case.eps)
        out.append((gid, keys, scores.view(np.uint32), pos, int(emitted)))
    return out


def oracle_db(name):
    """The oracle's key-major database: (keys ascending, key offsets, branches, score bits, positions), a key's entries in group
    order (as tests/ref_fixtures.Fixture.db)."""
    res = oracle(name)
    keys = np.concatenate([r[1] for r in res])
    br = np.concatenate([np.full(len(r[1]), r[0], dtype=np.uint32) for r in res])
    rank = np.concatenate([np.full(len(r[1]), i, dtype=np.int64) for i, r in enumerate(res)])
    order = np.lexsort((rank, keys))
    uk, counts = np.unique(keys, return_counts=True)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return uk, off, br[order], np.concatenate([r[2] for r in res])[order], np.concatenate([r[3] for r in res])[order]


# ---- dense enumeration and ties -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dense_case(name, gid):
    """dense_group of one group of a case, computed once."""
    case, mats, _ = load(name)
    return dense_group(mats[case.groups == gid], case.k, case.eps, case.sigma)


def dense_group(mats, k, eps, sigma):
    """explore_group_pos by plain dense enumeration (gen_ref_golden.dense_window_scores): per key the max over the windows of the
    matrices in order, the first window on ties.  Returns (keys ascending, score bits, positions, scored count, candidates exactly
    on eps, keys whose kept score two or more windows reach)."""
    eps = np.float32(eps)
    best = np.full(sigma ** k, -np.inf, dtype=np.float32)
    pos = np.zeros(sigma ** k, dtype=np.uint32)
    reach = np.zeros(sigma ** k, dtype=np.uint16)
    emitted = on = 0
    for m in mats:
        for w in range(m.shape[0] - k + 1):
            s = gen.dense_window_scores(m, k, w)
            on += int((s == eps).sum())
            idx = np.flatnonzero(s > eps)
            emitted += len(idx)
            sv, bv = s[idx], best[idx]
            tie = idx[sv == bv]
            reach[tie] += 1
            up = idx[sv > bv]
            best[up], pos[up], reach[up] = s[up], w, 1
    rank = np.flatnonzero(reach > 0)
    keys = gen.dense_key(rank, k, sigma, co.bits(sigma))
    o = np.argsort(keys, kind="stable")
    return keys[o], best[rank][o].view(np.uint32), pos[rank][o], emitted, on, int((reach[rank] >= 2).sum())


def window_lists(mats, k, eps):
    """The oracle's per-window output of a group's matrices: (keys, scores, window, matrix) of every scored k-mer, concatenated in
    the order of the max-merge (matrices in order, windows in order)."""
    ks, ss, ws, ms = [], [], [], []
    for mi, m in enumerate(mats):
        best = co.prefix_max(m)
        for w in range(m.shape[0] - k + 1):
            keys, scores = co.window(m, k, w, eps, best)
            ks.append(keys); ss.append(scores)
            ws.append(np.full(len(keys), w, dtype=np.uint32)); ms.append(np.full(len(keys), mi, dtype=np.uint32))
    return np.concatenate(ks), np.concatenate(ss), np.concatenate(ws), np.concatenate(ms)


def tied_keys(lists, keys, bits, tile=None):
    """How many keys of a group (keys ascending, kept score bits) have their kept score reached by two or more windows; with `tile`,
    by two windows of one matrix that lie in different `tile`-window tiles."""
    allk, alls, allw, allm = lists
    hit = alls.view(np.uint32) == bits[np.searchsorted(keys, allk)]
    k_hit = allk[hit]
    if tile is None:
        _, cnt = np.unique(k_hit, return_counts=True)
        return int((cnt >= 2).sum())
    m_hit, t = allm[hit], allw[hit] // tile
    o = np.lexsort((t, m_hit, k_hit))
    k_hit, m_hit, t = k_hit[o], m_hit[o], t[o]
    first = np.flatnonzero(np.r_[True, (k_hit[1:] != k_hit[:-1]) | (m_hit[1:] != m_hit[:-1])])      # runs of one key in one matrix
    last = np.r_[first[1:], len(k_hit)] - 1
    return len(np.unique(k_hit[first[t[first] != t[last]]]))


def on_grid(mats, eps):
    """Every finite entry is -0.25 * an integer in 0..8 and +0.0 where zero, eps a multiple of 0.25: every sum is exact."""
    finite = mats[np.isfinite(mats)]
    return bool(np.array_equal(finite * 4, np.round(finite * 4)) and finite.min() >= -2.0 and finite.max() <= 0.0
                and not np.signbit(finite[finite == 0]).any() and not np.isposinf(mats).any() and eps * 4 == round(eps * 4))


def describe(name):
    """What tests/test_grid_paths_inputs.py asserts of a case and profiles/grid_paths_inputs.txt records: the exact path counts,
    the scored count, per group the keys whose kept score two or more windows reach (for `periodic` also those whose tying windows
    lie in different 32-window tiles), and -- where sigma^k <= 4^10 -- the candidates exactly on eps by dense enumeration (else -1).
    The per-window lists are merged here as the reference merges them (oracle.ref_build.merge_windows): the result must be the
    oracle's explore_group_pos."""
    from oracle import ref_build as rb
    case, mats, counts = load(name)
    out = dict(counts=counts, scored=0, tied=[], tied_across_tiles=[], on_eps=-1)
    for gid, keys, bits, pos, emitted in oracle(name):
        gm = mats[case.groups == gid]
        lists = window_lists(gm, case.k, case.eps)
        per_matrix = [[(0, lists[0][lists[3] == mi], lists[1][lists[3] == mi].view(np.uint32))] for mi in range(len(gm))]
        mk, ms, me = rb.merge_windows(per_matrix)
        assert np.array_equal(mk, keys) and np.array_equal(ms.view(np.uint32), bits) and me == emitted == len(lists[0]), (name, gid)
        first = lists[2][np.lexsort((np.arange(len(lists[0])), -lists[1], lists[0]))][np.r_[True, np.diff(np.sort(lists[0], kind="stable")) != 0]]
        assert np.array_equal(first, pos), (name, gid, "positions")
        out["scored"] += emitted
        out["tied"].append(tied_keys(lists, keys, bits))
        if case.family == "periodic":
            out["tied_across_tiles"].append(tied_keys(lists, keys, bits, tile=32))
    if case.sigma ** case.k <= 4 ** 10:
        out["on_eps"] = sum(dense_case(name, gid)[4] for gid in group_order(case))
    return out
