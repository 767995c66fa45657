"""The cases of tests/test_diff_files_inputs.py (host) and tests/test_gpu_diff_files.py / test_gpu_cli_diff_files.py (device), and the
definitions of ipkgpu_db_diff_files (include/ipkgpu.h) restated in plain Python: the bin of a key, the memory formula, the greedy cut
of the key ranges, and the comparison composed over them.  Test infrastructure only: nothing under ipk_amd/ imports it."""
import copy
import functools

import numpy as np

from tests import db_files as F
from tests import stream_cases as T
from tests.test_gpu_db_diff import COUNTS, N_KEYS, PERTURB, as_arrays, as_lists, perturbed, restate

HEADER5 = dict(F.HEADER, kmer_size=5)         # DNA k = 5: 10 key bits, shift 0 -- the keys 10 .. 1010 are bins of their own
OUTSIDE5 = 4 ** 5 + 3                         # a key beyond the code space of k = 5
BINS = 1 << 16
TOP = 1 << 32


# ---- the definitions --------------------------------------------------------------------------------------------------------------------

def bits_of(header):
    per = {"DNA": 2, "AA": 5}.get(header["sequence_type"])
    return min(32, per * header["kmer_size"]) if per else 32


def shift_of(header_a, header_b):
    return max(0, max(bits_of(header_a), bits_of(header_b)) - 16)


def bin_of(key, shift):
    return min(int(key) >> shift, BINS - 1)


def bin_interval(b, shift):
    return (b << shift, TOP if b == BINS - 1 else (b + 1) << shift)


def m(x):
    return max(x, 256)


def r(x):
    return max((x + 255) // 256 * 256, 256)


def sort_bytes(n):
    return 9 * n + 32768


def scanx(n):
    s = n // 8 + 4096
    return s + s // 16 + 16


def window_bytes(window, n_w, longest):
    return (window + 32) + (longest + 32 if longest > window else 0) + 3 * m(8 * n_w) + 4 * m(4 * n_w) + 3 * m(8 * (n_w + 1)) + scanx(n_w + 1)


def db_bytes(n, e, pos):
    return 3 * r(4 * n) + r(8 * (n + 1)) + r(8 * n) + r(8 * e) + (r(4 * e) if pos else 0)


def load_bytes(n, e, pos):
    return 2 * m(8 * n) + 2 * m(4 * n) + m(8 * e) + (m(4 * e) if pos else 0) + db_bytes(n, e, pos) + 2 * m(8 * n) + m(4 * n) + m(sort_bytes(n))


def range_bytes(fixed, n_a, e_a, pos_a, n_b, e_b, pos_b, max_records):
    ws = 2 * max(4 * max(n_a, 1), 16) + max(8 * (n_a + 1), 16) + 2 * max(4 * max(n_b, 1), 16) + max(8 * (n_b + 1), 16) + 64
    diff = db_bytes(n_a, e_a, pos_a) + db_bytes(n_b, e_b, pos_b) + ws + r(16 * min(max_records, e_a + e_b))
    return max(fixed + load_bytes(n_a, e_a, pos_a), fixed + db_bytes(n_a, e_a, pos_a) + load_bytes(n_b, e_b, pos_b), diff) + scanx(max(n_a, n_b) + 1)


def hist_pass_bytes(window, n_w, longest):
    """During a histogram pass: the histograms (beside the budget, but counted), the window and the heads' workspaces."""
    return BINS * 12 + (window + 32) + (longest + 32 if longest > window else 0) + 2 * m(8 * n_w) + 2 * m(4 * n_w)


class NoRoom(Exception):
    def __init__(self, b, need):
        super().__init__(f"bin {b} needs {need} bytes")
        self.bin, self.need = b, need


def histogram(lists, shift):
    """{bin: [records, entries]} of a database given as {key: entries}"""
    h = {}
    for key, lst in lists.items():
        c = h.setdefault(bin_of(key, shift), [0, 0])
        c[0] += 1
        c[1] += len(lst)
    return h


def greedy(hist_a, hist_b, shift, cost, avail):
    """[(lo, hi, n_a, e_a, n_b, e_b)]: from bin 0 upward, a range is closed before the first bin whose addition takes cost() beyond avail."""
    out, first, cur = [], 0, [0, 0, 0, 0]
    for b in sorted(set(hist_a) | set(hist_b)):                   # (an empty bin adds nothing: it never closes a range)
        add = list(hist_a.get(b, (0, 0))) + list(hist_b.get(b, (0, 0)))
        if cost(*[x + y for x, y in zip(cur, add)]) > avail:
            if cost(*add) > avail:
                raise NoRoom(b, cost(*add))
            out.append((bin_interval(first, shift)[0], bin_interval(b, shift)[0], *cur))
            first, cur = b, [0, 0, 0, 0]
        cur = [x + y for x, y in zip(cur, add)]
    if cost(*cur) > avail:                                        # (two empty files under a budget below the fixed part)
        raise NoRoom(0, cost(*cur))
    out.append((bin_interval(first, shift)[0], TOP, *cur))
    return out


class Side:
    """One file of a comparison: its lists, whether it is positioned, and what the streamed passes see of it at window `window`."""

    def __init__(self, lists, positioned, window, arrays=None):
        self.lists, self.pos = lists, positioned
        self.db = (arrays or as_arrays)(lists) if lists else F.synthetic(keys=[], counts=[])
        self.sizes = T.record_sizes(self.db, positioned)
        self.n, self.e, self.body = len(lists), sum(map(len, lists.values())), sum(self.sizes)
        self.window = max(min(window, self.body), 16)
        self.n_w = max([b - a for a, b in T.windows_of(self.sizes, self.window)] + [0])
        self.longest = max(self.sizes + [0])
        # what the heads alone tell
        self.n_w_bound = min(self.n, max(self.window // 16, 1))
        self.longest_bound = min(self.body, 16 + (10 if positioned else 8) * self.e)


def default_window(avail):
    return min(max(avail // 16, 4096), 256 << 20)


def needs_histogram(a, b, avail, max_records):
    """Whether the pair at the heads' totals (n_w and the longest record bounded from the heads) exceeds `avail`: then each file gets a
    histogram pass, and one pass per range -- even where the cut, with the passes' own figures, then makes one range of everything."""
    fixed = max(window_bytes(s.window, s.n_w_bound, s.longest_bound) for s in (a, b))
    return range_bytes(fixed, a.n, a.e, a.pos, b.n, b.e, b.pos, max_records) > avail


def plan(a, b, avail, max_records, header_a=HEADER5, header_b=HEADER5):
    """The ranges of ipkgpu_db_diff_files for the sides a and b under `avail` bytes: [(lo, hi, n_a, e_a, n_b, e_b)]."""
    fixed = max(window_bytes(s.window, s.n_w_bound, s.longest_bound) for s in (a, b))
    if range_bytes(fixed, a.n, a.e, a.pos, b.n, b.e, b.pos, max_records) <= avail:
        return [(0, TOP, a.n, a.e, b.n, b.e)]
    shift = shift_of(header_a, header_b)
    fixed = max(window_bytes(s.window, s.n_w, s.longest) for s in (a, b))
    cost = lambda na, ea, nb, eb: range_bytes(fixed, na, ea, a.pos, nb, eb, b.pos, max_records)
    return greedy(histogram(a.lists, shift), histogram(b.lists, shift), shift, cost, avail)


def least_budget(a, b, max_records, header_a=HEADER5, header_b=HEADER5):
    """The least avail under which the pair is compared: the most any one bin needs (or the whole pair, if that is less)."""
    shift = shift_of(header_a, header_b)
    ha, hb = histogram(a.lists, shift), histogram(b.lists, shift)
    fixed = max(window_bytes(s.window, s.n_w, s.longest) for s in (a, b))
    per_bin = max([range_bytes(fixed, *ha.get(x, (0, 0)), a.pos, *hb.get(x, (0, 0)), b.pos, max_records) for x in set(ha) | set(hb)]
                  + [range_bytes(fixed, 0, 0, a.pos, 0, 0, b.pos, max_records)])
    fixed_whole = max(window_bytes(s.window, s.n_w_bound, s.longest_bound) for s in (a, b))
    return min(per_bin, range_bytes(fixed_whole, a.n, a.e, a.pos, b.n, b.e, b.pos, max_records))


def in_range(lists, lo, hi):
    return {k: v for k, v in lists.items() if lo <= k < hi}


def composed(lists_a, lists_b, ranges, eps, positions, max_records=None):
    """restate over the ranges: the counts added, max_abs_diff the maximum, the records one behind the other (the first max_records)."""
    total, recs = None, []
    for lo, hi in ranges:
        c, rec = restate(in_range(lists_a, lo, hi), in_range(lists_b, lo, hi), eps, positions)
        recs.append(rec)
        if total is None:
            total = c
        else:
            d = max(np.float32(total["max_abs_diff"]), np.float32(c["max_abs_diff"]))
            total = {k: total[k] + c[k] for k in total}
            total["max_abs_diff"] = float(d)
    rec = np.concatenate(recs)
    return total, rec if max_records is None else rec[:max_records]


# ---- the base pair: tests/test_gpu_db_diff.py's lists, and a key beyond the code space -----------------------------------------------------

WINDOW = 2048                                 # "db_load_window_bytes" of the comparisons: several windows, the long records each longer than one


@functools.lru_cache(maxsize=None)
def base():
    """dict(lists, by_len) as the `base` fixture of tests/test_gpu_db_diff.py makes them (without its loads), plus OUTSIDE5."""
    rng = np.random.default_rng(21)
    keys = np.sort(rng.choice(np.arange(10, 1000), size=N_KEYS, replace=False))
    counts = rng.integers(1, 9, size=N_KEYS)
    at = rng.permutation(np.arange(1, N_KEYS - 1))[:len(COUNTS)]
    counts[at] = COUNTS
    lists = as_lists(F.synthetic(keys=keys, counts=counts, seed=22))
    by_len = {}
    for i, n in zip(at, COUNTS):
        by_len.setdefault(n, []).append(int(keys[i]))
    lists[OUTSIDE5] = [[11, np.float32(-1.25), 7], [12, np.float32(-2.25), 8], [13, np.float32(-0.5), 9]]
    return dict(lists=lists, by_len=by_len)


def perturbed_base(names):
    """The base lists with the perturbations of tests/test_gpu_db_diff.PERTURB; "last_key" takes the outside key away, so one more
    change is made to it where it stays."""
    B = perturbed(base(), names)
    if OUTSIDE5 in B and len(names) > 1:
        B[OUTSIDE5][1][1] = np.float32(-3.5)
    return B


def all_names():
    return list(PERTURB)


# ---- keys above 16 bits: small fabricated pairs ---------------------------------------------------------------------------------------------

def shifted_pairs():
    """{name: (header, lists_a, lists_b)}: pairs whose bins hold several keys (shift > 0)."""
    rng = np.random.default_rng(5)

    def lst(n, salt=0):
        return [[int(b), np.float32(-0.25 * (b % 17) - salt), int(b % 50)] for b in rng.permutation(300)[:n]]

    out = {}
    k9 = 4 ** 9
    keys = [0, 1, 2, 3, 4, 5, 6, 7, 1000, 1001, 1002, 1003, 70000, 70001, 70002, k9 - 4, k9 - 3, k9 - 2, k9 - 1, k9, k9 + 5]
    a = {k: lst(3 + k % 5) for k in keys}
    b = copy.deepcopy(a)
    del b[1]; del b[1002]; del b[k9 - 1]
    b[70003] = lst(4); b[k9 + 6] = lst(2)
    b[2][0][1] = np.float32(b[2][0][1] - 1); b[k9 - 2][-1][1] = np.float32(b[k9 - 2][-1][1] + 2); b[k9][0][1] = np.float32(9)
    out["dna_k9"] = (dict(F.HEADER, kmer_size=9), a, b)
    keys = [0, 15, 16, 17, 31, 32, 5000, 5001, 20 ** 4 - 1, 20 ** 4, (1 << 20) - 1, 1 << 20]
    a = {k: lst(2 + k % 7) for k in keys}
    b = copy.deepcopy(a)
    del b[16]; del b[1 << 20]
    b[33] = lst(5); b[5001][0][1] = np.float32(1)
    out["aa_k4"] = (dict(F.HEADER, sequence_type="AA", kmer_size=4), a, b)
    keys = [0, 65535, 65536, 0xFFFF0000, 0xFFFFFFFF]
    a = {k: lst(6) for k in keys}
    b = copy.deepcopy(a)
    b[65536][2][1] = np.float32(0.125); del b[0xFFFFFFFF][0]; b[0xFFFF0001] = lst(3); del b[65535]
    out["dna_k16"] = (dict(F.HEADER, kmer_size=16), a, b)
    return out


# ---- many short records: more than 256 in one window, and a pair for the budget ------------------------------------------------------------

def many_records(n, seed, k=8, per_key=3):
    """{key: entries} of n keys of DNA k, per_key entries each (made without a permutation per key: n may be large)."""
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.choice(4 ** k, size=n, replace=False))
    first = rng.integers(0, 3000, size=n)
    sc = (-6.0 * rng.random((n, per_key))).astype(np.float32)
    return {int(key): [[int(first[i]) + j, sc[i, j], (i + j) & 0xFFFF] for j in range(per_key)] for i, key in enumerate(keys)}


def fast_arrays(lists, seed=3):
    """as_arrays for many keys: the arrays straight from the lists (F.synthetic draws a permutation per key)."""
    # (defined last, used by Side(arrays=fast_arrays))
    from ipk_amd import dbfile
    keys = np.array(sorted(lists), np.uint32)
    counts = np.array([len(lists[int(k)]) for k in keys], np.int64)
    flat = [e for k in keys for e in lists[int(k)]]
    rng = np.random.default_rng(seed)
    fv = (rng.random(len(keys)) * 4.0 - 2.0).astype(np.float32)
    return dict(keys=keys, off=np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), br=np.array([e[0] for e in flat], np.uint32),
                sc=np.array([e[1] for e in flat], np.float32), pos=np.array([e[2] for e in flat], np.uint32), fv=fv,
                order=np.argsort(dbfile.filter_sort_code(fv, keys), kind="stable").astype(np.uint32))
