"""The cases of tests/test_join_files_inputs.py (host) and tests/test_gpu_join_files.py / test_gpu_cli_join_files.py (device), and the
definitions of ipkgpu_db_join_files (include/ipkgpu.h) restated in plain Python: the memory formula phase by phase, the writer's piece,
the plan (the heads' shortcut, the histograms, the greedy cut over S shards) and the join composed over key ranges on the host.  The
bins, the window's bytes and the terms m, r, sort, scanx, db and load are tests/diff_files_cases.py's; the join and its cases are
tests/join_cases.py's.  Test infrastructure only: nothing under ipk_amd/ imports it."""
import functools

import numpy as np

from ipk_amd import dbfile
from oracle import ipk_oracle as co
from tests import db_files as F
from tests import diff_files_cases as D
from tests import join_cases as J
from tests import stream_cases as T

WINDOW = D.WINDOW                             # "db_load_window_bytes" of every case
TOP = D.TOP
K8 = J.K8
K16 = dict(F.HEADER, kmer_size=16)            # 32 key bits: shift 16, a bin holds 65 536 keys
N_NODES = 6001                                # MIF0's N of the cases (tests/test_gpu_db_join.py's)
PIECE_MIN, PIECE_MAX = 64 << 10, 256 << 20    # the clamp of the writer's piece


# ---- the formula ----------------------------------------------------------------------------------------------------------------------------

def scan_bytes(n):
    return n // 8 + 4096


def join_bytes(n, e, n_srcs, pos):
    """ipkgpu_db_join_bytes: what a join of n keys and e entries in all sources holds on top of them."""
    m, r = D.m, D.r
    keys_ws = (m(56 * (n_srcs + 1)) + m(8 * (n_srcs + 1)) + 3 * m(8 * n) + 3 * m(4 * n) + 2 * m(8 * (n + 1)) + m(D.sort_bytes(n)) + m(scan_bytes(max(n, e) + 1)) + 256
               + 2 * m(4 * J.BRANCH_SLOTS))
    dup_ws = (m(8 * (n + 1)) + m(8 * e) + (m(4 * e) if pos else 0) + m(4 * e) + m(8 * (e + 1)) + m(4 * (e // (J.WAVE_LIST + 1) + 1))
              + (4 * m(8 * e) + m(17 * e + 32768) if e > J.LDS_LIST else 0))
    result = r(4 * max(n, 1)) + r(8 * (n + 1)) + r(8 * max(e, 1)) + (r(4 * max(e, 1)) if pos else 0)
    return keys_ws + dup_ws + result


def phases(fixed, n, e, pos, write_piece, longest_joined):
    """The four phases of one range and the scans' term beside them: dict(loads, join, filter, write, scanx)."""
    N, E = sum(n), sum(e)
    resident, loads = 0, 0
    for ns, es in zip(n, e):
        loads = max(loads, fixed + resident + D.load_bytes(ns, es, pos))
        resident += D.db_bytes(ns, es, pos)
    joined = D.db_bytes(N, E, pos)
    body = 16 * N + (10 if pos else 8) * E
    return dict(loads=loads, join=resident + join_bytes(N, E, len(n), pos), filter=joined + 2 * max(8 * N, 16) + max(D.sort_bytes(N), 16),
                write=joined + D.m(4 * N) + D.m(8 * (N + 1)) + 2 * D.r(min(max(write_piece, longest_joined), body)), scanx=D.scanx(N + 1))


def range_bytes(fixed, n, e, pos, write_piece, longest_joined):
    p = phases(fixed, n, e, pos, write_piece, longest_joined)
    return max(p["loads"], p["join"], p["filter"], p["write"]) + p["scanx"]


def write_piece_of(avail):
    return min(max(avail // 16, PIECE_MIN), PIECE_MAX)


# ---- what the passes see of a shard --------------------------------------------------------------------------------------------------------

class Shard:
    """One shard file: its keys and entry counts in FILE order, and what a streamed pass at window `window` sees of it."""

    def __init__(self, keys, counts, positioned, window=WINDOW):
        self.keys, self.counts, self.pos = np.asarray(keys, np.int64), np.asarray(counts, np.int64), positioned
        self.sizes = (16 + (10 if positioned else 8) * self.counts).tolist()
        self.n, self.e, self.body = len(self.keys), int(self.counts.sum()), sum(self.sizes)
        self.window = max(min(window, self.body), 16)
        self.n_w = max([b - a for a, b in T.windows_of(self.sizes, self.window)] + [0])
        self.longest = max(self.sizes + [0])
        self.n_w_bound = min(self.n, max(self.window // 16, 1))                  # what the head alone tells
        self.longest_bound = min(self.body, 16 + (10 if positioned else 8) * self.e)

    @classmethod
    def of_arrays(cls, db, positioned, window=WINDOW):
        order = np.asarray(db["order"], np.int64)
        cnt = (db["off"][1:] - db["off"][:-1]).astype(np.int64)
        return cls(np.asarray(db["keys"], np.int64)[order], cnt[order], positioned, window)

    def histogram(self, shift):
        h = {}
        for key, c in zip(self.keys.tolist(), self.counts.tolist()):
            x = h.setdefault(D.bin_of(key, shift), [0, 0])
            x[0] += 1
            x[1] += c
        return h


def joined_bound(longest):
    """The bound of the longest joined record from the shards' longest records."""
    return 16 + sum(max(x - 16, 0) for x in longest)


def figures(shards, from_heads):
    """(fixed, longest_joined) from the heads' bounds, or as the histogram passes see them."""
    if from_heads:
        return max(D.window_bytes(s.window, s.n_w_bound, s.longest_bound) for s in shards), joined_bound([s.longest_bound for s in shards])
    return max(D.window_bytes(s.window, s.n_w, s.longest) for s in shards), joined_bound([s.longest for s in shards])


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------

class NoRoom(Exception):
    def __init__(self, b, need, interval):
        super().__init__(f"bin {b}, the keys [{interval[0]}, {interval[1]}), needs {need} bytes")
        self.bin, self.need, self.interval = b, need, interval


def fits_whole(shards, avail):
    """The heads' shortcut: one range [0, 2^32), no histogram pass."""
    if sum(s.n for s in shards) == 0:
        return True
    fixed, lj = figures(shards, True)
    return range_bytes(fixed, [s.n for s in shards], [s.e for s in shards], shards[0].pos, write_piece_of(avail), lj) <= avail


def plan(shards, avail, header):
    """The ranges of ipkgpu_db_join_files under `avail` bytes: [(lo, hi, [n_s], [e_s])]."""
    S, pos = len(shards), shards[0].pos
    if fits_whole(shards, avail):
        return [(0, TOP, [s.n for s in shards], [s.e for s in shards])]
    shift = D.shift_of(header, header)
    fixed, lj = figures(shards, False)
    wp = write_piece_of(avail)
    cost = lambda n, e: range_bytes(fixed, n, e, pos, wp, lj)
    hists = [s.histogram(shift) for s in shards]
    out, first, cur_n, cur_e = [], 0, [0] * S, [0] * S
    for b in sorted(set().union(*hists)):                                        # (a bin without a record adds nothing: it closes no range)
        add_n, add_e = [h.get(b, (0, 0))[0] for h in hists], [h.get(b, (0, 0))[1] for h in hists]
        if cost([x + y for x, y in zip(cur_n, add_n)], [x + y for x, y in zip(cur_e, add_e)]) > avail:
            if cost(add_n, add_e) > avail:
                raise NoRoom(b, cost(add_n, add_e), D.bin_interval(b, shift))
            out.append((D.bin_interval(first, shift)[0], D.bin_interval(b, shift)[0], cur_n, cur_e))
            first, cur_n, cur_e = b, [0] * S, [0] * S
        cur_n, cur_e = [x + y for x, y in zip(cur_n, add_n)], [x + y for x, y in zip(cur_e, add_e)]
    out.append((D.bin_interval(first, shift)[0], TOP, cur_n, cur_e))
    return out


def worst_range_bytes(shards, ranges, avail):
    """The formula's figure for the ranges of a plan: the heads' figures where the plan is the shortcut's."""
    fixed, lj = figures(shards, fits_whole(shards, avail))
    return max(range_bytes(fixed, n, e, shards[0].pos, write_piece_of(avail), lj) for _, _, n, e in ranges)


def _least_fixed_point(f):
    """The least A with f(A) <= A for a non-decreasing f whose values do not grow faster than A: the writer's piece is avail / 16."""
    a = f(0)
    while f(a) > a:
        a = f(a)
    return a


def least_budget(shards, header):
    """The least avail the plan accepts: the most any one bin needs, or the whole set at the heads' figures if that is less.  One byte
    less and the plan is NoRoom."""
    pos, shift = shards[0].pos, D.shift_of(header, header)
    hists = [s.histogram(shift) for s in shards]
    fixed, lj = figures(shards, False)
    bins = [([h.get(b, (0, 0))[0] for h in hists], [h.get(b, (0, 0))[1] for h in hists]) for b in sorted(set().union(*hists))]
    per_bin = _least_fixed_point(lambda a: max([range_bytes(fixed, n, e, pos, write_piece_of(a), lj) for n, e in bins] + [0]))
    fixed_h, lj_h = figures(shards, True)
    whole = _least_fixed_point(lambda a: range_bytes(fixed_h, [s.n for s in shards], [s.e for s in shards], pos, write_piece_of(a), lj_h))
    return min(per_bin, whole)


def whole_budget(shards):
    """The least avail under which the heads' shortcut holds."""
    fixed_h, lj_h = figures(shards, True)
    return _least_fixed_point(lambda a: range_bytes(fixed_h, [s.n for s in shards], [s.e for s in shards], shards[0].pos, write_piece_of(a), lj_h))


# ---- the join composed over key ranges, on the host ---------------------------------------------------------------------------------------

def in_range(db, lo, hi):
    """A shard's records with lo <= key < hi, as a shard."""
    return T.restrict(db, {k for k in map(int, db["keys"]) if lo <= k < hi}, True)


def restated_ranges(shards, ranges):
    """[J.restate of the shards' records in each range], for the ranges that hold a record."""
    return [J.restate([in_range(s, lo, hi) for s in shards]) for lo, hi, n, _ in ranges if sum(n)]


def filter_values(want, which, thr):
    """The filter values of a joined database on the host: the sequential MIF0 oracle over every key's scores with N_NODES, or the random
    filter's draw per k-mer code; as float32, the file's form."""
    off = want["off"].astype(np.int64)
    if which == "mif0":
        return np.array([co.mif0(want["sc"][off[i]:off[i + 1]], N_NODES, thr) for i in range(len(want["keys"]))], np.float64).astype(np.float32)
    return (dbfile.splitmix_unit(want["keys"]) if len(want["keys"]) else np.zeros(0)).astype(np.float32)


def records_in_file_order(want, fv):
    """[(sort code, key, filter bits, [(branch, score bits, position)])] of a filtered database in the order its file holds them."""
    off = want["off"].astype(np.int64)
    code = dbfile.filter_sort_code(fv, want["keys"])
    recs = [(int(code[i]), int(want["keys"][i]), int(np.float32(fv[i]).view(np.uint32)),
             [(int(want["br"][j]), int(want["sc"][j].view(np.uint32)), int(want["pos"][j])) for j in range(off[i], off[i + 1])]) for i in range(len(code))]
    return sorted(recs, key=lambda x: x[0])


def composed_file(shards, ranges, which, thr):
    """Per range: the restated join, its filter values, its records in filter order (a range file); then the host merge's rule over the
    range files -- always the record with the smallest (sort code, key) next.  The code's low word is the key, so one integer orders both."""
    files = [records_in_file_order(w, filter_values(w, which, thr)) for w in restated_ranges(shards, ranges)]
    out, at = [], [0] * len(files)
    while True:
        live = [i for i in range(len(files)) if at[i] < len(files[i])]
        if not live:
            return out
        i = min(live, key=lambda j: files[j][at[j]][0])
        out.append(files[i][at[i]])
        at[i] += 1


def whole_file(shards, which, thr):
    want = J.restate(shards)
    return records_in_file_order(want, filter_values(want, which, thr))


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------

STRADDLE_GAP = (120, 30000)                   # keys of `straddle` that no shard holds, between its first and second cluster
STRADDLE_DUP = 30000                          # its DUP_ROWS keys: STRADDLE_DUP + i
STRADDLE_ENTRYLESS = 30020                    # entry-less in every shard
LAST8 = 4 ** 8 - 1
STRADDLE_HEAVY = 150                          # entries per shard of its keys 0 and 65535: the bins that set the least budget, so a range holds a few dozen keys


def _own(s, key, n=3):
    """n entries of shard s for `key` with branches no other shard has (10000 (s + 1) + ...)."""
    return [(10000 * (s + 1) + (7 * key + j) % 5000, np.float32(-0.25 * ((key + 3 * j) % 23) - 0.5), (key + j) & 0xFFFF) for j in range(n)]


def straddle():
    """DNA k = 8 (every key a bin of its own), 3 shards.  Keys 0 .. 119 and 65416 .. 65535: held by two shards each, 0 and 65535 (the
    first and the last bin) by all three with 150 entries each, every shard with branches of its own -- no duplicate can exist there.  Keys 30000 .. 30010:
    join_cases.DUP_ROWS, branch 7 in two or three shards.  Key 30020: entry-less in every shard.  No shard holds a key in 120 .. 29999
    or 30021 .. 65415."""
    shards = []
    for s in range(3):
        keys, lists = [], []
        for key in range(0, 120):
            if key == 0 or key % 3 != s:
                keys.append(key); lists.append(_own(s, key, STRADDLE_HEAVY if key == 0 else 3))
        for i, (_, scores, _) in enumerate(J.DUP_ROWS):
            lst = [(20 + s, np.float32(-5.0), 1000 + 10 * s + i)]
            if scores[s] is not None:
                lst.append((7, np.float32(scores[s]), 100 * s + i))
            lst.append((30 + s, np.float32(-5.5), 2000 + 10 * s + i))
            keys.append(STRADDLE_DUP + i); lists.append(lst)
        keys.append(STRADDLE_ENTRYLESS); lists.append([])
        for key in range(LAST8 - 119, LAST8 + 1):
            if key == LAST8 or key % 3 != s:
                keys.append(key); lists.append(_own(s, key, STRADDLE_HEAVY if key == LAST8 else 2 + key % 3))
        shards.append(J.shard(keys, lists, seed=40 + s))
    return dict(name="straddle", header=K8, shards=shards)


TOP_SHARED = [0, (1 << 31) - 1, 1 << 31, 0xFFFFFFFF]


def top():
    """A k = 16 head (32 key bits, shift 16), 3 shards.  Keys 0, 2^31 - 1, 2^31 and 0xFFFFFFFF are in every shard -- 2^31 with branch 7
    in all three --, and each shard has keys of its own around them: the bins 0, 1, 32767, 32768, 32769 and 65535."""
    shards = []
    for s in range(3):
        keys = sorted(TOP_SHARED + [5 + s, 65535 - s, 65536 + s, (1 << 31) - 2 - s, (1 << 31) + 1 + s, (1 << 31) + 70000 + s, 0xFFFF0000 + s, 0xFFFFFFFE - s - 1])
        lists = []
        for key in keys:
            lst = _own(s, key % 100003, 4 + s)
            if key == 1 << 31:
                lst.insert(2, (7, np.float32([-3.0, -1.0, -2.0][s]), 50 + s))
            lists.append(lst)
        shards.append(J.shard(keys, lists, seed=50 + s))
    return dict(name="top", header=K16, shards=shards)


HEAVY_KEY = 30000


def heavy_bin():
    """DNA k = 8, 2 shards: three light keys and key 30000 with 3000 entries in each shard (one branch in both).  Its budget is one byte
    below the least the plan accepts: that bin alone needs more."""
    shards = []
    for s in range(2):
        heavy = [(3000 * s + j, np.float32(-0.001 * j - 0.5), j & 0xFFFF) for j in range(3000)]
        if s == 1:
            heavy[-1] = (5, np.float32(-0.25), 9)
        shards.append(J.shard([10, 20, HEAVY_KEY, 40000], [_own(s, 10), _own(s, 20), heavy, _own(s, 40000)], seed=60 + s))
    return dict(name="heavy_bin", header=K8, shards=shards)


OWN_CASES = ["straddle", "top"]
CASE_NAMES = J.CASE_NAMES + OWN_CASES


@functools.lru_cache(maxsize=None)
def case(name):
    """A case by name: join_cases' or this module's, with want = the restatement of the whole join.  Built once; not to be changed."""
    if name in J.CASE_NAMES:
        return J.case(name)
    c = {"straddle": straddle, "top": top, "heavy_bin": heavy_bin}[name]()
    c["want"] = J.restate(c["shards"])
    return c


@functools.lru_cache(maxsize=None)
def sides(name, positioned):
    return tuple(Shard.of_arrays(s, positioned) for s in case(name)["shards"])


@functools.lru_cache(maxsize=None)
def budget_of(name, positioned):
    """The budget a case is run under: the least the plan accepts; for heavy_bin one byte less."""
    least = least_budget(sides(name, positioned), case(name)["header"])
    return least - 1 if name == "heavy_bin" else least


def threshold_of(header):
    from ipk_amd import score_threshold
    return score_threshold(header["omega"], 4, header["kmer_size"])
