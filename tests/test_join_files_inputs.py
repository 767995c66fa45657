"""CPU suite: the inputs of the ipkgpu_db_join_files tests and the restatements they are checked against (tests/join_files_cases.py) --
the library's host arithmetic against the restated formula, the formula's monotony and its phases, the properties of the cases under the
restated plan alone (how many ranges, which of them hold duplicates, where the shared keys lie, the bin that does not fit), and the
composition argument on the host: per range the restated join, the filter and the order, then the host merge's rule, is the whole."""
import ctypes
import os
import re

import numpy as np
import pytest

from ipk_amd import engine as E
from tests import diff_files_cases as D
from tests import join_cases as J
from tests import join_files_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ipkgpu_db_join_files", "ipkgpu_db_join_files_range_bytes", "ipkgpu_db_join_files_num_ranges", "ipkgpu_db_join_files_range", "ipkgpu_db_join_files_stat"]
KINDS = [False, True]


def test_the_library_exports_and_the_header_declares_the_entry_points():
    lib = ctypes.CDLL(os.path.join(ROOT, "ipk_amd", "libipkgpu.so"))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ipkgpu.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in E.ABI_SYMBOLS
    assert len(E.JOIN_FILES_STATS) == 15


def random_args(rng):
    scale = int(rng.choice([1, 10, 1000, 100000]))
    S = int(rng.integers(1, 6))
    n, e = [int(x) for x in rng.integers(0, 40, S) * scale], [int(x) for x in rng.integers(0, 40, S) * scale]
    return int(rng.integers(0, 1 << 22)), n, e, bool(rng.integers(2)), int(rng.choice([X.PIECE_MIN, 1 << 20, X.PIECE_MAX])), int(rng.integers(16, 1 << 21))


def test_the_library_s_arithmetic_is_the_restated_formula():
    rng = np.random.default_rng(2)
    for _ in range(300):
        fixed, n, e, pos, wp, lj = random_args(rng)
        assert E.join_bytes(sum(n), sum(e), len(n), pos) == X.join_bytes(sum(n), sum(e), len(n), pos)
        assert E.join_files_range_bytes(fixed, n, e, pos, wp, lj) == X.range_bytes(fixed, n, e, pos, wp, lj)


def test_the_formula_is_monotone_and_at_least_each_phase():
    rng = np.random.default_rng(3)
    for _ in range(200):
        fixed, n, e, pos, wp, lj = random_args(rng)
        whole = X.range_bytes(fixed, n, e, pos, wp, lj)
        p = X.phases(fixed, n, e, pos, wp, lj)
        for name in ("loads", "join", "filter", "write"):
            assert whole >= p[name] + p["scanx"], name
        # every phase holds what stays resident in it: the shards loaded so far, all of them, the join
        assert p["loads"] >= fixed + sum(D.db_bytes(a, b, pos) for a, b in zip(n[:-1], e[:-1])) + D.load_bytes(n[-1], e[-1], pos)
        assert p["join"] >= sum(D.db_bytes(a, b, pos) for a, b in zip(n, e)) + X.join_bytes(sum(n), sum(e), len(n), pos)
        assert p["filter"] > D.db_bytes(sum(n), sum(e), pos) and p["write"] > D.db_bytes(sum(n), sum(e), pos)
        # The write is never the largest phase: the join holds the sources (at least db of the sums) and, by its bound, more than 72 bytes
        # a key and 28 an entry beside them, the write 44 and 16 with a whole body staged twice.  So the piece, which bounds what the
        # writer really takes, cannot move the formula's value.
        assert p["write"] <= p["join"]
        for s in range(len(n)):                                            # monotone in every n and every e: what lets the greedy cut stop
            for which in (n, e):
                more_n, more_e = list(n), list(e)
                (more_n if which is n else more_e)[s] += int(rng.choice([1, 17, 4097]))
                assert X.range_bytes(fixed, more_n, more_e, pos, wp, lj) >= whole
        assert X.range_bytes(fixed + 5, n, e, pos, wp, lj) >= whole and X.range_bytes(fixed, n, e, pos, wp * 2, lj) >= whole
        assert X.range_bytes(fixed, n, e, pos, wp, lj * 2) >= whole
    # the writer's staging is in it: with a body beyond the piece the write phase grows with the piece, two buffers of it
    n, e = [1000, 1000], [40000, 40000]
    small, large = X.phases(0, n, e, False, 1 << 16, 16), X.phases(0, n, e, False, 1 << 18, 16)
    assert large["write"] - small["write"] == 2 * ((1 << 18) - (1 << 16))
    assert X.phases(0, n, e, False, 1 << 16, 1 << 18)["write"] == large["write"]          # the piece is raised to the longest joined record


def test_the_writer_s_piece_and_the_joined_bound():
    assert X.write_piece_of(0) == X.write_piece_of(16 * (64 << 10)) == 64 << 10 and X.write_piece_of(16 * (64 << 10) + 16) == (64 << 10) + 1
    assert X.write_piece_of(1 << 40) == 256 << 20
    assert X.joined_bound([0, 0]) == 16 and X.joined_bound([16 + 80, 0, 16 + 24]) == 16 + 104


@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_every_case_is_planned_and_bounded(name, positioned):
    """At its budget every case has a plan whose ranges tile [0, 2^32), hold the shards' totals, each fit the budget -- and one byte less
    is no plan at all.  The cases stay small."""
    c, shards = X.case(name), X.sides(name, positioned)
    budget = X.budget_of(name, positioned)
    ranges = X.plan(shards, budget, c["header"])
    assert ranges[0][0] == 0 and ranges[-1][1] == X.TOP and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    for s in range(len(shards)):
        assert sum(r[2][s] for r in ranges) == shards[s].n and sum(r[3][s] for r in ranges) == shards[s].e
    assert all(sum(r[2]) > 0 for r in ranges) or sum(s.n for s in shards) == 0     # the greedy cut opens every range with a bin that holds a record
    assert X.worst_range_bytes(shards, ranges, budget) <= budget
    with pytest.raises(X.NoRoom):
        X.plan(shards, budget - 1, c["header"])
    assert len(X.plan(shards, X.whole_budget(shards), c["header"])) == 1 and X.fits_whole(shards, X.whole_budget(shards))
    assert len(c["want"]["keys"]) <= 4096 and sum(len(s["br"]) for s in c["shards"]) <= 61000


def routes_and_drops(name, ranges):
    return [(w["route"], w["dropped"]) for w in X.restated_ranges(X.case(name)["shards"], ranges)]


@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
def test_straddle(positioned):
    """At least 3 ranges; the keys all shards hold lie in the first and in the last bin; one range's lists hold DUP_ROWS' duplicates and
    take route 1, others hold none and take route 0; key 30020 is entry-less in every shard; and no shard holds a key in the gaps.

    A case with an interior range WITHOUT a record of any shard was wanted too.  The plan -- ipkgpu_db_diff_files' greedy cut -- cannot
    make one: a range is opened by the bin whose addition did not fit, and that bin holds a record.  So the record-less key
    intervals of this case (120 .. 29999 and 30021 .. 65415, tens of thousands of empty bins each) lie INSIDE ranges, which is what is
    checked here; the library's skip of a record-less range cannot be reached through a plan and has no test."""
    c, shards = X.case("straddle"), X.sides("straddle", positioned)
    ranges = X.plan(shards, X.budget_of("straddle", positioned), c["header"])
    assert len(ranges) >= 3
    per = [J.lists_of(s) for s in c["shards"]]
    in_all = [k for k in per[0] if all(k in p for p in per)]
    assert 0 in in_all and X.LAST8 in in_all
    assert D.bin_of(0, 0) == 0 and ranges[0][0] <= 0 < ranges[0][1] and D.bin_of(X.LAST8, 0) == D.BINS - 1 and ranges[-1][0] <= X.LAST8 < ranges[-1][1]
    got = routes_and_drops("straddle", ranges)
    with_dups = [i for i, (route, dropped) in enumerate(got) if dropped]
    assert with_dups and all(got[i][0] == 1 for i in with_dups)
    assert sum(d for _, d in got) == c["want"]["dropped"] == sum(sum(x is not None for x in row[1]) - 1 for row in J.DUP_ROWS)
    assert got[0] == (0, 0) and got[-1] == (0, 0) and 0 < sum(r for r, _ in got) < len(got)          # the route differs between ranges
    assert all(X.STRADDLE_ENTRYLESS in p and p[X.STRADDLE_ENTRYLESS] == [] for p in per)
    for lo, hi in (X.STRADDLE_GAP, (X.STRADDLE_ENTRYLESS + 1, X.LAST8 - 119)):
        assert not any(lo <= k < hi for p in per for k in p)
        assert sum(r[0] < lo and hi <= r[1] for r in ranges) == 1               # the whole interval inside one range
    # every cut falls on a key some shard holds: the empty bins close no range
    assert all(any(r[0] in p for p in per) for r in ranges[1:])


@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
def test_top(positioned):
    c, shards = X.case("top"), X.sides("top", positioned)
    assert D.bits_of(c["header"]) == 32 and D.shift_of(c["header"], c["header"]) == 16
    per = [J.lists_of(s) for s in c["shards"]]
    assert all(k in p for k in X.TOP_SHARED for p in per)
    assert [D.bin_of(k, 16) for k in X.TOP_SHARED] == [0, 32767, 32768, 65535]
    ranges = X.plan(shards, X.budget_of("top", positioned), c["header"])
    assert len(ranges) >= 2 and ranges[-1][1] == 1 << 32 and ranges[-1][0] <= 0xFFFFFFFF
    assert all(r[0] % 65536 == 0 for r in ranges)                               # cuts fall on bins of 65 536 keys
    assert c["want"]["dropped"] == 2 and c["want"]["shared_keys"] == 4


@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
def test_heavy_bin(positioned):
    c, shards = X.case("heavy_bin"), X.sides("heavy_bin", positioned)
    budget = X.budget_of("heavy_bin", positioned)
    assert not X.fits_whole(shards, budget)
    with pytest.raises(X.NoRoom) as ei:
        X.plan(shards, budget, c["header"])
    assert ei.value.bin == X.HEAVY_KEY and ei.value.interval == (X.HEAVY_KEY, X.HEAVY_KEY + 1) and budget < ei.value.need <= budget + 1
    # the light bins alone would fit: it is that bin, not the budget as such
    light = [X.Shard(s.keys[s.keys != X.HEAVY_KEY], s.counts[s.keys != X.HEAVY_KEY], positioned) for s in shards]
    assert X.least_budget(light, c["header"]) < budget


@pytest.mark.parametrize("which", ["mif0", "random"])
@pytest.mark.parametrize("name", ["straddle", "top"])
def test_the_join_composes_over_the_planned_ranges(name, which):
    """Per range join_cases.restate, the filter (the sequential MIF0 oracle with the WHOLE tree's N; the random filter's draw per code)
    and the order; then the host merge by (filter sort code, key): the records of the whole restatement, filtered and ordered, one by
    one -- keys, filter bits, branches, score bits and positions."""
    c = X.case(name)
    ranges = X.plan(X.sides(name, True), X.budget_of(name, True), c["header"])
    assert len(ranges) >= 2
    thr = X.threshold_of(c["header"])
    got, want = X.composed_file(c["shards"], ranges, which, thr), X.whole_file(c["shards"], which, thr)
    assert len(want) == len(c["want"]["keys"]) and got == want
    # (and the order is a matter of the filter: the records do not simply ascend by key)
    assert [r[1] for r in want] != sorted(r[1] for r in want)
