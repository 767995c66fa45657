"""CPU suite: the inputs of the ipkgpu_db_diff_files tests and the restatements they are checked against (tests/diff_files_cases.py) --
the bin rule, the memory formula and the greedy cut of include/ipkgpu.h restated in Python, the library's own host arithmetic against
them, and the properties the device tests count on: the base pair splits at its least budget, a cut falls between two keys only B holds,
the key beyond the code space lies in the last range, and the comparison composed over the planned ranges is the comparison of the whole."""
import ctypes
import os
import re

import numpy as np
import pytest

from ipk_amd import engine as E
from tests import diff_files_cases as D
from tests.test_gpu_db_diff import restate, same_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ipkgpu_db_load_key_range", "ipkgpu_db_diff_files", "ipkgpu_db_diff_files_num_ranges", "ipkgpu_db_diff_files_range",
       "ipkgpu_db_diff_files_stat", "ipkgpu_db_diff_files_range_bytes", "ipkgpu_db_stream_window_bytes"]


def test_the_library_exports_and_the_header_declares_the_entry_points():
    lib = ctypes.CDLL(os.path.join(ROOT, "ipk_amd", "libipkgpu.so"))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ipkgpu.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in E.ABI_SYMBOLS


def test_the_bin_rule():
    k5, k9, k16 = D.HEADER5, dict(D.HEADER5, kmer_size=9), dict(D.HEADER5, kmer_size=16)
    aa4, aa7, other = dict(D.HEADER5, sequence_type="AA", kmer_size=4), dict(D.HEADER5, sequence_type="AA", kmer_size=7), dict(D.HEADER5, sequence_type="RNA")
    assert [D.bits_of(h) for h in (k5, k9, k16, aa4, aa7, other)] == [10, 18, 32, 20, 32, 32]
    assert D.shift_of(k5, k5) == 0 and D.shift_of(k9, k9) == 2 and D.shift_of(k5, k9) == 2 and D.shift_of(aa4, k5) == 4 and D.shift_of(k16, k5) == 16
    assert D.bin_of(1010, 0) == 1010 and D.bin_of(D.OUTSIDE5, 0) == D.OUTSIDE5 and D.bin_of(70000, 0) == 65535
    assert D.bin_of(4 ** 9 - 1, 2) == 65535 and D.bin_of(4 ** 9, 2) == 65535 and D.bin_of(7, 2) == 1            # at or beyond 2^bits: the last bin
    assert D.bin_of(0xFFFFFFFF, 16) == 65535 and D.bin_of(65536, 16) == 1 and D.bin_of(65535, 16) == 0
    assert D.bin_interval(65535, 2) == (65535 << 2, 1 << 32) and D.bin_interval(3, 2) == (12, 16) and D.bin_interval(65535, 0) == (65535, 1 << 32)


def test_the_library_s_arithmetic_is_the_restated_formula():
    rng = np.random.default_rng(1)
    for _ in range(300):
        w, n_w, longest = (int(x) for x in (rng.integers(16, 1 << 20), rng.integers(0, 5000), rng.integers(0, 1 << 21)))
        assert E.stream_window_bytes(w, n_w, longest) == D.window_bytes(w, n_w, longest)
        scale = int(rng.choice([1, 10, 1000, 100000]))
        na, ea, nb, eb = (int(x) for x in rng.integers(0, 40, 4) * scale)
        pa, pb, mr = bool(rng.integers(2)), bool(rng.integers(2)), int(rng.choice([0, 5, 1 << 40]))
        fixed = int(rng.integers(0, 1 << 22))
        assert E.diff_files_range_bytes(fixed, na, ea, pa, nb, eb, pb, mr) == D.range_bytes(fixed, na, ea, pa, nb, eb, pb, mr)
    # monotone in every count: what lets a greedy cut stop at the first bin that does not fit
    base = (1000, 50, 700, True, 40, 900, False, 30)
    for i in (0, 1, 2, 4, 5, 7):
        more = list(base)
        more[i] += 17
        assert D.range_bytes(*more) >= D.range_bytes(*base)


def test_the_greedy_cut():
    cost = lambda na, ea, nb, eb: 10 + na + ea + nb + eb
    ha = {1: [1, 5], 2: [1, 5], 7: [1, 20], 9: [1, 1]}
    hb = {2: [1, 5], 8: [1, 1], 65535: [2, 2]}
    assert D.greedy(ha, hb, 0, cost, 10 ** 6) == [(0, D.TOP, 4, 31, 4, 8)]
    got = D.greedy(ha, hb, 0, cost, 31)
    assert got == [(0, 7, 2, 10, 1, 5), (7, 8, 1, 20, 0, 0), (8, D.TOP, 1, 1, 3, 3)]
    assert D.greedy(ha, hb, 4, cost, 31)[1][:2] == (7 << 4, 8 << 4)
    with pytest.raises(D.NoRoom) as ei:
        D.greedy(ha, hb, 0, cost, 30)
    assert ei.value.bin == 7 and ei.value.need == 31


@pytest.fixture(scope="module")
def pair():
    lists = D.base()["lists"]
    B = D.perturbed_base(D.all_names())
    return lists, B, D.Side(lists, True, D.WINDOW), D.Side(B, True, D.WINDOW)


def test_the_base_pair_splits_at_its_least_budget(pair):
    A, B, a, b = pair
    assert max(a.longest, b.longest) > D.WINDOW and a.n_w > 1                   # a record longer than the window, windows of several records
    least = D.least_budget(a, b, 0)
    ranges = D.plan(a, b, least, 0)
    assert len(ranges) >= 4
    key3000 = D.base()["by_len"][3000][0]
    assert any(lo == key3000 for lo, *_ in ranges)                              # (k = 5: shift 0, the key is its bin)
    assert ranges[0][0] == 0 and ranges[-1][1] == D.TOP and all(x[1] == y[0] for x, y in zip(ranges, ranges[1:]))
    with pytest.raises(D.NoRoom):
        D.plan(a, b, least - 1, 0)
    assert len(D.plan(a, b, 2 * least, 0)) < len(ranges)                         # twice the least: fewer ranges (here the whole pair fits) ...
    assert len(D.plan(a, b, 3 * least // 2, 0)) in range(2, len(ranges))          # ... one and a half times: fewer, and still split
    assert D.plan(a, b, 1 << 40, 0) == [(0, D.TOP, a.n, a.e, b.n, b.e)]
    # every range's counts are those of the lists restricted to it, and every range fits
    for lo, hi, na, ea, nb, eb in ranges:
        ra, rb = D.in_range(A, lo, hi), D.in_range(B, lo, hi)
        assert (na, ea, nb, eb) == (len(ra), sum(map(len, ra.values())), len(rb), sum(map(len, rb.values())))
    # the outside key lies in the last range, which ends at 2^32 and not at 4^5
    assert ranges[-1][0] <= D.OUTSIDE5 < ranges[-1][1] and D.OUTSIDE5 >= 4 ** 5 and D.OUTSIDE5 in A


def test_a_cut_falls_between_two_keys_only_b_holds(pair):
    A, B, a, b = pair
    only_b = sorted(set(B) - set(A))
    assert len(only_b) >= 3
    for mr in (0, 5, 1 << 30):                                                  # at the budgets the device tests use
        least = D.least_budget(a, b, mr)
        for avail in (least, 3 * least // 2):
            cuts = [lo for lo, *_ in D.plan(a, b, avail, mr)[1:]]
            assert any(x < c <= y for c in cuts for x, y in zip(only_b, only_b[1:])), (mr, avail)


@pytest.mark.parametrize("eps", [1e-2, 0.0])
def test_the_restatement_composed_over_the_planned_ranges_is_the_whole(pair, eps):
    A, B, a, b = pair
    for x, y, sx, sy in ((A, B, a, b), (B, A, b, a)):
        want_c, want_r = restate(x, y, eps, True)
        for factor in (1, 2):
            ranges = [(lo, hi) for lo, hi, *_ in D.plan(sx, sy, factor * D.least_budget(sx, sy, 0), 0)]
            got_c, got_r = D.composed(x, y, ranges, eps, True)
            assert got_c == want_c
            same_records(got_r, want_r)
    assert want_c["scores_differ"] > 0 and want_c["keys_only_a"] > 0 and want_c["keys_only_b"] > 0 and want_c["positions_differ"] > 0


def test_the_shifted_pairs_put_several_keys_into_one_bin():
    for name, (header, A, B) in D.shifted_pairs().items():
        shift = D.shift_of(header, header)
        assert shift > 0, name
        bins = [D.bin_of(k, shift) for k in sorted(set(A) | set(B))]
        assert len(set(bins)) < len(bins), name                                 # keys that differ only below the shift share a bin
        assert D.BINS - 1 in bins, name
        c, _ = restate(A, B, 1e-2, True)
        assert c["keys_only_a"] and c["keys_only_b"] and c["scores_differ"], name
    assert {0, 65535, 65536, 0xFFFF0000, 0xFFFFFFFF} <= set(D.shifted_pairs()["dna_k16"][1])
