"""CPU: the cases of tests/rounded_paths.py are what they claim -- tenth-valued inputs on which a slip in the association of the
look-ahead bounds changes scored k-mers, in every kernel family's shape -- and the oracle that the GPU tests
(tests/test_gpu_rounded_paths.py) compare with agrees with itself on them.  tests/test_grid_paths_inputs.py pins it to the
reference's compiled code on the same names.  The floors here are conditions on the inputs, no measurement of the engine.  Needs
no GPU.

The deviations (rounded_paths.deviations), each the sum over windows of the symmetric difference of the window's key set:
  D1  joins below the top level keep `score >= bound` (oracle/ipk_oracle.c compiled with IPKO_DEVIATE_INNER_GE into a temporary
      directory; the default library is untouched)
  D3  the bounds from a prefix sum restarted at the window's first column
  D4  the prefix sums accumulated in float64 and rounded once            } the long case
  D5  the prefix sum restarted at every multiple of 2048 sites, base added }"""
import numpy as np
import pytest

from oracle import ipk_oracle as co
from tests import grid_paths as gp
from tests import long_lists as ll
from tests import rounded_paths as rp

NAMES = list(rp.CASES)
TABLE = [n for n in NAMES if n != rp.LONG]


@pytest.fixture(scope="module")
def inner_ge(tmp_path_factory):
    return rp.inner_ge_library(tmp_path_factory.mktemp("deviating_oracle"))


def test_the_table_holds_one_case_per_family():
    have = {(c.sigma, c.k) for n, c in rp.CASES.items() if n != rp.LONG}
    assert {(4, k) for k in (6, 7, 8, 9, 11, 12, 13, 14, 15)} | {(20, 6)} <= have and have & {(20, 4), (20, 5)}
    for k in (13, 14):                                # one case within the big-list cap and one beyond it, the latter sliced
        sliced = sorted(bool(c.opts.get("slice_long_lists")) for c in rp.CASES.values() if (c.sigma, c.k) == (4, k))
        assert sliced == [False, True]
    for n in TABLE:
        c = rp.CASES[n]
        assert c.groups.tolist() == [7, 3, 7, 3] and gp.group_order(c) == [7, 3]
        windows = c.sites - c.k + 1
        if c.sigma == 4 and c.k <= 10:
            assert windows == 131
        if c.sigma == 4 and c.k in (11, 12):
            assert windows == 67
        if c.sigma == 4 and c.k >= 13:
            assert c.k + 2 <= c.sites <= c.k + 6
    long = rp.CASES[rp.LONG]
    assert (long.sigma, long.k, long.family) == (4, 10, "long") and long.sites > 2 * rp.CHUNK + long.k
    assert long.groups.tolist() == [7, 3]                                    # one matrix a group, no twins
    assert set(rp.COUNTS) == set(rp.CASES)


def test_the_default_oracle_does_not_deviate(inner_ge):
    """The switch is off in the library every other test loads: on a case that D1 changes, the default build is not the deviating one."""
    case, mats = rp.load("dna_k6_floor")
    ref = rp.window_keys(mats[0], case.k, case.eps)
    assert rp.changed(ref, rp.window_keys(mats[0], case.k, case.eps, L=co.lib())).sum() == 0
    assert rp.changed(ref, rp.window_keys(mats[0], case.k, case.eps, L=inner_ge)).sum() > 0


@pytest.mark.parametrize("name", NAMES)
def test_conditions(name, inner_ge):
    case, mats = rp.load(name)
    # (a) tenth-valued entries, a tenth-valued threshold, shapes and twins
    ints = np.round(mats.astype(np.float64) * -10)
    assert np.array_equal(mats, np.float32(-0.1) * ints.astype(np.float32)) and not np.signbit(mats[mats == 0]).any()
    assert case.eps == float(np.float32(round(case.eps * 10) / 10))
    assert mats.shape == (len(case.groups), case.heavy + case.sites, case.sigma)
    if name != rp.LONG:
        assert np.array_equal(mats[2:, 1:], mats[:2, :-1])                  # the shifted twins of a group
    assert (mats[:, :case.heavy] < -99).all() and (mats[:, case.heavy + 1:] > -1).all()
    d = rp.describe(name, inner_ge)
    print(name, d)
    assert d == rp.COUNTS[name], f"{name}: the recorded counts moved: {d}"
    # (b)
    assert 0 < d["scored"] <= rp.MAX_SCORED
    # (c) the deviations decide (profiles/rounded_bounds_inputs.txt names the cases that meet one of D1, D3 only)
    if name == rp.LONG:
        assert min(d["D4"], d["D5_beyond_2048"], d["D5_beyond_4096"]) >= rp.DEVIATION_FLOOR
    else:
        assert min(d[x] for x in ("D1", "D3") if x not in rp.ONE_DEVIATION.get(name, ())) >= rp.DEVIATION_FLOOR
        assert len(rp.ONE_DEVIATION.get(name, ())) <= 1
    # (d) half lists on both sides of the family's fast capacity, by the oracle's own list building
    fam, cap = gp.family(case.sigma, case.k)
    if cap and name != rp.LONG:
        sizes = np.array([r[2:] for r in ll.longest_half_lists(mats, case.k, case.eps)]).max(axis=1)
        for over, below in ((d["over_cap"], d["below_cap"]), (int((sizes > cap).sum()), int((sizes <= cap).sum()))):
            if fam == "exact":
                assert (over >= 3) if case.opts.get("slice_long_lists") else (over == 0 and d["longest"] > gp.ROWS_CAP)
            else:
                assert over >= 5 and below >= 5
        if name not in rp.NONE_BEYOND_CAP and (fam != "exact" or case.opts.get("slice_long_lists")):
            assert max(d["D1_over_cap"], d["D3_over_cap"]) >= 1             # a deviation changes a window beyond the capacity
    # (e) ties across windows
    assert len(d["tied"]) == 2 and min(d["tied"]) >= rp.TIED_FLOOR


@pytest.mark.parametrize("name", NAMES)
def test_the_two_oracle_calls_agree(name):
    case, mats = rp.load(name)
    for gid, keys, bits, pos, emitted in rp.oracle(name):
        k2, s2, e2 = co.explore_group(mats[case.groups == gid], case.k, case.eps)
        assert np.array_equal(k2, keys) and np.array_equal(s2.view(np.uint32), bits) and e2 == emitted
        assert np.all(bits.view(np.float32) > np.float32(case.eps))
