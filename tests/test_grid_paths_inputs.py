"""CPU: the cases of tests/grid_paths.py are what they claim -- exact-sum inputs whose windows reach every list-size path of the
scoring kernels with candidates exactly on the bounds and scores that tie across windows -- and the oracle that the GPU tests
(tests/test_gpu_grid_paths.py) compare with is pinned on them: to plain dense enumeration where that reaches, and to the
reference's compiled code where its binaries are present.  Needs no GPU."""
import numpy as np
import pytest

from oracle import gen_ref_golden as gen
from oracle import ipk_oracle as co
from oracle import ref_build as rb
from tests import grid_paths as gp
from tests import long_lists as ll
from tests import rounded_paths as rp

needs_binaries = pytest.mark.skipif(not rb.available(), reason="the reference binaries are not in oracle/_ref/ "
                                    "(oracle.ref_build.build() found no reference tree and none were carried along)")
NAMES = list(gp.CASES)
DENSE = [n for n in NAMES if gp.CASES[n].sigma ** gp.CASES[n].k <= 4 ** 10]
TWO_WINDOWS = [n for n in NAMES if 4 ** 10 < gp.CASES[n].sigma ** gp.CASES[n].k <= gen.DENSE_LIMIT]


def test_the_table_holds_one_case_per_path():
    have = {(c.sigma, c.k, c.family) for c in gp.CASES.values()}
    assert {(4, k, "grid") for k in (6, 8, 9, 10, 11, 12, 13, 14, 15)} | {(4, 10, "periodic"), (20, 5, "grid"), (20, 6, "grid")} <= have
    for c in gp.CASES.values():
        assert len(c.groups) == 4 and gp.group_order(c) == [7, 3] and c.groups.tolist() == [7, 3, 7, 3]
        windows = c.sites - c.k + 1
        if c.sigma == 4 and c.k <= 10:
            assert windows == 131 and windows % 40 == 11 and windows % 128 == 3
        if c.sigma == 4 and c.k in (11, 12):
            assert windows == 67
        if c.sigma == 4 and c.k >= 13:
            assert c.k + 2 <= c.sites <= c.k + 6
    long = [c for c in gp.CASES.values() if c.opts.get("slice_long_lists")]
    assert sorted(c.k for c in long) == [13, 14, 15]
    assert gp.PERIOD == 37 and all(np.gcd(gp.PERIOD, t) == 1 for t in (32, 40, 128))


@pytest.mark.parametrize("name", NAMES)
def test_conditions(name):
    """The conditions stated at grid_paths.CASES, and the recorded path counts."""
    case, mats, counts = gp.load(name)
    assert gp.on_grid(mats, case.eps)
    assert mats.shape == (4, case.sites, case.sigma)
    span = gp.PERIOD if case.family == "periodic" else case.sites
    assert np.array_equal(mats[2:, 1:span], mats[:2, :span - 1])                  # the shifted twins of a group
    if case.family == "periodic":
        assert np.array_equal(mats[:, gp.PERIOD:], mats[:, :-gp.PERIOD])
    assert (case.ninf > 0) == bool(np.isinf(mats).any())
    # the float64 classifier counts what the oracle's own list building gives, window by window
    hls = gp.half_lists(mats, case.k, case.eps)
    assert [tuple(r) for r in hls[:, :2].tolist()] == [(nl, nr) for _, _, nl, nr in ll.longest_half_lists(mats, case.k, case.eps)]
    d = gp.describe(name)
    print(name, d)
    assert counts == gp.COUNTS[name], f"{name}: the path counts moved: {counts}"
    for path, floor in case.floors.items():
        if path.startswith("max_"):
            assert counts[path[4:]] <= floor, f"{name}: '{path[4:]}' is {counts[path[4:]]}, above {floor}"
        else:
            assert counts[path] >= floor, f"{name}: only {counts[path]} windows reach the path '{path}' (floor {floor})"
    assert counts["on_bound"] >= 1000
    assert 0 < d["scored"] <= gp.MAX_SCORED
    assert len(d["tied"]) == 2 and min(d["tied"]) >= 50, d["tied"]
    if case.family == "periodic":
        assert min(d["tied_across_tiles"]) >= 50, d["tied_across_tiles"]
    if name in DENSE:
        assert d["on_eps"] >= 1000
    if case.sigma == 4 and case.k == 15:                 # the key-range passes fix the left half's first symbol: the right half is the long one
        assert int((hls[:, 1] > gp.BIG_CAP).sum()) >= 3


@pytest.mark.parametrize("name", NAMES)
def test_the_two_oracle_calls_agree(name):
    case, mats, _ = gp.load(name)
    for gid, keys, bits, pos, emitted in gp.oracle(name):
        k2, s2, e2 = co.explore_group(mats[case.groups == gid], case.k, case.eps)
        assert np.array_equal(k2, keys) and np.array_equal(s2.view(np.uint32), bits) and e2 == emitted
        assert np.all(bits.view(np.float32) > np.float32(case.eps))


@pytest.mark.parametrize("name", DENSE)
def test_oracle_against_dense_enumeration(name):
    """Max over the windows, the first window on ties, nothing that scores exactly eps: keys, score bits, positions, scored count."""
    case, mats, _ = gp.load(name)
    for gid, keys, bits, pos, emitted in gp.oracle(name):
        dk, db, dp, de, on, tied = gp.dense_case(name, gid)
        assert np.array_equal(dk, keys), f"{name} group {gid}: key sets differ ({len(keys)} vs {len(dk)})"
        assert np.array_equal(db, bits), f"{name} group {gid}: score bits differ"
        assert np.array_equal(dp, pos), f"{name} group {gid}: first-window positions differ"
        assert de == emitted and on > 0 and tied >= 50
        assert not (bits.view(np.float32) == np.float32(case.eps)).any()


@pytest.mark.parametrize("name", TWO_WINDOWS)
def test_first_two_windows_against_dense_enumeration(name):
    """Beyond 4^10 candidates a window: the oracle's first two windows of every matrix are the dense sets above eps."""
    case, mats, _ = gp.load(name)
    bits = co.bits(case.sigma)
    for m in mats:
        best = co.prefix_max(m)
        for w in (0, 1):
            keys, scores = co.window(m, case.k, w, case.eps, best)
            s = gen.dense_window_scores(m, case.k, w)
            rank = np.flatnonzero(s > np.float32(case.eps))
            want = gen.dense_key(rank, case.k, case.sigma, bits)
            o = np.argsort(want, kind="stable")
            assert np.array_equal(keys, want[o]) and np.array_equal(scores.view(np.uint32), s[rank][o].view(np.uint32)), (name, w)


@needs_binaries
@pytest.mark.parametrize("name", NAMES + [gp.TENTH.name] + list(rp.CASES))
def test_oracle_against_the_live_reference(name):
    """Also on every case of tests/rounded_paths.py: where the bounds round, the oracle's restated sort and break logic could itself
    differ from the reference's."""
    case, mats, _ = gp.load(name)
    per_matrix = rb.ref_windows_many(mats, case.k, case.eps, case.sigma)
    for gid, keys, bits, pos, emitted in gp.oracle(name):
        rk, rs, rp, re_ = rb.merge_windows([per_matrix[i] for i in np.flatnonzero(case.groups == gid)], positions=True)
        assert np.array_equal(rk, keys) and np.array_equal(rs.view(np.uint32), bits), (name, gid)
        assert np.array_equal(rp, pos) and re_ == emitted, (name, gid)


def test_tenth_case_has_lists_beyond_the_capacity():
    """Entries -0.1 * an integer: sums round, so the oracle's own list building counts the half lists (not the float64 classifier)."""
    case, mats, _ = gp.load(gp.TENTH.name)
    assert case.sites - case.k + 1 == 131
    sizes = ll.longest_half_lists(mats, case.k, case.eps)
    over = sum(max(nl, nr) > 160 for _, _, nl, nr in sizes)
    print(gp.TENTH.name, "windows with a half list beyond 160:", over)
    assert over >= gp.TENTH_OVER_CAP
    assert sum(r[4] for r in gp.oracle(gp.TENTH.name)) <= gp.MAX_SCORED
