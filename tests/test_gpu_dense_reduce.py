"""GPU suite: the dense reduce of 6-byte pairs (reduce_buckets_kernel<16384, 512, false, PAIR6>, DNA k = 8..10) on the fabricated slices
of tests/dense_reduce_cases.py, with its non-temporal copy-out stores (the default) and with the plain stores they replaced
(debug_flags bit 15): both against the float64 enumeration of the cases' boxes (tests/test_dense_reduce_inputs.py pins it to the
oracle) and against each other bit for bit -- group-major keys and score bits, key-major counts and entries."""
import functools

import numpy as np
import pytest

import ipk_amd
from ipk_amd.synth import synth_matrices
from oracle import ipk_oracle as co
from tests import comp_paths as cp
from tests import dense_reduce_cases as dc

pytestmark = pytest.mark.gpu

PLAIN = 32768                                   # debug_flags: plain copy-out stores
DENSE = 7                                       # variant: dense tables behind the pair pool (sparse inputs take compressed ones by default)
GROUPS = [1, 3, 130]


@pytest.fixture(scope="module")
def eng():
    e = ipk_amd.Engine(0)
    yield e
    e.set_option("debug_flags", 0)
    e.set_option("variant", 0)
    e.close()


def _options(e, flags=0):
    e.set_option("debug_flags", flags)
    e.set_option("variant", DENSE)


def _group_major(e, case):
    """[(keys, score bits) per group], scored count"""
    res = e.score_groups(case.mats, case.groups, case.k, cp.EPS)
    try:
        assert not e.last_tables_compressed(), "the call did not take dense tables"
        out = []
        for gi in range(len(cp.group_order(case))):
            gk, gs = res.group(gi)
            out.append((np.array(gk, dtype=np.uint32), np.array(gs).view(np.uint32).copy()))
        return out, res.emitted
    finally:
        res.free()


def _key_major(e, case):
    parts = e.score_groups_keymajor(case.mats, case.groups, case.k, cp.EPS, n_owners=1)
    try:
        return parts.counts_tensor().cpu().numpy().copy(), parts.entries_tensor().cpu().numpy().view(np.uint32).copy(), parts.emitted
    finally:
        parts.free()


@functools.lru_cache(maxsize=None)
def _expect(n_groups):
    return cp.case_expect(dc.case(n_groups))


def _same(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} against {len(want)}"
    d = np.flatnonzero(np.asarray(got).ravel() != np.asarray(want).ravel())
    assert len(d) == 0, f"{what}: {len(d)} differ, the first at {int(d[0])}"


def _check(e, case, expect):
    runs = {}
    for flags in (0, PLAIN):
        _options(e, flags)
        runs[flags] = (_group_major(e, case), _key_major(e, case))
    for flags, ((got, emitted), (counts, entries, emitted_km)) in runs.items():
        assert emitted == emitted_km == sum(r[4] for r in expect)
        for gi, (gid, keys, bits, _, _) in enumerate(expect):
            _same(got[gi][0], keys.astype(np.uint32), f"flags {flags}: group {gid}: keys against the enumeration")
            _same(got[gi][1], bits, f"flags {flags}: group {gid}: score bits against the enumeration")
    _same(runs[0][1][0], runs[PLAIN][1][0], "key-major counts: non-temporal against plain stores")
    _same(runs[0][1][1], runs[PLAIN][1][1], "key-major entries: non-temporal against plain stores")


@pytest.mark.parametrize("n_groups", GROUPS)
def test_fabricated_slices(eng, n_groups):
    """Empty slices; slices of 1 .. 5, 511 and 512 pairs; a `dups` slice of 70 chunks or more (equal keys: the maximum wins) beside
    `dense` and a slice of fewer chunks than wavefronts; slot 0 and slot 16 383 alone; a full block between empty ones; 520 slices."""
    _check(eng, dc.case(n_groups), _expect(n_groups))


def test_a_second_call_does_not_see_the_first_calls_table(eng):
    """`dense` and `dups` first, then slot 0 and slot 16 383 alone in the same slices."""
    _check(eng, dc.case(1), _expect(1))
    case = dc.second_call_case()
    _check(eng, case, cp.case_expect(case))


@pytest.mark.parametrize("k", [9, 10])
def test_random_matrices_against_the_oracle(eng, k):
    """Five groups of two matrices of 40 sites: 16 and 64 slices a group."""
    mats = synth_matrices(10, 40, 4, 0.05, 900 + k)
    groups = np.repeat(np.array([7, 3, 12, 5, 9], dtype=np.uint32), 2)
    eps = ipk_amd.log_threshold(1.5, 4, k)
    want = [co.explore_group(mats[groups == gid], k, eps) for gid in (7, 3, 12, 5, 9)]
    for flags in (0, PLAIN):
        _options(eng, flags)
        res = eng.score_groups(mats, groups, k, eps)
        try:
            assert not eng.last_tables_compressed()
            assert res.emitted == sum(w[2] for w in want)
            for gi, (keys, scores, _) in enumerate(want):
                gk, gs = res.group(gi)
                _same(gk, keys, f"flags {flags}: group {gi}: keys against the oracle")
                _same(np.array(gs).view(np.uint32), scores.view(np.uint32), f"flags {flags}: group {gi}: score bits against the oracle")
        finally:
            res.free()
