"""CPU suite: the fabricated slices of tests/dense_reduce_cases.py are what they claim -- pairs, keys and chunk bounds per slice --
and their expectation (direct enumeration) is the oracle's."""
import numpy as np
import pytest

from oracle import ipk_oracle as co
from tests import comp_paths as cp
from tests import dense_reduce_cases as dc

GROUPS = [1, 3, 130]


def _stats(case, name):
    return [cp.slice_stats(case, g, b) for (g, b), v in sorted(case.slices.items(), key=lambda kv: kv[0]) if v == name or v[0] == name]


def test_geometry():
    assert cp.geometry(4, dc.K) == (dc.TBL, dc.WAVES, dc.NB) and cp.chunk_pairs(dc.TBL) == dc.CHUNK
    assert [cp.geometry(4, k)[2] for k in (9, 10)] == [16, 64]


@pytest.mark.parametrize("n_groups", GROUPS)
def test_every_slice_is_what_it_claims(n_groups):
    case = dc.case(n_groups)
    assert case.mats.shape[1] == 35 and len(cp.group_order(case)) == n_groups
    seen = 0
    for n in dc.COUNTS:
        for st in _stats(case, f"odd_{n}"):
            # n pairs on n keys: at least one chunk and none with more than n pairs; 1 .. 5 cover every count modulo 4
            assert st["pairs"] == st["keys"] == n and st["slots"].tolist() == list(range(5, 5 + n)) and st["chunks_floor"] == 1
            seen += 1
    assert sorted(n % 4 for n in dc.COUNTS[:5]) == [0, 1, 1, 2, 3] and dc.COUNTS[-2:] == (dc.CHUNK - 1, dc.CHUNK)
    if n_groups == 130:
        assert seen >= 4 * len(dc.COUNTS)
    for st in _stats(case, "slot_0"):
        assert st["slots"].tolist() == [0] and st["pairs"] == 1
    for st in _stats(case, f"slot_{dc.TBL - 1}"):
        assert st["slots"].tolist() == [dc.TBL - 1] and st["pairs"] == 1
    for st in _stats(case, "block_3"):
        assert st["blocks"][2:5].tolist() == [0, 64, 0] and st["keys"] == 64                   # a full block between empty ones
    if n_groups > 1:
        assert _stats(case, "slot_0") and _stats(case, f"slot_{dc.TBL - 1}") and _stats(case, "block_3")
    dense, = _stats(case, "dense")
    assert dense["keys"] == dense["pairs"] == dc.TBL and dense["chunks_floor"] == dc.TBL // dc.CHUNK
    for few in _stats(case, "few_chunks_2"):
        assert few["pairs"] == 256 and few["chunks_floor"] == 1 and 2 < dc.WAVES               # at most two chunks (one per matrix): fewer than wavefronts
    assert n_groups == 1 or len(_stats(case, "few_chunks_2")) == 1
    dups = _stats(case, "dups")
    nwin = case.mats.shape[1] - dc.K + 1
    assert len(dups) == 2
    for st in dups:
        assert st["keys"] == 128 and st["pairs"] == 128 * nwin * cp.dups_m(dc.K)
        assert st["chunks_floor"] >= 48                                                          # six chunks or more for each of 8 wavefronts
    g = next(g for (g, b), v in case.slices.items() if v[0] == "dups")
    tied, first, middle, last = cp.dups_stats(case, g)
    assert tied >= 1 / 3 and min(first, middle, last) >= 1                                      # equal keys, equal bits; the maximum early, in the middle, late
    # nothing anywhere else
    for gi, gid in enumerate(cp.group_order(case)):
        touched = set((cp.group_pairs(case, gid)[0] // dc.TBL).tolist())
        assert touched == {b for (gg, b), v in case.slices.items() if gg == gi and v != "empty"}


def test_the_second_call():
    second = dc.second_call_case()
    assert [cp.slice_stats(second, 0, b)["slots"].tolist() for b in range(4)] == [[0], [], [], [dc.TBL - 1]]
    assert cp.slice_stats(dc.case(1), 0, 2)["keys"] == dc.TBL


@pytest.mark.parametrize("n_groups", GROUPS)
def test_expectation_is_the_oracles(n_groups):
    case = dc.case(n_groups)
    for gid, keys, bits, pos, n in cp.case_expect(case):
        ok, os_, oe = co.explore_group(case.mats[case.groups == gid], dc.K, cp.EPS)
        assert np.array_equal(ok, keys) and np.array_equal(os_.view(np.uint32), bits) and oe == n
