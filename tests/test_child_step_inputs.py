"""CPU suite: the fabricated inputs of tests/child_step_cases.py contain every class of child-node step and single-step half join
that tests/test_gpu_child_step_paths.py is there for -- classified from the matrices with oracle/np_oracle.py, so an input that
no longer reaches a class fails here instead of passing idly on the GPU.  Needs no GPU."""
import numpy as np
import pytest

from oracle import ipk_oracle as co
from oracle import np_oracle as no
from tests import child_step_cases as cc


@pytest.mark.parametrize("k", cc.KS)
def test_inputs_reach_every_class(k):
    """Both tails of k together: all-16 and empty 2-symbol nodes and all-64 3-symbol nodes in every slot (so bits 15 | 16, 31 | 32,
    47 | 48 and 63 of a ballot are set and meet a clear neighbour), every sub-step empty and full, alone and beside full ones, single
    -step half joins with 1, 63 and 64 candidates and second children of every length, empty halves, a last tile of one window
    and one with an odd count."""
    found = set()
    for tail in cc.TAILS:
        found |= cc.classify(k, tail)[0]
    missing = cc.required(k) - found
    assert not missing, f"k = {k}: no window reaches {sorted(map(str, missing))}"


@pytest.mark.parametrize("k,tail", cc.cases())
def test_shapes(k, tail):
    c = cc.case(k, tail)
    assert c.sites <= 200 and c.mats.shape[1:] == (c.sites, cc.SIGMA) and len(c.mats) == len(c.groups)
    assert (c.sites - k + 1) % cc.TILE[k] == tail
    assert sorted(set(c.groups.tolist())) == sorted(cc.GROUPS2)
    # exact inputs: entries -0.25 * an integer, every column's best entry +0.0 or the column dead
    assert np.array_equal(c.mats * 4, np.round(c.mats * 4))
    cmax = c.mats.max(axis=2)
    assert np.isin(cmax, (0.0, -2.0)).all() and (cmax == -2.0).sum() > 0


@pytest.mark.parametrize("k", (8, 10, 12))
def test_node_masks_give_the_oracles_windows(k):
    """The classifier's nodes are the oracle's: per window, the pairs of both half lists that pass eps are the scored k-mers of
    oracle/ipk_oracle (counted), on the case's first matrix."""
    c = cc.case(k, 3)
    m = c.mats[0]
    best_np, best_c = no.prefix_max(m), co.prefix_max(m)
    hl = k // 2
    for w in range(0, c.sites - k + 1, 7):
        masks, n_l, n_r = cc.window_nodes(m, best_np, k, w)
        keys, _ = co.window(m, k, w, cc.EPS, best_c)
        left, right = cc_sums(m[w:w + hl]), cc_sums(m[w + hl:w + k])
        assert n_l == int((left > cc.EPS - m[w + hl:w + k].max(axis=1).sum()).sum())
        assert len(keys) == int(((left[:, None] + right[None, :]) > cc.EPS).sum())
        assert (len(keys) == 0) == (min(int(x.sum()) for x in masks) == 0)


def cc_sums(cols):
    s = np.zeros(1)
    for c in cols:
        s = (s[:, None] + c[None, :].astype(np.float64)).ravel()
    return s
