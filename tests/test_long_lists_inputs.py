"""CPU: the inputs of tests/test_gpu_long_lists.py are what they claim -- windows whose half lists are well beyond the big-list
kernels' capped capacity (6144 entries), counted by the oracle.  Pins the inputs; needs no GPU."""
import numpy as np
import pytest

from oracle import ar_oracle
from oracle import ipk_oracle as co
from tests import long_lists as ll


def _sizes(mats, k, eps):
    return [(nl, nr) for _, _, nl, nr in ll.longest_half_lists(mats, k, eps)]


def test_k13_right_half_is_long():
    mats, eps = ll.k13_input()
    sizes = _sizes(mats, 13, eps)
    assert max(nr for _, nr in sizes) == 4 ** 7 >= ll.LONG
    assert all(nl <= 4 ** 6 for nl, _ in sizes)                   # a 6-symbol left half always fits


def test_k14_both_halves_of_one_window_are_long():
    mats, groups, eps = ll.k14_input()
    sizes = _sizes(mats[groups == 5], 14, eps)
    assert any(nl >= ll.LONG and nr >= ll.LONG for nl, nr in sizes), sizes
    # the two matrices of the group differ
    assert not np.array_equal(mats[0], mats[1])


@pytest.mark.parametrize("k,both", [(15, False), (16, True)])
def test_key_range_inputs_are_long(k, both):
    mats, groups, eps = ll.keyrange_input(k)
    sizes = _sizes(mats[groups == 5], k, eps)
    assert any(nr >= ll.LONG for _, nr in sizes), sizes
    if both:
        assert any(nl >= ll.LONG and nr >= ll.LONG for nl, nr in sizes), sizes


@pytest.mark.parametrize("k", [13, 15])
def test_flat_columns_fill_every_slice(k):
    mats, eps = ll.flat_input(k)
    nl, nr = ll.half_list_sizes(mats[0], k, 0, eps)
    assert (nl, nr) == (4 ** (k // 2), 4 ** (k - k // 2)) and nr >= ll.LONG
    assert eps < float(np.float32(k * np.log10(0.25))) - 0.25    # below every score, whatever the order of the sum


def test_split_sum_is_the_oracle_order():
    """k equal terms added in DC's split order: the score the oracle gives every k-mer of flat columns (small k: 4^8 k-mers)."""
    v = np.float32(np.log10(0.25))
    for k in (5, 7, 8):
        m = np.full((k, 4), v, np.float32)
        keys, scores = co.window(m, k, 0, float(np.float32(k * np.log10(0.25) - 0.5)))
        assert len(keys) == 4 ** k
        assert np.all(scores.view(np.uint32) == ll.split_sum_bits(v, k))


def test_cli_file_keeps_the_long_list(tmp_path):
    """The matrices as read back from the .raxml.ancestralProbs file, under the CLI's omega: the 7-symbol list stays long."""
    mats, _ = ll.k13_input()
    path = tmp_path / "ar.raxml.ancestralProbs"
    ll.write_probs_file(path, ll.CLI_LABELS, mats)
    back, order = ar_oracle.read_file(path, 4)
    assert order == list(ll.CLI_LABELS)
    back = np.stack([back[lab] for lab in ll.CLI_LABELS])
    eps = co.log_threshold(ll.CLI_OMEGA, 4, 13)
    assert max(nr for _, nr in _sizes(back, 13, eps)) >= ll.LONG
