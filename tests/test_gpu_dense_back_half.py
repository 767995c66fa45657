"""The dense back half behind the reduce: km_write_lines_kernel with its non-temporal stores (a workgroup's 64 keys, 64 groups per
visit) and km_count_mask_slice_kernel (a thread per mask word and slice of the groups), bit for bit against the oracle's database
and against the writers they stand beside: km_write_kernel (debug_flags bit 9) and the line writer with plain stores (bit 14)."""
import functools

import numpy as np
import pytest

import ipk_amd
from ipk_amd.synth import synth_matrices
from oracle import db_oracle as dbo
from oracle import ipk_oracle as co
from tests.test_gpu_parity import _check_parts_against_oracle

pytestmark = pytest.mark.gpu

V = 64                                    # groups per visit of the line writer
LINES, LINES_PLAIN, TILES = 1024, 1024 | 16384, 512   # debug_flags: line writer whatever the group count | with plain stores | km_write_kernel
SHAPES = {"dense": (4, 6, 200, 0.6, 77),              # every key holds 100 or more of the first 128 groups, some all 128
          "sparse": (4, 8, 60, 0.6, 77),              # 29 % of a group's slots filled: short runs, visits that bring a key nothing
          "dna_k2": (4, 2, 40, 0.6, 77),              # 16 keys: less than a mask word
          "aa_k2": (20, 2, 40, 0.3, 77)}              # 400 keys: a partial last mask word
G_MAX = {"dense": 2 * V + 40, "sparse": 300, "dna_k2": 130, "aa_k2": 130}


@functools.lru_cache(maxsize=None)
def _shape(name):
    """The shape's matrices (one per group, group ids from 2) and the oracle's result per group, computed once."""
    sigma, k, sites, alpha, seed = SHAPES[name]
    mats = synth_matrices(G_MAX[name], sites, sigma, alpha, seed)
    eps = co.log_threshold(1.5, sigma, k)
    per_group = []
    for g in range(G_MAX[name]):
        keys, scores, e = co.explore_group(mats[g:g + 1], k, eps)
        # (the oracle packs amino-acid keys five bits per symbol: the engine's slots are the dense base-sigma codes)
        per_group.append((dbo.dense_code(np.asarray(keys), sigma, k).astype(np.int64), np.asarray(scores).view(np.uint32).copy(), int(e)))
    return mats, eps, per_group


def _expected(name, n_groups, owners):
    """(scored count, counts [owners, ceil(T / owners)], entries [n, 2] uint32) as the oracle has them: owner-major, key, group order."""
    sigma, k = SHAPES[name][:2]
    T = sigma ** k
    _, _, per_group = _shape(name)
    present = np.zeros((n_groups, T), dtype=bool)
    score = np.zeros((n_groups, T), dtype=np.uint32)
    for g in range(n_groups):
        present[g, per_group[g][0]] = True
        score[g, per_group[g][0]] = per_group[g][1]
    slots = (T + owners - 1) // owners
    counts = np.zeros((owners, slots), dtype=np.int64)
    blocks = []
    for o in range(owners):
        keys = np.arange(o, T, owners)
        counts[o, :len(keys)] = present[:, keys].sum(axis=0)
        kk, gg = np.nonzero(present[:, keys].T)               # key-major, groups ascending within a key
        blocks.append(np.stack([(gg + 2).astype(np.uint32), score[gg, keys[kk]]], axis=1))
    return sum(p[2] for p in per_group[:n_groups]), counts, np.concatenate(blocks), present


def _run(name, n_groups, owners, flags, variant, batches=False, kmc_pass=0):
    sigma, k = SHAPES[name][:2]
    mats, eps, _ = _shape(name)
    eng = ipk_amd.Engine(0)
    try:
        eng.set_option("debug_flags", flags)
        eng.set_option("variant", variant)
        if batches:
            eng.set_option("workspace_bytes", 70 * (sigma ** k) * 4)
        if kmc_pass:
            eng.set_option("debug_kmc_pass", kmc_pass)
        parts = eng.score_groups_keymajor(mats[:n_groups], np.arange(n_groups, dtype=np.uint32) + 2, k, eps, n_owners=owners)
        out = (parts.emitted, parts.counts_tensor().cpu().numpy().copy(), parts.entries_tensor().cpu().numpy().copy(),
               list(parts.owner_offsets))
        parts.free()
        return out
    finally:
        eng.close()


def _same_as_expected(out, name, n_groups, owners):
    emitted, counts, entries, _ = _expected(name, n_groups, owners)
    assert out[0] == emitted
    assert out[1].shape[0] == owners and np.array_equal(out[1][:, :counts.shape[1]], counts) and not out[1][:, counts.shape[1]:].any()
    assert np.array_equal(out[2].view(np.uint32), entries)
    assert [int(x) for x in out[3]] == [0] + np.cumsum(counts.sum(axis=1)).tolist()


def _writers_agree(name, n_groups, owners, batches=False):
    outs = [_run(name, n_groups, owners, flags, 7, batches=batches) for flags in (LINES, LINES_PLAIN, TILES)]
    for other in outs[1:]:
        assert outs[0][0] == other[0] and outs[0][3] == other[3]
        assert np.array_equal(outs[0][1], other[1]) and np.array_equal(outs[0][2], other[2])
    _same_as_expected(outs[0], name, n_groups, owners)
    sigma, k = SHAPES[name][:2]
    mats, eps, _ = _shape(name)
    _check_parts_against_oracle(outs[0][0], outs[0][1], outs[0][2], outs[0][3], mats[:n_groups], np.arange(n_groups, dtype=np.uint32) + 2, sigma, k, eps)


def _per_visit(name, n_groups):
    """[visits, keys]: a key's entries among the groups of each visit of V."""
    present = _expected(name, n_groups, 1)[3]
    return np.stack([present[g0:g0 + V].sum(axis=0) for g0 in range(0, n_groups, V)])


def _longest_run(per_visit):
    """The longest [tail | a visit's entries] run of the line writer with one owner: a key's stores end at the last 128-byte line
    boundary (16 entries) of its run, the rest waits as the tail."""
    pos = np.concatenate([[0], np.cumsum(per_visit.sum(axis=0))[:-1]])
    tail = np.zeros_like(pos)
    longest = 0
    for n in per_visit:
        total = tail + n
        over = (pos + total) & 15
        cut = np.where(over <= total, total - over, 0)
        longest = max(longest, int(total.max()))
        tail, pos = total - cut, pos + cut
    return longest


def test_shapes_cover_what_the_cases_are_for():
    """A seed that stops producing full visits, runs of two store instructions or empty visits fails here, not silently."""
    dense = _per_visit("dense", 2 * V + 40)
    assert (dense >= V).any()                      # a key with an entry from every group of a visit
    assert _longest_run(dense) > 64                # a run that takes two store instructions
    sparse = _per_visit("sparse", 300)
    assert sparse.max() < V and (sparse[:-1] < 16).any()      # short runs: a visit that leaves some key less than a line
    # (at 300 groups every key gets at least two entries even from the last visit's 44 groups: the visit that brings a key
    #  nothing is the one-group visit of the V + 1 case)
    sparse = _per_visit("sparse", V + 1)
    assert ((sparse == 0).any(axis=0) & (sparse > 0).any(axis=0)).any()      # a key that a visit brings nothing, with entries elsewhere


@pytest.mark.parametrize("owners", [1, 3])
@pytest.mark.parametrize("n_groups", [V - 1, V, V + 1, 2 * V + 40])
def test_dense_shape_full_visits_and_long_runs(n_groups, owners):
    """Full visits and runs of two store instructions per key; a last visit of 1 and of 40 groups; owners whose blocks start at odd
    offsets (a workgroup's keys fall into different owner blocks)."""
    _writers_agree("dense", n_groups, owners)


@pytest.mark.parametrize("owners", [1, 3])
@pytest.mark.parametrize("n_groups", [300, V + 1])
def test_sparse_shape_short_runs_and_empty_visits(n_groups, owners):
    _writers_agree("sparse", n_groups, owners)


@pytest.mark.parametrize("name", ["dense", "sparse"])
def test_two_batches_append_in_the_middle_of_a_line(name):
    """Batches of fewer groups than a visit; every batch after the first starts from cursors that stand inside a line."""
    _writers_agree(name, 2 * V + 40, 3, batches=True)


@pytest.mark.parametrize("variant", [7, 6], ids=["dense", "compressed"])
@pytest.mark.parametrize("name,n_groups,owners", [("dense", 1, 1), ("dense", 3, 3), ("dense", 97, 1), ("dense", 130, 3),
                                                  ("dense", V, 1), ("dense", 2 * V + 40, 3), ("sparse", 300, 1),
                                                  ("dna_k2", 130, 1), ("aa_k2", 130, 3), ("aa_k2", 3, 1)])
def test_counts_from_the_masks(name, n_groups, owners, variant):
    """The counts row against the oracle; fewer groups than quarters, a key space below a mask word and one with a partial last
    word.  The compressed tables' writers start from the per-quarter counts (qpack), so their entries check those."""
    _same_as_expected(_run(name, n_groups, owners, 0, variant), name, n_groups, owners)


@pytest.mark.parametrize("n_groups,kmc_pass", [(130, 64), (2 * V + 40, 100)])
def test_counts_of_the_compressed_writers_passes(n_groups, kmc_pass):
    """More groups than a pass of the compressed writer: counts per pass from a shifted mask pointer, the last pass of 2 groups
    (fewer than quarters) and of 96."""
    _same_as_expected(_run("dense", n_groups, 3, 0, 6, kmc_pass=kmc_pass), "dense", n_groups, 3)
