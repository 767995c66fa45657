"""The half joins of the candidate-per-lane scoring kernel (DNA k = 8, 9, 10), path by path: windows whose two half joins fit one
step, windows with one or with both halves beyond 64 candidates (each half then built by its own size: single step, or rows of
the first child against the second child's list in registers), a second child with more than 32 entries (one row per step), half
lists at and past the capacity of 160, tile tails, and the final join's row reservation under chunk rolls.  Every input is
classified on the CPU from its matrices, so that a case which no longer reaches its path fails instead of passing idly; every
result is compared bit for bit with the oracle (keys and raw score bits) through the per-branch call and the key-major call."""
import functools

import numpy as np
import pytest

from ipk_amd.synth import synth_matrices
from oracle import ipk_oracle as co
from tests import db_check as dc
from tests.grid_paths import all_sums as _all_sums, classify, half as _half, split as _split

pytestmark = pytest.mark.gpu
SIGMA = 4
CAP = 160                                    # half-list capacity of the k <= 10 kernels
GROUPS = np.array([11, 11, 4, 4], dtype=np.uint32)


def _oracle(mats, groups, k, eps):
    groups = np.asarray(groups, dtype=np.uint32)
    out = {}
    for gid in dict.fromkeys(groups.tolist()):
        keys, scores, emitted = co.explore_group(mats[groups == gid], k, eps)
        out[int(gid)] = (keys, scores.view(np.uint32), int(emitted))
    return out


def _check(engine, mats, groups, k, eps, ref):
    """The per-branch call and the key-major call against the oracle, entry by entry."""
    mats = np.ascontiguousarray(mats, dtype=np.float32)
    groups = np.asarray(groups, dtype=np.uint32)
    gids = list(ref)
    total = sum(r[2] for r in ref.values())
    expect = {g: dc.Expect(r[0], r[1], r[2], SIGMA, k, 1) for g, r in ref.items()}

    def oracle(gid):
        return ref[gid][0], ref[gid][1]

    res = engine.score_groups(mats, groups, k, eps)
    try:
        assert res.emitted == total
        keys, bits = dc.result_tensors(res)
        dc.check_groups(res.group_ids, res.offsets, keys, bits, gids, expect, oracle=oracle)
        del keys, bits
    finally:
        res.free()
    parts = engine.score_groups_keymajor(mats, groups, k, eps, n_owners=1)
    try:
        assert parts.emitted == total and parts.num_entries == sum(len(r[0]) for r in ref.values())
        db = engine.merge_parts_ptrs(SIGMA, k, 0, 1, [parts.counts_ptr()], [parts.entries_ptr() + 8 * int(parts.owner_offsets[0])])
        try:
            dk, off, entries = dc.db_tensors(db)
            dc.check_db(dk, off, entries, gids, expect, SIGMA, k, owner=0, world=1, oracle=oracle)
            del dk, off, entries
        finally:
            db.free()
    finally:
        parts.free()


@functools.lru_cache(maxsize=None)
def _case(k, alpha, sites=300):
    """(matrices, eps, path counts, oracle result) of synth_matrices(4, sites, 4, alpha, seed=7) as 2 groups x 2 matrices."""
    mats = synth_matrices(4, sites, SIGMA, alpha, seed=7)
    eps = co.log_threshold(1.5, SIGMA, k)
    return mats, eps, classify(mats, k, eps), _oracle(mats, GROUPS, k, eps)


# floors per path: conditions on the inputs, not measurements
FLOORS = {10: dict(single=50, one_long=50, both_long=50, one_row=10, over_cap=5),
          9: dict(single=50, one_long=50),
          8: dict(one_long=20)}


@pytest.mark.parametrize("k", [10, 9, 8])
def test_paths(engine, k):
    """291+ windows per matrix (no multiple of the tile's 40: a tile tail and partial steps), every path above its floor."""
    mats, eps, n, ref = _case(k, 0.12)
    print({key: v for key, v in n.items() if key != "cap_lists"})
    for path, floor in FLOORS[k].items():
        assert n[path] >= floor, f"k = {k}: only {n[path]} windows reach the path '{path}' (floor {floor})"
    _check(engine, mats, GROUPS, k, eps, ref)


def test_k8_both_halves_long(engine):
    """The 2 | 2 children of k = 8 with both halves beyond 64 candidates: flatter columns (alpha = 0.3)."""
    mats, eps, n, ref = _case(8, 0.3)
    print({key: v for key, v in n.items() if key != "cap_lists"})
    assert n["both_long"] >= 20 and n["one_long"] >= 20
    _check(engine, mats, GROUPS, 8, eps, ref)


@pytest.mark.parametrize("k", [10, 8])
def test_single_window_in_the_last_tile(engine, k):
    """41 windows per matrix: the last tile holds one window (half a window pair, alone in its wavefront)."""
    mats, eps, n, ref = _case(k, 0.12, sites=41 + k - 1)
    assert n["one_long"] + n["both_long"] >= 10
    _check(engine, mats, GROUPS, k, eps, ref)


def test_rows_meet_chunk_rolls(engine):
    """debug_flags bit 3: every wavefront rebases its store window every 8 chunks, so the reservations by the rows' last lanes
    meet chunk rolls and rebases."""
    mats, eps, n, ref = _case(10, 0.12)
    engine.set_option("debug_flags", 8)
    try:
        _check(engine, mats, GROUPS, 10, eps, ref)
    finally:
        engine.set_option("debug_flags", 0)


def _capacity_input(k, side, want):
    """One window (k sites) and a threshold under which the `side` half list has exactly `want` entries -- `want` half sums lie
    above the half's threshold and the next one below it, both by more than 5e-4, far beyond float32 rounding of these sums
    (< 1e-4) -- while the other half, its columns scaled to be more peaked, keeps 1 .. CAP entries by the same margin."""
    la, lb, ra, rb = _split(k)
    hl = la + lb
    for seed in range(200):
        m = synth_matrices(1, k, SIGMA, 0.5, seed=9000 + seed)[0]
        if side == "L":
            m[hl:] *= np.float32(3.0)
        else:
            m[:hl] *= np.float32(3.0)
        cmax = m.max(axis=1).astype(np.float64)
        m_l, m_r = cmax[:hl].sum(), cmax[hl:].sum()
        mine = np.sort(_all_sums(m[:hl] if side == "L" else m[hl:]))[::-1]
        if len(mine) <= want or mine[want - 1] - mine[want] < 2e-3:
            continue
        eps_h = 0.5 * (mine[want - 1] + mine[want])
        eps = float(np.float32(eps_h + (m_r if side == "L" else m_l)))
        eps_l, eps_r = eps - m_r, eps - m_l
        left, right = _all_sums(m[:hl]), _all_sums(m[hl:])
        if min(np.abs(left - eps_l).min(), np.abs(right - eps_r).min()) < 5e-4:
            continue
        nla, nlb, nl = _half(m[:hl], la, lb, eps_l)
        nra, nrb, nr = _half(m[hl:], ra, rb, eps_r)
        assert nl == int((left > eps_l).sum()) and nr == int((right > eps_r).sum())     # (the child thresholds lose no pair)
        if (nl, nr)[side == "R"] == want and 1 <= (nl, nr)[side == "L"] <= CAP:
            return m[None], eps, (nl, nr)
    raise AssertionError(f"no one-window input with a {side} half list of exactly {want} entries among 200 seeds")


@pytest.mark.parametrize("want", [CAP, CAP + 1], ids=["exactly_cap", "cap_plus_1"])
@pytest.mark.parametrize("side", ["L", "R"])
@pytest.mark.parametrize("k", [10, 9])
def test_capacity_edge(engine, k, side, want):
    """A half list of exactly 160 entries stays in the kernel; one of 161 is queued for the big-list kernel.  Both match."""
    mats, eps, lens = _capacity_input(k, side, want)
    print(k, side, lens)
    assert lens[side == "R"] == want
    ref = _oracle(mats, [6], k, eps)
    assert ref[6][2] > 0
    _check(engine, mats, [6], k, eps, ref)
