"""The pair pool behind the candidate-per-lane join (DNA k = 8, 9, 10) holds its chunks in two planes -- f32 scores, then u16 slots
of the bucket's table, 6 bytes per scored k-mer -- and reduce_buckets_kernel reads them four pairs per lane and load.  Everything
here is compared bit for bit with the oracle (co.explore_group, tests/db_check.py): group-major keys, score bits and scored
counts, and the key-major database for one and for two owners."""
import numpy as np
import pytest

import ipk_amd
from ipk_amd.synth import synth_matrices
from oracle import ipk_oracle as co
from tests import db_check as dc

pytestmark = pytest.mark.gpu
SIGMA = 4


def _oracle(mats, groups, k, eps):
    """{gid: (keys, score bits, scored count)} in first-seen group order."""
    groups = np.asarray(groups, dtype=np.uint32)
    out = {}
    for gid in dict.fromkeys(groups.tolist()):
        keys, scores, emitted = co.explore_group(mats[groups == gid], k, eps)
        out[int(gid)] = (keys, scores.view(np.uint32), int(emitted))
    return out


def _check(engine, mats, groups, k, eps, ref=None, sigma=SIGMA, worlds=(1, 2)):
    """One group-major call and one key-major call per owner count, each against the oracle entry by entry."""
    mats = np.ascontiguousarray(mats, dtype=np.float32)
    groups = np.asarray(groups, dtype=np.uint32)
    ref = ref if ref is not None else _oracle(mats, groups, k, eps)
    gids = list(ref)
    total = sum(r[2] for r in ref.values())

    def oracle(gid):
        return ref[gid][0], ref[gid][1]

    res = engine.score_groups(mats, groups, k, eps)
    try:
        assert res.emitted == total
        expect = {g: dc.Expect(r[0], r[1], r[2], sigma, k, 1) for g, r in ref.items()}
        keys, bits = dc.result_tensors(res)
        dc.check_groups(res.group_ids, res.offsets, keys, bits, gids, expect, oracle=oracle)
        del keys, bits
    finally:
        res.free()
    for world in worlds:
        expect = {g: dc.Expect(r[0], r[1], r[2], sigma, k, world) for g, r in ref.items()}
        parts = engine.score_groups_keymajor(mats, groups, k, eps, n_owners=world)
        try:
            assert parts.emitted == total and parts.num_entries == sum(len(r[0]) for r in ref.values())
            for owner in range(world):
                db = engine.merge_parts_ptrs(sigma, k, owner, world, [parts.counts_ptr() + 4 * owner * parts.slots],
                                             [parts.entries_ptr() + 8 * int(parts.owner_offsets[owner])])
                try:
                    dk, off, entries = dc.db_tensors(db)
                    dc.check_db(dk, off, entries, gids, expect, sigma, k, owner=owner, world=world, oracle=oracle)
                    del dk, off, entries
                finally:
                    db.free()
        finally:
            parts.free()
    return ref


@pytest.mark.parametrize("variant", [7, 6], ids=["dense", "compressed"])
@pytest.mark.parametrize("k", [8, 9, 10])
def test_dense_and_compressed_tables(engine, k, variant):
    """Both epilogues of the reduce behind the two-plane pool (variant 7 forces dense tables, 6 the compressed form)."""
    mats = synth_matrices(6, 700, SIGMA, 0.1, 6100 + k)
    groups = np.repeat(np.arange(3, dtype=np.uint32) + 21, 2)
    engine.set_option("variant", variant)
    try:
        _check(engine, mats, groups, k, co.log_threshold(1.5, SIGMA, k))
    finally:
        engine.set_option("variant", 0)


def _peaked(key, k):
    """A matrix of exactly k sites (one window) whose only surviving k-mer is `key` (dense code, first symbol most significant)."""
    m = np.full((k, SIGMA), -6.0, dtype=np.float32)                    # three symbols at 1e-6 each ...
    for i in range(k):
        m[i, (key >> (2 * (k - 1 - i))) & 3] = np.float32(np.log10(1.0 - 3e-6))   # ... and the peak
    return m


@pytest.mark.parametrize("k", [8, 10])
def test_slot_extremes(engine, k):
    """Slot 0 of bucket 0 (all-A), slot 16383 of the last bucket (all-T, key 4^k - 1), and slot 0x3FFF of a middle bucket with the
    key after it (slot 0 of the next bucket): the u16 plane's extremes, one window each."""
    eps = co.log_threshold(1.5, SIGMA, k)
    nb = 4 ** k // 16384
    mid = (nb // 2 - 1) * 16384 + 0x3FFF
    cases = [[0], [4 ** k - 1], [mid, mid + 1]]
    for want in cases:                                                  # one group at a time: the smallest call there is
        mats = np.stack([_peaked(key, k) for key in want])
        ref = _oracle(mats, [5] * len(want), k, eps)
        assert ref[5][0].tolist() == want, "the input does not isolate the intended k-mers"
        _check(engine, mats, [5] * len(want), k, eps, ref=ref)
    mats = np.stack([_peaked(key, k) for want in cases for key in want])
    groups = [7, 3, 9, 9]
    ref = _oracle(mats, groups, k, eps)
    assert [ref[g][0].tolist() for g in (7, 3, 9)] == cases
    _check(engine, mats, groups, k, eps, ref=ref)


def test_chunk_roll_inside_a_join_step(engine):
    """Flat columns, about 600 pairs per window: buckets fill their 512-pair chunks inside single join steps; with a 40-chunk first
    pool the launch is redone, its overflowing stores absorbed by the spare chunk past the pool's last id (3-KB chunks)."""
    k = 10
    mats = synth_matrices(4, 600, SIGMA, 1.0, 123)
    groups = [1, 1, 2, 2]
    eps = co.log_threshold(1.5, SIGMA, k)
    ref = _check(engine, mats, groups, k, eps)
    engine.set_option("debug_pool_chunks", 40)
    try:
        _check(engine, mats, groups, k, eps, ref=ref)
    finally:
        engine.set_option("debug_pool_chunks", 0)


@pytest.mark.parametrize("k", [8, 10])
def test_rebasing(engine, k):
    """debug_flags bit 3: every wavefront moves its store window every 8 chunks (of 3072 bytes now); group-major and key-major."""
    mats = synth_matrices(6, 700, SIGMA, 0.1, 99 + k)
    groups = np.array([0, 0, 1, 1, 2, 2], dtype=np.uint32)
    eps = co.log_threshold(1.5, SIGMA, k)
    ref = _oracle(mats, groups, k, eps)
    for pool_chunks in (0, 40):
        engine.set_option("debug_flags", 8)
        engine.set_option("debug_pool_chunks", pool_chunks)
        try:
            _check(engine, mats, groups, k, eps, ref=ref, worlds=(1,))
        finally:
            engine.set_option("debug_flags", 0)
            engine.set_option("debug_pool_chunks", 0)


def test_chunk_tails_and_empty_result(engine):
    """A small input: every chunk closes partly filled, with counts that are no multiples of four -- the reduce's four-pair loads
    must ignore what lies behind a chunk's count.  And thresholds nobody passes: no chunk is ever opened."""
    k = 8
    mats = synth_matrices(2, 64, SIGMA, 0.1, 808)
    _check(engine, mats, [4, 4], k, co.log_threshold(1.5, SIGMA, k))
    ref = _oracle(mats, [4, 4], k, 0.5)
    assert ref[4][2] == 0 and len(ref[4][0]) == 0
    res = engine.score_groups(mats, np.array([4, 4], np.uint32), k, 0.5)
    assert res.emitted == 0 and res.num_entries == 0 and res.group_ids.tolist() == [4]
    res.free()
    for world in (1, 2):
        parts = engine.score_groups_keymajor(mats, np.array([4, 4], np.uint32), k, 0.5, n_owners=world)
        assert parts.emitted == 0 and parts.num_entries == 0
        parts.free()


def test_minus_infinity_columns(engine):
    """log10(0) entries and a dead column (later prefix sums are -inf, bounds NaN) at k = 10."""
    k = 10
    mats = synth_matrices(2, 120, SIGMA, 0.2, 2110)
    mats[0, 7, 2] = -np.inf
    mats[0, 60, 0] = -np.inf
    mats[1, 40, :] = -np.inf
    _check(engine, mats, [0, 1], k, co.log_threshold(1.5, SIGMA, k))
    _check(engine, mats, [3, 3], k, co.log_threshold(1.5, SIGMA, k))


@pytest.mark.parametrize("sigma,k,sites,alpha", [(4, 12, 80, 0.1), (20, 6, 30, 0.03)], ids=["dna_k12", "aa_k6"])
def test_unchanged_neighbours(engine, sigma, k, sites, alpha):
    """The row-per-lane join (k = 12) and the exact partition (AA k = 6) keep their 8-byte pairs."""
    mats = synth_matrices(4, sites, sigma, alpha, 1200 + k)
    _check(engine, mats, [3, 3, 8, 8], k, co.log_threshold(1.5, sigma, k), sigma=sigma)


@pytest.mark.parametrize("k,chunk_bytes", [(8, 3072), (10, 3072), (12, 2048)], ids=["k8_planes", "k10_planes", "k12_pairs8"])
def test_pool_bytes_follow_the_layout(k, chunk_bytes):
    """The layout is really taken: a context's first pool of N chunks (debug_pool_chunks; one window, so it never runs out) holds
    (N + 1) chunks -- the spare one behind the last id -- of 512 pairs x 6 bytes at k = 8, 10 and of 256 pairs x 8 bytes at k = 12."""
    n = 4096
    mats = _peaked(5, k)[None]
    eps = co.log_threshold(1.5, SIGMA, k)
    ref = _oracle(mats, [2], k, eps)
    eng = ipk_amd.Engine(0)
    try:
        eng.set_option("debug_pool_chunks", n)
        _check(eng, mats, [2], k, eps, ref=ref, worlds=(1,))
        assert eng.get_option("debug_pool_bytes") == (n + 1) * chunk_bytes
    finally:
        eng.close()


@pytest.mark.parametrize("variant", [7, 6, 0], ids=["dense", "compressed", "default"])
@pytest.mark.parametrize("k", [8, 10])
def test_big_list_windows_join_the_two_plane_pool(engine, k, variant):
    """A permissive threshold on flat columns: half lists beyond the fast path's capacity, so the windows are queued for the big-list
    kernel, which appends to the same pool (score_overflow_stream_kernel<..., PAIR6>: few windows, or compressed tables) --
    its pairs must lie in the planes the reduce reads."""
    mats = synth_matrices(4, k + 4, SIGMA, 1.0, 900 + k)
    engine.set_option("variant", variant)
    try:
        _check(engine, mats, [6, 6, 2, 2], k, np.float32(-0.9 * k))
    finally:
        engine.set_option("variant", 0)
