"""GPU suite: the kernels against what the REFERENCE'S OWN compiled code gave -- the fixtures of tests/golden/ref/ (recorded by
oracle/gen_ref_golden.py from the binaries of oracle/ref_build.py), not the oracle.  Every scoring comparison is exact: key sets,
raw score bits, first-window positions, scored counts.  The grid fixtures put many candidates exactly on eps and many equal scores
in different windows and matrices, so the strict comparisons and the keep-first-window rule of every kernel family are on trial.
The engine fixture is shared by the session: every test restores the options it sets."""
import os

import numpy as np
import pytest

import ipk_amd
from ipk_amd import keyrange
from oracle import db_oracle as dbo
from oracle import gen_ref_golden as gen
from oracle import ipk_oracle as co
from oracle import ref_build as rb
from tests import ref_fixtures as rf

pytestmark = pytest.mark.gpu

ONE_CALL = [n for n in rf.SCORE_NAMES if rf.load(n).k <= (14 if rf.load(n).sigma == 4 else 6)]   # what one call takes (max_k)
KEY_RANGE = [n for n in rf.SCORE_NAMES if n not in ONE_CALL]                                        # DNA k = 15, 16
VARIANT_OK = [n for n in ONE_CALL if rf.load(n).k <= (12 if rf.load(n).sigma == 4 else 6)]        # every variant exists there
K13_K14 = [n for n in ONE_CALL if rf.load(n).k >= 13]
# the positioned key-major call takes the exact partition, which the library offers from 65 keys on (DNA k >= 4)
KM_POSITIONS = [n for n in ONE_CALL if rf.load(n).sigma ** rf.load(n).k > 64]


def check_group_major(engine, fx, device=False):
    mats = fx.mats
    if device:
        import torch
        mats = torch.from_numpy(fx.mats).cuda()
    res = engine.score_groups(mats, fx.mat_group, fx.k, fx.eps)
    try:
        assert res.group_ids.tolist() == fx.group_ids
        for gi in range(len(fx.group_ids)):
            gk, gs = res.group(gi)
            assert np.array_equal(gk, fx.keys[gi]), f"{fx.name} group {gi}: key sets differ ({len(gk)} vs {len(fx.keys[gi])})"
            assert np.array_equal(gs.view(np.uint32), fx.score_bits[gi]), f"{fx.name} group {gi}: score bits differ"
        assert res.emitted == sum(fx.emitted), f"{fx.name}: scored count {res.emitted} vs {sum(fx.emitted)}"
    finally:
        res.free()


def shard(fx, owner, world):
    """Owner's part of the fixture's key-major database: (keys, offsets, branches, score bits, positions)."""
    keys, off, br, sc, pos = fx.db()
    off = off.astype(np.int64)
    mine = (dbo.dense_code(keys, fx.sigma, fx.k) % np.uint64(world)) == np.uint64(owner)
    counts = np.diff(off)
    ent = np.repeat(mine, counts)
    return keys[mine], np.concatenate([[0], np.cumsum(counts[mine])]).astype(np.uint64), br[ent], sc[ent], pos[ent]


def assert_db(db, want, what, positions=False):
    br, sc = db.entries()
    assert np.array_equal(db.keys(), want[0]), f"{what}: keys differ"
    assert np.array_equal(db.key_offsets(), want[1]), f"{what}: offsets differ"
    assert np.array_equal(br, want[2]), f"{what}: branches differ"
    assert np.array_equal(sc.view(np.uint32), want[3]), f"{what}: score bits differ"
    if positions:
        assert np.array_equal(db.positions(), want[4]), f"{what}: positions differ"


# ---- group-major ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ONE_CALL)
def test_score_groups_host_and_device_input(engine, name):
    fx = rf.load(name)
    check_group_major(engine, fx)
    check_group_major(engine, fx, device=True)


@pytest.mark.parametrize("variant", [1, 3, 4, 6, 7])
@pytest.mark.parametrize("name", VARIANT_OK)
def test_every_scoring_variant(engine, name, variant):
    """The global-atomic reduce (1), the exact partition with dense and compressed tables (3, 4), the chunk-fed LDS reduce in both
    table forms (6, 7): the reference's sets from each."""
    engine.set_option("variant", variant)
    try:
        check_group_major(engine, rf.load(name))
    finally:
        engine.set_option("variant", 0)


@pytest.mark.parametrize("name", K13_K14)
def test_k13_k14_with_list_slicing_on(engine, name):
    engine.set_option("slice_long_lists", 1)
    try:
        check_group_major(engine, rf.load(name))
    finally:
        engine.set_option("slice_long_lists", 0)


@pytest.mark.parametrize("name", ONE_CALL)
def test_score_groups_positions(engine, name):
    fx = rf.load(name)
    res = engine.score_groups_positions(fx.mats, fx.mat_group, fx.k, fx.eps)
    try:
        assert res.group_ids.tolist() == fx.group_ids
        for gi in range(len(fx.group_ids)):
            a, b = int(res.offsets[gi]), int(res.offsets[gi + 1])
            assert np.array_equal(res.keys()[a:b], fx.keys[gi]), f"group {gi}: key sets differ"
            assert np.array_equal(res.scores()[a:b].view(np.uint32), fx.score_bits[gi]), f"group {gi}: score bits differ"
            assert np.array_equal(res.positions()[a:b], fx.positions[gi]), f"group {gi}: first-window positions differ"
        assert res.emitted == sum(fx.emitted)
    finally:
        res.free()


# ---- key-major -------------------------------------------------------------------------------------------------------------------

def test_keymajor_positions_refuses_tiny_key_spaces(engine):
    """DNA k = 2, 3 (at most 64 keys) have no positioned key-major call: it must say so, not return something else."""
    fx = rf.load("grid_dna_k3")
    with pytest.raises(ipk_amd.IpkGpuError):
        engine.score_groups_keymajor_positions(fx.mats, fx.mat_group, fx.k, fx.eps)


@pytest.mark.parametrize("name", ONE_CALL)
def test_keymajor_one_and_three_owners(engine, name):
    fx = rf.load(name)
    parts = engine.score_groups_keymajor(fx.mats, fx.mat_group, fx.k, fx.eps, n_owners=1)
    assert parts.emitted == sum(fx.emitted)
    db = engine.db_from_parts(parts, fx.sigma, fx.k)
    assert_db(db, shard(fx, 0, 1), fx.name)
    db.free(); parts.free()
    world = 3
    parts = engine.score_groups_keymajor(fx.mats, fx.mat_group, fx.k, fx.eps, n_owners=world)
    assert parts.emitted == sum(fx.emitted)
    for o in range(world):
        a, b = int(parts.owner_offsets[o]), int(parts.owner_offsets[o + 1])
        db = engine.merge_parts(fx.sigma, fx.k, o, world, parts.counts_tensor()[o:o + 1].contiguous(),
                                parts.entries_tensor()[a:b].contiguous(), np.zeros(1, np.uint64))
        assert_db(db, shard(fx, o, world), f"{fx.name} owner {o}")
        db.free()
    parts.free()


@pytest.mark.parametrize("name", KM_POSITIONS)
def test_keymajor_positions(engine, name):
    fx = rf.load(name)
    parts = engine.score_groups_keymajor_positions(fx.mats, fx.mat_group, fx.k, fx.eps)
    assert parts.emitted == sum(fx.emitted)
    db = engine.db_from_parts(parts, fx.sigma, fx.k)
    assert_db(db, shard(fx, 0, 1), fx.name, positions=True)
    db.free(); parts.free()


@pytest.mark.parametrize("name", KEY_RANGE)
def test_key_range_passes(engine, name):
    """DNA k = 15, 16 as tests/test_gpu_keyrange.py::check_passes drives them: every class against its range of the database."""
    fx = rf.load(name)
    k, lead = fx.k, fx.k - 14
    ok, ooff, obr, osc, _ = fx.db()
    ooff = ooff.astype(np.int64)
    total, seen = 0, 0
    for j, cls, base, span in keyrange.plan(4, k, 4 ** lead):
        parts = engine.score_groups_keyrange(fx.mats, fx.mat_group, k, fx.eps, j, cls)
        assert parts.key_base == base and parts.slots == span
        total += parts.emitted
        db = engine.db_from_parts(parts, 4, k)
        a, b = np.searchsorted(ok, [base, base + span]) if base + span < 2 ** 32 else (np.searchsorted(ok, base), len(ok))
        keys, off = db.keys(), db.key_offsets().astype(np.int64)
        br, sc = db.entries()
        assert np.array_equal(keys, ok[a:b]), (name, cls)
        assert np.array_equal(off, ooff[a:b + 1] - ooff[a])
        assert np.array_equal(br, obr[ooff[a]:ooff[b]]) and np.array_equal(sc.view(np.uint32), osc[ooff[a]:ooff[b]])
        seen += len(keys)
        db.free(); parts.free()
    assert seen == len(ok) and total == sum(fx.emitted)


# ---- MIF0 past one 64-entry chunk ------------------------------------------------------------------------------------------------

def _mif0_database(n_groups, alpha, beta, seed, positive_group=None):
    """n_groups groups of one 3-site matrix (one window, k = 3).  Group g admits symbol a at the second site iff g < alpha[a] and
    symbol b at the third iff g < beta[b] (the first site admits symbol 0 only), so the k-mer (0, a, b) has an entry from exactly
    min(alpha[a], beta[b]) groups.  Admitted symbols get random log-probabilities, some exactly 0; the rest are -inf."""
    rng = np.random.default_rng(seed)
    mats = np.full((n_groups, 3, 4), -np.inf, dtype=np.float32)
    g = np.arange(n_groups)
    mats[:, 0, 0] = np.where(rng.random(n_groups) < 0.2, 0.0, -rng.random(n_groups)).astype(np.float32)
    for s in range(4):
        mats[g < alpha[s], 1, s] = -rng.random(int((g < alpha[s]).sum())).astype(np.float32)
        mats[g < beta[s], 2, s] = -rng.random(int((g < beta[s]).sum())).astype(np.float32)
    mats[0, :, 0] = 0.0                                              # the k-mer (0, 0, 0) of group 0 scores exactly 0.0f
    if positive_group is not None:
        mats[positive_group, 0, 0] = np.float32(2.5)                 # positive log scores: the clamp to a probability of 1
    return mats, (np.arange(n_groups, dtype=np.uint32) * 3 + 2)


def _reference_mif0(lists, N, thr):
    if rb.available():
        return rb.ref_mif0(lists, N, thr)
    return np.array([co.mif0(s, N, thr) for s in lists], dtype=np.float64)     # pinned by tests/test_ref_pin.py


@pytest.mark.parametrize("case", ["chunk_edges", "every_key_in_every_group"])
def test_mif0_beyond_one_chunk(engine, case):
    """mif0_kernel takes a k-mer's entries 64 at a time: entry lists of 1, 63, 64, 65, 128, 129 and 200 entries (whole chunks,
    a partial last chunk, N == n and N > n) against the reference's filter.cpp; relative 1e-9 as in
    test_mif0_filter_values_and_order (the device's pow / log2 may differ from the host's in the last bit)."""
    if case == "chunk_edges":
        n_groups, N = 200, 200
        mats, groups = _mif0_database(n_groups, [200, 129, 128, 65], [200, 64, 63, 1], 64, positive_group=5)
        want_counts = {1, 63, 64, 65, 128, 129, 200}
    else:
        n_groups, N = 130, 130                                       # two whole chunks and a last one of 2; N == n for every key
        mats, groups = _mif0_database(n_groups, [130] * 4, [130] * 4, 65)
        want_counts = {130}
    k, sigma = 3, 4
    thr = ipk_amd.score_threshold(1.5, sigma, k)
    parts = engine.score_groups_keymajor(mats, groups, k, np.float32(-50.0), n_owners=1)
    db = engine.db_from_parts(parts, sigma, k)
    try:
        off = db.key_offsets().astype(np.int64)
        _, sc = db.entries()
        counts = np.diff(off)
        assert want_counts <= set(counts.tolist()) and db.num_keys == 16
        if case == "chunk_edges":
            assert (sc == 0.0).any() and (sc > 0.0).any()
        else:
            assert np.all(counts == N)
        lists = [sc[off[i]:off[i + 1]] for i in range(db.num_keys)]
        ref = _reference_mif0(lists, N, thr)
        db.filter_mif0(engine, N, thr)
        fv64, fv32, order = db.filter_values(f64=True), db.filter_values(), db.filter_order()
        for i in range(db.num_keys):
            print(f"{case} key {i}: n = {counts[i]}, device {fv64[i]!r}, reference {ref[i]!r}")
            assert abs(fv64[i] - ref[i]) <= 1e-9 * max(1.0, abs(ref[i])), (i, int(counts[i]), fv64[i], ref[i])
        assert np.array_equal(fv32.view(np.uint32), fv64.astype(np.float32).view(np.uint32))
        assert np.array_equal(order, np.argsort(fv32, kind="stable").astype(order.dtype))
    finally:
        db.free(); parts.free()


# ---- the live binaries ---------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not rb.available(), reason="the reference binaries are not in oracle/_ref/ (they are built where the reference "
                    "tree is and carried along; nothing of the reference tree itself is read here)")
def test_score_groups_against_the_live_reference(engine):
    rng = np.random.default_rng(int(os.environ.get("IPK_TEST_SEED", "20261019")))
    n_cases = int(os.environ.get("IPK_REF_CASES", "30"))
    cases = [rf.random_case(rng) for _ in range(n_cases)]
    cases.append(("tenth", gen.tenth_matrices(4, 40, 4, 3), 4, 8, float(np.float32(-2.5))))   # rounded inner bounds decide k-mers here
    families = {}
    for case, (family, mats, sigma, k, eps) in enumerate(cases):
        families[family] = families.get(family, 0) + 1
        n_mats = len(mats)
        groups = (rng.integers(0, max(1, n_mats // 2 + 1), size=n_mats).astype(np.uint32) * 11 + 3)
        order = list(dict.fromkeys(groups.tolist()))
        per_matrix = rb.ref_windows_many(mats, k, eps, sigma)
        res = engine.score_groups(mats, groups, k, eps)
        try:
            assert res.group_ids.tolist() == order, case
            emitted = 0
            for gi, gid in enumerate(order):
                keys, scores, e = rb.merge_windows([per_matrix[i] for i in np.flatnonzero(groups == gid)])
                gk, gs = res.group(gi)
                assert np.array_equal(gk, keys), (case, family, sigma, k, "keys")
                assert np.array_equal(gs.view(np.uint32), scores.view(np.uint32)), (case, family, sigma, k, "score bits")
                emitted += e
            assert res.emitted == emitted, (case, family, sigma, k, res.emitted, emitted)
        finally:
            res.free()
    print(f"live sweep on the device: {len(cases)} cases {families}, no difference")
    assert families.get("grid", 0) >= n_cases // 4 and families.get("synth", 0) >= n_cases // 4
