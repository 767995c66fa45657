"""GPU suite: the option "slice_long_lists" -- DNA k >= 13 windows whose half lists exceed the big-list kernels' capped capacity
(6144 entries) are scored one class of leading symbols at a time instead of failing the call.  Every comparison is exact (key sets,
raw score bits, scored counts, positions, file bytes) against the oracle; the inputs are pinned by tests/test_long_lists_inputs.py.
The engine fixture is shared by the session: every test restores the option."""
import contextlib
import functools

import numpy as np
import pytest
from click.testing import CliRunner

import ipk_amd
from ipk_amd import cli, dbfile, keyrange
from ipk_amd import distributed as D
from ipk_amd.synth import synth_matrices
from oracle import ar_oracle
from oracle import db_oracle as dbo
from oracle import ipk_oracle as co
from tests import long_lists as ll

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def slicing(engine, on=1):
    """The option at `on`, restored to the default afterwards; yields a function that tells the windows sliced since."""
    engine.set_option("slice_long_lists", on)
    before = engine.get_option("debug_sliced_windows")
    try:
        yield lambda: engine.get_option("debug_sliced_windows") - before
    finally:
        engine.set_option("slice_long_lists", 0)


@functools.lru_cache(maxsize=None)
def oracle_groups(name):
    """The oracle's per-group results of a named input, computed once: (mats, groups, eps, [(gid, keys, scores)], emitted)."""
    if name == "k13":
        mats, eps = ll.k13_input()
        groups, k = np.array([7, 7], dtype=np.uint32), 13
    elif name == "k13x2":                                # the same matrices as two groups (the on-disk build cuts between groups)
        mats, eps = ll.k13_input()
        groups, k = np.array([5, 9], dtype=np.uint32), 13
    else:
        k = int(name[1:])
        mats, groups, eps = ll.keyrange_input(k)
    res, emitted = [], 0
    for gid in dict.fromkeys(groups.tolist()):
        keys, scores, e = co.explore_group(mats[groups == gid], k, eps)
        res.append((gid, keys, scores))
        emitted += e
    return mats, groups, eps, res, emitted


def oracle_db(name, k):
    return dbo.db_shard_arrays(dbo.build_db(oracle_groups(name)[3]), 4, k, 0, 1)


def check_per_branch(engine, name, k):
    """The comparison of tests/test_gpu_parity.py::check_against_oracle, against the cached oracle result."""
    mats, groups, eps, want, emitted = oracle_groups(name)
    res = engine.score_groups(mats, groups, k, eps)
    assert res.group_ids.tolist() == [g for g, _, _ in want]
    for gi, (gid, keys, scores) in enumerate(want):
        gk, gs = res.group(gi)
        assert np.array_equal(gk, keys), f"group {gid}: key sets differ ({len(gk)} vs {len(keys)})"
        assert np.array_equal(gs.view(np.uint32), scores.view(np.uint32)), f"group {gid}: score bits differ"
    assert res.emitted == emitted
    res.free()


def check_database(engine, name, k, n_owners=1):
    """distributed.build_db_shard against the oracle's arrays, entry for entry."""
    mats, groups, eps, _, emitted = oracle_groups(name)
    ok, ooff, obr, osc = oracle_db(name, k)
    db, parts = D.build_db_shard(engine, mats, groups, k, eps, 4)
    assert parts.emitted == emitted
    br, sc = db.entries()
    assert np.array_equal(db.keys(), ok) and np.array_equal(db.key_offsets(), ooff)
    assert np.array_equal(br, obr) and np.array_equal(sc.view(np.uint32), osc)
    db.free(); parts.free()


# ---- 1: k = 13, the right half beyond the cap ------------------------------------------------------------------------------------

def test_k13_fails_by_default_and_matches_the_oracle_in_slices(engine):
    mats, groups, eps, _, _ = oracle_groups("k13")
    with pytest.raises(ipk_amd.IpkGpuError):
        engine.score_groups(mats, groups, 13, eps)
    with slicing(engine) as sliced:
        check_per_branch(engine, "k13", 13)
        assert sliced() == 3                              # the three windows of the first matrix: |R| = 4^7
        check_database(engine, "k13", 13)


# ---- 2: k = 14, both halves beyond the cap ---------------------------------------------------------------------------------------

def test_k14_both_halves_sliced(engine):
    with slicing(engine) as sliced:
        check_per_branch(engine, "k14", 14)
        assert sliced() == 4                              # two windows of each graded matrix; the ordinary group's fit
        check_database(engine, "k14", 14)


# ---- 3: key-range passes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,lead", [(15, 1), (16, 2), (14, 1)])
def test_key_range_passes(engine, k, lead):
    """As tests/test_gpu_keyrange.py::check_passes: every class against the oracle's range of the database, the counts summed."""
    mats, groups, eps, _, emitted = oracle_groups(f"k{k}")
    ok, ooff, obr, osc = oracle_db(f"k{k}", k)
    ooff = ooff.astype(np.int64)
    total, seen = 0, 0
    with slicing(engine) as sliced:
        for j, cls, base, span in keyrange.plan(4, k, 4 ** lead):
            parts = engine.score_groups_keyrange(mats, groups, k, eps, j, cls)
            assert parts.key_base == base and parts.slots == span
            total += parts.emitted
            db = engine.db_from_parts(parts, 4, k)
            a, b = np.searchsorted(ok, [base, base + span]) if base + span < 2 ** 32 else (np.searchsorted(ok, base), len(ok))
            keys, off = db.keys(), db.key_offsets().astype(np.int64)
            br, sc = db.entries()
            assert np.array_equal(keys, ok[a:b]), (k, lead, cls)
            assert np.array_equal(off, ooff[a:b + 1] - ooff[a])
            assert np.array_equal(br, obr[ooff[a]:ooff[b]]) and np.array_equal(sc.view(np.uint32), osc[ooff[a]:ooff[b]])
            seen += len(keys)
            db.free(); parts.free()
        assert sliced() > 0
    assert seen == len(ok) and total == emitted


# ---- 4: every slice full ---------------------------------------------------------------------------------------------------------

def _check_flat(db, parts, k, n_keys):
    bits = ll.split_sum_bits(np.float32(np.log10(0.25)), k)
    assert db.num_keys == n_keys and db.num_entries == n_keys and parts.emitted == 2 * n_keys
    keys = db.keys()
    assert keys[0] == 0 and keys[-1] == n_keys - 1 and np.all(np.diff(keys.astype(np.int64)) == 1)
    del keys
    br, sc = db.entries()
    assert np.all(br == 3) and np.all(sc.view(np.uint32) == bits)


def test_flat_columns_k13_whole_key_space(engine):
    mats, eps = ll.flat_input(13)
    with slicing(engine) as sliced:
        parts = engine.score_groups_keymajor(mats, np.array([3, 3], dtype=np.uint32), 13, eps)
        assert sliced() == 2
        db = engine.db_from_parts(parts, 4, 13)
        _check_flat(db, parts, 13, 4 ** 13)
        db.free(); parts.free()


def test_flat_columns_k15_one_class(engine):
    mats, eps = ll.flat_input(15)
    with slicing(engine) as sliced:
        parts = engine.score_groups_keyrange(mats, np.array([3, 3], dtype=np.uint32), 15, eps, 2, 0)
        assert sliced() == 2 and parts.key_base == 0 and parts.slots == 4 ** 13
        db = engine.db_from_parts(parts, 4, 15)
        _check_flat(db, parts, 15, 4 ** 13)
        db.free(); parts.free()


# ---- 5: positions ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _k13_positions_oracle():
    from tests.test_gpu_positions_db import oracle_positions_db
    mats, groups, eps, _, _ = oracle_groups("k13")
    return oracle_positions_db(mats, groups, 13, eps)


def test_positioned_database(engine):
    from tests.test_gpu_positions_db import assert_same, positioned
    mats, groups, eps, _, _ = oracle_groups("k13")
    want = _k13_positions_oracle()
    with slicing(engine) as sliced:
        got = positioned(engine, mats, groups, 13, eps)
        assert sliced() == 3
    assert_same(got[:5], want[:5])
    assert got[5] == want[5], "scored phylo-k-mer count differs"
    # the two matrices score some k-mers alike: those keep the earlier window (sequence = matrix rank * windows + start)
    assert len(np.unique(got[4])) > 1


def test_positioned_database_with_owners(engine):
    from tests.test_gpu_positions_ranks import check_owners
    mats, groups, eps, _, _ = oracle_groups("k13")
    want = _k13_positions_oracle()
    with slicing(engine):
        parts = engine.score_groups_keymajor_positions_owners(mats, groups, 13, eps, n_owners=2)
        assert parts.emitted == want[5] and parts.num_entries == len(want[2])
        check_owners(engine, [parts], want, 4, 13, 2)
        parts.free()


def test_group_major_positions(engine):
    mats, groups, eps, _, _ = oracle_groups("k13")
    keys, scores, pos, emitted = co.explore_group_pos(mats, 13, eps)
    with pytest.raises(ipk_amd.IpkGpuError):
        engine.score_groups_positions(mats, groups, 13, eps)
    with slicing(engine) as sliced:
        res = engine.score_groups_positions(mats, groups, 13, eps)
        assert sliced() == 3
    gk, gs = res.group(0)
    assert np.array_equal(gk, keys) and np.array_equal(gs.view(np.uint32), scores.view(np.uint32))
    assert np.array_equal(res.positions(), pos) and res.emitted == emitted
    res.free()


# ---- 6: nothing changes where nothing is sliced ----------------------------------------------------------------------------------

def test_ordinary_input_writes_the_same_bytes(engine, tmp_path):
    from tests.test_gpu_ondisk import _in_memory_file
    mats = synth_matrices(4, 200, 4, 0.1, 1406)
    groups = np.array([5, 5, 9, 9], dtype=np.uint32)
    off = _in_memory_file(engine, mats, groups, 14, 4, tmp_path / "off.ipk", "mif0", 11)
    with slicing(engine) as sliced:
        on = _in_memory_file(engine, mats, groups, 14, 4, tmp_path / "on.ipk", "mif0", 11)
        assert sliced() == 0
    assert on == off and (tmp_path / "on.ipk").read_bytes() == (tmp_path / "off.ipk").read_bytes()


# ---- 7: on disk ------------------------------------------------------------------------------------------------------------------

def test_on_disk_pieces(engine, tmp_path):
    from tests.test_gpu_ondisk import _in_memory_file, _on_disk_file
    mats, groups, eps, _, emitted = oracle_groups("k13x2")
    assert eps == co.log_threshold(1.5, 4, 13)                   # (the threshold the two builders of test_gpu_ondisk use)
    with slicing(engine) as sliced:
        n_keys, n_entries, e = _in_memory_file(engine, mats, groups, 13, 4, tmp_path / "mem.ipk", "mif0", 5)
        assert e == emitted and sliced() == 3
        r = _on_disk_file(engine, mats, groups, 13, 4, tmp_path / "disk.ipk", tmp_path / "w", "mif0", 5, budget_bytes=4 << 30)
        assert sliced() == 6
    assert r["pieces"] >= 2 and r["emitted"] == emitted and r["totals"] == (n_keys, n_entries)
    assert (tmp_path / "disk.ipk").read_bytes() == (tmp_path / "mem.ipk").read_bytes()
    ok = oracle_db("k13x2", 13)[0]
    assert n_keys == len(ok)


# ---- 8: the command line ---------------------------------------------------------------------------------------------------------

def test_cli_builds_k13(tmp_path):
    """`ipk.py build -k 13` sets the option on its own engine: the build completes (it ended in the capped-lists error before) and
    its records equal the oracle pipeline on the matrices as read back from the file."""
    k = 13
    ar_dir = tmp_path / "AR"; ar_dir.mkdir()
    mats, _ = ll.k13_input()
    ll.write_probs_file(ar_dir / "ar.raxml.ancestralProbs", ll.CLI_LABELS, mats)
    with open(tmp_path / "map.tsv", "w") as fh:
        for lab in ll.CLI_LABELS:
            fh.write(f"{lab}\t7\n")
    out = tmp_path / "DB.ipk"
    res = CliRunner().invoke(cli.ipk, ["build", "-w", str(tmp_path), "--ar-dir", str(ar_dir), "--mapping", str(tmp_path / "map.tsv"),
                                       "-k", str(k), "--omega", str(ll.CLI_OMEGA), "-o", str(out), "--num-tree-nodes", "3"])
    assert res.exit_code == 0, (res.output, res.exception)
    hdr, (keys, fvs, counts, eoff, br, sc) = dbfile.read_db(out, as_arrays=True)
    back, _ = ar_oracle.read_file(ar_dir / "ar.raxml.ancestralProbs", 4)
    gk, gs, _ = co.explore_group(np.stack([back[lab] for lab in ll.CLI_LABELS]), k, co.log_threshold(ll.CLI_OMEGA, 4, k))
    ok, ooff, obr, osc = dbo.db_shard_arrays(dbo.build_db([(7, gk, gs)]), 4, k, 0, 1)
    ooff = ooff.astype(np.int64)
    assert hdr["kmer_size"] == k and hdr["total_num_kmers"] == len(ok) and hdr["total_num_entries"] == len(obr)
    assert np.all(np.diff(fvs) >= 0) and len(np.unique(keys)) == len(keys) == len(ok)
    pos = np.searchsorted(ok, keys)
    assert np.array_equal(ok[pos], keys)
    assert np.array_equal(counts, (ooff[pos + 1] - ooff[pos]).astype(np.uint64))
    assert np.all(counts == 1)                                   # one group: every record has one entry, ooff[pos] is its row
    assert np.array_equal(br, obr[ooff[pos]]) and np.array_equal(sc.view(np.uint32), osc[ooff[pos]])
    thr = co.score_threshold(ll.CLI_OMEGA, 4, k)
    for i in np.linspace(0, len(keys) - 1, 50).astype(np.int64):
        ref = co.mif0(osc[ooff[pos[i]]:ooff[pos[i] + 1]].view(np.float32), 3, thr)
        assert abs(fvs[i] - ref) <= 1e-6 * max(1.0, abs(ref))
