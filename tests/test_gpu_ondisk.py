"""GPU suite: the on-disk build -- spill blocks (ipkgpu_parts_spill / ipkgpu_spill_merge), the device budget and ipk_amd/ondisk.py.
Every comparison is bit for bit or byte for byte."""
import os

import numpy as np
import pytest
import torch
from click.testing import CliRunner

import ipk_amd
from ipk_amd import cli, dbfile, ondisk
from ipk_amd import distributed as D
from ipk_amd.synth import synth_matrices
from oracle import ipk_oracle as co
from tests import db_check as dc

pytestmark = pytest.mark.gpu

TREE_INDEX, NEWICK, OMEGA = [(1, 0.0), (3, 0.5), (5, 1.0)], "((a:1,b:1):1,c:1);", 1.5
MIB = 1 << 20


def _groups(n_groups, per_group=2, first=5):
    return np.repeat(np.arange(first, first + n_groups, dtype=np.uint32), per_group)


def _eps(sigma, k):
    return co.log_threshold(OMEGA, sigma, k)


def _in_memory_file(engine, mats, groups, k, sigma, path, filt, n_nodes):
    """The default build: one key-major call, filter, file.  Returns (k-mers, entries, scored count)."""
    seq = "DNA" if sigma == 4 else "AA"
    db, parts = D.build_db_shard(engine, mats, groups, k, _eps(sigma, k), sigma)
    if filt == "mif0":
        db.filter_mif0(engine, n_nodes, ipk_amd.score_threshold(OMEGA, sigma, k))
        dbfile.write_db_device(engine, db, path, seq, TREE_INDEX, NEWICK, k, OMEGA)
    else:
        keys = db.keys()
        fv = (dbfile.splitmix_unit(keys) if db.num_keys else np.zeros(0)).astype(np.float32)
        order = np.argsort(dbfile.filter_sort_code(fv, keys), kind="stable")
        br, sc = db.entries()
        dbfile.write_db(path, seq, TREE_INDEX, NEWICK, k, OMEGA, keys, db.key_offsets(), br, sc, fv, order)
    out = (db.num_keys, db.num_entries, parts.emitted)
    db.free(); parts.free()
    return out


def _on_disk_file(engine, mats, groups, k, sigma, path, work, filt, n_nodes, **kw):
    return ondisk.build_db_file(engine, mats, groups, k, _eps(sigma, k), sigma, str(path), str(work), "DNA" if sigma == 4 else "AA",
                                TREE_INDEX, NEWICK, OMEGA, filt, n_nodes, **kw)


def _db_arrays(db):
    br, sc = db.entries()
    return db.keys().copy(), db.key_offsets().copy(), br, sc.view(np.uint32)


# ---- 1, 2: the round trip of a piece's blocks, and their bytes -----------------------------------------------------------------

SHAPES = [(4, 8, 32, 300, 3), (4, 12, 32, 400, 3), (4, 12, 5, 400, 3), (20, 4, 32, 120, 2), (20, 6, 32, 300, 2), (4, 13, 32, 100, 2),
          (4, 2, 32, 40, 3)]


@pytest.mark.parametrize("sigma,k,B,sites,n_groups", SHAPES)
def test_blocks_round_trip(engine, tmp_path, sigma, k, B, sites, n_groups):
    """Parts split B ways are spilled and come back: every block's bits, u16 counts and entries are what numpy derives from the
    parts' own rows, the row rebuilt from them is the parts' row, and the database ipkgpu_spill_merge makes of one block equals
    the one ipkgpu_merge_parts_ptrs makes of the same block while it is still on the device."""
    groups = _groups(n_groups)
    mats = synth_matrices(len(groups), sites, sigma, 0.1 if sigma == 4 else 0.03, 900 + k)
    parts = engine.score_groups_keymajor(mats, groups, k, _eps(sigma, k), n_owners=B)
    assert parts.n_owners == B and parts.num_entries > 0
    counts = parts.counts_tensor().cpu().numpy().view(np.uint32)
    entries = parts.entries_tensor().cpu().numpy().view(np.uint32)
    written = engine.parts_spill(parts, tmp_path, 7)
    size, empty = 0, 0
    for o in range(B):
        path = ondisk.block_path(tmp_path, 7, o)
        size += os.path.getsize(path)
        blk = ondisk.read_block(path)
        a, b = int(parts.owner_offsets[o]), int(parts.owner_offsets[o + 1])
        assert (blk["sigma"], blk["k"], blk["n_owners"], blk["owner"], blk["piece"], blk["slots"]) == (sigma, k, B, o, 7, parts.slots)
        bits, c16 = ondisk.pack_counts(counts[o])
        assert blk["n_keys"] == len(c16) and blk["n_entries"] == b - a
        assert np.array_equal(blk["bits"], bits) and np.array_equal(blk["counts"], c16)
        assert np.array_equal(blk["entries"], entries[a:b])
        # the dense row back out of the block's bits and counts
        occ = np.unpackbits(blk["bits"].view(np.uint8), bitorder="little")[:parts.slots].astype(bool)
        row = np.zeros(parts.slots, dtype=np.uint32)
        row[occ] = blk["counts"]
        assert np.array_equal(row, counts[o])
        empty += b == a
        got = engine.spill_merge(sigma, k, o, B, [path])
        want = engine.merge_parts_ptrs(sigma, k, o, B, [parts.counts_ptr() + 4 * o * parts.slots], [parts.entries_ptr() + 8 * a])
        for name, x, y in zip(("keys", "key offsets", "branches", "score bits"), _db_arrays(got), _db_arrays(want)):
            assert np.array_equal(x, y), (name, o)
        got.free(); want.free()
    assert written == size
    assert size <= B * parts.slots * 4 + 8 * parts.num_entries + 72 * B      # never larger than the dense rows (heads and padding aside)
    if k == 2:
        assert empty >= 16                                                    # 16 keys, 32 owners: blocks without a key are files too
    parts.free()


def test_a_piece_without_matrices(engine, tmp_path):
    """n_mats = 0: B blocks of head and zero bits; merged beside a real piece they change nothing."""
    sigma, k, B = 4, 8, 4
    groups = _groups(2)
    mats = synth_matrices(4, 200, sigma, 0.1, 31)
    none = engine.score_groups_keymajor(np.zeros((0, 200, sigma), np.float32), np.zeros(0, np.uint32), k, _eps(sigma, k), n_owners=B)
    some = engine.score_groups_keymajor(mats, groups, k, _eps(sigma, k), n_owners=B)
    engine.parts_spill(none, tmp_path, 0)
    engine.parts_spill(some, tmp_path, 1)
    for o in range(B):
        blk = ondisk.read_block(ondisk.block_path(tmp_path, 0, o))
        assert blk["n_keys"] == 0 and blk["n_entries"] == 0 and not blk["bits"].any()
        assert os.path.getsize(ondisk.block_path(tmp_path, 0, o)) == 64 + 8 * ((some.slots + 63) // 64)
        both = engine.spill_merge(sigma, k, o, B, [ondisk.block_path(tmp_path, 0, o), ondisk.block_path(tmp_path, 1, o)])
        one = engine.spill_merge(sigma, k, o, B, [ondisk.block_path(tmp_path, 1, o)])
        for x, y in zip(_db_arrays(both), _db_arrays(one)):
            assert np.array_equal(x, y)
        both.free(); one.free()
    none.free(); some.free()


# ---- 3: every batch against the oracle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sigma,k,sites", [(4, 10, 600), (20, 5, 200)])
def test_batches_match_the_oracle(engine, tmp_path, sigma, k, sites):
    B, n_groups, cuts = 8, 9, [0, 4, 5, 9]
    groups = _groups(n_groups)
    alpha = 0.05 if sigma == 4 else 0.03
    mats = synth_matrices(len(groups), sites, sigma, alpha, 4000 + k)
    eps = _eps(sigma, k)
    gids = list(dict.fromkeys(groups.tolist()))
    expect = dc.oracle_digests(lambda gid: mats[groups == gid], gids, k, eps, sigma, world=B)
    emitted = 0
    for p in range(len(cuts) - 1):
        sel = slice(2 * cuts[p], 2 * cuts[p + 1])
        parts = engine.score_groups_keymajor(mats[sel], groups[sel], k, eps, n_owners=B)
        emitted += parts.emitted
        engine.parts_spill(parts, tmp_path, p)
        parts.free()
    assert emitted == sum(expect[g].emitted for g in gids)
    for b in range(B):
        db = engine.spill_merge(sigma, k, b, B, [ondisk.block_path(tmp_path, p, b) for p in range(len(cuts) - 1)])
        keys, off, entries = dc.db_tensors(db)
        dc.check_db(keys, off, entries, gids, expect, sigma, k, owner=b, world=B)
        del keys, off, entries
        db.free()


# ---- 4: the same file as the in-memory build ------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", ["mif0", "random"])
@pytest.mark.parametrize("sigma,k,sites", [(4, 8, 300), (4, 12, 300), (20, 6, 150)])
def test_same_file_as_the_in_memory_build(tmp_path, sigma, k, sites, filt):
    """Whatever the piece cuts and the batch count, with interleaved group ids in the input."""
    engine = ipk_amd.Engine(0)
    try:
        _same_file(engine, tmp_path, sigma, k, sites, filt)
    finally:
        engine.close()


def _same_file(engine, tmp_path, sigma, k, sites, filt):
    n_groups = 7
    groups = np.array([9, 4, 9, 11, 4, 2, 30, 11, 2, 6, 30, 8, 6, 8], dtype=np.uint32)          # 7 groups, their matrices interleaved
    mats = synth_matrices(len(groups), sites, sigma, 0.1 if sigma == 4 else 0.03, 77 + k)
    one = tmp_path / "one.ipk"
    n_keys, n_entries, emitted = _in_memory_file(engine, mats, groups, k, sigma, one, filt, 15)
    want = one.read_bytes()
    cases = [(32, [n_groups]), (32, [1]), (5, [2, 1, 4]), (1, [3, 4])] if (sigma, k) == (4, 8) else [(5, [2, 1, 4]), (32, [1])]
    for i, (B, sizes) in enumerate(cases):
        out, work = tmp_path / f"ondisk{i}.ipk", tmp_path / f"w{i}"
        r = _on_disk_file(engine, mats, groups, k, sigma, out, work, filt, 15, batches=B, budget_bytes=8 << 30, piece_sizes=sizes)
        assert r["totals"] == (n_keys, n_entries) and r["emitted"] == emitted and r["batches"] == B
        assert [g1 - g0 for g0, g1 in r["piece_ranges"]][:len(sizes)] == sizes[:r["pieces"]]
        assert out.read_bytes() == want, (B, sizes)
        assert not (work / "hashmaps").exists()
        assert r["spilled_bytes"] <= r["dense_bytes"] + 72 * B * r["pieces"]
    assert engine.get_option("device_budget_bytes") == 0                     # the builder restores the options it sets


def test_planner_cuts_and_kept_files(tmp_path):
    """The builder's own cuts (first piece one group, then by the bytes seen) under a budget that forces several pieces."""
    sigma, k = 4, 10
    groups = _groups(24)
    mats = synth_matrices(len(groups), 1000, sigma, 0.05, 5)
    eng = ipk_amd.Engine(0)
    try:
        one = tmp_path / "one.ipk"
        _in_memory_file(eng, mats, groups, k, sigma, one, "mif0", 49)
        out = tmp_path / "ondisk.ipk"
        r = _on_disk_file(eng, mats, groups, k, sigma, out, tmp_path / "w", "mif0", 49, batches=4, budget_bytes=256 * MIB, keep_files=True)
        assert r["piece_ranges"][0] == (0, 1) and r["pieces"] >= 2 and r["piece_ranges"][-1][1] == 24
        assert r["held_peak"] <= 256 * MIB
        assert out.read_bytes() == one.read_bytes()
        assert sorted(os.listdir(tmp_path / "w" / "hashmaps"))[:4] == ["0.ipk", "1.ipk", "2.ipk", "3.ipk"]
        assert os.path.exists(ondisk.block_path(tmp_path / "w" / "hashmaps", 0, 0))
    finally:
        eng.close()


# ---- 5: the valve ----------------------------------------------------------------------------------------------------------------

# Measured on an MI355X by tools/ondisk_probe.py --floor (cfg2-shaped groups: 2 matrices x 10000 sites, k = 10, alpha 0.05, 32 batches):
VALVE_SITES = 10000
VALVE_FLOOR_BYTES = 325548672             # F: held peak of the on-disk build of VALVE_GROUPS groups with one-group pieces
VALVE_BUDGET = 621 * MIB            # b = 2 F rounded up to a MiB
VALVE_GROUPS = 174                  # G: the database's entries alone (8 bytes each) exceed 2 b


def test_the_valve(tmp_path):
    """A database that does not fit the device is built under a budget it exceeds several times over.

    cfg2-shaped groups (2 matrices x 10000 sites, k = 10, alpha 0.05).  Under device_budget_bytes = b on a fresh engine the in-memory
    key-major call over all G groups fails with IPKGPU_ERR_NOMEM and leaves the engine usable; the on-disk build under the same b
    completes, writes the bytes of an unbudgeted in-memory build, and never holds more than b.
    F (the held peak of an on-disk build of this shape with one-group pieces), b = 2 F rounded up to a MiB and G (the database's
    entries alone, 8 bytes x about 0.95 M per group, exceed 2 b) are measured on the device: VALVE_FLOOR_BYTES, VALVE_BUDGET,
    VALVE_GROUPS above (F = 325548672 bytes, b = 621 MiB, G = 174).  The engine sizes its pair pool by the memory it may count on, so
    the same build given 64 GiB holds 6.1 GB for one group, nearly all of it spare chunks; F is the held peak under the least
    budget (whole MiB, found by bisection, tools/ondisk_probe.py --floor) with which the build with one-group pieces completes."""
    BUDGET, FLOOR_BYTES, GROUPS, SITES = VALVE_BUDGET, VALVE_FLOOR_BYTES, VALVE_GROUPS, VALVE_SITES
    sigma, k = 4, 10
    groups = _groups(GROUPS, first=1)
    mats = np.concatenate([synth_matrices(2 * min(50, GROUPS - g), SITES, sigma, 0.05, 42, first_mat=2 * g) for g in range(0, GROUPS, 50)])
    assert BUDGET >= 2 * FLOOR_BYTES and BUDGET % MIB == 0 and BUDGET - 2 * FLOOR_BYTES < MIB
    eps = _eps(sigma, k)
    plain = ipk_amd.Engine(0)
    try:
        one = tmp_path / "one.ipk"
        n_keys, n_entries, emitted = _in_memory_file(plain, mats, groups, k, sigma, one, "mif0", 2 * GROUPS)
    finally:
        plain.close()
    assert 8 * n_entries > 2 * BUDGET                                          # the entries alone are beyond twice the budget
    eng = ipk_amd.Engine(0)
    try:
        eng.set_option("device_budget_bytes", BUDGET)
        with pytest.raises(ipk_amd.IpkGpuError) as ei:                         # (i) the in-memory call does not fit ...
            eng.score_groups_keymajor(mats, groups, k, eps, n_owners=1)
        assert ei.value.code == 3
        small = eng.score_groups_keymajor(mats[:2], groups[:2], k, eps, n_owners=1)   # ... and the engine still works
        assert small.num_entries > 0
        small.free()
        eng.set_option("device_budget_bytes", 0)
        eng.mem_stats(reset_peak=True)
        out = tmp_path / "ondisk.ipk"
        r = _on_disk_file(eng, mats, groups, k, sigma, out, tmp_path / "w", "mif0", 2 * GROUPS, budget_bytes=BUDGET)   # (ii)
        print(f"valve: F = {FLOOR_BYTES}, b = {BUDGET}, G = {GROUPS}: held_peak {r['held_peak']}, {r['pieces']} pieces, entries {n_entries}, "
              f"stages {r['stage1_s']:.2f} / {r['stage2_s']:.2f} / {r['stage3_s']:.2f} s, spilled {r['spilled_bytes']} bytes")
        assert r["totals"] == (n_keys, n_entries) and r["emitted"] == emitted
        assert out.read_bytes() == one.read_bytes()                            # (iii)
        assert 0 < r["held_peak"] <= BUDGET                                    # (iv)
    finally:
        eng.close()


# ---- 6: a budget below one group's need -----------------------------------------------------------------------------------------

def test_budget_below_one_group(tmp_path):
    sigma, k = 4, 10
    groups = _groups(3)
    mats = synth_matrices(len(groups), 2000, sigma, 0.05, 8)
    eng = ipk_amd.Engine(0)
    try:
        with pytest.raises(ondisk.OnDiskError) as ei:
            _on_disk_file(eng, mats, groups, k, sigma, tmp_path / "never.ipk", tmp_path / "w", "mif0", 7, budget_bytes=2 * MIB)
        msg = str(ei.value)
        assert "one branch group needs at least" in msg and "bytes" in msg and str(2 * MIB) in msg
        need = int(msg.split("at least ")[1].split(" bytes")[0])
        assert need > 2 * MIB
        assert not (tmp_path / "w" / "hashmaps").exists() and not (tmp_path / "never.ipk").exists()
        assert eng.get_option("device_budget_bytes") == 0
        parts = eng.score_groups_keymajor(mats, groups, k, _eps(sigma, k), n_owners=1)       # the engine is usable afterwards
        assert parts.num_entries > 0
        parts.free()
    finally:
        eng.close()


# ---- 7: bad blocks -----------------------------------------------------------------------------------------------------------------

def test_bad_blocks_are_refused_by_name(engine, tmp_path):
    """Host checks, not device faults: every refusal names the file and comes with IPKGPU_ERR_INVALID."""
    sigma, B = 4, 4
    groups = _groups(2)
    mats = synth_matrices(4, 200, sigma, 0.1, 12)
    d8, d9 = tmp_path / "k8", tmp_path / "k9"
    d8.mkdir(); d9.mkdir()
    for k, d in ((8, d8), (9, d9)):
        parts = engine.score_groups_keymajor(mats, groups, k, _eps(sigma, k), n_owners=B)
        engine.parts_spill(parts, d, 0)
        parts.free()
    good = ondisk.block_path(d8, 0, 1)

    def refused(paths, owner=1, n_owners=B, k=8):
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            engine.spill_merge(sigma, k, owner, n_owners, paths)
        assert ei.value.code == 1
        return str(ei.value)

    cut = tmp_path / "cut.blk"
    cut.write_bytes(open(good, "rb").read()[:-16])
    assert str(cut) in refused([good, str(cut)]) and "size" in refused([str(cut)])
    other = ondisk.block_path(d8, 0, 2)
    assert other in refused([good, other]) and "another batch" in refused([other])
    k9 = ondisk.block_path(d9, 0, 1)
    assert k9 in refused([k9]) and "another k" in refused([k9])
    assert good in refused([good], owner=1, n_owners=8) and "another number of batches" in refused([good], owner=1, n_owners=8)
    # a body that disagrees with its head: a count changed, the file's size kept
    raw = bytearray(open(good, "rb").read())
    blk = ondisk.read_block(good)
    at = 64 + 8 * len(blk["bits"])
    raw[at] ^= 1
    bad = tmp_path / "body.blk"
    bad.write_bytes(bytes(raw))
    assert str(bad) in refused([str(bad)])
    db = engine.spill_merge(sigma, 8, 1, B, [good])                           # the context is unharmed
    assert db.num_entries == blk["n_entries"]
    db.free()


# ---- 8: what is not spilled -------------------------------------------------------------------------------------------------------

def test_positioned_and_key_range_parts_are_refused(engine, tmp_path):
    mats = synth_matrices(4, 120, 20, 0.03, 3)
    groups = _groups(2)
    pos = engine.score_groups_keymajor_positions_owners(mats, groups, 4, _eps(20, 4), n_owners=4)
    with pytest.raises(ipk_amd.IpkGpuError) as ei:
        engine.parts_spill(pos, tmp_path, 0)
    assert ei.value.code == 1 and "position" in str(ei.value)
    pos.free()
    dna = synth_matrices(4, 100, 4, 0.1, 3)
    kr = engine.score_groups_keyrange(dna, groups, 15, _eps(4, 15), 1, 2)
    with pytest.raises(ipk_amd.IpkGpuError) as ei:
        engine.parts_spill(kr, tmp_path, 0)
    assert ei.value.code == 1 and "key-range" in str(ei.value)
    kr.free()
    assert os.listdir(tmp_path) == []


def test_mem_stats_and_budget(tmp_path):
    """held follows the context's allocations, the peak is a high-water mark, and a budget refuses what would exceed it."""
    eng = ipk_amd.Engine(0)
    try:
        assert eng.mem_stats() == (0, 0)
        mats = synth_matrices(4, 500, 4, 0.1, 1)
        parts = eng.score_groups_keymajor(mats, _groups(2), 8, _eps(4, 8), n_owners=1)
        held, peak = eng.mem_stats()
        assert 0 < held <= peak
        parts.free()
        eng.set_option("device_budget_bytes", held // 4)
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            eng.score_groups_keymajor(synth_matrices(40, 2000, 4, 0.1, 2), _groups(20), 12, _eps(4, 12), n_owners=1)
        assert ei.value.code == 3
        assert eng.get_option("last_refused_bytes") > held // 4
        eng.set_option("device_budget_bytes", 0)
        parts = eng.score_groups_keymajor(mats, _groups(2), 8, _eps(4, 8), n_owners=1)
        assert parts.num_entries > 0
        parts.free()
    finally:
        eng.close()


# ---- 9: the command line ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", ["mif0", "random"])
def test_cli_on_disk_writes_the_default_bytes(tmp_path, filt):
    from tests.test_cli import _reference_workdir
    tree_file, ar_dir, _ = _reference_workdir(tmp_path, 8, 64, 108)
    base = ["build", "-t", str(tree_file), "-k", "8", "--ar-dir", str(ar_dir), "--filter", filt]
    one, two = tmp_path / "DB.ipk", tmp_path / "DB_ondisk.ipk"
    res = CliRunner().invoke(cli.ipk, base + ["-w", str(tmp_path / "work"), "-o", str(one)])
    assert res.exit_code == 0, (res.output, res.exception)
    res = CliRunner().invoke(cli.ipk, base + ["-w", str(tmp_path / "work2"), "-o", str(two), "--on-disk"])
    assert res.exit_code == 0, (res.output, res.exception)
    for line in ("Computation time:", "Filtering time:", "Merge time:", "32 batches"):
        assert line in res.output
    assert two.read_bytes() == one.read_bytes()
    assert not (tmp_path / "work2" / "hashmaps").exists()
