"""GPU suite: the positioned database on several ranks -- ipkgpu_score_groups_keymajor_positions_owners_device (positions split by
owner), ipkgpu_merge_parts_positions_ptrs (merge_copy_pos_kernel), positions through the exchange, the shard files and the CLI --
against oracle/ipk_oracle.py::explore_group_pos.  All comparisons are exact: keys, offsets, branch ids, raw score bits, positions,
file bytes."""
import os

import numpy as np
import pytest

import ipk_amd
from ipk_amd import dbfile
from ipk_amd import distributed as D
from ipk_amd import engine as E
from ipk_amd.synth import synth_matrices
from oracle import db_oracle as dbo
from oracle import ipk_oracle as co
from tests.test_gpu_positions_db import assert_same, cfg_share, oracle_positions_db, positioned

pytestmark = pytest.mark.gpu


def oracle_shard(want, sigma, k, owner, world):
    """Owner's shard of oracle_positions_db's database: the keys with dense code % world == owner."""
    keys, off, br, bits, pos = want[:5]
    sel = dbo.dense_code(keys, sigma, k) % np.uint64(world) == np.uint64(owner)
    counts = np.diff(off.astype(np.int64))
    rows = np.repeat(sel, counts)
    return keys[sel], np.concatenate([[0], np.cumsum(counts[sel])]).astype(np.uint64), br[rows], bits[rows], pos[rows]


def db_arrays(db):
    br, sc = db.entries()
    pos = db.positions()
    assert pos is not None, "the merged database carries no positions"
    return db.keys().copy(), db.key_offsets().copy(), br, sc.view(np.uint32), pos.copy()


def merge_owner(engine, parts, sigma, k, owner, world):
    """Owner `owner` merges its block of every source in `parts` (rank order) -- what the all-to-all delivers."""
    cps = [p.counts_ptr() + 4 * owner * p.slots for p in parts]
    eps = [p.entries_ptr() + 8 * int(p.owner_offsets[owner]) for p in parts]
    pps = [p.positions_ptr() + 4 * int(p.owner_offsets[owner]) for p in parts]
    return engine.merge_parts_positions_ptrs(sigma, k, owner, world, cps, eps, pps)


def check_owners(engine, parts, want, sigma, k, world):
    total = 0
    for o in range(world):
        db = merge_owner(engine, parts, sigma, k, o, world)
        got = db_arrays(db)
        assert_same(got, oracle_shard(want, sigma, k, o, world))
        total += len(got[0])
        db.free()
    assert total == len(want[0])


def interleaved(n_groups, first=0):
    """Matrix indices of groups [first, first + n_groups) of two matrices each: every group's first matrix, then every second one."""
    g = np.arange(first, first + n_groups)
    return np.concatenate([2 * g, 2 * g + 1])


@pytest.mark.parametrize("world,sigma,k", [(2, 20, 6), (3, 20, 3), (8, 4, 8), (3, 4, 12), (2, 4, 13), (1, 20, 4)])
def test_simulated_ranks(engine, world, sigma, k):
    """1. P ranks emulated on one GPU: each scores its shard_range of 7 groups (2 interleaved matrices each) with n_owners = P; owner o
    merges block o of every rank.  (8 ranks: one has no groups and takes part through n_mats = 0.)  One rank: the new call plus
    db_from_parts equals the existing positioned call."""
    n_groups, sites = 7, 30 if k >= 12 else 40
    mats = synth_matrices(n_groups * 2, sites, sigma, 0.1, 900 + k)
    ids = np.arange(n_groups, dtype=np.uint32) * 3 + 5
    groups = np.repeat(ids, 2)
    eps = co.log_threshold(1.5, sigma, k)
    want = oracle_positions_db(mats, groups, k, eps)
    if world == 1:
        idx = interleaved(n_groups)
        parts = engine.score_groups_keymajor_positions_owners(mats[idx], groups[idx], k, eps, n_owners=1)
        pos_parts = parts.positions_tensor().cpu().numpy().view(np.uint32).copy()
        db = engine.db_from_parts(parts, sigma, k)
        got = db_arrays(db)
        assert np.array_equal(got[4], pos_parts)
        assert_same(got, positioned(engine, mats[idx], groups[idx], k, eps)[:5])
        assert_same(got, want[:5])
        assert parts.emitted == want[5]
        db.free(); parts.free()
        return
    parts = []
    for r in range(world):
        g0, g1 = D.shard_range(n_groups, world, r)
        idx = interleaved(g1 - g0, g0)
        p = engine.score_groups_keymajor_positions_owners(mats[idx], groups[idx], k, eps, n_owners=world)
        assert p.n_owners == world and p.positions_ptr(), "the parts carry no positions"
        if g1 == g0:
            assert p.num_entries == 0 and p.emitted == 0
        parts.append(p)
    assert sum(p.emitted for p in parts) == want[5]
    assert sum(p.num_entries for p in parts) == len(want[2])
    check_owners(engine, parts, want, sigma, k, world)
    for p in parts:
        p.free()


def test_batches_with_owners():
    """2. several batches (merged per owner inside the call) at n_owners = 3, and several writer passes (more than 256 groups in one
    batch) at n_owners = 2, give the one-batch shards."""
    eng = ipk_amd.Engine(0)
    try:
        sigma, k = 20, 4
        mats = synth_matrices(12, 40, sigma, 0.05, 515)
        groups = np.repeat(np.arange(6, dtype=np.uint32) + 3, 2)
        eps = co.log_threshold(1.5, sigma, k)
        want = oracle_positions_db(mats, groups, k, eps)
        whole = eng.score_groups_keymajor_positions_owners(mats, groups, k, eps, n_owners=3)
        assert whole.time_ms(E.T_SCORE_LAUNCHES) == 1
        check_owners(eng, [whole], want, sigma, k, 3)
        eng.set_option("workspace_bytes", 1 << 20)
        split = eng.score_groups_keymajor_positions_owners(mats, groups, k, eps, n_owners=3)
        assert split.time_ms(E.T_SCORE_LAUNCHES) > 1, "the small workspace did not split the call into batches"
        assert split.emitted == whole.emitted == want[5]
        assert np.array_equal(split.owner_offsets, whole.owner_offsets)
        for a, b in ((split.counts_tensor(), whole.counts_tensor()), (split.entries_tensor(), whole.entries_tensor()),
                     (split.positions_tensor(), whole.positions_tensor())):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
        check_owners(eng, [split], want, sigma, k, 3)
        split.free(); whole.free()
        eng.set_option("workspace_bytes", 8 << 30)
        sigma, k = 20, 6
        mats = synth_matrices(300, 10, sigma, 0.03, 516)
        groups = np.arange(300, dtype=np.uint32) + 11
        eps = co.log_threshold(1.5, sigma, k)
        want = oracle_positions_db(mats, groups, k, eps)
        parts = eng.score_groups_keymajor_positions_owners(mats, groups, k, eps, n_owners=2)
        assert parts.time_ms(E.T_SCORE_LAUNCHES) == 1 and parts.emitted == want[5]
        check_owners(eng, [parts], want, sigma, k, 2)
        parts.free()
    finally:
        eng.close()


def test_ties_with_owners(engine):
    """3. equal scores in both matrices of a group (identical flat columns) at n_owners = 2: every position is the first window's."""
    sigma, k = 4, 6
    col = np.log10(np.array([0.4, 0.3, 0.2, 0.1], dtype=np.float32))
    flat = np.tile(col, (2, 25, 1)).astype(np.float32)
    eps = co.log_threshold(1.0, sigma, k)
    want = oracle_positions_db(flat, [0, 0], k, eps)
    parts = engine.score_groups_keymajor_positions_owners(flat, np.array([0, 0], dtype=np.uint32), k, eps, n_owners=2)
    pos = parts.positions_tensor().cpu().numpy()
    assert len(pos) == len(want[4]) > 0 and np.all(pos == 0)
    one = positioned(engine, flat, [0, 0], k, eps)
    assert np.all(one[4] == 0) and len(one[4]) == len(pos)
    check_owners(engine, [parts], want, sigma, k, 2)
    parts.free()


def test_native_exchange_single_rank_comm():
    """4. the in-library exchange on a one-rank communicator with positioned pieces: sizes (bit 63 set), counts, entries and positions
    travel rank 0 -> rank 0; two pieces, then three with an empty positioned one; a positioned piece next to a plain one is refused by
    exchange_merge and the engine stays usable."""
    import torch
    sigma, k = 20, 4
    mats = synth_matrices(8, 40, sigma, 0.05, 8081)
    groups = np.array([3, 3, 9, 9, 4, 4, 1, 1], dtype=np.uint32)
    eps = co.log_threshold(1.5, sigma, k)
    want = oracle_positions_db(mats, groups, k, eps)
    eng = ipk_amd.Engine(0)
    try:
        eng.comm_init(eng.comm_unique_id(), 0, 1)
        dev = torch.from_numpy(mats).cuda()
        parts = [eng.score_groups_keymajor_positions_owners(dev[a:b], groups[a:b], k, eps, n_owners=1) for a, b in ((0, 4), (4, 8))]
        assert sum(p.emitted for p in parts) == want[5]
        db, exposed = eng.exchange_merge([eng.exchange_begin(p) for p in parts], sigma, k)
        assert exposed >= 0.0
        assert_same(db_arrays(db), want[:5])
        db.free()
        empty = eng.score_groups_keymajor_positions_owners(dev[0:0], groups[0:0], k, eps, n_owners=1)
        assert empty.num_entries == 0 and empty.emitted == 0 and empty.positions_ptr()
        db, _ = eng.exchange_merge([eng.exchange_begin(parts[0]), eng.exchange_begin(empty), eng.exchange_begin(parts[1])], sigma, k)
        assert_same(db_arrays(db), want[:5])
        db.free()
        plain = eng.score_groups_keymajor(dev[4:8], groups[4:8], k, eps, n_owners=1)
        with pytest.raises(ipk_amd.IpkGpuError, match="with and without positions") as ei:
            eng.exchange_merge([eng.exchange_begin(parts[0]), eng.exchange_begin(plain)], sigma, k)
        assert ei.value.code == 1
        # the engine and its communicator are still good: the positioned exchange again, and a plain one
        db, _ = eng.exchange_merge([eng.exchange_begin(p) for p in parts], sigma, k)
        assert_same(db_arrays(db), want[:5])
        db.free()
        plain0 = eng.score_groups_keymajor(dev[0:4], groups[0:4], k, eps, n_owners=1)
        db, _ = eng.exchange_merge([eng.exchange_begin(plain0), eng.exchange_begin(plain)], sigma, k)
        assert db.positions() is None
        br, sc = db.entries()
        assert_same((db.keys(), db.key_offsets(), br, sc.view(np.uint32)), want[:4])
        db.free(); plain.free(); plain0.free(); empty.free()
        for p in parts:
            p.free()
    finally:
        eng.close()


RANK_SHAPE = (20, 4, 2, 30)          # sigma, k, matrices per group, sites


def _rank_inputs(n_groups):
    sigma, k, mpg, sites = RANK_SHAPE
    mats = synth_matrices(n_groups * mpg, sites, sigma, 0.05, 4343)
    groups = np.repeat(np.arange(n_groups, dtype=np.uint32) + 50, mpg)
    return mats, groups, co.log_threshold(1.5, sigma, k)


def _rank_worker(rank, world, port, out_dir, n_groups):
    """One process per rank (both on GPU 0, gloo transport): build_db_shard(positions=True) end to end."""
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        sigma, k, mpg, _ = RANK_SHAPE
        mats, groups, eps = _rank_inputs(n_groups)
        g0, g1 = D.shard_range(n_groups, world, rank)
        eng = ipk_amd.Engine(0)
        db, parts = D.build_db_shard(eng, torch.from_numpy(mats[g0 * mpg:g1 * mpg]).cuda(), groups[g0 * mpg:g1 * mpg], k, eps, sigma,
                                     dist, world, rank, pieces=min(4, n_groups // 2), positions=True)
        keys, off, br, bits, pos = db_arrays(db)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), keys=keys, off=off, br=br, sc=bits, pos=pos, emitted=parts.emitted)
        db.free(); parts.free(); eng.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n_groups", [6, 3, 11])
def test_two_rank_build_with_positions(tmp_path, n_groups):
    """5. two ranks on GPU 0 over gloo: 6 groups (3 per rank, 3 pieces each), 3 groups (shards of 2 and 1, one piece), 11 groups (6
    and 5, 4 pieces each)."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    world = 2
    mp.spawn(_rank_worker, args=(world, port, str(tmp_path), n_groups), nprocs=world, join=True)
    sigma, k = RANK_SHAPE[:2]
    mats, groups, eps = _rank_inputs(n_groups)
    want = oracle_positions_db(mats, groups, k, eps)
    tot = 0
    for r in range(world):
        z = np.load(tmp_path / f"rank{r}.npz")
        assert_same((z["keys"], z["off"], z["br"], z["sc"], z["pos"]), oracle_shard(want, sigma, k, r, world))
        tot += int(z["emitted"])
    assert tot == want[5]


@pytest.mark.parametrize("filt", ["mif0", "random"])
def test_cli_keep_positions_two_ranks_writes_the_same_file(tmp_path, filt):
    """6. `build --keep-positions -s amino -k 4` as two rank processes: byte-identical to the one-process file."""
    import socket
    import torch.multiprocessing as mp
    from click.testing import CliRunner
    from ipk_amd import cli
    from tests.test_cli import _cli_rank
    from tests.test_loader import write_probs
    ar_dir = tmp_path / "AR"; ar_dir.mkdir()
    labels = [f"{i}_X{j}" for i in range(5) for j in range(2)]
    write_probs(ar_dir / "ar.raxml.ancestralProbs", 20, labels, 30, 23, extras=False)
    with open(tmp_path / "map.tsv", "w") as fh:
        for i, lab in enumerate(labels):
            fh.write(f"{lab}\t{3 + i // 2}\n")
    args = ["build", "-w", str(tmp_path), "--ar-dir", str(ar_dir), "--mapping", str(tmp_path / "map.tsv"), "-s", "amino", "-k", "4",
            "--omega", "1.5", "--filter", filt, "--num-tree-nodes", "11", "--keep-positions"]
    one = tmp_path / "one.ipk"
    res = CliRunner().invoke(cli.ipk, args + ["-o", str(one)])
    assert res.exit_code == 0, (res.output, res.exception)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_cli_rank, args=(2, port, str(tmp_path), args), nprocs=2, join=True)
    assert open(tmp_path / "multi.ipk", "rb").read() == open(one, "rb").read()
    hdr, recs = dbfile.read_db(tmp_path / "multi.ipk")
    assert hdr["positions_loaded"] is True and hdr["sequence_type"] == "AA" and len(recs) == hdr["total_num_kmers"] > 0


def test_scale_share_eight_owners(engine):
    """7. a 4-group share of cfg4 (4 x 2 x 3000 sites, AA k = 6) at n_owners = 8: all eight shards in full against the oracle."""
    mats, groups, k, eps = cfg_share("cfg4", 4)
    sigma = mats.shape[2]
    want = oracle_positions_db(mats, groups, k, eps, threads=min(16, len(os.sched_getaffinity(0))))
    parts = engine.score_groups_keymajor_positions_owners(mats, groups, k, eps, n_owners=8)
    assert parts.emitted == want[5] and parts.num_entries == len(want[2])
    check_owners(engine, [parts], want, sigma, k, 8)
    parts.free()
