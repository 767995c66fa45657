"""CPU suite: distributed.exchange_parts with positions (gloo, world_size 2 and 3, numpy stand-ins for the device steps as in
tests/test_distributed_cpu.py).  Rank o receives block o of every rank's positions, in rank order, laid out as the entries."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ipk_amd import distributed as D
from ipk_amd.synth import synth_matrices
from oracle import db_oracle as dbo
from oracle import ipk_oracle as co

MPG, SITES = 2, 24


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def rank_parts(mats, groups_of_rank, sigma, k, eps, world):
    """One rank's positioned parts from the oracle: np_parts' (counts, entries, owner_offsets) and the positions aligned with the
    entries (owner-major, ascending key, group order)."""
    res = []
    for g in groups_of_rank:
        keys, scores, pos, _ = co.explore_group_pos(mats[g * MPG:(g + 1) * MPG], k, eps)
        res.append((100 + g, keys, scores, pos))
    counts, entries, owner_off = dbo.np_parts([r[:3] for r in res], sigma, k, world)
    rows = []                                                        # (owner, dense code, group index, position)
    for gi, (_, keys, _, pos) in enumerate(res):
        dense = dbo.dense_code(keys, sigma, k)
        rows += [(int(d) % world, int(d), gi, int(p)) for d, p in zip(dense.tolist(), pos.tolist())]
    rows.sort(key=lambda r: r[:3])
    positions = np.array([r[3] for r in rows], dtype=np.uint32).view(np.int32)
    assert len(positions) == len(entries)
    return counts, entries, owner_off, positions


def _worker(rank, world, port, sigma, k, n_groups, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mats = synth_matrices(n_groups * MPG, SITES, sigma, 0.2, 77)
        eps = co.log_threshold(1.5, sigma, k)
        g0, g1 = D.shard_range(n_groups, world, rank)
        counts, entries, owner_off, positions = rank_parts(mats, range(g0, g1), sigma, k, eps, world)
        got = D.exchange_parts(torch.from_numpy(counts), torch.from_numpy(entries), owner_off, dist, world, torch.from_numpy(positions))
        assert len(got) == 4
        rc, re_, rs, rp = got
        # the plain call is unchanged: three values, the same counts and entries
        rc0, re0, rs0 = D.exchange_parts(torch.from_numpy(counts), torch.from_numpy(entries), owner_off, dist, world)
        assert torch.equal(rc, rc0) and torch.equal(re_, re0) and rs == rs0
        np.savez(os.path.join(out_dir, f"recv{rank}.npz"), rc=rc.numpy(), re=re_.numpy(), rs=np.array(rs), rp=rp.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,sigma,k,n_groups", [(2, 4, 6, 5), (3, 4, 5, 5), (2, 20, 3, 5), (3, 20, 3, 2)])
def test_positions_travel_with_their_entries(tmp_path, world, sigma, k, n_groups):
    """(3, 20, 3, 2): two groups on three ranks -- the third rank has none and takes part with empty blocks."""
    mp.spawn(_worker, args=(world, _free_port(), sigma, k, n_groups, str(tmp_path)), nprocs=world, join=True)
    mats = synth_matrices(n_groups * MPG, SITES, sigma, 0.2, 77)
    eps = co.log_threshold(1.5, sigma, k)
    sent = [rank_parts(mats, range(*D.shard_range(n_groups, world, r)), sigma, k, eps, world) for r in range(world)]
    if n_groups < world:
        assert len(sent[-1][1]) == 0 and len(sent[-1][3]) == 0
    for o in range(world):
        z = np.load(tmp_path / f"recv{o}.npz")
        want_pos, want_ent, sizes = [], [], []
        for r in range(world):
            _, entries, off, positions = sent[r]
            a, b = int(off[o]), int(off[o + 1])
            want_pos.append(positions[a:b]); want_ent.append(entries[a:b]); sizes.append(b - a)
        assert z["rs"].tolist() == sizes
        assert np.array_equal(z["rp"], np.concatenate(want_pos))
        assert np.array_equal(z["re"], np.concatenate(want_ent))
        assert np.array_equal(z["rc"], np.stack([sent[r][0][o] for r in range(world)]))
    assert sum(len(np.load(tmp_path / f"recv{o}.npz")["rp"]) for o in range(world)) == sum(len(s[3]) for s in sent)


def test_one_rank_returns_its_own_positions():
    counts = torch.zeros((1, 4), dtype=torch.int32)
    entries = torch.zeros((3, 2), dtype=torch.int32)
    pos = torch.tensor([5, 6, 7], dtype=torch.int32)
    got = D.exchange_parts(counts, entries, np.array([0, 3], np.uint64), None, 1, pos)
    assert len(got) == 4 and got[3] is pos and got[2] == [3]
    assert len(D.exchange_parts(counts, entries, np.array([0, 3], np.uint64), None, 1)) == 3
