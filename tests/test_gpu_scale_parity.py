"""GPU suite: the database's whole content against the oracle at the shapes bench.py times.

bench.py times the 2nd, 3rd, ... distributed.build_db_shard call of a fresh context on cfg2 (1000 groups, one batch), on a rank's share
of cfg2 and cfg3 (8 ranks: 125 groups) and on cfg4.  Several paths switch on only there or only after a first call (a pair pool past
4 GiB, tiles drawn from per-group counters, km_write_lines, the persistent reduce with many more slices than CUs, the compressed writers
over 125 groups of k = 12, calls that skip the post-pass-1 wait and size their buffers from the previous call, workspaces grown with a
margin).  Here every key, entry and score bit of those calls is compared with the oracle (tests/db_check.py: per-group digests, the
shard transposed back to group-major on the device), and the repeated calls with the first one, byte for byte.
"""
import threading
import time

import numpy as np
import pytest
import torch

import ipk_amd
from ipk_amd import distributed as D
from ipk_amd import engine as E
from ipk_amd.synth import CONFIGS, synth_matrices
from oracle import ipk_oracle as co
from tests import db_check as dc

pytestmark = pytest.mark.gpu
WORLD = 8                                         # the owners of an 8-GPU node


@pytest.fixture(scope="module", autouse=True)
def device_memory_peak():
    """Samples the device's memory in use while the module runs and prints the peak at its end."""
    peak, done = [0], threading.Event()
    free, total = torch.cuda.mem_get_info()
    base = total - free

    def sample():
        while not done.wait(0.05):
            f, _ = torch.cuda.mem_get_info()
            peak[0] = max(peak[0], total - f)
    t = threading.Thread(target=sample, daemon=True)
    t0 = time.perf_counter()
    t.start()
    yield
    done.set()
    t.join()
    print(f"\nscale parity: {time.perf_counter() - t0:.0f} s, peak device memory in use {peak[0] / 2 ** 30:.1f} GiB "
          f"(at the start {base / 2 ** 30:.1f} GiB, of {total / 2 ** 30:.0f} GiB)")


class Shape:
    """A bench.py workload: config `name`, groups [g_lo, g_hi), matrices as bench builds them (first_mat = g_lo * mats_per_group)."""

    def __init__(self, name, g_lo, g_hi):
        cfg = CONFIGS[name]
        self.cfg, self.g_lo, self.g_hi = cfg, g_lo, g_hi
        self.sigma, self.k, self.mpg, self.sites = cfg["sigma"], cfg["k"], cfg["mats_per_group"], cfg["sites"]
        self.eps = ipk_amd.log_threshold(cfg["omega"], self.sigma, self.k)
        self.gids = list(range(g_lo, g_hi))
        self.groups = np.repeat(np.arange(g_lo, g_hi, dtype=np.uint32), self.mpg)

    def group_mats(self, gid):
        return synth_matrices(self.mpg, self.sites, self.sigma, self.cfg["alpha"], self.cfg["seed"], first_mat=gid * self.mpg)

    def device_matrices(self):
        n_mats = len(self.groups)
        d = torch.empty((n_mats, self.sites, self.sigma), dtype=torch.float32, device="cuda")
        step = max(1, min(n_mats, (64 << 20) // (self.sites * self.sigma * 4)))
        for m0 in range(0, n_mats, step):
            m1 = min(n_mats, m0 + step)
            d[m0:m1].copy_(torch.from_numpy(synth_matrices(m1 - m0, self.sites, self.sigma, self.cfg["alpha"], self.cfg["seed"],
                                                           first_mat=self.g_lo * self.mpg + m0)))
        torch.cuda.synchronize()
        return d

    def expect(self):
        return dc.oracle_digests(self.group_mats, self.gids, self.k, self.eps, self.sigma, world=WORLD)

    def oracle(self, gid):
        keys, scores, _ = co.explore_group(self.group_mats(gid), self.k, self.eps)
        return keys, scores.view(np.uint32)


def _emitted(expect, gids):
    return sum(expect[g].emitted for g in gids)


def _check_db_calls(eng, sh, d_logp, expect):
    """The first build_db_shard call against the oracle, then two more on the same context and input (the calls bench.py times)
    byte-identical to it.  Returns the first call's scoring launch count."""
    db, parts = D.build_db_shard(eng, d_logp, sh.groups, sh.k, sh.eps, sh.sigma)
    launches = parts.time_ms(E.T_SCORE_LAUNCHES)
    assert parts.emitted == _emitted(expect, sh.gids)
    keys, off, entries = dc.db_tensors(db)
    dc.check_db(keys, off, entries, sh.gids, expect, sh.sigma, sh.k, oracle=sh.oracle)
    first = (keys.clone(), off.clone(), entries.clone())
    del keys, off, entries
    db.free(); parts.free()
    for call in (2, 3):
        db, parts = D.build_db_shard(eng, d_logp, sh.groups, sh.k, sh.eps, sh.sigma)
        assert parts.emitted == _emitted(expect, sh.gids), f"call {call}: scored count"
        got = dc.db_tensors(db)
        for name, a, b in zip(("keys", "key offsets", "entries"), first, got):
            assert torch.equal(a, b), f"call {call}: {name} differ from the first call's"
        del got
        db.free(); parts.free()
    del first
    return launches


def _check_owner_blocks(eng, sh, d_logp, expect, first=None, keep=True):
    """A key-major call for 8 owners; every owner's block merged alone equals the oracle's database restricted to the keys with
    dense_code % 8 == owner.  Returns (counts, entries, owner_offsets) copies (keep) for byte comparisons of later calls, which
    pass them as `first`."""
    parts = eng.score_groups_keymajor(d_logp, sh.groups, sh.k, sh.eps, n_owners=WORLD)
    assert parts.emitted == _emitted(expect, sh.gids)
    if first is not None:
        assert np.array_equal(parts.owner_offsets, first[2]), "owner offsets differ from the first call's"
        assert torch.equal(parts.counts_tensor(), first[0]), "counts differ from the first call's"
        assert torch.equal(parts.entries_tensor(), first[1]), "entries differ from the first call's"
        parts.free()
        return first
    for o in range(WORLD):
        db = eng.merge_parts_ptrs(sh.sigma, sh.k, o, WORLD, [parts.counts_ptr() + 4 * o * parts.slots],
                                  [parts.entries_ptr() + 8 * int(parts.owner_offsets[o])])
        keys, off, entries = dc.db_tensors(db)
        dc.check_db(keys, off, entries, sh.gids, expect, sh.sigma, sh.k, owner=o, world=WORLD, oracle=sh.oracle)
        del keys, off, entries
        db.free()
    out = (parts.counts_tensor().clone(), parts.entries_tensor().clone(), parts.owner_offsets.copy()) if keep else None
    parts.free()
    return out


def _check_group_major(eng, sh, d_logp, expect):
    res = eng.score_groups(d_logp, sh.groups, sh.k, sh.eps)
    assert res.emitted == _emitted(expect, sh.gids)
    keys, bits = dc.result_tensors(res)
    dc.check_groups(res.group_ids, res.offsets, keys, bits, sh.gids, expect, oracle=sh.oracle)
    del keys, bits
    res.free()


@pytest.fixture(scope="module")
def cfg2_expect():
    """The oracle's digests of all 1000 cfg2 groups (the rank shares are subsets of them)."""
    return Shape("cfg2", 0, 1000).expect()


def test_cfg2_one_batch_of_1000_groups(cfg2_expect):
    """bench.py --gpus 1: cfg2 in one call, one batch (a pair pool well past 4 GiB), three calls on one context."""
    sh = Shape("cfg2", 0, 1000)
    d_logp = sh.device_matrices()
    assert _emitted(cfg2_expect, sh.gids) * 8 > 4 << 30, "workload too small to put the pair pool beyond 4 GiB"
    eng = ipk_amd.Engine(0)
    try:
        eng.set_option("workspace_bytes", 64 << 30)
        assert _check_db_calls(eng, sh, d_logp, cfg2_expect) == 1, "the 1000 groups were not scored in one batch"
        _check_group_major(eng, sh, d_logp, cfg2_expect)
    finally:
        eng.close()


def test_cfg2_rank_shares_on_one_context(cfg2_expect):
    """An 8-GPU rank's calls (125 groups, 8 owners): share 3, then share 4 on the same context -- whose first call runs on the
    estimates share 3 left behind -- three calls each; then both shares group-major."""
    eng = ipk_amd.Engine(0)
    try:
        shares = []
        for r in (3, 4):
            sh = Shape("cfg2", *D.shard_range(1000, WORLD, r))
            d_logp = sh.device_matrices()
            first = _check_owner_blocks(eng, sh, d_logp, cfg2_expect)
            for _ in range(2):
                _check_owner_blocks(eng, sh, d_logp, cfg2_expect, first)
            del first
            shares.append((sh, d_logp))
        for sh, d_logp in shares:
            _check_group_major(eng, sh, d_logp, cfg2_expect)
    finally:
        eng.close()


@pytest.mark.parametrize("name,rank,n_groups", [("cfg3", 3, 1000), ("cfg4", 5, 250)])
def test_rank_share(name, rank, n_groups):
    """cfg3's share 3 (k = 12: row-per-lane kernel, persistent reduce, compressed writers) and cfg4's share 5 (AA k = 6: exact
    partition, compressed tables): three database calls, one for 8 owners, group-major."""
    sh = Shape(name, *D.shard_range(n_groups, WORLD, rank))
    expect = sh.expect()
    d_logp = sh.device_matrices()
    eng = ipk_amd.Engine(0)
    try:
        _check_db_calls(eng, sh, d_logp, expect)
        _check_owner_blocks(eng, sh, d_logp, expect, keep=False)
        _check_group_major(eng, sh, d_logp, expect)
    finally:
        eng.close()
