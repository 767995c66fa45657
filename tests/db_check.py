"""Whole-content check of database shards and group-major results against per-group oracle digests, at any size.

A helper of the scale tests (pytest does not collect it: no test_ prefix).  The oracle's entries of ~1 G-entry workloads cannot be held
in memory, so every group is reduced to (entry count, scored count, digest of keys | score bits), computed in a thread pool (the C
oracle releases the GIL).  The shard is turned back into per-group form on its own device: a key per entry, a stable sort by the
entries' group, one slice per group copied to the host and digested the same way.  Everything works on torch tensors of any device
(CPU tensors in tests/test_db_check.py, engine memory wrapped by db_tensors / result_tensors on the GPU).
"""
import collections
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import db_oracle as dbo
from oracle import ipk_oracle as co


def workers():
    """Threads for host work: the CPUs this process may use (a GPU box grants 16 of many), at most 16."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(16, n))


def digest(keys, bits):
    """Digest of one group's (or one group's owner slice of) keys ascending and their score bits, both u32."""
    h = hashlib.blake2b(digest_size=16)
    h.update(np.ascontiguousarray(keys, dtype=np.uint32).tobytes())
    h.update(np.ascontiguousarray(bits, dtype=np.uint32).tobytes())
    return h.hexdigest()


def owner_of(keys, sigma, k, world):
    """Owner of each packed key (dense code % world, the kmer_batch rule), numpy."""
    return (dbo.dense_code(keys, sigma, k) % np.uint64(world)).astype(np.int64)


class Expect:
    """One group's oracle result in digest form: n entries, scored count, digest, and per owner of `world` (n, digest)."""

    def __init__(self, keys, bits, emitted, sigma, k, world):
        self.n, self.emitted, self.digest = len(keys), int(emitted), digest(keys, bits)
        self.owners = []
        if world > 1:
            own = owner_of(keys, sigma, k, world)
            for o in range(world):
                sel = own == o
                self.owners.append((int(sel.sum()), digest(keys[sel], bits[sel])))

    def of(self, owner, world):
        return (self.n, self.digest) if world == 1 else self.owners[owner]


def oracle_digests(make_mats, group_ids, k, eps, sigma, world=1, pool=None):
    """{gid: Expect} for every group; make_mats(gid) gives the group's matrices [n, sites, sigma] (generated in the worker, so that
    no more than a pool's worth of groups is in memory at once)."""
    def one(gid):
        keys, scores, emitted = co.explore_group(make_mats(gid), k, eps)
        return gid, Expect(keys, scores.view(np.uint32), emitted, sigma, k, world)
    gids = [int(g) for g in group_ids]
    if pool is not None:
        return dict(pool.map(one, gids))
    with ThreadPoolExecutor(workers()) as ex:
        return dict(ex.map(one, gids))


def _require(cond, msg):
    if not cond:
        raise AssertionError(msg)


def dense_code_t(keys, sigma, k):
    """dense_code on a torch int64 tensor."""
    if sigma == 4:
        return keys
    out = keys.new_zeros(keys.shape)
    mul = 1
    for d in range(k):
        out += ((keys >> (5 * d)) & 31) * mul
        mul *= sigma
    return out


def _first_difference(gid, got_keys, got_bits, want_keys, want_bits):
    n = min(len(got_keys), len(want_keys))
    diff = np.flatnonzero((got_keys[:n] != want_keys[:n]) | (got_bits[:n] != want_bits[:n]))
    i = int(diff[0]) if len(diff) else n
    def at(a, j):
        return hex(int(a[j])) if j < len(a) else None
    return (f"group {gid}: first difference at index {i}: key {at(got_keys, i)} (expected {at(want_keys, i)}), score bits "
            f"{at(got_bits, i)} (expected {at(want_bits, i)}); {len(got_keys)} entries (expected {len(want_keys)})")


def _compare_groups(slices, expect, owner, world, sigma, k, oracle, what):
    """slices: iterator of (gid, keys u32, bits u32) host arrays, digested in a thread pool (a bounded number in flight); the first
    group that differs is recomputed by `oracle(gid) -> (keys, bits)` for the message."""
    nw = workers()
    pending = collections.deque()

    def drain(limit):
        while len(pending) > limit:
            gid, keys, bits, fut = pending.popleft()
            if fut.result() != expect[gid].of(owner, world):
                return gid, keys, bits
        return None

    bad = None
    with ThreadPoolExecutor(nw) as ex:
        for gid, keys, bits in slices:
            pending.append((gid, keys, bits, ex.submit(lambda a, b: (len(a), digest(a, b)), keys, bits)))
            bad = drain(2 * nw)
            if bad:
                break
        if not bad:
            bad = drain(0)
    if bad is None:
        return
    gid, keys, bits = bad
    want_n, _ = expect[gid].of(owner, world)
    msg = f"{what}: group {gid}: {len(keys)} entries (expected {want_n}) or their content differ from the oracle's"
    if oracle is not None:
        wk, wb = oracle(gid)
        wk, wb = np.asarray(wk, np.uint32), np.asarray(wb, np.uint32)
        if world > 1:
            sel = owner_of(wk, sigma, k, world) == owner
            wk, wb = wk[sel], wb[sel]
        msg = f"{what}: " + _first_difference(gid, keys, bits, wk, wb)
    raise AssertionError(msg)


def check_db(keys, offsets, entries, group_ids, expect, sigma, k, owner=0, world=1, oracle=None):
    """One owner's database shard against the oracle, entry by entry.

    keys int32 [n] (u32 packed codes), offsets int64 [n + 1], entries int32 [m, 2] (branch, score bits): torch tensors on one device.
    group_ids: the groups in group order (the order a key's entries must follow).  expect: {gid: Expect}.  Checks that keys strictly
    ascend and belong to `owner`, that no key has zero entries, that every entry names a group of the call and a key's entries are in
    group order, and that every group's (key, score bits) -- the shard transposed back to group-major -- equals the oracle's."""
    import torch
    dev = keys.device
    n, m = keys.shape[0], entries.shape[0]
    _require(offsets.shape[0] == n + 1, f"{offsets.shape[0]} key offsets for {n} keys")
    off = offsets.to(torch.int64)
    _require(int(off[0]) == 0 and int(off[-1]) == m, f"key offsets span [{int(off[0])}, {int(off[-1])}), the shard has {m} entries")
    cnt = off[1:] - off[:-1]
    _require(bool((cnt > 0).all()), f"{int((cnt <= 0).sum())} keys with no entries (or offsets that run backwards)")
    k64 = keys.to(torch.int64) & 0xFFFFFFFF
    _require(n < 2 or bool((k64[1:] > k64[:-1]).all()), "keys do not strictly ascend")
    if world > 1:
        _require(bool((dense_code_t(k64, sigma, k) % world == owner).all()), f"keys of another owner in owner {owner}'s shard")
    # group index of every entry (position in group_ids); unknown branch ids fail
    gids = torch.as_tensor(np.asarray(group_ids, dtype=np.int64), device=dev)
    sorted_ids, perm = torch.sort(gids)
    branch = entries[:, 0].to(torch.int64) & 0xFFFFFFFF
    pos = torch.searchsorted(sorted_ids, branch).clamp_(max=len(gids) - 1)
    _require(bool((sorted_ids[pos] == branch).all()), "an entry names a branch that is not one of the call's groups")
    gidx = perm[pos].to(torch.int32)
    del pos, branch
    # a key's entries in group order: strictly ascending group index inside every key (a group holds a key once)
    starts = torch.zeros(m, dtype=torch.bool, device=dev)
    starts[off[:-1]] = True
    _require(m < 2 or bool(((gidx[1:] > gidx[:-1]) | starts[1:]).all()), "a key's entries are not in group order (or repeat a group)")
    del starts
    # back to group-major: key of every entry, stable sort by group (keys stay ascending inside a group)
    key_of = torch.repeat_interleave(keys, cnt)
    gsorted, order = torch.sort(gidx, stable=True)
    per_group = torch.bincount(gsorted.to(torch.int64), minlength=len(gids)).cpu().numpy()
    del gsorted, gidx
    bounds = np.concatenate([[0], np.cumsum(per_group)])
    bits_col = entries[:, 1]

    def slices():
        for gi, gid in enumerate(group_ids):
            sel = order[int(bounds[gi]):int(bounds[gi + 1])]
            yield int(gid), key_of[sel].cpu().numpy().view(np.uint32), bits_col[sel].cpu().numpy().view(np.uint32)

    _compare_groups(slices(), expect, owner, world, sigma, k, oracle, f"owner {owner} of {world}")


def check_groups(result_group_ids, offsets, keys, score_bits, group_ids, expect, oracle=None):
    """Group-major result (CSR: host offsets [g + 1], keys / score bits int32 tensors) against the oracle, group by group:
    the result's groups must be `group_ids` in that order."""
    got = [int(g) for g in result_group_ids]
    _require(got == [int(g) for g in group_ids], "the result's groups differ from the call's (or their order)")
    off = np.asarray(offsets, dtype=np.int64)

    def slices():
        for gi, gid in enumerate(got):
            a, b = int(off[gi]), int(off[gi + 1])
            yield gid, keys[a:b].cpu().numpy().view(np.uint32), score_bits[a:b].cpu().numpy().view(np.uint32)

    _compare_groups(slices(), expect, 0, 1, 4, 0, oracle, "group-major result")


def db_tensors(db):
    """(keys int32 [n], key offsets int64 [n + 1], entries int32 [m, 2]): zero-copy views of an engine database's device arrays."""
    import torch
    from ipk_amd.engine import _device_tensor
    keys = _device_tensor(db.keys_device_ptr(), (db.num_keys,), "int32", db)
    off = _device_tensor(db.key_offsets_device_ptr(), (db.num_keys + 1, 2), "int32", db).view(torch.int64)   # u64 offsets
    entries = _device_tensor(db.entries_device_ptr(), (db.num_entries, 2), "int32", db)
    return keys, off.reshape(-1), entries


def result_tensors(res):
    """(keys int32, score bits int32): zero-copy views of a group-major result's device arrays."""
    from ipk_amd.engine import _device_tensor
    return (_device_tensor(res.keys_device_ptr(), (res.num_entries,), "int32", res),
            _device_tensor(res.scores_device_ptr(), (res.num_entries,), "int32", res))
