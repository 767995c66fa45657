"""The scale tests' checker (tests/db_check.py) on small databases built from the oracle: it passes the oracle's own database and
group-major result, and fails each of them after one subtle corruption (CPU only)."""
import numpy as np
import pytest
import torch

from ipk_amd.synth import synth_matrices
from oracle import db_oracle as dbo
from oracle import ipk_oracle as co
from tests import db_check as dc

CASES = {"dna_k8": (4, 8, 60, 0.15), "aa_k4": (20, 4, 24, 0.05)}
GROUPS = [31, 7, 19, 4]


def _case(name, world):
    sigma, k, sites, alpha = CASES[name]
    mats = synth_matrices(2 * len(GROUPS), sites, sigma, alpha, 4100 + k)
    by_gid = {gid: mats[2 * i:2 * i + 2] for i, gid in enumerate(GROUPS)}
    eps = co.log_threshold(1.5, sigma, k)
    expect = dc.oracle_digests(lambda gid: by_gid[gid], GROUPS, k, eps, sigma, world=world)
    ref = [(gid,) + co.explore_group(by_gid[gid], k, eps)[:2] for gid in GROUPS]
    return sigma, k, expect, ref


def _oracle(ref):
    table = {gid: (keys, scores.view(np.uint32)) for gid, keys, scores in ref}
    return lambda gid: table[gid]


def _shard(ref, sigma, k, owner, world):
    keys, off, br, sc = dbo.db_shard_arrays(dbo.build_db(ref), sigma, k, owner, world)
    entries = np.stack([br, sc], axis=1).view(np.int32)
    return torch.from_numpy(keys.view(np.int32).copy()), torch.from_numpy(off.astype(np.int64)), torch.from_numpy(entries.copy())


def _key_with_entries(off, at_least):
    cnt = np.diff(off.numpy())
    i = int(np.flatnonzero(cnt >= at_least)[0])
    return i, int(off[i])


def _flip_score_bit(keys, off, entries):
    entries[len(entries) // 2, 1] ^= 1                                  # lowest mantissa bit of one score
    return keys, off, entries


def _swap_two_entries_of_a_key(keys, off, entries):
    _, a = _key_with_entries(off, 2)
    entries[[a, a + 1]] = entries[[a + 1, a]]
    return keys, off, entries


def _drop_an_entry(keys, off, entries):
    i, a = _key_with_entries(off, 2)
    off = off.clone()
    off[i + 1:] -= 1
    return keys, off, torch.cat([entries[:a], entries[a + 1:]])


def _duplicate_an_entry(keys, off, entries):
    i, a = _key_with_entries(off, 1)
    off = off.clone()
    off[i + 1:] += 1
    return keys, off, torch.cat([entries[:a + 1], entries[a:]])


def _move_an_entry_to_the_next_key(keys, off, entries):
    i, _ = _key_with_entries(off[1:], 2)                                  # key i + 1 keeps at least one entry
    off = off.clone()
    off[i + 1] += 1                                                      # key i + 1's first entry becomes key i's last
    return keys, off, entries


def _rename_a_group(keys, off, entries):
    e = entries.clone()
    e[e[:, 0] == GROUPS[1], 0] = GROUPS[2]
    return keys, off, e


MUTATIONS = [_flip_score_bit, _swap_two_entries_of_a_key, _drop_an_entry, _duplicate_an_entry, _move_an_entry_to_the_next_key,
             _rename_a_group]


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("world", [1, 3])
def test_checker_passes_the_oracle_database(name, world):
    sigma, k, expect, ref = _case(name, world)
    for o in range(world):
        keys, off, entries = _shard(ref, sigma, k, o, world)
        assert len(keys) > 10 and len(entries) > len(keys), "the case must have keys shared by several groups"
        dc.check_db(keys, off, entries, GROUPS, expect, sigma, k, owner=o, world=world, oracle=_oracle(ref))


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("mutate", MUTATIONS, ids=[m.__name__[1:] for m in MUTATIONS])
def test_checker_fails_a_corrupted_database(name, world, mutate):
    sigma, k, expect, ref = _case(name, world)
    keys, off, entries = mutate(*_shard(ref, sigma, k, world - 1, world))
    with pytest.raises(AssertionError):
        dc.check_db(keys, off, entries, GROUPS, expect, sigma, k, owner=world - 1, world=world, oracle=_oracle(ref))


def test_checker_names_the_first_difference():
    sigma, k, expect, ref = _case("dna_k8", 1)
    keys, off, entries = _flip_score_bit(*_shard(ref, sigma, k, 0, 1))
    with pytest.raises(AssertionError, match=r"group \d+: first difference at index \d+: key 0x[0-9a-f]+ .*score bits"):
        dc.check_db(keys, off, entries, GROUPS, expect, sigma, k, oracle=_oracle(ref))


def test_checker_rejects_a_key_of_another_owner():
    sigma, k, expect, ref = _case("dna_k8", 3)
    keys, off, entries = _shard(ref, sigma, k, 1, 3)
    keys = keys.clone()
    keys[0] -= 1                                                         # still below keys[1], but owned by owner 0
    with pytest.raises(AssertionError, match="another owner"):
        dc.check_db(keys, off, entries, GROUPS, expect, sigma, k, owner=1, world=3)


@pytest.mark.parametrize("name", list(CASES))
def test_group_major_check(name):
    sigma, k, expect, ref = _case(name, 1)
    keys = torch.from_numpy(np.concatenate([r[1] for r in ref]).view(np.int32).copy())
    bits = torch.from_numpy(np.concatenate([r[2] for r in ref]).view(np.int32).copy())
    off = np.concatenate([[0], np.cumsum([len(r[1]) for r in ref])])
    dc.check_groups(GROUPS, off, keys, bits, GROUPS, expect)
    bad = bits.clone()
    bad[len(bad) // 3] ^= 1
    with pytest.raises(AssertionError, match="first difference"):
        dc.check_groups(GROUPS, off, keys, bad, GROUPS, expect, oracle=_oracle(ref))
    off2 = off.copy()
    off2[2] += 1                                                         # an entry of group 2 counted in group 1
    with pytest.raises(AssertionError):
        dc.check_groups(GROUPS, off2, keys, bits, GROUPS, expect)
    with pytest.raises(AssertionError, match="groups differ"):
        dc.check_groups(GROUPS[::-1], off, keys, bits, GROUPS, expect)
