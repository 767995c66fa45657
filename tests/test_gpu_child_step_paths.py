"""The child-node steps and the single-step half joins of the DNA k = 8..12 scoring kernel on the fabricated inputs of
tests/child_step_cases.py (tests/test_child_step_inputs.py asserts what they contain): full and empty 16-lane slots in every slot
position, every sub-step of a 3-symbol node empty and full, half joins of 1, 63 and 64 candidates with second children of every
length, tile tails of one window and of an odd count.  Every result is compared bit for bit with oracle/ipk_oracle (keys, raw score
bits, scored count) through the per-branch call and the key-major call, and the count-only pre-pass of a fresh engine's first call
must count the same k-mers."""
import functools

import numpy as np
import pytest

import ipk_amd
from oracle import ipk_oracle as co
from tests import child_step_cases as cc
from tests import db_check as dc

pytestmark = pytest.mark.gpu
SIGMA = cc.SIGMA


@functools.lru_cache(maxsize=None)
def _ref(k, tail):
    """Per group: (keys, score bits, scored count) of the oracle, computed once per case."""
    c = cc.case(k, tail)
    out = {}
    for gid in dict.fromkeys(c.groups.tolist()):
        keys, scores, emitted = co.explore_group(c.mats[c.groups == gid], k, cc.EPS)
        out[int(gid)] = (keys, scores.view(np.uint32), int(emitted))
    return out


def _check(engine, c, ref):
    """The per-branch call and the key-major call against the oracle, entry by entry."""
    gids = list(ref)
    total = sum(r[2] for r in ref.values())
    expect = {g: dc.Expect(r[0], r[1], r[2], SIGMA, c.k, 1) for g, r in ref.items()}

    def oracle(gid):
        return ref[gid][0], ref[gid][1]

    res = engine.score_groups(c.mats, c.groups, c.k, cc.EPS)
    try:
        assert res.emitted == total
        keys, bits = dc.result_tensors(res)
        dc.check_groups(res.group_ids, res.offsets, keys, bits, gids, expect, oracle=oracle)
        del keys, bits
    finally:
        res.free()
    parts = engine.score_groups_keymajor(c.mats, c.groups, c.k, cc.EPS, n_owners=1)
    try:
        assert parts.emitted == total and parts.num_entries == sum(len(r[0]) for r in ref.values())
        db = engine.merge_parts_ptrs(SIGMA, c.k, 0, 1, [parts.counts_ptr()], [parts.entries_ptr() + 8 * int(parts.owner_offsets[0])])
        try:
            dk, off, entries = dc.db_tensors(db)
            dc.check_db(dk, off, entries, gids, expect, SIGMA, c.k, owner=0, world=1, oracle=oracle)
            del dk, off, entries
        finally:
            db.free()
    finally:
        parts.free()


@pytest.mark.parametrize("k,tail", cc.cases())
def test_child_steps(engine, k, tail):
    c = cc.case(k, tail)
    ref = _ref(k, tail)
    assert sum(r[2] for r in ref.values()) > 0
    _check(engine, c, ref)


@pytest.mark.parametrize("k,tail", cc.cases())
def test_count_only_pass(k, tail):
    """A fresh engine's first call sizes its pair pool with the count-only form of the kernel over a sample of the groups -- both
    of the case's two.  No half list of these inputs exceeds the fast capacity (asserted), so it counts every scored k-mer."""
    c = cc.case(k, tail)
    ref = _ref(k, tail)
    assert cc.classify(k, tail)[1] == []
    eng = ipk_amd.Engine(0)
    try:
        res = eng.score_groups(c.mats, c.groups, k, cc.EPS)
        try:
            assert eng.get_option("debug_count_pass_queued") == 0
            assert eng.get_option("debug_count_pass_pairs") == res.emitted == sum(r[2] for r in ref.values())
        finally:
            res.free()
    finally:
        eng.close()
