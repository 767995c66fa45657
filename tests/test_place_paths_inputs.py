"""CPU suite: the properties of the inputs of tests/test_gpu_place_paths.py (tests/place_cases.py, from reuse_pool() on), counted
with the host oracle.  Conditions on inputs, no measurement of the engine.

Every test prints the counts it asserts on (pytest -s); profiles/place_paths_inputs.txt records them."""
import numpy as np
import pytest

from tests import place_cases as pc
from tests import place_oracle as po


def note(line):
    print("| " + line)


# ---- 1. many queries per workgroup ---------------------------------------------------------------------------------------------------

def reuse_counts(G):
    """Of the pairs (i - G, i), i >= G, of reuse_draw(G): how many are different scoring queries with a common branch; and per kind of
    empty query (no window, no key found, no byte) how many follow a query that scored all 300 branches."""
    c, draw, sets = pc.reuse_pool(), pc.reuse_draw(G), pc.reuse_branch_sets()
    want = pc.expected_at(c, pc.LOG_EPS, 7)
    kind = {}
    for d, (q, w) in enumerate(zip(c.queries, want)):
        if w["n_branches"] == 0:
            kind[d] = "no byte" if q == "" else "no window" if w["n_kmers"] == 0 else "no key found"
    sharing, after_full = 0, {"no byte": 0, "no window": 0, "no key found": 0}
    for i in range(G, len(draw)):
        a, b = int(draw[i - G]), int(draw[i])
        sharing += a != b and bool(sets[a] & sets[b])
        if b in kind and len(sets[a]) == 300:
            after_full[kind[b]] += 1
    return len(draw), sharing, after_full


def test_reuse_pool_is_the_72_queries_and_the_empty_one():
    c = pc.reuse_pool()
    assert len(c.queries) == 73 and len(set(c.queries)) == 73 and c.queries[-1] == ""
    assert set(c.queries[:72]) == set(pc.main_case().queries) | set(pc.order_case().queries)
    empty = sum(1 for s in pc.reuse_branch_sets()[:72] if not s)
    note(f"reuse pool: 72 distinct queries + \"\"; {empty} of the 72 score no branch; {sum(len(s) == 300 for s in pc.reuse_branch_sets())} score all 300")
    assert empty >= 10 and max(len(s) for s in pc.reuse_branch_sets()) == 300


@pytest.mark.parametrize("G", [8192, 1024])
def test_consecutive_queries_of_a_workgroup_share_branches(G):
    """A stale S or C shows only on a branch that a workgroup's previous query and the next one both score: at least half of the
    pairs (i - G, i) are different queries whose branch sets intersect, three turns of the grid happen, and every kind of empty
    query follows a query that touched all 300 branches."""
    n, sharing, after_full = reuse_counts(G)
    assert n == 2 * G + G // 2 + 37 and n > 2 * G
    note(f"reuse G = {G}: N = {n}; {sharing} of {n - G} pairs (i - G, i) differ and share a branch ({sharing / (n - G):.3f}); "
         f"empty after a 300-branch query: {after_full}")
    assert sharing >= 0.5 * (n - G)
    assert all(v >= 1 for v in after_full.values())


# ---- 2. table bounds -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("top", [4095, 4096, 63, 64])
def test_bound_cases_put_the_last_branch_among_the_best(top):
    c = pc.bound_case(top)
    keys, off, br, sc = c.db
    cnt = np.diff(off.astype(np.int64))
    assert br.max() == top and c.view.n_branches == top + 1 and 90 <= len(keys) <= 100 and cnt.min() >= 1 and cnt.max() <= 150
    for i in range(len(keys)):                                          # the precondition survived the planting
        assert len(set(br[int(off[i]):int(off[i + 1])].tolist())) == cnt[i]
    under = sum(top in br[int(off[i]):int(off[i + 1])] for i in range(len(keys)))
    best7 = [q for q, w in enumerate(c.expected(7)) if top in [p[0] for p in w["placements"]]]
    first = [q for q, w in enumerate(c.expected(7)) if w["placements"] and w["placements"][0][0] == top]
    note(f"bound top = {top}: B = {top + 1}, b_pad = {max((top + 64) & ~63, 64)}, {len(keys)} keys, {len(br)} entries; branch {top} under {under} keys, "
         f"in the best 7 of queries {best7}, first of {first}; most branches a query scores: {max(w['n_branches'] for w in c.expected(7))}")
    assert under >= 30 and len(best7) >= 1 and len(first) >= 1
    assert any(top in [p[0] for p in w["placements"]] for w in c.expected(64))


# ---- 3. lookup -----------------------------------------------------------------------------------------------------------------------

LOOKUPS = [(s, k, t) for s, k in pc.LOOKUP_SHAPES for t in (False, True)]


@pytest.mark.parametrize("sigma,k,tail", LOOKUPS)
def test_lookup_cases(sigma, k, tail):
    """The prefix table restated with np.searchsorted: slot sizes 0, 1 (and 2 and >= 256 where a slot has that many codes); code 0 and
    the largest valid code are keys and the table is flat behind the last key; every kind of absent code is a window of a query that
    finds fewer keys than it has windows; a found window straddles the edge of a 64-window tile."""
    c = pc.lookup_case(sigma, k, tail)
    keys = c.db[0].astype(np.int64)
    bits = po.ALPHABET[sigma][1] * k
    shift, slots = pc.lookup_shift(sigma, k), 1 << min(bits, 16)
    assert shift == {(4, 9): 2, (4, 12): 8, (4, 13): 10, (4, 15): 14, (20, 3): 0, (20, 4): 4, (20, 5): 9}[(sigma, k)]
    table = np.searchsorted(keys, np.arange(slots + 1, dtype=np.int64) << shift)          # place_index_kernel's definition
    assert table[0] == 0 and table[-1] == len(keys) and (np.diff(keys) > 0).all() and keys[-1] < (1 << bits)
    size = np.diff(table)
    sizes = set(size.tolist())
    capacity = max(len(pc.slot_codes(c.R + j, sigma, k)) for j in (2, 3))
    assert {0, 1} <= sizes
    if shift:
        assert 2 in sizes and size[c.R + 5] == 1 and size[c.R + 7] == 1
        if not tail:
            assert size[c.R + 2] == min(capacity, 1025 if (1 << shift) > 1024 else 1024) and size[c.R + 9] == 2
    if capacity >= 256:
        assert size.max() >= 256
    for j in (0, 1, 3, 4, 6, 8, 10):                                                         # empty slots around the planted ones
        assert size[c.R + j] == 0
    top = pc.code_of_rank(sigma ** k - 1, sigma, k)
    assert keys[0] == 0
    if tail:
        assert keys[-1] == pc.slot_codes(c.R + 11, sigma, k)[0] and keys[-1] < top and (table[c.R + 12:] == len(keys)).all()
    else:
        assert keys[-1] == top and (table[(top >> shift) + 1:] == len(keys)).all()
        if sigma == 20:
            assert pc.decode(top, sigma, k) == "V" * k and (top >> shift) + 1 < slots      # slots beyond V..V: empty to the table's end
    cnt = np.diff(c.db[1].astype(np.int64))
    assert c.db[2].max() < 200 and cnt.min() >= 1 and cnt.max() <= 40
    want = c.expected(7)
    kset = set(keys.tolist())
    wins = [po.window_codes(q, sigma, k) for q in c.queries]
    assert {63, 64, 65, 66, 127, 129} <= {len(w) for w in wins} and max(len(w) for w in wins) > 3 * 64
    seen = {}
    for name, codes in c.absent.items():
        assert codes and not (set(codes) & kset), name
        seen[name] = sum(1 for q, w in enumerate(wins) if want[q]["n_found"] < want[q]["n_kmers"] and {x for _, x in w} & set(codes))
        assert seen[name] >= 1, name
    expect = {"neighbour", "empty_slot"} | ({"above_last"} if tail else {"above_full", "beside_single"} if shift else set())
    assert expect <= set(c.absent)
    if (sigma, k) == (4, 15) and not tail:
        assert "gap_in_full" in c.absent                                 # a slot of 16 384 codes with 1025 keys: absent codes between them
    straddle = sum(1 for w in wins for s, x in w if x in kset and s % 64 + k > 64)
    found_planted = {n: sum(1 for w in wins for _, x in w if x in set(v)) for n, v in c.planted.items()}
    assert straddle >= 1 and all(v >= 1 for v in found_planted.values())
    note(f"lookup sigma {sigma} k {k}{' tail' if tail else ''}: shift {shift}, {len(keys)} keys, R = {c.R}; slot sizes 0: {int((size == 0).sum())}, "
         f"1: {int((size == 1).sum())}, 2: {int((size == 2).sum())}, largest {int(size.max())}; queries with each absent kind {seen}; "
         f"found windows across a tile edge {straddle}; windows found {sum(w['n_found'] for w in want)} of {sum(w['n_kmers'] for w in want)}")


# ---- 4. long query, inexact threshold -------------------------------------------------------------------------------------------------

def test_the_threshold_is_inexact_and_the_long_query_long():
    assert pc.EPS_INEXACT.dtype == np.float32 and abs(float(pc.EPS_INEXACT) + 3.40775) < 1e-5
    c = pc.long_case()
    W, found, S, Cn = po.accumulate(c.view, c.queries[0], c.sigma, c.k)
    note(f"long query: {len(c.queries[0])} symbols, W = {W}, {found} windows found, largest count {int(Cn.max())}, {int((Cn > 0).sum())} branches")
    assert W == 69993 and found >= 10000 and Cn.max() >= 3500 and (Cn > 0).sum() == 300


@pytest.mark.parametrize("name", ["order_case", "main_case", "long_case"])
def test_a_fused_penalty_changes_a_tenth_of_the_scores(name):
    """S + (float)(W - C) * log_eps has two roundings under EPS_INEXACT: adding the penalty with one rounding (what fmaf does) changes
    the bits of at least 10 % of the scored (query, branch) pairs of each group, some of them among a query's best 64."""
    changed, pairs, in_top = pc.fused_penalty_changes(getattr(pc, name)(), pc.EPS_INEXACT, 64)
    note(f"fused penalty, {name}: {changed} of {pairs} scored pairs change their bits, {in_top} of them among their query's best 64")
    assert changed >= 0.1 * pairs and in_top >= 1
    if name != "long_case":                                              # the contrast: the earlier suite's threshold decides nothing
        exact = pc.fused_penalty_changes(getattr(pc, name)(), pc.LOG_EPS, 64)
        note(f"fused penalty, {name}, log_eps = {pc.LOG_EPS}: {exact[0]} of {exact[1]}")
        assert exact[0] == 0 and exact[1] == pairs


# ---- 5. duplicate check ----------------------------------------------------------------------------------------------------------------

def test_duplicate_databases_have_one_fault_beyond_the_first_pass():
    for which, branch, apart in (("tile", 40000, 47), ("apart", 40000, 200), ("last", 70000, 80)):
        keys, off, br, sc, bad = pc.dup_db(which)
        assert br.max() == 70000                                         # B = 70 001: three passes of 32 768
        faults = []
        for i in range(len(keys)):
            seg = br[int(off[i]):int(off[i + 1])]
            u, n = np.unique(seg, return_counts=True)
            faults += [(int(keys[i]), int(b), np.nonzero(seg == b)[0].tolist()) for b in u[n > 1]]
        assert len(faults) == 1 and faults[0][0] == bad and faults[0][1] == branch
        at = faults[0][2]
        assert len(at) == 2 and at[1] - at[0] == apart and (at[0] // 64 == at[1] // 64) == (which == "tile")
        assert (bad == keys[-1]) == (which == "last") and branch // 32768 == (1 if branch == 40000 else 2)
        note(f"duplicate \"{which}\": key {bad} names branch {branch} at places {at} of {int(off[list(keys).index(bad) + 1] - off[list(keys).index(bad)])}")
    c = pc.dup_control_case()
    keys, off, br, sc = c.db
    for i in range(len(keys)):
        seg = br[int(off[i]):int(off[i + 1])]
        assert len(np.unique(seg)) == len(seg)
    assert {32767, 32768, 65535, 65536, 40000} <= set(br[:int(off[1])].tolist()) and 40000 in br[int(off[1]):int(off[2])] and br.max() == 70000
    assert all(w["n_found"] >= 1 for w in c.expected(7))


# ---- 6. host paths -----------------------------------------------------------------------------------------------------------------------

def test_budget_arithmetic():
    """Half of 64 MB holds fewer than 200 slices of the big-branch case: workgroups place several queries each."""
    c = pc.big_branch_case()
    b_pad = (c.view.n_branches + 63) & ~63
    assert b_pad == 70016 and (32 << 20) // (12 * b_pad) < 200
    note(f"budget: a slice is {12 * b_pad} bytes, half of 64 MB holds {(32 << 20) // (12 * b_pad)} of them")


def test_budgeted_batches_cannot_be_one():
    """The 1500 queries of budget_draw() need more than twice BUDGET_ROOM for their sequences, offsets and results: a call whose peak
    stays within the budget took three batches at least.  No query alone comes near the room."""
    c, draw = pc.reuse_pool(), pc.budget_draw()
    lengths = np.array([len(c.queries[d]) for d in draw])
    whole = int(lengths.sum()) + len(draw) * pc.PLACE_QUERY_BYTES_7
    note(f"budget batches: {len(draw)} queries, {int(lengths.sum())} sequence bytes + {len(draw)} x {pc.PLACE_QUERY_BYTES_7} = {whole} bytes "
         f"against a room of {pc.BUDGET_ROOM} ({whole / pc.BUDGET_ROOM:.2f} times); the longest query {int(lengths.max())}")
    assert pc.PLACE_QUERY_BYTES_7 == 160 and whole > 2 * pc.BUDGET_ROOM and lengths.max() + pc.PLACE_QUERY_BYTES_7 < pc.BUDGET_ROOM // 32
    assert c.view.n_branches == 300 and 12 * 320 * 4 * 64 > pc.BUDGET_ROOM          # the global slices of a full grid (4 x 64 CUs or more) do not fit either
