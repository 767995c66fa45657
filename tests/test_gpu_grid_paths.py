"""GPU suite: the exact-sum cases of tests/grid_paths.py through every scoring entry point.  Their windows reach the long half joins,
the big-list kernels, the list slices and the second tiles of every kernel family with thousands of candidates exactly on a bound
and thousands of keys whose score ties across windows, tiles and matrices, so a `>=` at the final join of any of these paths, or
a tie broken for the later window, changes a key set, a scored count or a position here.  (A `>=` at an inner half join does not: on
exact sums a half-list candidate exactly on its bound never passes the final join.  There inputs whose bounds round decide: the
tenth-valued case below -- with `>=` in half_join_rows it scores 545 716 k-mers instead of 545 574 -- and, for every kernel family,
tests/test_gpu_rounded_paths.py, which reuses the checkers of this file by case name.)  Expected values come from the oracle, pinned on these very
cases by tests/test_grid_paths_inputs.py; every comparison is exact (key sets, raw score bits, positions, scored counts) through
tests/db_check.py.  Every test first asserts, through the CPU classifier, that its case still reaches its paths.  The engine fixture
is shared by the session: every test restores the options it sets."""
import contextlib
import functools

import numpy as np
import pytest

import ipk_amd
from ipk_amd import keyrange
from tests import db_check as dc
from tests import grid_paths as gp
from tests import long_lists as ll
from tests import rounded_paths as rp

pytestmark = pytest.mark.gpu

ONE_CALL = [n for n, c in gp.CASES.items() if c.k <= (14 if c.sigma == 4 else 6)]
KEY_RANGE = [n for n in gp.CASES if n not in ONE_CALL]                                   # DNA k = 15
VARIANT_OK = [n for n in ONE_CALL if gp.CASES[n].k <= 12]                               # every variant exists there (and for AA)
LONG = [n for n in ONE_CALL if gp.CASES[n].opts.get("slice_long_lists")]               # half lists beyond the capped capacity
VARIANTS = [1, 3, 4, 6, 7]
# debug_pool_limit_bytes under which the pool of a batch of the case's two groups does not fit and that of one group does (on an
# MI355X a wavefront's open chunks, one per key bucket, outweigh the pairs: twice the value fits both groups, half of it neither)
POOL_LIMIT = {"dna_k10": 32 << 20, "dna_k12": 16 << 20}


@functools.lru_cache(maxsize=None)
def on_its_paths(name):
    """The case with its paths asserted: (case, matrices, exact path counts).  A case that has drifted fails here, before the engine runs."""
    case, mats, counts = gp.load(name)
    if name in rp.CASES:                                 # sums round: the recorded counts come from the oracle's own list building
        counts = rp.cheap_counts(name)
        assert counts == {key: rp.COUNTS[name][key] for key in counts}, f"{name}: the recorded counts moved: {counts}"
        return case, mats, counts
    if case.family == "tenth":
        over = sum(max(nl, nr) > 160 for _, _, nl, nr in ll.longest_half_lists(mats, case.k, case.eps))
        assert over >= gp.TENTH_OVER_CAP, f"{name}: only {over} windows with a half list beyond 160"
        return case, mats, counts
    assert counts == gp.COUNTS[name], f"{name}: the path counts moved: {counts}"
    for path, floor in case.floors.items():
        if path.startswith("max_"):
            assert counts[path[4:]] <= floor, f"{name}: '{path[4:]}' is {counts[path[4:]]}, above {floor}"
        else:
            assert counts[path] >= floor, f"{name}: only {counts[path]} windows reach the path '{path}' (floor {floor})"
    assert counts["on_bound"] >= 1000
    return case, mats, counts


@functools.lru_cache(maxsize=None)
def expected(name, world=1):
    """({gid: db_check.Expect}, scored count, entries) of the case from the oracle."""
    case = on_its_paths(name)[0]
    res = gp.oracle(name)
    return ({r[0]: dc.Expect(r[1], r[2], r[4], case.sigma, case.k, world) for r in res}, sum(r[4] for r in res),
            sum(len(r[1]) for r in res))


def _oracle_of(name):
    by_gid = {r[0]: r for r in gp.oracle(name)}
    return lambda gid: (by_gid[gid][1], by_gid[gid][2])


@contextlib.contextmanager
def options(engine, name, **extra):
    """The options the case needs (slice_long_lists for the long lists of k >= 13) and `extra`, all back to their defaults afterwards;
    yields a function that tells the windows sliced since."""
    opts = dict(gp.load(name)[0].opts, **extra)
    before = engine.get_option("debug_sliced_windows")
    try:
        for key, value in opts.items():
            engine.set_option(key, value)
        yield lambda: engine.get_option("debug_sliced_windows") - before
    finally:
        for key in opts:
            engine.set_option(key, 0)


def check_group_major(engine, name, res, positions=False):
    """A group-major result against the oracle: groups in first-seen order, every group's keys and score bits, the scored count,
    and with `positions` the window that keeps each k-mer."""
    expect, emitted, entries = expected(name)
    want = gp.oracle(name)
    try:
        assert res.emitted == emitted, f"{name}: scored count {res.emitted}, the oracle's {emitted}"
        assert res.num_entries == entries, f"{name}: {res.num_entries} entries, the oracle's {entries}"
        keys, bits = dc.result_tensors(res)
        dc.check_groups(res.group_ids, res.offsets, keys, bits, [r[0] for r in want], expect, oracle=_oracle_of(name))
        del keys, bits
        if positions:
            got = res.positions()
            for gi, r in enumerate(want):
                a, b = int(res.offsets[gi]), int(res.offsets[gi + 1])
                diff = np.flatnonzero(got[a:b] != r[3])
                assert len(diff) == 0, (f"{name} group {r[0]}: {len(diff)} positions differ, the first at key {hex(int(r[1][diff[0]]))}: "
                                        f"window {int(got[a + diff[0]])}, the oracle's {int(r[3][diff[0]])}")
    finally:
        res.free()


def check_database(engine, name, db, owner=0, world=1, positions=False):
    """An owner's key-major database against the oracle, entry by entry; with `positions` (one owner) the window starts too."""
    case = gp.load(name)[0]
    expect = expected(name, world)[0]
    try:
        dk, off, entries = dc.db_tensors(db)
        dc.check_db(dk, off, entries, gp.group_order(case), expect, case.sigma, case.k, owner=owner, world=world, oracle=_oracle_of(name))
        del dk, off, entries
        if positions:
            assert world == 1
            want = gp.oracle_db(name)
            assert np.array_equal(db.keys(), want[0]) and np.array_equal(db.key_offsets(), want[1])
            diff = np.flatnonzero(db.positions() != want[4])
            assert len(diff) == 0, f"{name}: {len(diff)} positions of the key-major database differ, the first at entry {int(diff[0])}"
    finally:
        db.free()


def check_keymajor(engine, name, world):
    case, mats, _ = on_its_paths(name)
    _, emitted, entries = expected(name)
    parts = engine.score_groups_keymajor(mats, case.groups, case.k, case.eps, n_owners=world)
    try:
        assert parts.emitted == emitted and parts.num_entries == entries
        for o in range(world):
            db = engine.merge_parts_ptrs(case.sigma, case.k, o, world, [parts.counts_ptr() + 4 * o * parts.slots],
                                         [parts.entries_ptr() + 8 * int(parts.owner_offsets[o])])
            check_database(engine, name, db, o, world)
    finally:
        parts.free()


# ---- group-major -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ONE_CALL)
def test_score_groups_host_and_device_input(engine, name):
    import torch
    case, mats, counts = on_its_paths(name)
    with options(engine, name) as sliced:
        check_group_major(engine, name, engine.score_groups(mats, case.groups, case.k, case.eps))
        if name in LONG:
            assert sliced() == counts["over_cap"]          # exactly the windows with a half list beyond the cap take slices
        check_group_major(engine, name, engine.score_groups(torch.from_numpy(mats).cuda(), case.groups, case.k, case.eps))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", VARIANT_OK)
def test_every_scoring_variant(engine, name, variant):
    """The global-atomic reduce with the tiles kernel and its big-list kernel (1), the exact partition with dense and compressed
    tables (3, 4), the chunk-fed LDS reduce in both table forms (6, 7)."""
    case, mats, _ = on_its_paths(name)
    with options(engine, name, variant=variant):
        check_group_major(engine, name, engine.score_groups(mats, case.groups, case.k, case.eps))


@pytest.mark.parametrize("name", ONE_CALL)
def test_score_groups_positions(engine, name):
    """The positioned kernels: among equal scores the first window of the first matrix keeps its position -- the shifted twins of a
    group tie one window apart, the periodic case 37 windows apart (another tile, another wavefront)."""
    case, mats, counts = on_its_paths(name)
    with options(engine, name) as sliced:
        check_group_major(engine, name, engine.score_groups_positions(mats, case.groups, case.k, case.eps), positions=True)
        if name in LONG:
            assert sliced() == counts["over_cap"]


@pytest.mark.parametrize("name", LONG)
def test_long_lists_fail_loudly_without_the_option(engine, name):
    """The same input with slice_long_lists off: an error from every entry point, not a result with k-mers missing."""
    case, mats, counts = on_its_paths(name)
    assert counts["over_cap"] >= 3 and engine.get_option("slice_long_lists") == 0
    for call in (engine.score_groups, engine.score_groups_positions, engine.score_groups_keymajor):
        with pytest.raises(ipk_amd.IpkGpuError):
            call(mats, case.groups, case.k, case.eps)


# ---- key-major -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ONE_CALL)
def test_keymajor_one_and_three_owners(engine, name):
    with options(engine, name):
        check_keymajor(engine, name, 1)
        check_keymajor(engine, name, 3)


@pytest.mark.parametrize("name", ONE_CALL)            # (every case has more than 64 keys: the positioned key-major call exists)
def test_keymajor_positions(engine, name):
    case, mats, _ = on_its_paths(name)
    _, emitted, entries = expected(name)
    with options(engine, name):
        parts = engine.score_groups_keymajor_positions(mats, case.groups, case.k, case.eps)
        try:
            assert parts.emitted == emitted and parts.num_entries == entries
            check_database(engine, name, engine.db_from_parts(parts, case.sigma, case.k), positions=True)
        finally:
            parts.free()


@pytest.mark.parametrize("name", KEY_RANGE)
def test_key_range_passes(engine, name):
    """DNA k = 15 as tests/test_gpu_long_lists.py::test_key_range_passes walks it: every class of the first symbol against its range
    of the oracle's database, the scored counts summed; the right halves beyond the cap are sliced."""
    case, mats, counts = on_its_paths(name)
    assert case.k == 15 and int((gp.half_lists(mats, case.k, case.eps)[:, 1] > gp.BIG_CAP).sum()) >= 3
    assert check_key_range(engine, name) > 0


def check_key_range(engine, name):
    """Every key-range pass of a DNA k = 15 / 16 case against its range of the oracle's database; returns the windows sliced."""
    case, mats, counts = on_its_paths(name)
    k, lead = case.k, case.k - 14
    assert lead >= 1
    ok, ooff, obr, osc, _ = gp.oracle_db(name)
    ooff = ooff.astype(np.int64)
    total, seen = 0, 0
    with options(engine, name) as sliced:
        for j, cls, base, span in keyrange.plan(4, k, 4 ** lead):
            parts = engine.score_groups_keyrange(mats, case.groups, k, case.eps, j, cls)
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
        n_sliced = sliced()
    assert seen == len(ok) and total == expected(name)[1]
    return n_sliced


# ---- stress modes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dna_k10", "dna_k10_periodic", "dna_k12"])
def test_chunk_rolls_and_rebases(engine, name):
    """debug_flags bit 3 (tests/test_gpu_half_join_paths.py::test_rows_meet_chunk_rolls): every wavefront rolls its chunks and rebases
    its store window every 8 chunks, so candidates on the bounds and tying windows meet the rolls."""
    case, mats, _ = on_its_paths(name)
    with options(engine, name, debug_flags=8):
        check_group_major(engine, name, engine.score_groups(mats, case.groups, case.k, case.eps))
        check_keymajor(engine, name, 1)


def launches(res):
    n = res.time_ms(4)                                     # IPKGPU_T_SCORE_LAUNCHES
    res.free()
    return n


@pytest.mark.parametrize("name", ["dna_k10", "dna_k12"])
def test_pool_that_does_not_fit_halves_the_batch(engine, name):
    """debug_pool_limit_bytes (tests/test_gpu_parity.py::test_pool_that_does_not_fit_means_smaller_batches): the pair pool of the
    batch of two groups does not fit, the engine scores the groups one by one.  An engine of its own with the limit set before its
    first call: it has no pool yet and no calibration of the pairs a window gives."""
    case, mats, _ = on_its_paths(name)
    free = launches(engine.score_groups(mats, case.groups, case.k, case.eps))
    eng = ipk_amd.Engine(0)
    try:
        eng.set_option("debug_pool_limit_bytes", POOL_LIMIT[name])
        res = eng.score_groups(mats, case.groups, case.k, case.eps)
        assert res.time_ms(4) > free, "the limit did not force smaller batches"
        check_group_major(eng, name, res)
        check_group_major(eng, name, eng.score_groups_positions(mats, case.groups, case.k, case.eps), positions=True)
        check_keymajor(eng, name, 1)
    finally:
        eng.close()


def test_groups_in_different_batches(engine):
    """workspace_bytes below two score tables of k = 10 (tests/test_gpu_parity.py::test_workspace_batching): one group a batch, and
    the second batch's results appended behind the first's."""
    name = "dna_k10"
    case, mats, _ = on_its_paths(name)
    free = launches(engine.score_groups(mats, case.groups, case.k, case.eps))
    before = engine.get_option("workspace_bytes")
    engine.set_option("workspace_bytes", 4 ** 10 * 4)
    try:
        res = engine.score_groups(mats, case.groups, case.k, case.eps)
        assert res.time_ms(4) > free, "the two groups were scored in one batch"
        check_group_major(engine, name, res)
        check_group_major(engine, name, engine.score_groups_positions(mats, case.groups, case.k, case.eps), positions=True)
        check_keymajor(engine, name, 1)
    finally:
        engine.set_option("workspace_bytes", before)


# ---- where rounded inner bounds decide --------------------------------------------------------------------------------------------

def test_tenth_case(engine):
    """Entries -0.1 * an integer at k = 10 with half lists beyond 160: the default variant, the global-atomic reduce, key-major."""
    name = gp.TENTH.name
    case, mats, _ = on_its_paths(name)
    check_group_major(engine, name, engine.score_groups(mats, case.groups, case.k, case.eps))
    with options(engine, name, variant=1):
        check_group_major(engine, name, engine.score_groups(mats, case.groups, case.k, case.eps))
    check_keymajor(engine, name, 1)
