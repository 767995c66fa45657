"""GPU suite: the rounded-bound cases of tests/rounded_paths.py -- one per kernel family, and one whose prefix sums run over
two chunk boundaries of the prefix kernel -- through every scoring entry point.  Their entries are -0.1 * an integer, so the prefix
sums of the column maxima and every look-ahead bound eps - M(...) round, and hundreds to thousands of candidates lie within an ulp
of a bound: an inner join that keeps `>=`, a bound taken from differently associated prefix sums (restarted at the window or at a
chunk, accumulated wider and rounded once) changes key sets and scored counts here, as tests/test_rounded_paths_inputs.py shows for
each case on the CPU.  Expected values come from the oracle, pinned on these very cases to the reference's compiled code; every
comparison is exact (key sets, raw score bits, positions, scored counts) through the checkers of tests/test_gpu_grid_paths.py.
Every test first asserts the case's recorded CPU counts.  The engine fixture is shared by the session: every test restores the
options it sets."""
import pytest

from tests import rounded_paths as rp
from tests import test_gpu_grid_paths as tg

pytestmark = pytest.mark.gpu

TABLE = [n for n in rp.CASES if n != rp.LONG]
ONE_CALL = [n for n in TABLE if rp.CASES[n].k <= (14 if rp.CASES[n].sigma == 4 else 6)]
KEY_RANGE = [n for n in TABLE if n not in ONE_CALL]                                      # DNA k = 15, 16
VARIANT_OK = [n for n in ONE_CALL if rp.CASES[n].k <= 12]
SLICED = [n for n in ONE_CALL if rp.CASES[n].opts.get("slice_long_lists")]


def sliced_as_recorded(name, counts, sliced):
    if name in SLICED:
        assert sliced() == counts["over_cap"]              # exactly the windows with a half list beyond the cap take slices


@pytest.mark.parametrize("name", ONE_CALL)
def test_score_groups_host_and_device_input(engine, name):
    import torch
    case, mats, counts = tg.on_its_paths(name)
    with tg.options(engine, name) as sliced:
        tg.check_group_major(engine, name, engine.score_groups(mats, case.groups, case.k, case.eps))
        sliced_as_recorded(name, counts, sliced)
        tg.check_group_major(engine, name, engine.score_groups(torch.from_numpy(mats).cuda(), case.groups, case.k, case.eps))


@pytest.mark.parametrize("variant", tg.VARIANTS)
@pytest.mark.parametrize("name", VARIANT_OK)
def test_every_scoring_variant(engine, name, variant):
    case, mats, _ = tg.on_its_paths(name)
    with tg.options(engine, name, variant=variant):
        tg.check_group_major(engine, name, engine.score_groups(mats, case.groups, case.k, case.eps))


@pytest.mark.parametrize("name", ONE_CALL)
def test_score_groups_positions(engine, name):
    """A candidate that a rounded bound cuts from the first twin's window keeps the later window's position (the `cut` counts)."""
    case, mats, counts = tg.on_its_paths(name)
    with tg.options(engine, name) as sliced:
        tg.check_group_major(engine, name, engine.score_groups_positions(mats, case.groups, case.k, case.eps), positions=True)
        sliced_as_recorded(name, counts, sliced)


@pytest.mark.parametrize("name", ONE_CALL)
def test_keymajor_one_and_three_owners(engine, name):
    with tg.options(engine, name):
        tg.check_keymajor(engine, name, 1)
        tg.check_keymajor(engine, name, 3)


@pytest.mark.parametrize("name", ONE_CALL)
def test_keymajor_positions(engine, name):
    case, mats, _ = tg.on_its_paths(name)
    _, emitted, entries = tg.expected(name)
    with tg.options(engine, name):
        parts = engine.score_groups_keymajor_positions(mats, case.groups, case.k, case.eps)
        try:
            assert parts.emitted == emitted and parts.num_entries == entries
            tg.check_database(engine, name, engine.db_from_parts(parts, case.sigma, case.k), positions=True)
        finally:
            parts.free()


@pytest.mark.parametrize("name", KEY_RANGE)
def test_key_range_passes(engine, name):
    tg.check_key_range(engine, name)


@pytest.mark.parametrize("name", [n for n in ("dna_k9_tenth", "dna_k11_tenth") if n in rp.CASES])
def test_chunk_rolls_and_rebases(engine, name):
    """debug_flags bit 3 on one quad and one rows case: candidates an ulp from their bounds meet the chunk rolls."""
    case, mats, _ = tg.on_its_paths(name)
    with tg.options(engine, name, debug_flags=8):
        tg.check_group_major(engine, name, engine.score_groups(mats, case.groups, case.k, case.eps))
        tg.check_keymajor(engine, name, 1)


# ---- prefix sums over two chunk boundaries ------------------------------------------------------------------------------------------

def test_long_prefix_sums(engine):
    """More than 4096 sites a matrix: the bounds of the windows behind sites 2048 and 4096 are differences of prefix sums that the
    prefix kernel carries over its chunk boundaries.  Group-major, positions, key-major."""
    name = rp.LONG
    case, mats, _ = tg.on_its_paths(name)
    assert case.sites > 2 * rp.CHUNK + case.k
    tg.check_group_major(engine, name, engine.score_groups(mats, case.groups, case.k, case.eps))
    tg.check_group_major(engine, name, engine.score_groups_positions(mats, case.groups, case.k, case.eps), positions=True)
    tg.check_keymajor(engine, name, 1)


@pytest.mark.parametrize("per_workgroup", [1, 2, 8])
def test_long_prefix_sums_at_every_chunk_length(engine, per_workgroup):
    """debug_prefix_mats: a workgroup of the prefix kernel that takes M matrices sums them in chunks of 2048 / M sites."""
    name = rp.LONG
    case, mats, _ = tg.on_its_paths(name)
    engine.set_option("debug_prefix_mats", per_workgroup)
    try:
        tg.check_group_major(engine, name, engine.score_groups(mats, case.groups, case.k, case.eps))
    finally:
        engine.set_option("debug_prefix_mats", 0)


def test_long_prefix_sums_in_two_batches(engine):
    """workspace_bytes below two score tables of k = 10: the two groups (one matrix each) fall into two batches."""
    name = rp.LONG
    case, mats, _ = tg.on_its_paths(name)
    free = tg.launches(engine.score_groups(mats, case.groups, case.k, case.eps))
    before = engine.get_option("workspace_bytes")
    engine.set_option("workspace_bytes", 4 ** 10 * 4)
    try:
        res = engine.score_groups(mats, case.groups, case.k, case.eps)
        assert res.time_ms(4) > free, "the two groups were scored in one batch"
        tg.check_group_major(engine, name, res)
    finally:
        engine.set_option("workspace_bytes", before)
