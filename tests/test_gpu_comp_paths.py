"""GPU suite: the fabricated slices of tests/comp_paths.py through the compressed back half -- the LDS max-reduce
(reduce_buckets_pipe_kernel, reduce_buckets_kernel<.., true>, reduce_ranges_kernel<.., true>, reduce_ranges_pos_kernel), compress_slice,
the compressed key-major writers (per block, per run), their passes, and the merge of batches -- bit for bit against the direct
enumeration of the cases' boxes: scored count, counts, entries, owner offsets, group-major keys and score bits, positions.
tests/test_comp_paths_inputs.py asserts on the CPU what every case holds (full blocks beside empty ones, empty wavefront regions,
a value room filled to its last unit, fewer chunks than wavefronts, tens of chunks per wavefront, the slice sequences a persistent
workgroup meets) and that the enumeration is the oracle's.  Every call must report compressed tables."""
import functools

import numpy as np
import pytest
import torch

import ipk_amd
from ipk_amd import engine as E
from tests import comp_paths as cp
from tests.test_gpu_parity import _check_parts_against_oracle

pytestmark = pytest.mark.gpu

PER_SLICE, PER_BLOCK, PER_RUN = 2048, 4096, 8192          # debug_flags: reduce with a workgroup per slice | writer per 64-key block | per run of blocks
STREAM = [(11, 1), (11, 2), (11, 3), (12, 1), (12, 3)]   # (k, groups) of the stream variant's compressed tables


@functools.lru_cache(maxsize=None)
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _case(k, n_groups):
    return cp.build(k, n_groups, _cus())


def _load(key):
    """(k, groups): the case built for this device's CU count; ("nine", k), ("block", k), ("small", k), ("aa", 6): comp_paths.nine_groups,
    full_block, small_dna, aa_k6."""
    if key[0] in ("aa", "k14"):
        return cp.aa_k6() if key[0] == "aa" else cp.k14()
    return {"nine": cp.nine_groups, "block": cp.full_block, "small": cp.small_dna, "big": cp.big_box}[key[0]](key[1]) if isinstance(key[0], str) else _case(*key)


@functools.lru_cache(maxsize=None)
def _want(key, owners):
    case = _load(key)
    return cp.key_major(cp.case_expect(case), owners)


@pytest.fixture(scope="module")
def eng():
    e = ipk_amd.Engine(0)
    yield e
    e.close()


def _options(e, **opts):
    for name in ("debug_flags", "variant", "debug_kmc_pass", "slice_long_lists"):
        e.set_option(name, opts.get(name, 0))


def _first_diff(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} against {len(want)}"
    d = np.flatnonzero(np.asarray(got) != np.asarray(want))
    assert len(d) == 0, f"{what}: {len(d)} differ, the first at {int(d[0])}: {got[d[0]]} against {want[d[0]]}"


def _check_parts(e, parts, want, owners, positions=False, oracle_of=None):
    """Parts against `comp_paths.key_major`; the counts rows are compared on the device (4^13 slots)."""
    emitted, per_owner, entries, pos, offsets = want
    try:
        assert e.last_tables_compressed(), "the call did not take compressed tables"
        assert parts.emitted == emitted, f"scored count {parts.emitted}, expected {emitted}"
        assert [int(x) for x in parts.owner_offsets] == offsets
        counts = parts.counts_tensor()
        assert counts.shape[0] == owners
        for o, (slots, n) in enumerate(per_owner):
            nz = torch.nonzero(counts[o]).flatten()
            _first_diff(nz.cpu().numpy(), slots, f"owner {o}: slots with entries")
            _first_diff(counts[o][nz].cpu().numpy(), n, f"owner {o}: counts")
        got = parts.entries_tensor().cpu().numpy().view(np.uint32)
        _first_diff(got[:, 0], entries[:, 0], "group ids")
        _first_diff(got[:, 1], entries[:, 1], "score bits")
        if positions:
            _first_diff(parts.positions_tensor().cpu().numpy().view(np.uint32), pos, "positions")
        if oracle_of is not None:                          # and through tests/db_check.py, as the dense suite does
            case = oracle_of
            dense = np.zeros((owners, int(counts.shape[1])), dtype=np.int64)
            for o, (slots, n) in enumerate(per_owner):
                dense[o, slots] = n
            _check_parts_against_oracle(parts.emitted, dense, got.view(np.int32), offsets, case.mats, case.groups, 4, case.k, cp.EPS)
    finally:
        parts.free()


def _check_group_major(e, res, expect):
    try:
        assert e.last_tables_compressed(), "the call did not take compressed tables"
        assert res.emitted == sum(r[4] for r in expect)
        assert res.num_entries == sum(len(r[1]) for r in expect)
        for gi, (gid, keys, bits, _, _) in enumerate(expect):
            gk, gs = res.group(gi)
            _first_diff(gk, keys.astype(np.uint32), f"group {gid}: keys")
            _first_diff(gs.view(np.uint32), bits, f"group {gid}: score bits")
    finally:
        res.free()


# ---- DNA k = 11, 12: stream variant, 128-KB slices ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [PER_BLOCK, PER_RUN, PER_SLICE | PER_BLOCK, PER_SLICE | PER_RUN],
                         ids=["pipe-block", "pipe-run", "slice-block", "slice-run"])
@pytest.mark.parametrize("k,n_groups", STREAM)
def test_reduce_and_writer_forms(eng, k, n_groups, flags):
    """The persistent reduce and the workgroup-per-slice reduce, each in front of the writer per block and per run: one owner."""
    case = _case(k, n_groups)
    _options(eng, debug_flags=flags)
    parts = eng.score_groups_keymajor(case.mats, case.groups, k, cp.EPS, n_owners=1)
    _check_parts(eng, parts, _want((k, n_groups), 1), 1, oracle_of=case if flags in (PER_BLOCK, PER_SLICE | PER_RUN) and (k, n_groups) != (12, 1) else None)


@pytest.mark.parametrize("flags", [0, PER_SLICE], ids=["pipe", "slice"])
@pytest.mark.parametrize("k,n_groups", STREAM)
def test_three_owners_and_group_major(eng, k, n_groups, flags):
    case = _case(k, n_groups)
    _options(eng, debug_flags=flags)
    parts = eng.score_groups_keymajor(case.mats, case.groups, k, cp.EPS, n_owners=3)
    _check_parts(eng, parts, _want((k, n_groups), 3), 3, oracle_of=case if n_groups == 3 else None)
    _check_group_major(eng, eng.score_groups(case.mats, case.groups, k, cp.EPS), cp.case_expect(case))


@pytest.mark.parametrize("n_groups", [1, 3])
def test_exact_partition_reduce_at_k12(eng, n_groups):
    """Variant 4: the same slices through reduce_ranges_kernel<.., true> (values in place in the pair pool)."""
    case = _case(12, n_groups)
    for flags in (PER_BLOCK, PER_RUN):
        _options(eng, variant=4, debug_flags=flags)
        parts = eng.score_groups_keymajor(case.mats, case.groups, 12, cp.EPS, n_owners=1)
        _check_parts(eng, parts, _want((12, n_groups), 1), 1)
    _options(eng, variant=4)
    _check_group_major(eng, eng.score_groups(case.mats, case.groups, 12, cp.EPS), cp.case_expect(case))


@pytest.mark.parametrize("k", [12, 13])
def test_big_box_from_the_long_list_path(eng, k):
    """One 32 768-key window fills a slice: the same reduce, epilogue and writers fed by the big-list kernels (k = 13: in slices,
    its right half list of 16 384 exceeds the capped capacity).  Both reduces and writers at k = 12, three owners, group-major,
    positions."""
    case = cp.big_box(k)
    long_lists = dict(slice_long_lists=1) if k == 13 else {}
    for flags in ((PER_BLOCK, PER_SLICE | PER_RUN) if k == 12 else (PER_BLOCK, PER_RUN)):
        _options(eng, debug_flags=flags, **long_lists)
        parts = eng.score_groups_keymajor(case.mats, case.groups, k, cp.EPS, n_owners=1)
        _check_parts(eng, parts, _want(("big", k), 1), 1, oracle_of=case if k == 12 else None)
    _options(eng, **long_lists)
    parts = eng.score_groups_keymajor(case.mats, case.groups, k, cp.EPS, n_owners=3)
    _check_parts(eng, parts, _want(("big", k), 3), 3)
    _check_group_major(eng, eng.score_groups(case.mats, case.groups, k, cp.EPS), cp.case_expect(case))
    parts = eng.score_groups_keymajor_positions(case.mats, case.groups, k, cp.EPS)
    _check_parts(eng, parts, _want(("big", k), 1), 1, positions=True)
    _options(eng)


# ---- positions: two trips per slice of reduce_ranges_pos_kernel ---------------------------------------------------------------------------

@pytest.mark.parametrize("k,n_groups", [(12, 1), (12, 3), (13, 1)])
def test_positions(eng, k, n_groups):
    """The positioned calls: the window start of the winning pair, among equal score bits the smallest rank * nwin + start; slices
    whose first half (the first trip's slots) is empty, and whose second is."""
    case = _case(k, n_groups)
    _options(eng)
    parts = eng.score_groups_keymajor_positions(case.mats, case.groups, k, cp.EPS)
    _check_parts(eng, parts, _want((k, n_groups), 1), 1, positions=True, oracle_of=case if k == 12 else None)
    parts = eng.score_groups_keymajor_positions_owners(case.mats, case.groups, k, cp.EPS, n_owners=3)
    _check_parts(eng, parts, _want((k, n_groups), 3), 3, positions=True, oracle_of=case if k == 12 else None)


def test_k13_exact_partition(eng):
    """DNA k = 13: compressed tables by default (reduce_ranges_kernel), key-major with one and three owners, group-major."""
    case = _case(13, 1)
    _options(eng)
    for owners in (1, 3):
        parts = eng.score_groups_keymajor(case.mats, case.groups, 13, cp.EPS, n_owners=owners)
        _check_parts(eng, parts, _want((13, 1), owners), owners)
    _check_group_major(eng, eng.score_groups(case.mats, case.groups, 13, cp.EPS), cp.case_expect(case))


def test_k14_three_owners(eng):
    """DNA k = 14 (8192 slices a group, a counts row of 2^28 slots): `corners` and `dense`, three owners."""
    case = cp.k14()
    _options(eng)
    parts = eng.score_groups_keymajor(case.mats, case.groups, 14, cp.EPS, n_owners=3)
    _check_parts(eng, parts, _want(("k14", 14), 3), 3)


# ---- 64-KB slices: the PAIR6 reduce of DNA k = 8, 10 under variant 6, and amino acids k = 6 ------------------------------------------------

@pytest.mark.parametrize("flags", [PER_BLOCK, PER_RUN], ids=["block", "run"])
@pytest.mark.parametrize("k", [8, 10])
def test_pair6_compressed_reduce(eng, k, flags):
    """reduce_buckets_kernel<16384, 512, true, PAIR6>: 8 wavefronts of 32 blocks; both writers, one and three owners, group-major."""
    case = cp.small_dna(k)
    _options(eng, variant=6, debug_flags=flags)
    for owners in (1, 3):
        parts = eng.score_groups_keymajor(case.mats, case.groups, k, cp.EPS, n_owners=owners)
        _check_parts(eng, parts, _want(("small", k), owners), owners)
    _check_group_major(eng, eng.score_groups(case.mats, case.groups, k, cp.EPS), cp.case_expect(case))


def test_positions_in_one_trip_at_k10(eng):
    """A 16 384-slot slice fits the positions reduce whole: one trip."""
    case = cp.small_dna(10)
    _options(eng)
    parts = eng.score_groups_keymajor_positions(case.mats, case.groups, 10, cp.EPS)
    _check_parts(eng, parts, _want(("small", 10), 1), 1, positions=True)


def test_amino_acids_k6(eng):
    """16 000-slot slices, 250 real blocks of 256 (`last_block_partial`): key-major with one and three owners on both writers,
    group-major, and the positioned calls (one trip)."""
    case = cp.aa_k6()
    for flags in (PER_BLOCK, PER_RUN):
        _options(eng, debug_flags=flags)
        for owners in (1, 3):
            parts = eng.score_groups_keymajor(case.mats, case.groups, 6, cp.EPS, n_owners=owners)
            _check_parts(eng, parts, _want(("aa", 6), owners), owners)
    _options(eng)
    expect = [(gid, cp.pack_aa(keys), bits, pos, n) for gid, keys, bits, pos, n in cp.case_expect(case)]
    _check_group_major(eng, eng.score_groups(case.mats, case.groups, 6, cp.EPS), expect)
    parts = eng.score_groups_keymajor_positions(case.mats, case.groups, 6, cp.EPS)
    _check_parts(eng, parts, _want(("aa", 6), 1), 1, positions=True)
    parts = eng.score_groups_keymajor_positions_owners(case.mats, case.groups, 6, cp.EPS, n_owners=3)
    _check_parts(eng, parts, _want(("aa", 6), 3), 3, positions=True)


# ---- batches and writer passes --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [PER_BLOCK, PER_RUN], ids=["block", "run"])
@pytest.mark.parametrize("form", ["batches", "passes"])
def test_nine_groups_in_batches_and_passes(form, flags):
    """Nine groups of `neighbours` / `dups` at k = 11: under a workspace of three and a half groups (three batches of three, merged:
    merge_sources) and under debug_kmc_pass = 4 (writer passes of 4, 4 and 1 groups)."""
    case = cp.nine_groups(11)
    e = ipk_amd.Engine(0)                                       # (fresh: the batch size follows the pool rate a context has learnt)
    try:
        e.set_option("debug_flags", flags)
        if form == "batches":
            # per group as make_plan prices it before a context's first call: 4 bytes a slot and 256 pairs of 8 bytes a window, a quarter more
            per_group = 4 ** 11 * 4 + len(case.mats) / 9 * (case.mats.shape[1] - 11 + 1) * 256 * 8 * 1.25
            e.set_option("workspace_bytes", int(3.5 * per_group))
        else:
            e.set_option("debug_kmc_pass", 4)
        for owners in (1, 3):
            parts = e.score_groups_keymajor(case.mats, case.groups, 11, cp.EPS, n_owners=owners)
            if form == "batches" and owners == 1:               # (a batch whose pool did not fit is halved: never fewer than three)
                assert parts.time_ms(E.T_SCORE_LAUNCHES) >= 3
            if form == "passes":                                # (passes of 4, 4 and 1 need the nine groups in one batch)
                assert parts.time_ms(E.T_SCORE_LAUNCHES) == 1
            _check_parts(e, parts, _want(("nine", 11), owners), owners)
    finally:
        e.close()


@pytest.mark.parametrize("flags", [PER_BLOCK, PER_RUN], ids=["block", "run"])
def test_a_key_block_beyond_the_lds_stage(eng, flags):
    """130 groups hold the same full 64-key block: 8320 entries of one key block against the 4224 the writer stages in LDS."""
    case = cp.full_block(11)
    assert 64 * len(cp.group_order(case)) == 8320 > cp.KMC_CAP
    _options(eng, debug_flags=flags)
    parts = eng.score_groups_keymajor(case.mats, case.groups, 11, cp.EPS, n_owners=1)
    assert parts.time_ms(E.T_SCORE_LAUNCHES) == 1              # (one batch: two of 65 groups would stay below KMC_CAP)
    _check_parts(eng, parts, _want(("block", 11), 1), 1)
