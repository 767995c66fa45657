"""CPU suite: the fabricated slices of tests/comp_paths.py are what they claim -- per pattern the exact keys, pairs, occupancy per
64-slot block and per wavefront region, value room and chunk bounds; the workgroup sequences of the persistent reduce for two CU
counts --, their expectation (direct enumeration) is the oracle's explore_group_pos bit for bit (and the live reference's where its
binaries are present), and three wrong back halves change it."""
import numpy as np
import pytest

from oracle import ipk_oracle as co
from oracle import ref_build as rb
from tests import comp_paths as cp

CASES = [(11, 1), (11, 2), (11, 3), (12, 1), (12, 3), (13, 1)]          # (k, groups); tests/test_gpu_comp_paths.py runs the same
CUS = [256, 64]
W = cp.BPW * cp.BLOCK                                                    # slots of a wavefront region


def _stats(case, name):
    """slice_stats of every slice of the case that carries pattern `name`."""
    return [(g, b, cp.slice_stats(case, g, b)) for (g, b), v in sorted(case.slices.items(), key=lambda kv: kv[0]) if v == name or v[0] == name]


def _blocks(st, first, n):
    return st["blocks"][first:first + n].tolist()


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("k,n_groups", CASES)
def test_every_pattern_is_what_it_claims(k, n_groups, cus):
    case = cp.build(k, n_groups, cus)
    tbl, waves, nb = cp.geometry(4, k)
    nwin = case.mats.shape[1] - k + 1
    assert (tbl, waves) == (32768, 16) and nb == 4 ** k // tbl
    assert len(case.mats) <= 200 and case.mats.shape[1] <= 60
    names = {v if isinstance(v, str) else v[0] for v in case.slices.values()}
    want = {"dense", "dups", "few_chunks_17"} | {"corners"} | ({"few_chunks_1"} if n_groups == 3 and k == 12 else set())
    if n_groups == 1 or (k, n_groups) == (11, 2):
        want |= (set(cp.CATALOGUE) | {"few_chunks_1"}) - ({"one_wave_rest"} if n_groups > 1 else set())
    assert want <= names, want - names
    seen = 0
    for g, b, st in _stats(case, "corners"):
        assert st["slots"].tolist() == [0, 31, 32, 63, 64, tbl - 1] and st["pairs"] == 7 and st["room"] == 4 and st["used"] == 3 and st["chunks_floor"] == 1
        seen += 1
    for g, b, st in _stats(case, "neighbours"):
        assert _blocks(st, cp.BPW + 10, 5) == [64, 0, 1, 1, 64] and _blocks(st, 2 * cp.BPW + 30, 5) == [64, 0, 1, 1, 64]
        assert st["keys"] == st["pairs"] == 4 * 64 + 4 and st["waves"].tolist() == [0, 130, 64, 66] + [0] * 12
        blk = (cp.BPW + 12) * 64
        assert {blk, blk + 64 + 63, 96 * 64, 97 * 64 + 63} <= set(st["slots"].tolist())          # lane 0, lane 63, twice
        seen += 1
    for g, b, st in _stats(case, "alternate"):
        assert _blocks(st, 4 * cp.BPW, cp.BPW) == [64, 0] * 16 and _blocks(st, 5 * cp.BPW, cp.BPW) == [0, 64] * 16
        assert st["keys"] == st["pairs"] == 2048 and st["waves"].tolist() == [0] * 4 + [1024, 1024] + [0] * 10
        seen += 1
    for which, regions in (("first", [W] + [0] * 15), ("last", [0] * 15 + [W]), ("rest", [0] + [W] * 15)):
        for g, b, st in _stats(case, "one_wave_" + which):
            assert st["waves"].tolist() == regions and st["keys"] == st["pairs"] == sum(regions)
            assert set(st["blocks"].tolist()) == {0, 64}
            seen += 1
    for g, b, st in _stats(case, "dense"):
        assert st["keys"] == st["pairs"] == tbl and st["blocks"].tolist() == [64] * (tbl // 64)
        assert st["room"] == st["used"] == tbl // 2 and st["chunks_floor"] == tbl // cp.CH      # the value room filled to its last unit
        # an overrun of its value area shows in a neighbour: the value areas follow one another in (group, slice) order
        around = [case.slices.get((g, b - 1)), case.slices.get((g, b + 1)), case.slices.get(((g + 1) % n_groups, b))]
        later = [v for (gg, bb), v in case.slices.items() if (gg, bb) > (g, b) and v != "empty"]
        assert later and any(v not in (None, "empty", "dense") for v in around), around
        seen += 1
    for n in (1, 3, 4095):
        for g, b, st in _stats(case, f"odd_{n}"):
            assert st["slots"].tolist() == list(range(5, 5 + n)) and st["pairs"] == n
            assert st["room"] == st["used"] == (n + 1) // 2 and 2 * st["room"] == n + 1          # the 4-byte hole of an odd count
            seen += 1
    for n in (1, 2, 15, 16, 17):
        for g, b, st in _stats(case, f"few_chunks_{n}"):
            assert st["pairs"] == 128 * n and st["keys"] == 128 * min(n, 8) and st["slots"].max() == 128 * min(n, 8) - 1
            assert st["chunks_floor"] == (n + 1) // 2 <= n                    # between ceil(pairs / 256) chunks and one per matrix
            assert (st["chunks_floor"] < waves) == (n < 2 * waves)            # fewer chunks than wavefronts may draw them
            seen += 1
    for g, b, st in _stats(case, "dups"):
        per_slice = 2 ** k // len(cp.dups_slices(k, case.slices[(g, b)][1]))
        assert per_slice in (128, 256) and st["keys"] == per_slice and st["pairs"] == per_slice * nwin * cp.dups_m(k, case.slices[(g, b)][1])
        assert st["room"] == (min(st["pairs"], tbl) + 1) // 2 and st["room"] > st["used"]
        trips = st["chunks_floor"] // (waves * cp.RPIPE_D)
        # at least 640 chunks: 40 per wavefront, 20 trips of D = 2
        assert st["chunks_floor"] >= cp.DUPS_CHUNKS == 640 and st["chunks_floor"] // waves >= 40 and trips >= cp.DUPS_TRIPS == 20, (trips, st["chunks_floor"])
        seen += 1
    for g in sorted({g for (g, b), v in case.slices.items() if v[0] == "dups"}):
        tied, first, middle, last = cp.dups_stats(case, g)
        assert tied >= 1 / 3 and min(first, middle, last) >= 1, (tied, first, middle, last)      # a third of the keys tie; the maximum in the first, a middle and the last matrix
    assert seen == sum(v != "empty" for v in case.slices.values())
    # and nothing anywhere else: every other slice of every group is empty
    for gi, gid in enumerate(cp.group_order(case)):
        keys = cp.group_pairs(case, gid)[0]
        touched = set((keys // tbl).tolist())
        assert touched == {b for (g, b), v in case.slices.items() if g == gi and v != "empty"}


@pytest.mark.parametrize("k,n_groups", [(11, 2), (12, 1), (13, 1)])
def test_the_odd_counts_stand_in_consecutive_slices(k, n_groups):
    case = cp.build(k, n_groups, 256)
    (g1, b1, _), (g3, b3, _), (g4, b4, _) = _stats(case, "odd_1")[0], _stats(case, "odd_3")[0], _stats(case, "odd_4095")[0]
    assert (b3, b4) == (b1 + 1, b1 + 2) and g1 == g3 == g4


@pytest.mark.parametrize("cus", CUS)
def test_a_persistent_workgroup_meets_every_sequence(cus):
    """DNA k = 12, three groups: each sequence of comp_paths.SEQUENCES stands on consecutive slices of one workgroup (w, w + G, ...),
    the `last_*` ones on its last slice; a slice named empty holds no pair."""
    case = cp.build(12, 3, cus)
    tbl, waves, nb = cp.geometry(4, 12)
    assert sorted(case.sequences) == sorted(cp.SEQUENCES)
    assert len({w for w, _, _ in case.sequences.values()}) == len(cp.SEQUENCES)                 # a workgroup each
    for seq, (w, j, where) in case.sequences.items():
        items = cp.workgroup_items(w, 3, nb, cus)
        assert len(items) == 3 * nb // cus and items[0] == (0, w) and items[1] == divmod(w + cus, nb)
        assert items[j:j + len(where)] == where
        if seq.startswith("last_"):
            assert j == len(items) - 1
        for (g, b), name in zip(where, cp.SEQUENCES[seq]):
            got = case.slices[(g, b)]
            assert (got if isinstance(got, str) else got[0]) == name
            assert (cp.slice_stats(case, g, b)["pairs"] == 0) == (name == "empty")


def test_group_counts_at_k11():
    """One group: fewer slices than CUs; two: as many as an MI355X has CUs; three: half the workgroups hold two slices."""
    nb = cp.geometry(4, 11)[2]
    assert nb == 128 and cp.geometry(4, 12)[2] == 512
    assert [len(cp.workgroup_items(w, 1, nb, 256)) for w in (0, 127, 128)] == [1, 1, 0]
    assert [len(cp.workgroup_items(w, 2, nb, 256)) for w in (0, 255)] == [1, 1]
    assert [len(cp.workgroup_items(w, 3, nb, 256)) for w in (0, 127, 128, 255)] == [2, 2, 1, 1]
    case = cp.build(11, 3, 256)
    assert {"last_dups", "last_empty", "few17_dense"} <= set(case.sequences)


@pytest.mark.parametrize("k,n_groups", CASES)
def test_scores_positive_zero_tied_and_decided_by_rank(k, n_groups):
    case = cp.build(k, n_groups, 256)
    nwin = case.mats.shape[1] - k + 1
    finite = case.mats[case.mats > cp.NEG]
    assert np.array_equal(finite * 4, np.round(finite * 4)) and finite.min() >= -2.0 and finite.max() <= 2.5
    assert not np.signbit(finite[finite == 0]).any() and np.isfinite(case.mats).all()
    positive = zero = tied = by_rank = 0
    for gid, keys, bits, pos, n in cp.expect(k, n_groups, 256):
        score = bits.view(np.float32)
        positive += int((score > 0).sum()); zero += int((score == 0).sum())
        pk, ps, pw, pr = cp.group_pairs(case, gid)
        at = np.searchsorted(keys, pk)
        win = ps.astype(np.float32).view(np.uint32) == bits[at]               # pairs that reach their key's kept score
        tied += int((np.bincount(at[win], minlength=len(keys)) >= 2).sum())
        # a winner (rank r, start s) beside a pair of equal bits with a larger rank and a SMALLER start
        best_seq = np.full(len(keys), np.iinfo(np.int64).max)
        np.minimum.at(best_seq, at[win], (pr * nwin + pw)[win])
        by_rank += int((win & (pr > best_seq[at] // nwin) & (pw < best_seq[at] % nwin)).sum())
        assert np.array_equal(best_seq % nwin, pos)
    assert positive >= 1 and zero >= 1 and tied >= 1 and by_rank >= 1, (positive, zero, tied, by_rank)


def test_a_slice_with_an_empty_first_half():
    """reduce_ranges_pos_kernel's first trip keeps slots below TBL / 2: `one_wave_last` leaves it nothing, `one_wave_first` its second."""
    case = cp.build(13, 1, 256)
    st = _stats(case, "one_wave_last")[0][2]
    assert st["slots"].min() >= 32768 // 2 and st["keys"] > 0
    st = _stats(case, "one_wave_first")[0][2]
    assert st["slots"].max() < 32768 // 2


def _same(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and x[4] == y[4] and all(np.array_equal(p, q) for p, q in zip(x[1:4], y[1:4])) for x, y in zip(a, b))


@pytest.mark.parametrize("k,n_groups", CASES)
def test_expectation_is_the_oracles(k, n_groups):
    case = cp.build(k, n_groups, 256)
    for gid, keys, bits, pos, n in cp.expect(k, n_groups, 256):
        mats = case.mats[case.groups == gid]
        ok, os_, oe = co.explore_group(mats, k, cp.EPS)
        assert np.array_equal(ok, keys) and np.array_equal(os_.view(np.uint32), bits) and oe == n
        pk, ps, pp, pe = co.explore_group_pos(mats, k, cp.EPS)
        assert np.array_equal(pk, keys) and np.array_equal(ps.view(np.uint32), bits) and np.array_equal(pp, pos) and pe == n


@pytest.mark.skipif(not rb.available(), reason="the reference binaries are not in oracle/_ref/")
@pytest.mark.parametrize("k,n_groups", [(11, 3), (12, 3)])
def test_expectation_is_the_live_references(k, n_groups):
    case = cp.build(k, n_groups, 256)
    for gid, keys, bits, pos, n in cp.expect(k, n_groups, 256):
        want = rb.ref_explore_group(case.mats[case.groups == gid], k, cp.EPS, 4, positions=True)
        assert np.array_equal(want[0], keys) and np.array_equal(want[1].view(np.uint32), bits)
        assert np.array_equal(want[2], pos) and want[3] == n


@pytest.mark.parametrize("k,n_groups", [(11, 3), (12, 1), (12, 3)])
def test_wrong_back_halves_change_the_expectation(k, n_groups):
    """Last writer wins instead of the maximum; the latest window instead of the earliest among equal bits; block bits one block off."""
    right = cp.expect(k, n_groups, 256)
    last_writer = cp.expect(k, n_groups, 256, rule="last_writer")
    assert any(not np.array_equal(a[2], b[2]) for a, b in zip(right, last_writer))               # score bits
    latest = cp.expect(k, n_groups, 256, rule="max_last")
    assert all(np.array_equal(a[2], b[2]) for a, b in zip(right, latest))
    assert any(not np.array_equal(a[3], b[3]) for a, b in zip(right, latest))                    # positions only
    shifted = cp.shift_blocks(right)
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(right, shifted))                   # key sets
    assert _same(right, cp.expect(k, n_groups, 256))


# ---- the 64-KB families: DNA k = 8, 10 (variant 6) and amino acids k = 6 -----------------------------------------------------------------

OTHERS = {"dna_k8": lambda: cp.small_dna(8), "dna_k10": lambda: cp.small_dna(10), "aa_k6": cp.aa_k6, "nine": lambda: cp.nine_groups(11),
          "block": lambda: cp.full_block(11), "dna_k14": cp.k14, "big_box_k12": lambda: cp.big_box(12), "big_box_k13": lambda: cp.big_box(13)}


@pytest.mark.parametrize("name", sorted(OTHERS))
def test_expectation_of_the_other_cases_is_the_oracles(name):
    from oracle import db_oracle as dbo
    case = OTHERS[name]()
    assert len(case.mats) <= 200 and case.mats.shape[1] <= 60
    for gid, keys, bits, pos, n in cp.case_expect(case):
        pk, ps, pp, pe = co.explore_group_pos(case.mats[case.groups == gid], case.k, cp.EPS)
        assert np.array_equal(dbo.dense_code(pk, case.sigma, case.k).astype(np.int64), keys)
        assert np.array_equal(ps.view(np.uint32), bits) and np.array_equal(pp, pos) and pe == n
        if case.sigma == 20:
            assert np.array_equal(cp.pack_aa(keys), pk)


@pytest.mark.parametrize("k", [8, 10])
def test_small_dna_slices(k):
    """8 wavefronts of 32 blocks over 16 384 slots; no box beyond 64 keys (half lists of at most 64 against the capacity of 160)."""
    case = cp.small_dna(k)
    tbl, waves, nb = cp.geometry(4, k)
    assert (tbl, waves, nb) == (16384, 8, 4 ** k // 16384)
    admitted = (case.mats > cp.NEG).sum(axis=2)
    for m in admitted:
        if (m == 2).all():                                                    # (a dups matrix: 2^(k - k // 2) <= 32 per half)
            continue
        for i in range(cp.ISLANDS):
            assert np.prod(np.maximum(m[i * (k + 1):i * (k + 1) + k], 1)) <= 64
    st = _stats(case, "dense")[0][2]
    assert st["keys"] == st["pairs"] == tbl and st["room"] == st["used"] == tbl // 2
    st = _stats(case, "one_wave_last")[0][2]
    assert st["waves"].tolist() == [0] * 7 + [W]
    st = _stats(case, "alternate")[0][2]
    assert _blocks(st, 4 * cp.BPW, cp.BPW) == [64, 0] * 16 and _blocks(st, 5 * cp.BPW, cp.BPW) == [0, 64] * 16
    assert [s[2]["keys"] for n in (1, 3, 4095) for s in _stats(case, f"odd_{n}")] == [1, 3, 4095]
    for g, b, st in _stats(case, "dups"):
        assert st["pairs"] == st["keys"] * (case.mats.shape[1] - k + 1) * cp.dups_m(k) and st["keys"] in (128, 256)


def test_amino_acid_slices():
    """16 000 slots: 250 real blocks; keys in blocks 248 and 249 and nothing in the padding; the corners; a tie decided by rank."""
    case = cp.aa_k6()
    assert cp.geometry(20, 6) == (16000, 8, 4000)
    st = cp.slice_stats(case, 0, 0)
    assert st["slots"].tolist() == [0, 31, 32, 63, 64, 15999] and st["pairs"] == 7
    st = cp.slice_stats(case, 0, 1)
    assert st["slots"].tolist() == list(range(15880, 16000)) and _blocks(st, 247, 9) == [0, 56, 64] + [0] * 6
    st = cp.slice_stats(case, 0, 2)
    assert _blocks(st, 0, 3) == [64, 16, 0] and st["keys"] == 80
    st = cp.slice_stats(case, 0, 3999)
    assert st["slots"].tolist() == [0, 15999]
    assert [cp.slice_stats(case, 1, b)["keys"] for b in (0, 10, 200, 210)] == [16] * 4
    (gid, keys, bits, pos, n), _ = cp.case_expect(case)
    assert pos[keys == 63].tolist() == [7]                  # (rank 1, start 7) against (rank 2, start 0) on equal bits
    pk, ps, pw, pr = cp.group_pairs(case, gid)
    assert sorted(zip(pr[pk == 63].tolist(), pw[pk == 63].tolist())) == [(1, 7), (2, 0)] and len(set(ps[pk == 63].tolist())) == 1


@pytest.mark.parametrize("k", [12, 13])
def test_big_box_is_one_window_on_the_long_list_path(k):
    """One window fills slice 5: 32 768 keys from 32 768 pairs, the value room used to its last unit, at least 128 chunks; its right
    half admits 4096 (k = 12) or 16 384 (k = 13) suffixes, beyond every fast capacity (tests/grid_paths.py `family`: 384, 6144)."""
    case = cp.big_box(k)
    st = cp.slice_stats(case, 0, 5)
    assert st["keys"] == st["pairs"] == 32768 and st["blocks"].tolist() == [64] * 512
    assert st["room"] == st["used"] == 16384 and st["chunks_floor"] == 128
    m = case.mats[-1]
    admitted = (m > cp.NEG).sum(axis=1)
    assert (admitted[k:] == 0).all() and int(np.prod(admitted[:k])) == 32768              # one window, one box
    assert int(np.prod(admitted[k // 2:k])) == (4096 if k == 12 else 16384) > 6144 * (k == 13) + 384 * (k == 12)
    assert [cp.slice_stats(case, 0, b)["keys"] for b in (4, 6)] == [6, 6]                  # `corners` before and after it


@pytest.mark.parametrize("name", ["dna_k8", "dna_k10", "aa_k6"])
def test_other_families_score_positive_zero_and_tied(name):
    case = OTHERS[name]()
    positive = zero = tied = 0
    for gid, keys, bits, pos, n in cp.case_expect(case):
        score = bits.view(np.float32)
        positive += int((score > 0).sum()); zero += int((score == 0).sum())
        pk, ps, pw, pr = cp.group_pairs(case, gid)
        at = np.searchsorted(keys, pk)
        win = ps.astype(np.float32).view(np.uint32) == bits[at]
        tied += int((np.bincount(at[win], minlength=len(keys)) >= 2).sum())
    assert positive >= 1 and zero >= 1 and tied >= 1, (positive, zero, tied)


def test_chunk_floor_of_the_64_kb_families():
    """512 pairs a chunk at 16 384 slots (kernels_score.hpp:494), 256 elsewhere."""
    assert [cp.chunk_pairs(t) for t in (16384, 16000, 32768)] == [512, 256, 256]
    case = cp.small_dna(10)
    g, b, st = _stats(case, "dense")[0]
    assert st["chunks_floor"] == 16384 // 512
