"""GPU suite: the key-range load (Engine.load_db(path, key_range=)) against tests/stream_cases.restrict, and Engine.diff_files
(ipkgpu_db_diff_files) against Engine.diff_dbs of the two loads and against tests/test_gpu_db_diff.restate -- under budgets that give one
range, a few, and as many as the least feasible budget gives; the ranges reported against the plan restated in tests/diff_files_cases.py."""
import copy

import numpy as np
import pytest

import ipk_amd
from ipk_amd import dbfile
from tests import db_files as F
from tests import diff_files_cases as D
from tests import stream_cases as T
from tests.test_gpu_db_diff import PERTURB, as_lists, restate, same_records
from tests.test_gpu_db_load import scores_a_small_call
from tests.test_gpu_db_select import check

pytestmark = pytest.mark.gpu

KINDS = [False, True]                                # plain, positioned
TOP = 1 << 32


def with_window(engine, cap, chunk, call):
    engine.set_option("db_load_window_bytes", cap)
    engine.set_option("db_load_chunk_bytes", chunk)
    try:
        return call()
    finally:
        engine.set_option("db_load_window_bytes", 0)
        engine.set_option("db_load_chunk_bytes", 0)


def under(engine, avail, call):
    """call() with `avail` bytes of device memory on top of what the engine holds (None: no budget) -> (result, held, peak)."""
    engine.set_option("release_workspaces", 1)
    held = engine.mem_stats()[0]
    old = engine.get_option("device_budget_bytes")
    if avail is not None:
        engine.set_option("device_budget_bytes", held + avail)
    engine.mem_stats(reset_peak=True)
    try:
        return call(), held, engine.mem_stats()[1]
    finally:
        engine.set_option("device_budget_bytes", old)


def same_bits(got, want):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


# ---- the key-range load -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("positioned", KINDS)
def test_key_range_load_against_the_restriction(engine, tmp_path, positioned):
    db = T.stream_db()
    path = F.write(tmp_path / "stream.ipk", db, positioned)
    head = dict(dbfile.file_info(path))
    keys = [int(k) for k in db["keys"]]
    first, last, mid, later = keys[0], keys[-1], keys[70], keys[130]
    assert last == T.OUTSIDE
    ranges = [(0, TOP), (5, 5), (mid, mid + 1), (0, first), (0, first + 1), (last, TOP), (keys[-2], TOP), (mid, later), (mid + 1, later + 1),
              (T.OUTSIDE, T.OUTSIDE + 1), (0, T.OUTSIDE), (T.OUTSIDE + 1, TOP), (TOP, TOP)]
    window = T.window_cap(positioned, "several")
    assert max(T.record_sizes(db, positioned)) > window                      # one record is longer than the window
    for lo, hi in ranges:
        want = T.restrict(db, {k for k in keys if lo <= k < hi}, positioned)
        v = with_window(engine, window, T.CHUNK, lambda: engine.load_db(path, key_range=(lo, hi)))
        try:
            check(v, want, positioned, head)
            times = engine.load_times()
            assert times["windows"] == len(T.windows_of(T.record_sizes(db, positioned), window)) and times["records_kept"] == len(want["keys"])
        finally:
            v.free()
    assert len(T.restrict(db, {k for k in keys if mid <= k < later}, positioned)["keys"]) == 60
    v = engine.load_db(path, key_range=(mid, later))                         # the default window: one
    try:
        check(v, T.restrict(db, {k for k in keys if mid <= k < later}, positioned), positioned, head)
    finally:
        v.free()
    for bad in ((6, 5), (0, TOP + 1)):
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            engine.load_db(path, key_range=bad)
        assert ei.value.code == 1
    with pytest.raises(ValueError):
        engine.load_db(path, key_range=(0, 5), mu=0.5)


def test_key_range_load_keeps_records_without_entries(engine, tmp_path):
    db = F.synthetic(keys=[3, 8, 9, 20, 21], counts=[2, 0, 3, 0, 1], seed=4)
    path = F.write(tmp_path / "entryless.ipk", db)
    v = engine.load_db(path, key_range=(8, 21))
    try:
        check(v, T.restrict(db, {8, 9, 20}, False), False, dict(dbfile.file_info(path)))
        assert v.keys().tolist() == [8, 9, 20] and v.key_offsets().tolist() == [0, 0, 3, 3]
    finally:
        v.free()


# ---- diff_files on the base pair -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def base(engine, tmp_path_factory):
    d = tmp_path_factory.mktemp("diff_files")
    lists = D.base()["lists"]
    arrays = D.Side(lists, True, D.WINDOW).db
    paths = {pos: F.write(d / f"a{int(pos)}.ipk", arrays, pos, D.HEADER5) for pos in KINDS}
    loaded = {pos: engine.load_db(paths[pos]) for pos in KINDS}
    yield dict(lists=lists, paths=paths, db=loaded, dir=d)
    for x in loaded.values():
        x.free()


def one_way(engine, path_a, path_b, side_a, side_b, db_a, db_b, eps, budgets, max_records=(None,), headers=(D.HEADER5, D.HEADER5), window=D.WINDOW):
    """diff_files(a, b) under each budget factor (None: no budget; else times the least) against diff_dbs and the restatement."""
    positions = side_a.pos and side_b.pos
    want_c, want_r = restate(side_a.lists, side_b.lists, eps, positions)
    seen = []
    for m in max_records:
        m = len(want_r) + 10 if m is None else m
        ref_c, ref_r = engine.diff_dbs(db_a, db_b, eps=eps, max_records=m)
        assert ref_c == want_c
        least = D.least_budget(side_a, side_b, m, *headers)
        for factor in budgets:
            avail = None if factor is None else int(least * factor)
            (got_c, got_r, info), _, _ = under(engine, avail, lambda: with_window(engine, window, 0, lambda: engine.diff_files(path_a, path_b, eps=eps, max_records=m)))
            assert got_c == want_c == ref_c, (factor, m)
            assert np.float32(got_c["max_abs_diff"]).view(np.uint32) == np.float32(ref_c["max_abs_diff"]).view(np.uint32)
            same_records(got_r, want_r[:m])
            same_bits(got_r, ref_r)
            plan = D.plan(side_a, side_b, 1 << 50 if avail is None else avail, m, *headers)
            assert info["ranges"] == [(lo, hi) for lo, hi, *_ in plan], (factor, m)
            passes = 1 + len(plan) if avail is not None and D.needs_histogram(side_a, side_b, avail, m) else 1
            assert passes > 1 or len(plan) == 1
            assert (info["passes_a"], info["passes_b"]) == (passes, passes)
            assert info["body_bytes_read"] == passes * (side_a.body + side_b.body)
            if avail is not None:
                assert info["avail_bytes"] == avail and info["window_bytes"] == window
            seen.append(len(plan))
    return want_c, want_r, seen


BUDGETS = (None, 2, 1.5, 1)                              # no budget; twice, one and a half times and once the least feasible


@pytest.mark.parametrize("name", list(PERTURB) + ["all"])
def test_perturbed_copies_under_every_budget(engine, base, name):
    names = list(PERTURB) if name == "all" else [name]
    B = D.perturbed_base(names)
    a, b = D.Side(base["lists"], True, D.WINDOW), D.Side(B, True, D.WINDOW)
    path_b = F.write(base["dir"] / f"{name}.ipk", b.db, True, D.HEADER5)
    db_b = engine.load_db(path_b)
    try:
        for eps in (1e-2, 0.0):
            c, _, seen = one_way(engine, base["paths"][True], path_b, a, b, base["db"][True], db_b, eps, BUDGETS)
            assert seen[0] == 1 and seen[-1] >= 4 and 2 <= seen[2] < seen[-1]
            one_way(engine, path_b, base["paths"][True], b, a, db_b, base["db"][True], eps, BUDGETS)
        if name == "scores_moved":                                         # differences in two ranges: the larger one is reported, not their sum
            assert 0.49 < c["max_abs_diff"] < 0.51 and c["scores_differ"] >= 3
        if name == "last_key":                                             # the key beyond the code space, in A alone, is compared: the last range ends at 2^32
            assert c["keys_only_a"] == 1 and D.OUTSIDE5 not in B
    finally:
        db_b.free()


def test_the_record_list_is_cut_overall_not_per_range(engine, base):
    B = D.perturbed_base(list(PERTURB))
    a, b = D.Side(base["lists"], True, D.WINDOW), D.Side(B, True, D.WINDOW)
    path_b = F.write(base["dir"] / "cuts.ipk", b.db, True, D.HEADER5)
    db_b = engine.load_db(path_b)
    try:
        want_r = restate(base["lists"], B, 1e-2, True)[1]
        ranges = D.plan(a, b, D.least_budget(a, b, 0), 0)
        per_range = [len(restate(D.in_range(base["lists"], lo, hi), D.in_range(B, lo, hi), 1e-2, True)[1]) for lo, hi, *_ in ranges]
        # (five records cut per range would be more than five in all)
        assert sum(per_range) == len(want_r) and sum(1 for n in per_range if n) >= 3 and sum(min(n, 5) for n in per_range) > 5
        at_boundary = per_range[0]                                         # exactly the first range's records
        inside = per_range[0] + max(1, per_range[1] // 2)                  # a cut inside the second range
        assert 0 < at_boundary < inside < len(want_r)
        _, _, seen = one_way(engine, base["paths"][True], path_b, a, b, base["db"][True], db_b, 1e-2, (1.5, 1), max_records=(0, 5, at_boundary, inside, None))
        assert min(seen) >= 2
    finally:
        db_b.free()


# ---- shifts above 0 ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dna_k9", "aa_k4", "dna_k16"])
def test_bins_of_several_keys(engine, tmp_path, name):
    header, A, B = D.shifted_pairs()[name]
    window = 256
    a, b = D.Side(A, True, window), D.Side(B, True, window)
    paths = [F.write(tmp_path / f"{x}.ipk", s.db, True, header) for x, s in (("a", a), ("b", b))]
    dbs = [engine.load_db(p) for p in paths]
    try:
        for eps in (1e-2, 0.0):
            _, _, seen = one_way(engine, paths[0], paths[1], a, b, dbs[0], dbs[1], eps, (None, 1.25, 1), headers=(header, header), window=window)
            assert seen[0] == 1 and seen[-1] >= 2                              # (the fixed part is most of so small a pair's need: only the least splits)
            one_way(engine, paths[1], paths[0], b, a, dbs[1], dbs[0], eps, (1,), headers=(header, header), window=window)
    finally:
        for x in dbs:
            x.free()


def test_the_larger_of_two_heads_bit_counts_sets_the_shift(engine, tmp_path):
    header9, A, B = D.shifted_pairs()["dna_k9"]
    small = {k: v for k, v in B.items() if k < 4 ** 5}
    a, b = D.Side(A, True, 256), D.Side(small, False, 256)
    pa, pb = F.write(tmp_path / "a.ipk", a.db, True, header9), F.write(tmp_path / "b.ipk", b.db, False, D.HEADER5)
    da, db_ = engine.load_db(pa), engine.load_db(pb)
    try:
        assert D.shift_of(header9, D.HEADER5) == 2
        one_way(engine, pa, pb, a, b, da, db_, 1e-2, (None, 1), headers=(header9, D.HEADER5), window=256)
        one_way(engine, pb, pa, b, a, db_, da, 1e-2, (1,), headers=(D.HEADER5, header9), window=256)
    finally:
        da.free(); db_.free()


# ---- more than 256 records in one window; the budget -------------------------------------------------------------------------------------------------

def budget_for(a, b, n_ranges, header, max_records=0):
    """An avail under which the restated plan has n_ranges ranges."""
    whole = D.plan(a, b, 1 << 50, max_records, header, header)
    assert len(whole) == 1
    hi = D.range_bytes(max(D.window_bytes(s.window, s.n_w_bound, s.longest_bound) for s in (a, b)), a.n, a.e, a.pos, b.n, b.e, b.pos, max_records)
    for f in range(95, 5, -5):
        try:
            if len(D.plan(a, b, hi * f // 100, max_records, header, header)) == n_ranges:
                return hi * f // 100
        except D.NoRoom:
            break
    raise AssertionError("no such budget")


def changed(A, every):
    B = copy.deepcopy(A)
    for i, k in enumerate(sorted(B)):
        if i % every == 0:
            B[k][0][1] = np.float32(B[k][0][1] - 1)
        elif i % every == 1:
            del B[k]
    return B


def test_the_histogram_kernels_second_workgroup(engine, tmp_path):
    header = dict(F.HEADER, kmer_size=8)
    A = D.many_records(1500, 31, k=8, per_key=1)
    B = changed(A, 97)
    window = 16 << 10
    a, b = D.Side(A, False, window, D.fast_arrays), D.Side(B, True, window, D.fast_arrays)
    assert a.n_w > 2 * 256 and len(T.windows_of(a.sizes, a.window)) >= 3
    pa, pb = F.write(tmp_path / "a.ipk", a.db, False, header), F.write(tmp_path / "b.ipk", b.db, True, header)
    avail = budget_for(a, b, 2, header, 1 << 20)
    (c, rec, info), _, _ = under(engine, avail, lambda: with_window(engine, window, 0, lambda: engine.diff_files(pa, pb, eps=0.0, max_records=1 << 20)))
    want_c, want_r = restate(A, B, 0.0, False)
    assert c == want_c
    same_records(rec, want_r)
    assert info["ranges"] == [(lo, hi) for lo, hi, *_ in D.plan(a, b, avail, 1 << 20, header, header)] and len(info["ranges"]) == 2
    assert info["max_window_records"] == max(a.n_w, b.n_w) and info["longest_record_bytes"] == max(a.longest, b.longest)


def test_a_pair_larger_than_the_budget_is_compared(engine, tmp_path):
    """DNA k = 9 (two key bits below the bins), 30000 records of three entries: bodies of 1.2 MB (plain) and 1.4 MB (positioned).
    X = a third of what the whole pair needs by the header's formula; the window by the default rule, X / 16."""
    header = dict(F.HEADER, kmer_size=9)
    A = D.many_records(30000, 51, k=9)
    B = changed(A, 1000)
    whole = D.range_bytes(0, len(A), 3 * len(A), False, len(B), 3 * len(B), True, 0)
    X = whole // 3
    window = D.default_window(X)
    a, b = D.Side(A, False, window, D.fast_arrays), D.Side(B, True, window, D.fast_arrays)
    pa, pb = F.write(tmp_path / "a.ipk", a.db, False, header), F.write(tmp_path / "b.ipk", b.db, True, header)
    MR = 1 << 20
    plan = D.plan(a, b, X, MR, header, header)
    assert len(plan) >= 3 and a.body > X // 2
    # the formula's figure for the whole call: the worst range, and the histogram pass
    bound = max([D.range_bytes(max(D.window_bytes(s.window, s.n_w, s.longest) for s in (a, b)), na, ea, False, nb, eb, True, MR) for _, _, na, ea, nb, eb in plan]
                + [D.hist_pass_bytes(s.window, s.n_w, s.longest) for s in (a, b)])
    assert bound <= X
    ref_a, ref_b = engine.load_db(pa), engine.load_db(pb)
    try:
        ref_c, ref_r = engine.diff_dbs(ref_a, ref_b, eps=1e-2, max_records=MR)
    finally:
        ref_a.free(); ref_b.free()
    assert ref_c["scores_differ"] == 30 and ref_c["keys_only_a"] == 30

    def both():
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            engine.load_db(pa)
        assert ei.value.code == 3
        return engine.diff_files(pa, pb, eps=1e-2, max_records=MR)
    (c, rec, info), held, peak = under(engine, X, both)
    assert peak <= held + X
    assert c == ref_c
    same_bits(rec, ref_r)
    assert info["ranges"] == [(lo, hi) for lo, hi, *_ in plan] and info["window_bytes"] == window and info["passes_a"] == 1 + len(plan)
    engine.set_option("release_workspaces", 1)
    assert engine.mem_stats()[0] == held
    scores_a_small_call(engine)


def test_below_the_least_budget_the_bin_is_named(engine, base):
    B = D.perturbed_base(["scores_moved"])
    a, b = D.Side(base["lists"], True, D.WINDOW), D.Side(B, False, D.WINDOW)
    path_b = F.write(base["dir"] / "least.ipk", b.db, False, D.HEADER5)
    least = D.least_budget(a, b, 0)
    with pytest.raises(D.NoRoom) as want:
        D.plan(a, b, least - 1, 0)
    assert want.value.need == least
    engine.set_option("release_workspaces", 1)
    held = engine.mem_stats()[0]
    with pytest.raises(ipk_amd.IpkGpuError) as ei:
        under(engine, least - 1, lambda: with_window(engine, D.WINDOW, 0, lambda: engine.diff_files(base["paths"][True], path_b)))
    lo, hi = D.bin_interval(want.value.bin, 0)
    assert ei.value.code == 3 and f"bin {want.value.bin}, the keys [{lo}, {hi})" in str(ei.value) and f"need {least} bytes" in str(ei.value)
    engine.set_option("release_workspaces", 1)
    assert engine.mem_stats()[0] == held
    (c, _, info), _, _ = under(engine, least, lambda: with_window(engine, D.WINDOW, 0, lambda: engine.diff_files(base["paths"][True], path_b)))
    assert c["scores_differ"] == 2 and c["positions_differ"] == 0 and len(info["ranges"]) >= 4
    scores_a_small_call(engine)


# ---- refusals and recovery ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("positioned", KINDS)
def test_damaged_files_are_refused_and_the_next_call_succeeds(engine, tmp_path, positioned):
    want = F.synthetic(200, seed=11)
    good, bad = F.damaged(tmp_path, want, positioned)
    lists = as_lists(want)
    window = sum(T.record_sizes(want, positioned)[:4])
    side = D.Side(lists, positioned, window, lambda _: want)
    split = budget_for(side, side, 2, F.HEADER)
    engine.set_option("release_workspaces", 1)
    held = engine.mem_stats()[0]
    for avail in (None, split):
        for name, (path, record) in bad.items():
            for pair in ((path, good), (good, path)):
                with pytest.raises(ipk_amd.IpkGpuError) as ei:
                    under(engine, avail, lambda: with_window(engine, window, T.CHUNK, lambda: engine.diff_files(*pair)))
                assert ei.value.code == 1, name
                if record is not None:
                    assert f"record {record} at byte offset " in str(ei.value), (name, str(ei.value))
        (c, rec, info), _, _ = under(engine, avail, lambda: with_window(engine, window, T.CHUNK, lambda: engine.diff_files(good, good, eps=0.0, max_records=3)))
        assert c["keys_a"] == 200 and c["keys_only_a"] + c["keys_only_b"] + c["scores_differ"] + c["entries_only_a"] + c["entries_only_b"] == 0 and len(rec) == 0
        assert len(info["ranges"]) == (1 if avail is None else 2)
        engine.set_option("release_workspaces", 1)
        assert engine.mem_stats()[0] == held
    scores_a_small_call(engine)


def test_a_duplicate_key_inside_a_range_is_refused(engine, tmp_path):
    dup = F.write(tmp_path / "dup.ipk", F.synthetic(keys=[5, 9, 9, 200], counts=[2, 3, 1, 2], seed=3))
    good = F.write(tmp_path / "good.ipk", F.synthetic(keys=[5, 9, 200], counts=[2, 3, 2], seed=3))
    for pair in ((dup, good), (good, dup)):
        with pytest.raises(ipk_amd.IpkGpuError, match="more than one record") as ei:
            engine.diff_files(*pair)
        assert ei.value.code == 1
    with pytest.raises(ipk_amd.IpkGpuError):
        engine.diff_files(good, good, eps=-1.0)
    c, _, _ = engine.diff_files(good, good)
    assert c["keys_a"] == c["keys_b"] == 3


# ---- edges -----------------------------------------------------------------------------------------------------------------------------------------

def test_positioned_against_plain_nothing_and_itself(engine, base):
    lists = base["lists"]
    n_entries = sum(map(len, lists.values()))
    a = D.Side(lists, True, D.WINDOW)
    plain = D.Side(D.perturbed_base(["positions", "scores_moved"]), False, D.WINDOW)
    path_plain = F.write(base["dir"] / "plain_b.ipk", plain.db, False, D.HEADER5)
    db_plain = engine.load_db(path_plain)
    empty = D.Side({}, True, D.WINDOW)
    path_empty = F.write(base["dir"] / "empty.ipk", empty.db, True, D.HEADER5)
    db_empty = engine.load_db(path_empty)
    try:
        c, _, _ = one_way(engine, base["paths"][True], path_plain, a, plain, base["db"][True], db_plain, 1e-2, (None, 1))
        assert c["positions_differ"] == 0 and c["scores_differ"] == 3        # (scores_moved's two beyond eps, and the outside key's)
        one_way(engine, path_plain, base["paths"][True], plain, a, db_plain, base["db"][True], 1e-2, (1,))
        c, _, _ = one_way(engine, base["paths"][True], path_empty, a, empty, base["db"][True], db_empty, 1e-2, (None, 1), max_records=(0, 5, None))
        assert c["keys_only_a"] == len(lists) and c["entries_only_a"] == n_entries and c["keys_b"] == 0
        one_way(engine, path_empty, base["paths"][True], empty, a, db_empty, base["db"][True], 1e-2, (1,))
        one_way(engine, path_empty, path_empty, empty, empty, db_empty, db_empty, 1e-2, (None,))
        for other, side, db_o in ((base["paths"][True], a, base["db"][True]), (base["paths"][False], D.Side(lists, False, D.WINDOW), base["db"][False])):
            c, r, _ = one_way(engine, base["paths"][True], other, a, side, base["db"][True], db_o, 0.0, (None, 1), max_records=(10,))
            assert c == dict(keys_a=len(lists), keys_b=len(lists), keys_only_a=0, keys_only_b=0, entries_a=n_entries, entries_b=n_entries, entries_only_a=0,
                             entries_only_b=0, scores_differ=0, positions_differ=0, max_abs_diff=0.0) and len(r) == 0
    finally:
        db_plain.free(); db_empty.free()
