"""GPU suite: the k-mer set of a batch of queries (Engine.kmer_set), the restriction of a database to it (Engine.select_db(wanted=)) and
the streamed, restricted load (Engine.load_db(path, wanted=), Engine.place_file) against the numpy restatements of tests/stream_cases.py:
the set's words, every array of the restriction bit for bit, and placements equal to those on the whole database."""
import numpy as np
import pytest

import ipk_amd
from ipk_amd import dbfile
from tests import db_files as F
from tests import place_cases as pc
from tests import place_ext_cases as xc
from tests import place_oracle as po
from tests import select_cases as S
from tests import stream_cases as T
from tests.test_gpu_db_load import same_as_arrays, scores_a_small_call
from tests.test_gpu_db_select import check

pytestmark = pytest.mark.gpu

KINDS = [False, True]                                # plain, positioned
CAPS = ["longest", "several", "default"]


# ---- the set's bits ---------------------------------------------------------------------------------------------------------------------

def set_matches(engine, queries, sigma, k, ambiguity=False, strands="given"):
    codes = T.kmer_codes(queries, sigma, k, ambiguity, strands)
    s = engine.kmer_set(queries, sigma, k, ambiguity=ambiguity, strands=strands)
    try:
        assert (s.sigma, s.k, s.count) == (sigma, k, len(codes))
        got = s.words()
        assert got.dtype == np.uint32 and len(got) == T.n_words(sigma, k)
        assert np.array_equal(got, T.words_of(codes, sigma, k))
        del got
    finally:
        s.free()
    return codes


PLAIN_CASES = {"main_case": pc.main_case, "aa_case": pc.aa_case, "k16_case": pc.k16_case, "k2_case": pc.k2_case,
               "lookup_shift0": lambda: pc.lookup_case(20, 3), "lookup_shift16": lambda: xc.lookup_ext_case(4, 16)}
EXT_CASES = {"main_ext_case": (xc.main_ext_case, "both"), "aa_ext_case": (lambda: xc.aa_ext_case(3), "given"), "strand_case": (xc.strand_case, "both"),
             "alias_case": (xc.alias_case, "both"), "long_ext_case": (xc.long_ext_case, "both")}


@pytest.mark.parametrize("name", sorted(PLAIN_CASES))
def test_set_bits_of_the_placement_cases(engine, name):
    case = PLAIN_CASES[name]()
    if name.startswith("lookup"):
        assert pc.lookup_shift(case.sigma, case.k) == (0 if name == "lookup_shift0" else 16)
    assert set_matches(engine, case.queries, case.sigma, case.k)


@pytest.mark.parametrize("name", sorted(EXT_CASES))
def test_set_bits_with_ambiguity_and_both_strands(engine, name):
    make, strands = EXT_CASES[name]
    case = make()
    if name == "long_ext_case":
        assert max(len(q) for q in case.queries) >= 70000
    plain = set_matches(engine, case.queries, case.sigma, case.k)
    both = set_matches(engine, case.queries, case.sigma, case.k, True, strands)
    assert plain <= both and (plain < both or name in ("strand_case", "alias_case"))
    if strands == "both":
        assert set_matches(engine, case.queries, case.sigma, case.k, False, "both") <= both


def test_set_bits_at_the_tile_edges_and_of_nothing(engine):
    k = 8
    rng = np.random.default_rng(9)
    q = ["".join(rng.choice(list("ACGT"), n)) for n in (k - 1, k, 63 + k, 64 + k)]
    assert len(set_matches(engine, q[:1], 4, k)) == 0
    assert len(set_matches(engine, q[1:2], 4, k)) == 1
    assert len(set_matches(engine, q, 4, k, True, "both")) > 64
    two = ["ACGTNACNACGTACGT"]                                              # the windows over both N hold two ambiguous symbols: nothing
    assert T.kmer_codes(two, 4, k, True) and set_matches(engine, two, 4, k, True)
    assert len(set_matches(engine, ["ACNTNACG"], 4, k, True)) == 0
    assert len(set_matches(engine, [], 4, k)) == 0
    assert len(set_matches(engine, ["", ""], 20, 3, True)) == 0


def test_set_refusals(engine):
    for call in (lambda: engine.kmer_set(["ACGT"], 4, 17), lambda: engine.kmer_set(["ACGT"], 7, 4), lambda: engine.kmer_set(["ACGT"], 20, 7),
                 lambda: engine.kmer_set(["RHKD"], 20, 3, strands="both")):
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            call()
        assert ei.value.code == 1
    import ctypes as C
    off = np.array([0, 4, 2], np.uint64)
    out = C.c_void_p()
    assert engine._lib.ipkgpu_kmer_set_of_queries(engine._h, 4, 4, b"ACGT", off.ctypes.data, 2, None, C.byref(out)) == 1
    scores_a_small_call(engine)


# ---- select_keys(load_db) and load_wanted against the restatement --------------------------------------------------------------------

@pytest.fixture(scope="module")
def streamed(engine, tmp_path_factory):
    """The streamed file, plain and positioned, each loaded whole once, and the k-mer set of each kind's queries."""
    d = tmp_path_factory.mktemp("stream")
    db = T.stream_db()
    paths = {p: F.write(d / f"stream_{int(p)}.ipk", db, p) for p in KINDS}
    whole = {p: engine.load_db(paths[p]) for p in KINDS}
    sets = {p: engine.kmer_set(T.stream_queries(p), 4, T.K4) for p in KINDS}
    yield db, paths, whole, sets
    for x in list(whole.values()) + list(sets.values()):
        x.free()


def with_window(engine, cap, chunk, call):
    engine.set_option("db_load_window_bytes", cap)
    engine.set_option("db_load_chunk_bytes", chunk)
    try:
        return call()
    finally:
        engine.set_option("db_load_window_bytes", 0)
        engine.set_option("db_load_chunk_bytes", 0)


@pytest.mark.parametrize("positioned", KINDS)
@pytest.mark.parametrize("cap", CAPS)
def test_grid_against_the_restatement(engine, streamed, cap, positioned):
    db, paths, whole, sets = streamed
    codes = T.stream_wanted(positioned)
    assert sets[positioned].count == len(codes)
    window = T.window_cap(positioned, cap)
    for t in S.t_grid(db):
        for m in S.M_GRID:
            want = T.expected(db, codes, m, t, positioned)
            a = with_window(engine, window, T.CHUNK, lambda: engine.load_db(paths[positioned], keep_kmers=m, min_log_score=t, wanted=sets[positioned]))
            try:
                check(a, want, positioned, whole[positioned].header)
                times = engine.load_times()
            finally:
                a.free()
            if cap == "several" and m >= 200:
                sizes = T.record_sizes(db, positioned)
                assert times["windows"] == len(T.windows_of(sizes, window)) and times["records_kept"] == len(codes) - 1
                assert times["body_bytes_read"] == sum(sizes)
            if cap == "several":                                            # (the in-memory meaning, once per (M, t))
                b = engine.select_db(whole[positioned], keep_kmers=m, min_log_score=t, wanted=sets[positioned])
                try:
                    check(b, want, positioned, whole[positioned].header)
                finally:
                    b.free()
    same_as_arrays(whole[positioned], db, positioned)                       # the source is untouched


@pytest.mark.parametrize("positioned", KINDS)
def test_restriction_alone_the_empty_set_and_every_key(engine, streamed, positioned):
    db, paths, whole, sets = streamed
    r = engine.select_db(whole[positioned], wanted=sets[positioned])
    try:
        check(r, T.restrict(db, T.stream_wanted(positioned), positioned), positioned, whole[positioned].header)
    finally:
        r.free()
    every = set(range(4 ** T.K4))
    for queries, codes in (([], set()), (T.queries_naming(every, 4, T.K4), every)):
        s = engine.kmer_set(queries, 4, T.K4)
        try:
            assert s.count == len(codes)
            want = T.restrict(db, codes, positioned)
            assert len(want["keys"]) == (199 if codes else 0)               # (every key but 4^k, which is in no set)
            for make in (lambda: engine.select_db(whole[positioned], wanted=s),
                         lambda: with_window(engine, T.window_cap(positioned), T.CHUNK, lambda: engine.load_db(paths[positioned], wanted=s))):
                v = make()
                try:
                    check(v, want, positioned, whole[positioned].header)
                finally:
                    v.free()
        finally:
            s.free()


# ---- placement ------------------------------------------------------------------------------------------------------------------------------

def same_placements(a, b):
    for name in ("branches", "scores", "counts", "n_kmers", "n_found", "n_branches", "strand", "n_ambiguous"):
        x, y = getattr(a, name), getattr(b, name)
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), name
    tol = po.lwr_tolerance(a.n_branches.astype(np.float64))[:, None]
    assert (np.abs(a.lwr - b.lwr) <= tol * b.lwr).all()


PLACE_CASES = {"main_case": (pc.main_case, False, "given"), "main_ext_case": (xc.main_ext_case, True, "both"),
               "big_branch_case": (pc.big_branch_case, False, "given")}


@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_place")
    return {name: F.write(d / f"{name}.ipk", T.case_db_dict(make()), False, T.case_header(make())) for name, (make, _, _) in PLACE_CASES.items()}


@pytest.mark.parametrize("name", sorted(PLACE_CASES))
def test_placement_on_the_restricted_load_equals_placement_on_the_file(engine, case_files, name):
    make, ambiguity, strands = PLACE_CASES[name]
    case, path = make(), case_files[name]
    full = engine.load_db(path)
    try:
        if name == "big_branch_case":
            assert int(full.entries()[0].max()) + 1 > 4096                  # the global-tables path
        want = engine.place(full, case.queries, ambiguity=ambiguity, strands=strands)
        assert (want.n_found > 0).any()
        s = engine.kmer_set(case.queries, case.sigma, case.k, ambiguity=ambiguity, strands=strands)
        try:
            body = dbfile.file_info(path)["file_bytes"] - dbfile.file_info(path)["body_offset"]
            part = with_window(engine, max(body // 7, 16), 0, lambda: engine.load_db(path, wanted=s))
            try:
                assert engine.load_times()["windows"] >= 7 and 0 < part.num_keys <= full.num_keys
                same_placements(engine.place(part, case.queries, ambiguity=ambiguity, strands=strands), want)
            finally:
                part.free()
        finally:
            s.free()
    finally:
        full.free()


@pytest.mark.parametrize("name", ["main_case", "main_ext_case"])
def test_place_file_in_batches(engine, case_files, name):
    make, ambiguity, strands = PLACE_CASES[name]
    case, path = make(), case_files[name]
    queries = case.queries[:7]
    full = engine.load_db(path, mu=0.6, omega=1.75)
    try:
        want = engine.place(full, queries, ambiguity=ambiguity, strands=strands)
    finally:
        full.free()
    for batch in (1, 3, None):
        got = engine.place_file(path, queries, ambiguity=ambiguity, strands=strands, mu=0.6, omega=1.75, query_batch=batch)
        assert got.n == len(queries)
        same_placements(got, want)
    assert engine.place_file(path, []).n == 0


# ---- the budget ---------------------------------------------------------------------------------------------------------------------------

def test_a_file_larger_than_the_budget_loads_restricted(engine, tmp_path):
    """DNA k = 8, 20000 records, a body of about 1 MiB.  X comes from the header's memory formula at the window W = 64 KiB, with n_w from
    the restated cuts and (n_R, e_R) from the restatement; 31 blocks may each be rounded up by 255 bytes, and 64 KiB stand for the scans'
    and the sort's own workspaces, which the formula names and does not size."""
    db = F.synthetic(20000, seed=41, k=8)
    path = F.write(tmp_path / "big.ipk", db, False, dict(F.HEADER, kmer_size=8))
    rng = np.random.default_rng(42)
    short = np.flatnonzero((db["off"][1:] - db["off"][:-1]) <= 8)
    codes = set(db["keys"][rng.choice(short, 500, replace=False)].tolist())
    want = T.restrict(db, codes, False)
    n_r, e_r = len(want["keys"]), int(want["off"][-1])
    sizes = T.record_sizes(db, False)
    W = 64 << 10
    n_w = max(b - a for a, b in T.windows_of(sizes, W))
    X = max(4 * W, (W + 32) + (60 * n_w + 24) + 2 * (24 * n_r + 8 * e_r) + (28 * n_r + 8 + 8 * e_r) + 20 * n_r + 31 * 255 + (64 << 10))
    assert sum(sizes) > X and W <= X // 4 and max(sizes) <= W
    s = engine.kmer_set(T.queries_naming(codes, 4, 8), 4, 8)
    budget = engine.get_option("device_budget_bytes")
    try:
        assert s.count == 500
        engine.set_option("release_workspaces", 1)
        held = engine.mem_stats()[0]
        engine.set_option("device_budget_bytes", held + X)
        engine.mem_stats(reset_peak=True)
        try:
            with pytest.raises(ipk_amd.IpkGpuError) as ei:
                engine.load_db(path)
            assert ei.value.code == 3
            v = with_window(engine, W, 0, lambda: engine.load_db(path, wanted=s))
            assert engine.mem_stats()[1] <= held + X
        finally:
            engine.set_option("device_budget_bytes", budget)
        try:
            check(v, want, False, dict(dbfile.file_info(path)))
            engine.set_option("release_workspaces", 1)
            rounded = lambda b: max((b + 255) & ~255, 256)
            result = rounded(4 * n_r) + rounded(8 * (n_r + 1)) + rounded(8 * e_r) + rounded(8 * n_r) + rounded(4 * n_r) + rounded(4 * n_r)
            assert engine.mem_stats()[0] == held + result
        finally:
            v.free()
    finally:
        s.free()
    scores_a_small_call(engine)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------

def test_sets_of_another_alphabet_k_or_context_are_refused(engine, streamed):
    _, paths, whole, sets = streamed
    other = ipk_amd.Engine(0)
    try:
        wrong = [engine.kmer_set(["ACGTACGT"], 4, 5), engine.kmer_set(["RHKD"], 20, 4), other.kmer_set(["ACGT"], 4, 4)]
        for s in wrong:
            for call in (lambda: engine.load_db(paths[False], wanted=s), lambda: engine.select_db(whole[False], wanted=s)):
                with pytest.raises(ipk_amd.IpkGpuError) as ei:
                    call()
                assert ei.value.code == 1
        for s in wrong:
            s.free()
    finally:
        other.close()
    engine.load_db(paths[False], wanted=sets[False]).free()


@pytest.mark.parametrize("positioned", KINDS)
def test_damage_in_a_later_window_is_refused_and_the_next_load_succeeds(engine, tmp_path, positioned):
    want = F.synthetic(200, seed=11)
    good, bad = F.damaged(tmp_path, want, positioned)
    sizes = T.record_sizes(want, positioned)
    window = sum(sizes[:4])
    every = set(range(4 ** T.K4))
    s = engine.kmer_set(T.queries_naming(every, 4, T.K4), 4, T.K4)
    try:
        held = engine.mem_stats()[0]
        for name, (path, record) in bad.items():
            if record is not None:
                assert record >= 8                                          # the damage lies behind the first window
            with pytest.raises(ipk_amd.IpkGpuError) as ei:
                with_window(engine, window, T.CHUNK, lambda: engine.load_db(path, wanted=s))
            assert ei.value.code == 1, name
            if record is not None:
                assert f"record {record} at byte offset " in str(ei.value), (name, str(ei.value))
        v = with_window(engine, window, T.CHUNK, lambda: engine.load_db(good, wanted=s))
        try:
            check(v, T.restrict(want, every, positioned), positioned, dict(dbfile.file_info(good)))
        finally:
            v.free()
        engine.set_option("release_workspaces", 1)
        assert engine.mem_stats()[0] <= held
    finally:
        s.free()
    scores_a_small_call(engine)


def test_a_duplicate_key_among_the_kept_records_is_refused(engine, tmp_path):
    db = F.synthetic(keys=[5, 9, 9, 200], counts=[2, 3, 1, 2], seed=3)
    path = F.write(tmp_path / "dup.ipk", db)
    named, unnamed = engine.kmer_set(T.queries_naming({5, 9}, 4, T.K4), 4, T.K4), engine.kmer_set(T.queries_naming({5, 200}, 4, T.K4), 4, T.K4)
    try:
        with pytest.raises(ipk_amd.IpkGpuError, match="more than one record") as ei:
            engine.load_db(path, wanted=named)
        assert ei.value.code == 1
        v = engine.load_db(path, wanted=unnamed)                             # the check sees only the kept records
        try:
            assert v.keys().tolist() == [5, 200]
        finally:
            v.free()
    finally:
        named.free(); unnamed.free()
