"""GPU suite: Engine.select_db (ipkgpu_db_select) and Engine.load_db(path, ...) (ipkgpu_db_load_select) against the numpy restatement
of the definition (tests/select_cases.py): every array of the selection, bit for bit -- keys, offsets, entries, positions, filter
values in float and double, and the order."""
import numpy as np
import pytest

import ipk_amd
from ipk_amd import dbfile
from ipk_amd import distributed as D
from oracle import ipk_oracle as co
from tests import db_files as F
from tests import place_oracle as po
from tests import select_cases as S
from tests.test_gpu_db_load import same_as_arrays, scores_a_small_call

pytestmark = pytest.mark.gpu

T_NAMES = ["neg_inf", "below_all", "mid", "exact_bits", "pos_inf"]
KINDS = [False, True]                                # plain, positioned


@pytest.fixture(scope="module")
def edges(engine, tmp_path_factory):
    """The edge case: its arrays, its plain and positioned files, and both loaded once."""
    d = tmp_path_factory.mktemp("select")
    want = S.edges()
    paths = {p: F.write(d / f"edges_{int(p)}.ipk", want, p) for p in KINDS}
    dbs = {p: engine.load_db(paths[p]) for p in KINDS}
    yield want, paths, dbs
    for db in dbs.values():
        db.free()


def check(v, want, positioned, src_header=None):
    same_as_arrays(v, want, positioned)
    if src_header is not None:
        assert v.header == dict(src_header, total_num_kmers=len(want["keys"]), total_num_entries=int(want["off"][-1]),
                                file_bytes=src_header["body_offset"] + 16 * len(want["keys"]) + (10 if positioned else 8) * int(want["off"][-1]))
    else:
        assert v.header is None


@pytest.mark.parametrize("positioned", KINDS)
@pytest.mark.parametrize("ti", range(5), ids=T_NAMES)
def test_grid_against_the_restatement(engine, edges, ti, positioned):
    want, _, dbs = edges
    t = S.t_grid(want)[ti]
    for m in S.M_GRID:
        v = engine.select_db(dbs[positioned], keep_kmers=m, min_log_score=t)
        try:
            check(v, S.restate(want, m, t), positioned, dbs[positioned].header)
        finally:
            v.free()
    assert engine.select_time_ms() >= 0.0
    same_as_arrays(dbs[positioned], want, positioned)                       # the source is untouched


@pytest.mark.parametrize("positioned", KINDS)
@pytest.mark.parametrize("ti", range(5), ids=T_NAMES)
def test_load_select_is_select_of_load(engine, edges, ti, positioned):
    want, paths, dbs = edges
    t = S.t_grid(want)[ti]
    for m in S.M_GRID:
        a = engine.load_db(paths[positioned], keep_kmers=m, min_log_score=t)
        b = engine.select_db(dbs[positioned], keep_kmers=m, min_log_score=t)
        try:
            r = S.restate(want, m, t)
            check(a, r, positioned, dbs[positioned].header)
            check(b, r, positioned, dbs[positioned].header)
        finally:
            a.free(); b.free()


def test_identity(engine, edges):
    want, _, dbs = edges
    for positioned in KINDS:
        v = engine.select_db(dbs[positioned], keep_kmers=200, min_log_score=-np.inf)
        try:
            same_as_arrays(v, want, positioned)
            assert v.header == dbs[positioned].header
        finally:
            v.free()


def test_one_long_key_among_many_short_ones(engine, tmp_path):
    want, t = S.heavy()
    db = engine.load_db(F.write(tmp_path / "heavy.ipk", want, True, S.HEAVY_HEADER))
    try:
        for m in (3001, 1500):
            v = engine.select_db(db, keep_kmers=m, min_log_score=t)
            try:
                check(v, S.restate(want, m, t), True, db.header)
            finally:
                v.free()
    finally:
        db.free()


@pytest.mark.parametrize("case", ["single", "equal_fv"])
def test_one_key_and_equal_filter_values(engine, tmp_path, case):
    want = getattr(S, case)()
    n = len(want["keys"])
    db = engine.load_db(F.write(tmp_path / "c.ipk", want))
    try:
        for m in (0, 1, n // 2, n):
            for t in (S.NEG_INF, S.T_MID, S.POS_INF):
                v = engine.select_db(db, keep_kmers=m, min_log_score=t)
                try:
                    check(v, S.restate(want, m, t, positioned=False), False, db.header)
                finally:
                    v.free()
    finally:
        db.free()


def test_pairs_of_arguments(engine, edges):
    """mu and omega in place of keep_kmers and min_log_score: mu_kmers of the key count, log_threshold of the head's sigma and k."""
    want, paths, dbs = edges
    t = ipk_amd.log_threshold(2.5, 4, F.HEADER["kmer_size"])
    for make in (lambda: engine.select_db(dbs[False], mu=0.3, omega=2.5), lambda: engine.load_db(paths[False], mu=0.3, omega=2.5)):
        v = make()
        try:
            assert ipk_amd.engine.mu_kmers(0.3, 200) == 60
            check(v, S.restate(want, 60, t), False, dbs[False].header)
            assert v.omega == 2.5 and v.header["omega"] == 1.5              # the head's omega is not touched
        finally:
            v.free()
    with pytest.raises(ValueError):
        engine.select_db(dbs[False], mu=0.3, keep_kmers=5)
    with pytest.raises(ValueError):
        engine.select_db(dbs[False], omega=1.25)                            # below the file's omega
    with pytest.raises(ValueError):
        engine.load_db(paths[False], mu=1.5)


def test_refusals(engine, edges):
    _, paths, dbs = edges
    for call in (lambda: engine.select_db(dbs[False], keep_kmers=5, min_log_score=float("nan")),
                 lambda: engine.load_db(paths[False], keep_kmers=5, min_log_score=float("nan"))):
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            call()
        assert ei.value.code == 1
    built, parts = D.build_db_shard(engine, S.build_mats(), np.asarray(S.BUILD_GROUPS, np.uint32), S.BUILD_K,
                                    co.log_threshold(1.5, 4, S.BUILD_K), 4)
    try:
        with pytest.raises(ipk_amd.IpkGpuError, match="filter") as ei:
            engine.select_db(built, keep_kmers=5, min_log_score=-np.inf)
        assert ei.value.code == 1
    finally:
        built.free(); parts.free()
    import ctypes as C
    L, out = engine._lib, C.c_void_p()
    assert L.ipkgpu_db_select(engine._h, None, 5, C.c_float(0.0), C.byref(out)) == 1
    assert L.ipkgpu_db_select(engine._h, dbs[False]._h, 5, C.c_float(0.0), None) == 1
    assert L.ipkgpu_db_select(None, dbs[False]._h, 5, C.c_float(0.0), C.byref(out)) == 1
    assert L.ipkgpu_db_load_select(engine._h, None, 5, C.c_float(0.0), C.byref(out)) == 1
    assert L.ipkgpu_db_load_select(engine._h, str(paths[False]).encode(), 5, C.c_float(0.0), None) == 1
    scores_a_small_call(engine)


def test_device_budget_is_obeyed(engine, edges):
    want, _, dbs = edges
    engine.set_option("release_workspaces", 1)
    held = engine.mem_stats()[0]
    budget = engine.get_option("device_budget_bytes")
    engine.set_option("device_budget_bytes", held + 4096)                   # the keep flags alone take 4 bytes per entry (3.9 k entries)
    try:
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            engine.select_db(dbs[False], keep_kmers=100, min_log_score=S.T_MID)
        assert ei.value.code == 3
        assert engine.mem_stats()[0] <= held + 4096
    finally:
        engine.set_option("device_budget_bytes", budget)
    v = engine.select_db(dbs[False], keep_kmers=100, min_log_score=S.T_MID)
    try:
        check(v, S.restate(want, 100, S.T_MID), False, dbs[False].header)
    finally:
        v.free()
    scores_a_small_call(engine)


@pytest.mark.parametrize("positioned", KINDS)
def test_only_the_prefix_is_read(engine, edges, positioned):
    """The smallest chunk the option takes (one byte) and M = n / 10: the bytes read are at most the prefix plus a chunk."""
    want, paths, dbs = edges
    starts, body = F.record_starts(want, positioned)
    m = 20
    prefix = int(starts[m])
    engine.set_option("db_load_chunk_bytes", 1)
    try:
        v = engine.load_db(paths[positioned], keep_kmers=m)
        read = engine.load_times()["body_bytes_read"]
    finally:
        engine.set_option("db_load_chunk_bytes", 0)
    try:
        check(v, S.restate(want, m, -np.inf), positioned, dbs[positioned].header)
    finally:
        v.free()
    assert prefix <= read <= prefix + 1 and read < body
    engine.load_db(paths[positioned]).free()
    assert engine.load_times()["body_bytes_read"] == body


@pytest.mark.parametrize("positioned", KINDS)
def test_damage_behind_the_prefix_is_not_seen_and_inside_it_is(engine, tmp_path, positioned):
    want = F.synthetic(200, seed=11)
    _, bad = F.damaged(tmp_path, want, positioned)
    path, r = bad["truncated"]
    for m in (0, 1, r):
        v = engine.load_db(path, keep_kmers=m)
        try:
            check(v, S.restate(want, m, -np.inf), positioned, None if v.header is None else dict(dbfile.file_info(path)))
        finally:
            v.free()
    for m in (r + 1, 200):
        with pytest.raises(ipk_amd.IpkGpuError, match=f"record {r} at byte offset ") as ei:
            engine.load_db(path, keep_kmers=m)
        assert ei.value.code == 1
    path, r = bad["count_2_40"]
    engine.load_db(path, keep_kmers=r).free()
    for m in (r + 1, 199, 200, 1 << 40):
        with pytest.raises(ipk_amd.IpkGpuError, match=f"record {r} at byte offset ") as ei:
            engine.load_db(path, keep_kmers=m)
        assert ei.value.code == 1
    scores_a_small_call(engine)


@pytest.mark.parametrize("positioned", KINDS)
def test_round_trip_through_the_writer(engine, edges, tmp_path, positioned):
    want, _, dbs = edges
    for name, (m, t) in {"some": (150, S.T_MID), "empty": (150, S.POS_INF)}.items():
        v = engine.select_db(dbs[positioned], keep_kmers=m, min_log_score=t)
        try:
            r = S.restate(want, m, t)
            path = tmp_path / f"{name}.ipk"
            dbfile.write_db_device(engine, v, path, **dbfile.header_args(v.header))
            assert dbfile.check_file(path) == (len(r["keys"]), int(r["off"][-1]))
            back = engine.load_db(path)
            try:
                check(back, r, positioned, v.header)
                assert path.stat().st_size == v.header["file_bytes"]
            finally:
                back.free()
        finally:
            v.free()


def test_placement_on_a_selection(engine, edges):
    want, _, dbs = edges
    k = F.HEADER["kmer_size"]
    queries = S.queries_of(want, k)
    t = ipk_amd.log_threshold(2.5, 4, k)
    v = engine.select_db(dbs[False], mu=0.5, omega=2.5)
    try:
        r = S.restate(want, 100, t)
        assert 0 < len(r["keys"]) < 100
        res = engine.place(v, queries)                                      # the selection's omega gives the threshold
        po.check(res, po.place(po.DbView(r["keys"], r["off"], r["br"], r["sc"]), queries, 4, k, t, 7))
        assert (res.n_found > 0).any()
    finally:
        v.free()
    e = engine.select_db(dbs[False], keep_kmers=0)
    try:
        assert e.num_keys == 0 and e.num_entries == 0 and e.key_offsets().tolist() == [0]
        res = engine.place(e, queries)
        assert (res.branches == ipk_amd.engine.PLACE_NONE).all() and (res.n_found == 0).all() and (res.n_branches == 0).all()
        c, _ = engine.diff_dbs(e, e, eps=0.0)
        assert c["keys_a"] == 0 and c["entries_only_a"] == 0
    finally:
        e.free()


def test_selection_at_a_higher_omega_is_the_build_at_that_omega(engine):
    """DNA k = 8, two groups: built at omega 1.5 and at 1.8 (key-major, MIF0); the first selected at 1.8's threshold has the second's
    keys and, per key, its (branch, score bits)."""
    mats, groups = S.build_mats(), np.asarray(S.BUILD_GROUPS, np.uint32)
    made = []
    try:
        for w in S.BUILD_OMEGAS:
            db, parts = D.build_db_shard(engine, mats, groups, S.BUILD_K, co.log_threshold(w, 4, S.BUILD_K), 4)
            made += [db, parts]
            db.filter_mif0(engine, 3, ipk_amd.score_threshold(w, 4, S.BUILD_K))
        d1, d2 = made[0], made[2]
        v = engine.select_db(d1, min_log_score=co.log_threshold(S.BUILD_OMEGAS[1], 4, S.BUILD_K))
        made.append(v)
        assert v.header is None and 0 < d2.num_keys < d1.num_keys
        assert np.array_equal(v.keys(), d2.keys())

        def as_dict(db):
            br, sc = db.entries()
            return dict(keys=db.keys(), off=db.key_offsets(), br=br, sc=sc)
        assert S.entry_sets(as_dict(v)) == S.entry_sets(as_dict(d2))
        assert np.array_equal(v.keys()[v.filter_order()], d1.keys()[d1.filter_order()][np.isin(d1.keys()[d1.filter_order()], v.keys())])
    finally:
        for x in made:
            x.free()
