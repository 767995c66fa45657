"""GPU suite: Engine.join_dbs (ipkgpu_db_join) against the numpy restatement of tests/join_cases.py bit for bit, on both routes; the
filters over a join; the join of group-range builds against the one-call build byte for byte; refusals, the budget and the consumers.
The cases' properties are checked on the CPU (tests/test_join_inputs.py)."""
import numpy as np
import pytest

import ipk_amd
from ipk_amd import dbfile
from ipk_amd import distributed as D
from ipk_amd.synth import synth_matrices
from oracle import ipk_oracle as co
from tests import db_files as F
from tests import join_cases as J
from tests import union_cases as U
from tests.test_gpu_db_load import same_as_arrays, scores_a_small_call

pytestmark = pytest.mark.gpu

KINDS = [False, True]                                # plain, positioned
N_NODES, OMEGA = 6001, 1.5                           # MIF0's N for the cases (their branches lie below 100000; N only scales the values)
THR = ipk_amd.score_threshold(OMEGA, 4, 8)


def _bytes(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.fixture(scope="module")
def shard_files(tmp_path_factory):
    """(case name, positioned) -> the case's shard files, written once."""
    d = tmp_path_factory.mktemp("join")
    made = {}

    def get(name, positioned):
        if (name, positioned) not in made:
            made[name, positioned] = J.write_shards(d, J.case(name), positioned)
        return made[name, positioned]
    return get


def free_all(dbs):
    for d in dbs:
        d.free()


def same_join(db, want, positioned):
    """keys, key offsets, entries and positions bit for bit"""
    assert db.num_keys == len(want["keys"]) and db.num_entries == int(want["off"][-1])
    assert np.array_equal(db.keys(), want["keys"])
    assert np.array_equal(db.key_offsets(), want["off"])
    br, sc = db.entries()
    assert np.array_equal(br, want["br"]) and np.array_equal(sc.view(np.uint32), want["sc"].view(np.uint32))
    if positioned:
        assert np.array_equal(db.positions(), want["pos"])
    else:
        assert db.positions() is None


def join_on_route(engine, srcs, route):
    engine.set_option("join_route", route)
    try:
        return engine.join_dbs(srcs)
    finally:
        engine.set_option("join_route", 0)


@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
@pytest.mark.parametrize("name", J.CASE_NAMES)
def test_join_is_the_restatement_on_both_routes(engine, shard_files, name, positioned):
    want = J.case(name)["want"]
    srcs = [engine.load_db(p) for p in shard_files(name, positioned)]
    try:
        got = {}
        for route in (0, 1):
            j = join_on_route(engine, srcs, route)
            try:
                same_join(j, want, positioned)
                assert j.header is None
                st = engine.join_stats()
                assert st["shared_keys"] == want["shared_keys"] and st["entries_dropped"] == want["dropped"]
                assert st["route"] == (want["route"] if route == 0 else (1 if len(want["br"]) + want["dropped"] else 0))
                assert st["total_ms"] >= st["entry_copy_ms"] >= 0.0 and st["key_ms"] >= 0.0 and st["duplicate_ms"] >= 0.0
                got[route] = (j.keys().copy(), j.key_offsets().copy(), j.entries()[0].copy(), j.entries()[1].view(np.uint32).copy(),
                              None if not positioned else j.positions().copy())
            finally:
                j.free()
        for a, b in zip(got[0], got[1]):
            assert (a is None and b is None) or np.array_equal(a, b)
        for s, shard in zip(srcs, J.case(name)["shards"]):                    # the sources are untouched
            same_as_arrays(s, shard, positioned)
    finally:
        free_all(srcs)


@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
@pytest.mark.parametrize("name", ["duplicates", "wave_edges", "long_lists", "entryless", "many_sources"])
def test_filters_over_a_join(engine, shard_files, tmp_path, name, positioned):
    """The filter values of a join are those of a loaded file of the restatement (the same device filter: only the join differs), and
    MIF0's float values are the sequential oracle's."""
    c = J.case(name)
    want = c["want"]
    srcs = [engine.load_db(p) for p in shard_files(name, positioned)]
    try:
        j = engine.join_dbs(srcs)
    finally:
        free_all(srcs)
    ref = engine.load_db(F.write(tmp_path / "restated.ipk", J.with_filter(want, np.zeros(len(want["keys"]), np.float32)), positioned, c["header"]))
    try:
        same_join(ref, want, positioned)
        for which in ("mif0", "random"):
            for d in (j, ref):
                d.filter_mif0(engine, N_NODES, THR) if which == "mif0" else d.filter_random(engine)
            assert np.array_equal(j.filter_values().view(np.uint32), ref.filter_values().view(np.uint32)), which
            assert np.array_equal(j.filter_values(f64=True).view(np.uint64), ref.filter_values(f64=True).view(np.uint64)), which
            assert np.array_equal(j.filter_order(), ref.filter_order()), which
            if which == "mif0":
                off = want["off"].astype(np.int64)
                host = np.array([co.mif0(want["sc"][off[i]:off[i + 1]], N_NODES, THR) for i in range(len(want["keys"]))], np.float64).astype(np.float32)
                diff = np.flatnonzero(j.filter_values().view(np.uint32) != host.view(np.uint32))
                assert len(diff) <= 2, (len(diff), j.filter_values()[diff[:5]], host[diff[:5]])     # (the last bit of pow / log2: as test_mif0_order_matches_the_sequential_oracle)
    finally:
        j.free(); ref.free()


# ---- the join of group-range builds is the whole build -------------------------------------------------------------------------------

RANGES = [(0, 5), (5, 6), (6, 12)]
TREE_INDEX, NEWICK = [(1, 0.0), (3, 0.5), (5, 1.0)], "((a:1,b:1):1,c:1);"


def build_range(engine, mats, groups, lo, hi, sigma, k, positions):
    order = list(dict.fromkeys(groups.tolist()))
    sel = np.isin(groups, order[lo:hi])
    db, parts = D.build_db_shard(engine, mats[sel], groups[sel], k, co.log_threshold(OMEGA, sigma, k), sigma, positions=positions)
    parts.free()
    return db


@pytest.mark.parametrize("sigma,k,positions", [(4, 8, False), (20, 3, True)], ids=["dna_k8", "aa_k3_positions"])
def test_join_of_group_range_builds_is_the_whole_build(engine, tmp_path, sigma, k, positions):
    mats = synth_matrices(24, 64, sigma, 0.1 if sigma == 4 else 0.03, 4242)
    groups = np.repeat(np.arange(12, dtype=np.uint32) + 3, 2)
    seq = "DNA" if sigma == 4 else "AA"
    thr = ipk_amd.score_threshold(OMEGA, sigma, k)
    whole = build_range(engine, mats, groups, 0, 12, sigma, k, positions)
    shards = [build_range(engine, mats, groups, lo, hi, sigma, k, positions) for lo, hi in RANGES]
    try:
        assert whole.num_keys > 1000 and whole.num_entries > 2 * whole.num_keys
        j = engine.join_dbs(shards)                                          # fresh from_parts databases: no filter values, no order
        back = engine.join_dbs(shards[::-1])
        try:
            st = engine.join_stats()
            assert st["entries_dropped"] == 0 and st["shared_keys"] > 100
            assert j.num_entries == whole.num_entries == back.num_entries
            assert np.array_equal(j.keys(), whole.keys()) and np.array_equal(j.key_offsets(), whole.key_offsets())
            for a, b in zip(j.entries(), whole.entries()):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            if positions:
                assert np.array_equal(j.positions(), whole.positions())
            # the wrong order: the same keys and counts, another entry order -- the order is defined, not accidental
            assert np.array_equal(back.keys(), whole.keys()) and np.array_equal(back.key_offsets(), whole.key_offsets())
            assert not np.array_equal(back.entries()[0], whole.entries()[0])
            for which in ("mif0", "random"):
                a, b = tmp_path / f"join_{which}.ipk", tmp_path / f"whole_{which}.ipk"
                for d, path in ((j, a), (whole, b)):
                    dbfile.filter_and_write_device(engine, d, path, which, seq, TREE_INDEX, NEWICK, k, OMEGA, 13, thr)
                assert _bytes(a) == _bytes(b), which
                assert dbfile.file_info(a)["positions_loaded"] == positions
        finally:
            j.free(); back.free()
    finally:
        free_all(shards + [whole])


# ---- routes, refusals, budget, consumers -----------------------------------------------------------------------------------------------

def test_route_2_refuses_duplicates_and_names_one(engine, shard_files):
    srcs = [engine.load_db(p) for p in shard_files("duplicates", True)]
    clean = [engine.load_db(p) for p in shard_files("branch_ranges", True)]
    try:
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            join_on_route(engine, srcs, 2)
        assert ei.value.code == 1
        # the first dropped entry of the concatenated layout: key DUP_KEY, branch 7, first in source 0, again in source 1
        for w in (f"k-mer {J.DUP_KEY} ", "branch 7 ", "source 0", "source 1"):
            assert w in str(ei.value), (w, str(ei.value))
        j = join_on_route(engine, clean, 2)
        try:
            same_join(j, J.case("branch_ranges")["want"], True)
            assert engine.join_stats()["route"] == 0
        finally:
            j.free()
        with pytest.raises(ipk_amd.IpkGpuError):
            engine.set_option("join_route", 3)
    finally:
        free_all(srcs + clean)


def test_refusals_leave_the_engine_usable(engine, shard_files):
    c = J.case("first_place")
    srcs = [engine.load_db(p) for p in shard_files("first_place", False)]
    pos = engine.load_db(shard_files("first_place", True)[1])
    other = ipk_amd.Engine(0)
    foreign = other.load_db(shard_files("first_place", False)[0])
    try:
        def refused(call, *words):
            with pytest.raises(ipk_amd.IpkGpuError) as ei:
                call()
            assert ei.value.code == 1
            for w in words:
                assert w in str(ei.value), (w, str(ei.value))
            j = engine.join_dbs(srcs)                                        # the next join on the same engine succeeds
            try:
                same_join(j, c["want"], False)
            finally:
                j.free()
        refused(lambda: engine.join_dbs([]), "at least one source")
        refused(lambda: engine.join_dbs([srcs[0], pos]), "positioned and plain shards cannot be merged into one database", "source 1 has positions", "source 0 has none")
        refused(lambda: engine.join_dbs([srcs[0], foreign]), "source 1", "another context")

        class Null:
            _h = None
        refused(lambda: engine.join_dbs([srcs[0], Null()]), "source 1", "null")
        scores_a_small_call(engine)
    finally:
        foreign.free(); other.close()
        free_all(srcs + [pos])


def test_key_and_entry_limits_are_host_arithmetic():
    """The two size refusals cannot be reached with data a test may hold; their bound, ipkgpu_db_join_bytes, is host arithmetic and grows
    with every argument."""
    b = ipk_amd.Engine.join_bytes
    assert b(1000, 5000, 2, True) > b(1000, 5000, 2, False) > 8 * 5000
    assert b(2000, 5000, 2, False) > b(1000, 5000, 2, False) and b(1000, 6000, 2, False) > b(1000, 5000, 2, False)
    assert b(1000, 5000, 70, False) > b(1000, 5000, 2, False)


def test_join_bytes_bounds_the_long_lists(shard_files):
    """`long_lists` takes every stage -- the branch table, the three duplicate kernels and the sorted pass: the bound holds there too."""
    c = J.case("long_lists")
    eng = ipk_amd.Engine(0)
    try:
        srcs = [eng.load_db(p) for p in shard_files("long_lists", True)]
        eng.set_option("release_workspaces", 1)
        held = eng.mem_stats(reset_peak=True)[0]
        j = eng.join_dbs(srcs)
        assert eng.join_stats()["route"] == 1
        j.free()
        peak = eng.mem_stats()[1]
        need = eng.join_bytes(sum(len(s["keys"]) for s in c["shards"]), sum(len(s["br"]) for s in c["shards"]), 3, True)
        print(f"join bytes, long_lists: held {held}, peak {peak}, join_bytes {need}")
        assert held < peak <= held + need
    finally:
        eng.close()


def test_budget(shard_files):
    """On `tiles`: the held peak of the call, minus what the sources hold, stays within ipkgpu_db_join_bytes; under a budget one byte
    below that peak the join is IPKGPU_ERR_NOMEM, the sources stay intact and the join succeeds once the budget is lifted."""
    c = J.case("tiles")
    want = c["want"]
    for route in (0, 1):
        eng = ipk_amd.Engine(0)
        try:
            srcs = [eng.load_db(p) for p in shard_files("tiles", True)]
            eng.set_option("release_workspaces", 1)
            eng.set_option("join_route", route)
            held = eng.mem_stats(reset_peak=True)[0]
            j = eng.join_dbs(srcs)
            same_join(j, want, True)
            j.free()
            eng.set_option("release_workspaces", 1)                           # (the freed result's cached blocks go back)
            peak = eng.mem_stats()[1]
            need = eng.join_bytes(sum(len(s["keys"]) for s in c["shards"]), sum(len(s["br"]) for s in c["shards"]), 2, True)
            print(f"join budget, route {route}: held {held}, peak {peak}, join_bytes {need}")
            assert held < peak <= held + need
            assert eng.mem_stats()[0] == held
            eng.set_option("device_budget_bytes", peak - 1)
            with pytest.raises(ipk_amd.IpkGpuError) as ei:
                eng.join_dbs(srcs)
            assert ei.value.code == 3, str(ei.value)
            eng.set_option("device_budget_bytes", peak)
            eng.join_dbs(srcs).free()
            eng.set_option("device_budget_bytes", 0)
            for s, shard in zip(srcs, c["shards"]):
                same_as_arrays(s, shard, True)
            j = eng.join_dbs(srcs)
            same_join(j, want, True)
            j.free()
        finally:
            eng.close()


@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
def test_consumers_take_the_join(engine, shard_files, tmp_path, positioned):
    """diff, place, select and union over a joined, filtered database give what they give over the loaded file of the restatement."""
    c = J.case("branch_ranges")
    want = c["want"]
    srcs = [engine.load_db(p) for p in shard_files("branch_ranges", positioned)]
    try:
        j = engine.join_dbs(srcs)
    finally:
        free_all(srcs)
    j.filter_mif0(engine, N_NODES, THR)
    path = tmp_path / "whole.ipk"
    dbfile.write_db_device(engine, j, path, **dbfile.header_args(c["header"]))
    whole = engine.load_db(path)
    other = engine.load_db(F.write(tmp_path / "other.ipk", F.synthetic(seed=77, k=8, keys=np.arange(70000, 70050)), positioned, c["header"]))
    try:
        same_join(whole, want, positioned)
        counts, rec = engine.diff_dbs(j, whole, eps=0.0, max_records=10)
        assert len(rec) == 0
        for key in ("keys_only_a", "keys_only_b", "entries_only_a", "entries_only_b", "scores_differ", "positions_differ"):
            assert counts[key] == 0, key
        assert counts["keys_a"] == counts["keys_b"] == len(want["keys"]) and counts["max_abs_diff"] == 0.0
        reads = U.reads_of(want, 8)
        eps = ipk_amd.log_threshold(OMEGA, 4, 8)
        pa, pb = engine.place(j, reads, sigma=4, k=8, log_eps=eps), engine.place(whole, reads)
        assert pa.n_found.sum() > 0
        for name in ("branches", "counts", "n_kmers", "n_found", "n_branches"):
            assert np.array_equal(getattr(pa, name), getattr(pb, name)), name
        assert np.array_equal(pa.scores.view(np.uint32), pb.scores.view(np.uint32)) and np.array_equal(pa.lwr.view(np.uint64), pb.lwr.view(np.uint64))
        sa, sb = engine.select_db(j, mu=0.5), engine.select_db(whole, mu=0.5)
        try:
            assert sa.num_keys == sb.num_keys == 150 and np.array_equal(sa.keys(), sb.keys()) and np.array_equal(sa.key_offsets(), sb.key_offsets())
            assert np.array_equal(sa.entries()[1].view(np.uint32), sb.entries()[1].view(np.uint32)) and np.array_equal(sa.filter_order(), sb.filter_order())
        finally:
            sa.free(); sb.free()
        ua, ub = engine.union_dbs([j, other]), engine.union_dbs([whole, other])
        try:
            assert ua.num_keys == len(want["keys"]) + 50
            assert np.array_equal(ua.keys(), ub.keys()) and np.array_equal(ua.entries()[0], ub.entries()[0]) and np.array_equal(ua.filter_order(), ub.filter_order())
        finally:
            ua.free(); ub.free()
    finally:
        j.free(); whole.free(); other.free()
