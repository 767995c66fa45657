"""GPU suite: Engine.union_dbs (ipkgpu_db_union), dbfile.union_shard_files (ipkgpu_db_union_files), Engine.load_dbs, the union route
of the key-range build and the command line over shard sets -- against the numpy restatement of tests/union_cases.py bit for bit,
and against the host merge (ipkgpu_db_merge_files) byte for byte.  The cases' properties are checked on the CPU
(tests/test_union_inputs.py)."""
import numpy as np
import pytest
from click.testing import CliRunner

import ipk_amd
from ipk_amd import cli, dbfile, keyrange
from ipk_amd import distributed as D
from ipk_amd.synth import synth_matrices
from oracle import ipk_oracle as co
from tests import db_files as F
from tests import union_cases as U
from tests.test_gpu_db_load import same_as_arrays, scores_a_small_call

pytestmark = pytest.mark.gpu

KINDS = [False, True]                                # plain, positioned
MIB = 1 << 20


def _bytes(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(case name, positioned) -> (host-merged file, shard files), each written and merged once."""
    d = tmp_path_factory.mktemp("union")
    made = {}

    def get(name, positioned):
        if (name, positioned) not in made:
            made[name, positioned] = U.host_merged(d, U.case(name), positioned)
        return made[name, positioned]
    return get


def load_all(engine, paths):
    return [engine.load_db(p) for p in paths]


def free_all(dbs):
    for d in dbs:
        d.free()


@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_union_is_the_restatement_and_the_host_merge(engine, files, tmp_path, name, positioned):
    c = U.case(name)
    merged, paths = files(name, positioned)
    srcs = load_all(engine, paths)
    try:
        u = engine.union_dbs(srcs)
        try:
            same_as_arrays(u, c["want"], positioned)
            assert u.header is None
            t = engine.union_times()
            assert t["total_ms"] >= t["entry_copy_ms"] >= 0.0 and t["key_sort_ms"] >= 0.0 and t["order_sort_ms"] >= 0.0
            out = tmp_path / "union.ipk"
            dbfile.write_db_device(engine, u, out, **dbfile.header_args(c["header"]))
            assert _bytes(out) == _bytes(merged)
        finally:
            u.free()
        again = engine.union_dbs(srcs)                                       # the same arrays on a second call
        try:
            same_as_arrays(again, c["want"], positioned)
        finally:
            again.free()
        for s, shard in zip(srcs, c["shards"]):                              # the sources are untouched
            same_as_arrays(s, shard, positioned)
    finally:
        free_all(srcs)
    out2 = tmp_path / "union_files.ipk"
    totals = dbfile.union_shard_files(engine, out2, **dbfile.header_args(c["header"]), shard_paths=paths)
    assert totals == (len(c["want"]["keys"]), int(c["want"]["off"][-1]))
    assert _bytes(out2) == _bytes(merged)


@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
def test_single_entry_form_of_the_copy(engine, files, positioned):
    """Option "union_copy_bytes" = 8, the copy kernel's other form (one entry per store; the default stores pairs): the same bits in
    every case."""
    engine.set_option("union_copy_bytes", 8)
    try:
        for name in U.CASE_NAMES:
            srcs = load_all(engine, files(name, positioned)[1])
            try:
                u = engine.union_dbs(srcs)
                try:
                    same_as_arrays(u, U.case(name)["want"], positioned)
                finally:
                    u.free()
            finally:
                free_all(srcs)
    finally:
        engine.set_option("union_copy_bytes", 0)
    with pytest.raises(ipk_amd.IpkGpuError):
        engine.set_option("union_copy_bytes", 12)


@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
def test_load_dbs(engine, files, positioned):
    c = U.case("owners3")
    merged, paths = files("owners3", positioned)
    u, head = engine.load_dbs(paths)
    try:
        same_as_arrays(u, c["want"], positioned)
        info = dbfile.file_info(merged)
        assert u.header is head
        for key in ("sequence_type", "tree_index", "newick", "kmer_size", "omega", "positions_loaded", "total_num_kmers", "total_num_entries"):
            assert head[key] == info[key], key
    finally:
        u.free()


@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
def test_consumers_take_the_union(engine, files, positioned):
    """diff, place and select over the union give what they give over the loaded merged file."""
    c = U.case("owners8")
    merged, paths = files("owners8", positioned)
    whole = engine.load_db(merged)
    u, _ = engine.load_dbs(paths)
    try:
        counts, rec = engine.diff_dbs(u, whole, eps=0.0, max_records=10)
        assert len(rec) == 0
        for key in ("keys_only_a", "keys_only_b", "entries_only_a", "entries_only_b", "scores_differ", "positions_differ"):
            assert counts[key] == 0, key
        assert counts["keys_a"] == counts["keys_b"] == len(c["want"]["keys"]) and counts["max_abs_diff"] == 0.0
        reads = U.reads_of(c["want"], 8)
        pa, pb = engine.place(u, reads), engine.place(whole, reads)
        assert pa.n_found.sum() > 0
        for name in ("branches", "counts", "n_kmers", "n_found", "n_branches"):
            assert np.array_equal(getattr(pa, name), getattr(pb, name)), name
        assert np.array_equal(pa.scores.view(np.uint32), pb.scores.view(np.uint32)) and np.array_equal(pa.lwr.view(np.uint64), pb.lwr.view(np.uint64))
        sa, sb = engine.select_db(u, mu=0.5), engine.select_db(whole, mu=0.5)
        try:
            want = dict(keys=sb.keys().copy(), off=sb.key_offsets().copy(), fv=sb.filter_values().copy(), order=sb.filter_order().copy())
            want["br"], want["sc"] = sb.entries()
            want["pos"] = sb.positions()
            assert len(want["keys"]) == 300
            same_as_arrays(sa, want, positioned)
        finally:
            sa.free(); sb.free()
    finally:
        u.free(); whole.free()


def test_refusals_leave_the_engine_usable(engine, files, tmp_path):
    c = U.case("owners2")
    _, paths = files("owners2", False)
    _, paths_pos = files("owners2", True)
    a, b = load_all(engine, paths)
    # a key in two shards: shard 1 with one key of shard 0 added
    whole = U.case("owners1")["shards"][0]
    shared = int(c["shards"][0]["keys"][7])
    idx = np.nonzero((whole["keys"] % 2 == 1) | (whole["keys"] == shared))[0]
    twice = engine.load_db(F.write(tmp_path / "twice.ipk", U.take(whole, idx), False, c["header"]))
    pos = engine.load_db(paths_pos[1])
    empty = engine.load_db(files("owners5_one_empty", False)[1][4])
    assert empty.num_keys == 0
    mats = synth_matrices(4, 40, 4, 0.1, 9)
    fresh, parts = D.build_db_shard(engine, mats, np.array([5, 5, 9, 9], np.uint32), 8, co.log_threshold(1.5, 4, 8), 4)
    try:
        def refused(dbs, *words):
            with pytest.raises(ipk_amd.IpkGpuError) as ei:
                engine.union_dbs(dbs)
            assert ei.value.code == 1
            for w in words:
                assert w in str(ei.value), (w, str(ei.value))
            u = engine.union_dbs([a, b])                                     # the next union on the same engine succeeds
            try:
                same_as_arrays(u, c["want"], False)
            finally:
                u.free()
        refused([a, twice], f"k-mer {shared} ", "source 0", "source 1")
        refused([empty, a, twice], f"k-mer {shared} ", "source 1", "source 2")
        refused([a, pos], "positioned and plain shards cannot be merged into one database", "source 1 has positions", "source 0 has none")
        refused([a, fresh], "source 1", "no filter values")
        refused([], "at least one source")
        scores_a_small_call(engine)
    finally:
        free_all([a, b, twice, pos, empty, fresh, parts])


def test_one_source_gives_a_copy(engine, files):
    c = U.case("owners1")
    _, paths = files("owners1", True)
    src = engine.load_db(paths[0])
    u = engine.union_dbs([src])
    src.free()
    try:
        same_as_arrays(u, c["want"], True)
    finally:
        u.free()


def test_budget(tmp_path):
    """Under "device_budget_bytes" = held + union_bytes(...) the union succeeds and the held peak stays within the budget; with 1 MiB
    less than the smallest budget (whole MiB) at which it succeeds it is IPKGPU_ERR_NOMEM, the sources read back unchanged and the
    union succeeds once the budget is lifted.  A database of 7 MB of entries, so that a MiB matters."""
    rng = np.random.default_rng(21)
    keys = np.sort(rng.choice(4 ** 8, size=300, replace=False))
    db = F.synthetic(seed=21, k=8, keys=keys, counts=rng.integers(2500, 3500, size=300))
    shards = U.split(db, np.arange(300) % 2, 2)
    want = U.restate(shards)
    eng = ipk_amd.Engine(0)
    try:
        srcs = [eng.load_db(F.write(tmp_path / f"s{i}.ipk", s, True, U.K8)) for i, s in enumerate(shards)]
        old = eng.get_option("device_budget_bytes")
        try:
            held = eng.mem_stats(reset_peak=True)[0]
            need = eng.union_bytes(len(want["keys"]), int(want["off"][-1]), 2, True)
            assert need > 8 * MIB
            eng.set_option("device_budget_bytes", held + need)
            u = eng.union_dbs(srcs)
            same_as_arrays(u, want, True)
            u.free()
            peak = eng.mem_stats()[1]
            print(f"union budget: held {held}, union_bytes {need}, held peak {peak}")
            assert held < peak <= held + need

            def fits(mib):
                eng.set_option("device_budget_bytes", mib * MIB)
                try:
                    eng.union_dbs(srcs).free()
                    return True
                except ipk_amd.IpkGpuError as e:
                    assert e.code == 3, str(e)
                    return False
            lo, hi = held // MIB, -(-(held + need) // MIB)                      # lo: nothing can be taken; hi: shown above to fit
            assert not fits(lo) and fits(hi)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if fits(mid) else (mid, hi)
            print(f"union budget: smallest whole MiB that fits {hi}, formula {(held + need) / MIB:.2f} MiB")
            assert not fits(hi - 1)
            for s, shard in zip(srcs, shards):
                same_as_arrays(s, shard, True)
            eng.set_option("device_budget_bytes", 0)
            u = eng.union_dbs(srcs)
            same_as_arrays(u, want, True)
            u.free()
        finally:
            eng.set_option("device_budget_bytes", old)
    finally:
        eng.close()


# ---- built databases -------------------------------------------------------------------------------------------------------------------

GROUPS = np.array([5, 5, 9, 9], dtype=np.uint32)
TREE_INDEX, NEWICK, OMEGA = [(1, 0.0), (3, 0.5), (5, 1.0)], "((a:1,b:1):1,c:1);", 1.5


def _k14(engine, out, work, **kw):
    k = 14
    mats = synth_matrices(4, 200, 4, 0.1, 1414)
    return keyrange.build_db_file(engine, mats, GROUPS, k, co.log_threshold(OMEGA, 4, k), 4, str(out), str(work), "DNA", TREE_INDEX, NEWICK, OMEGA,
                                  "mif0", 11, passes=4, **kw)


@pytest.fixture(scope="module")
def k14_default(tmp_path_factory):
    """The default route's file at the k = 14 shape in 4 passes, and the held peak of that build on an engine of its own."""
    d = tmp_path_factory.mktemp("k14")
    eng = ipk_amd.Engine(0)
    try:
        r = _k14(eng, d / "files.ipk", d / "w")
        assert r["route"] == "files" and r["union_s"] == 0.0
        return _bytes(d / "files.ipk"), r["totals"], eng.mem_stats()[1]
    finally:
        eng.close()


def test_key_range_build_unites_on_the_device(k14_default, tmp_path):
    want, totals, _ = k14_default
    eng = ipk_amd.Engine(0)
    try:
        r = _k14(eng, tmp_path / "device.ipk", tmp_path / "w", union_on_device=True)
        assert r["route"] == "device" and r["totals"] == totals and r["merge_s"] == 0.0 and r["union_s"] > 0.0
        assert _bytes(tmp_path / "device.ipk") == want
        assert not (tmp_path / "w" / "passes").exists()
    finally:
        eng.close()


def test_key_range_build_falls_back_under_a_budget(k14_default, tmp_path):
    """The budget: the held peak of the default route's build, in whole MiB -- every pass of the file mode fits it by construction,
    and the device route, which holds the passes' databases and then the union beside them, does not."""
    want, totals, peak = k14_default
    eng = ipk_amd.Engine(0)
    try:
        eng.set_option("device_budget_bytes", -(-peak // MIB) * MIB)
        try:
            r = _k14(eng, tmp_path / "fallback.ipk", tmp_path / "w", union_on_device=True)
        finally:
            eng.set_option("device_budget_bytes", 0)
        print(f"fallback under {-(-peak // MIB)} MiB: route {r['route']}")
        assert r["route"] == "fallback" and r["totals"] == totals
        assert _bytes(tmp_path / "fallback.ipk") == want
        assert not (tmp_path / "w" / "passes").exists()
    finally:
        eng.close()


def test_two_owner_build_united_is_the_one_owner_database(engine):
    k = 8
    mats = synth_matrices(6, 64, 4, 0.1, 88)
    groups = np.array([1, 1, 2, 2, 3, 3], np.uint32)
    eps = co.log_threshold(OMEGA, 4, k)
    thr = ipk_amd.score_threshold(OMEGA, 4, k)
    one, parts1 = D.build_db_shard(engine, mats, groups, k, eps, 4)
    one.filter_mif0(engine, 7, thr)
    parts = engine.score_groups_keymajor(mats, groups, k, eps, n_owners=2)
    owners = []
    try:
        for o in range(2):
            a, b = int(parts.owner_offsets[o]), int(parts.owner_offsets[o + 1])
            db = engine.merge_parts(4, k, o, 2, parts.counts_tensor()[o:o + 1].contiguous(), parts.entries_tensor()[a:b].contiguous(), np.zeros(1, np.uint64))
            db.filter_mif0(engine, 7, thr)
            owners.append(db)
        u = engine.union_dbs(owners)
        try:
            assert u.num_keys == one.num_keys > 0 and u.num_entries == one.num_entries
            assert np.array_equal(u.keys(), one.keys()) and np.array_equal(u.key_offsets(), one.key_offsets())
            (ub, us), (ob, os_) = u.entries(), one.entries()
            assert np.array_equal(ub, ob) and np.array_equal(us.view(np.uint32), os_.view(np.uint32))
            assert np.array_equal(u.filter_values().view(np.uint32), one.filter_values().view(np.uint32))
            assert np.array_equal(u.filter_values(f64=True).view(np.uint64), one.filter_values(f64=True).view(np.uint64))
            assert np.array_equal(u.filter_order(), one.filter_order())
        finally:
            u.free()
    finally:
        free_all(owners + [one, parts, parts1])


# ---- the command line ------------------------------------------------------------------------------------------------------------------

def test_cli_merge_on_both_routes(files, tmp_path):
    for positioned in KINDS:
        merged, paths = files("many_sources", positioned)
        for on in ("device", "host"):
            out = tmp_path / f"{on}_{int(positioned)}.ipk"
            res = CliRunner().invoke(cli.ipk, ["merge", "--on", on, "-o", str(out)] + paths)
            assert res.exit_code == 0, (res.output, res.exception)
            assert f"merged on the {on}" in res.output
            assert _bytes(out) == _bytes(merged)


def test_cli_place_on_a_shard_set(files, tmp_path):
    c = U.case("owners3")
    merged, paths = files("owners3", False)
    q = tmp_path / "reads.fasta"
    q.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(U.reads_of(c["want"], 8))))
    for extra in ([], ["--mu", "0.5"], ["--omega", "1.75"]):
        one = CliRunner().invoke(cli.ipk, ["place", "-i", merged, "-q", str(q)] + extra)
        many = CliRunner().invoke(cli.ipk, ["place", "-q", str(q)] + [x for p in paths for x in ("-i", p)] + extra)
        assert one.exit_code == 0 and many.exit_code == 0, (one.output, many.output, many.exception)
        assert many.output == one.output and one.output.count("\n") >= 12
