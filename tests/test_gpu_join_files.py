"""GPU suite: Engine.join_files (ipkgpu_db_join_files) against dbfile.join_shard_files, the in-memory route, byte for byte -- at the
least budget the plan restated in tests/join_files_cases.py accepts, with room for everything and with "join_route" = 1; the ranges
reported against the restated plan, the device peak against the restated formula; the refusals; and the join of group-range builds
under a budget against the one-call build's file.  The cases' properties are checked on the CPU (tests/test_join_files_inputs.py)."""
import os

import numpy as np
import pytest

import ipk_amd
from ipk_amd import dbfile
from ipk_amd import distributed as DI
from ipk_amd.synth import synth_matrices
from oracle import ipk_oracle as co
from tests import diff_files_cases as D
from tests import join_cases as J
from tests import join_files_cases as X
from tests.test_gpu_diff_files import under, with_window

pytestmark = pytest.mark.gpu

KINDS = [False, True]
FILTERS = ["mif0", "random"]


def _bytes(path):
    with open(path, "rb") as fh:
        return fh.read()


def head_of(c):
    h = dbfile.header_args(c["header"])
    return h["sequence_type"], h["tree_index"], h["newick"], h["kmer_size"], h["omega"]


@pytest.fixture(scope="module")
def files(engine, tmp_path_factory):
    """(case, positioned) -> its shard files; (case, positioned, filter) -> the in-memory route's file with what it returned and the
    join's stats.  Each made once and only read afterwards."""
    d = tmp_path_factory.mktemp("join_files")
    shards, whole = {}, {}

    def shard_paths(name, positioned):
        if (name, positioned) not in shards:
            shards[name, positioned] = J.write_shards(d, X.case(name), positioned)
        return shards[name, positioned]

    def reference(name, positioned, which):
        key = (name, positioned, which)
        if key not in whole:
            out = str(d / f"{name}_{int(positioned)}_{which}_whole.ipk")
            ret = dbfile.join_shard_files(engine, out, *head_of(X.case(name)), shard_paths(name, positioned), which, X.N_NODES)
            whole[key] = dict(path=out, ret=ret, stats=engine.join_stats())
        return whole[key]
    return shard_paths, reference, d


def streamed(engine, c, paths, out, which, avail, route=0, tmp_dir=None):
    """join_files under `avail` bytes (None: no budget) at the cases' window -> (returned, ranges, stats, held, peak)."""
    def call():
        engine.set_option("join_route", route)
        try:
            return engine.join_files(paths, out, *head_of(c), which, X.N_NODES, X.threshold_of(c["header"]), tmp_dir=tmp_dir)
        finally:
            engine.set_option("join_route", 0)
    ret, held, peak = under(engine, avail, lambda: with_window(engine, X.WINDOW, 0, call))
    return ret, engine.join_files_ranges(), engine.join_files_stats(), held, peak


@pytest.mark.parametrize("which", FILTERS)
@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
@pytest.mark.parametrize("name", X.CASE_NAMES)
def test_streamed_join_is_the_in_memory_join(engine, files, tmp_path, name, positioned, which):
    shard_paths, reference, _ = files
    c, shards, paths = X.case(name), X.sides(name, positioned), shard_paths(name, positioned)
    ref = reference(name, positioned, which)
    want = _bytes(ref["path"])
    S, bodies = len(shards), sum(s.body for s in shards)

    # 1. the least budget the restated plan accepts
    budget = X.budget_of(name, positioned)
    plan = X.plan(shards, budget, c["header"])
    out = str(tmp_path / "least.ipk")
    ret, ranges, st, held, peak = streamed(engine, c, paths, out, which, budget)
    assert _bytes(out) == want
    assert ranges == [(lo, hi) for lo, hi, *_ in plan]
    worst = X.worst_range_bytes(shards, plan, budget)
    print(f"{name} {positioned} {which}: budget {budget}, {len(plan)} ranges, worst range {worst}, range peak {st['range_peak_bytes']}, peak {peak - held}")
    hist = 0 if X.fits_whole(shards, budget) else max(D.hist_pass_bytes(s.window, s.n_w, s.longest) for s in shards)
    assert 0 < st["range_peak_bytes"] <= worst <= budget
    assert st["range_peak_bytes"] <= peak - held <= max(worst, hist)                # (the histograms are counted, and taken beside the budget)
    assert ret == ref["ret"]
    assert st["shared_keys"] == ref["stats"]["shared_keys"] and st["entries_dropped"] == ref["stats"]["entries_dropped"] == ret[2]
    passes = S if X.fits_whole(shards, budget) else S * (1 + len(plan))
    assert st["passes"] == passes and st["body_bytes_read"] == (passes // S) * bodies
    assert st["avail_bytes"] == budget and st["window_bytes"] == X.WINDOW
    assert st["route1_ranges"] == sum(w["route"] for w in X.restated_ranges(c["shards"], plan))
    assert not os.path.exists(out + ".ranges")                                  # the range files and their directory are gone

    # 2. room for everything: one range, no histogram pass, nothing beside the output
    out = str(tmp_path / "room.ipk")
    ret, ranges, st, _, _ = streamed(engine, c, paths, out, which, None)
    assert _bytes(out) == want and ret == ref["ret"]
    assert ranges == [(0, 1 << 32)] and st["passes"] == S and st["hist_s"] == 0.0 and st["merge_s"] == 0.0
    assert sorted(os.listdir(tmp_path)) == ["least.ipk", "room.ipk"]

    # 3. always resolving duplicates gives the same bytes
    if which == "mif0":
        out = str(tmp_path / "route1.ipk")
        ret, ranges, st, _, _ = streamed(engine, c, paths, out, which, budget, route=1)
        assert _bytes(out) == want and ret == ref["ret"] and len(ranges) == len(plan)
        assert st["route1_ranges"] == sum(1 for w in X.restated_ranges(c["shards"], plan) if len(w["br"]) + w["dropped"])


def test_route_2_refuses_duplicates_and_leaves_no_file(engine, files, tmp_path):
    shard_paths, _, _ = files
    c, paths = X.case("straddle"), shard_paths("straddle", True)
    out, tmp = str(tmp_path / "refused.ipk"), str(tmp_path / "ranges_here")
    with pytest.raises(ipk_amd.IpkGpuError) as ei:
        streamed(engine, c, paths, out, "mif0", X.budget_of("straddle", True), route=2, tmp_dir=tmp)
    assert ei.value.code == 1
    for w in (f"k-mer {X.STRADDLE_DUP} ", "branch 7 ", "source 0", "source 1"):
        assert w in str(ei.value), (w, str(ei.value))
    assert engine.join_files_stats()["passes"] > 3                              # ranges before the duplicates were joined and written
    assert os.listdir(tmp_path) == []                                           # their files, the directory and the output are gone


def test_a_bin_that_does_not_fit_is_refused_before_any_load(engine, files, tmp_path):
    shard_paths, _, _ = files
    for positioned in KINDS:
        c, paths, shards = X.case("heavy_bin"), shard_paths("heavy_bin", positioned), X.sides("heavy_bin", positioned)
        budget = X.budget_of("heavy_bin", positioned)
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            streamed(engine, c, paths, str(tmp_path / "heavy.ipk"), "random", budget)
        assert ei.value.code == 3
        msg = str(ei.value)
        assert f"[{X.HEAVY_KEY}, {X.HEAVY_KEY + 1})" in msg and f"need {budget + 1} bytes" in msg and f"{budget} are there" in msg, msg
        for s, side in enumerate(shards):                                        # the records and entries of every shard in the bin
            assert f"1 records and 3000 entries of shard {s}" in msg, msg
        assert engine.join_files_stats()["passes"] == len(shards) and engine.join_files_ranges() == []     # the histogram passes, no load pass
        assert os.listdir(tmp_path) == []
        # one byte more and it is joined
        out = str(tmp_path / "fits.ipk")
        ret, ranges, st, _, _ = streamed(engine, c, paths, out, "random", budget + 1)
        assert len(ranges) >= 2 and st["passes"] == 2 * (1 + len(ranges)) and ret[2] == 1
        os.remove(out)


def test_a_mixed_set_is_refused_naming_the_file(engine, files, tmp_path):
    shard_paths, reference, _ = files
    plain, pos = shard_paths("straddle", False), shard_paths("straddle", True)
    c = X.case("straddle")
    out = str(tmp_path / "mixed.ipk")
    with pytest.raises(ipk_amd.IpkGpuError) as ei:
        streamed(engine, c, [plain[0], pos[1], plain[2]], out, "mif0", X.budget_of("straddle", False))
    assert ei.value.code == 1 and "positioned and plain shards cannot be merged into one database" in str(ei.value)
    assert f"{pos[1]} has positions, {plain[0]} has none" in str(ei.value)
    other_k = J.write_shards(tmp_path, X.case("top"), False)
    with pytest.raises(ipk_amd.IpkGpuError) as ei:
        streamed(engine, c, [plain[0], other_k[1]], out, "mif0", None)
    assert ei.value.code == 1 and other_k[1] + ": a shard of DNA, k = 16" in str(ei.value)
    assert not os.path.exists(out) and not os.path.exists(out + ".ranges")
    # the context still joins
    ret, ranges, _, _, _ = streamed(engine, c, plain, out, "mif0", X.budget_of("straddle", False))
    assert _bytes(out) == _bytes(reference("straddle", False, "mif0")["path"]) and len(ranges) >= 3


# ---- the join of group-range builds under a budget is the whole build -------------------------------------------------------------------

RANGES = [(0, 5), (5, 6), (6, 12)]
TREE_INDEX, NEWICK, OMEGA, N = [(1, 0.0), (3, 0.5), (5, 1.0)], "((a:1,b:1):1,c:1);", 1.5, 13


def build_range(engine, mats, groups, lo, hi, sigma, k, positions):
    order = list(dict.fromkeys(groups.tolist()))
    sel = np.isin(groups, order[lo:hi])
    db, parts = DI.build_db_shard(engine, mats[sel], groups[sel], k, co.log_threshold(OMEGA, sigma, k), sigma, positions=positions)
    parts.free()
    return db


@pytest.mark.parametrize("sigma,k,positions", [(4, 8, False), (20, 3, True)], ids=["dna_k8", "aa_k3_positions"])
def test_streamed_join_of_group_range_builds_is_the_whole_build(engine, tmp_path, sigma, k, positions):
    mats = synth_matrices(24, 64, sigma, 0.1 if sigma == 4 else 0.03, 4242)
    groups = np.repeat(np.arange(12, dtype=np.uint32) + 3, 2)
    seq = "DNA" if sigma == 4 else "AA"
    thr = ipk_amd.score_threshold(OMEGA, sigma, k)
    header = dict(sequence_type=seq, tree_index=TREE_INDEX, newick=NEWICK, kmer_size=k, omega=OMEGA)
    paths = []
    for i, (lo, hi) in enumerate(RANGES):
        d = build_range(engine, mats, groups, lo, hi, sigma, k, positions)
        try:
            paths.append(str(tmp_path / f"shard{i}.ipk"))
            dbfile.filter_and_write_device(engine, d, paths[-1], "random", seq, TREE_INDEX, NEWICK, k, OMEGA, N, thr)
        finally:
            d.free()
    # what the passes will see of each shard file: its records in file order
    shards = []
    for p in paths:
        _, recs = dbfile.read_db(p)
        shards.append(X.Shard([r[0] for r in recs], [len(r[2]) for r in recs], positions))
    budget = (X.least_budget(shards, header) + X.whole_budget(shards)) // 2
    plan = X.plan(shards, budget, header)
    assert len(plan) >= 2
    whole = build_range(engine, mats, groups, 0, 12, sigma, k, positions)
    try:
        assert whole.num_keys > 1000
        for which in FILTERS:
            a, b = str(tmp_path / f"join_{which}.ipk"), str(tmp_path / f"whole_{which}.ipk")
            dbfile.filter_and_write_device(engine, whole, b, which, seq, TREE_INDEX, NEWICK, k, OMEGA, N, thr)

            def call():
                return dbfile.join_shard_files_streamed(engine, a, seq, TREE_INDEX, NEWICK, k, OMEGA, paths, which, N)
            ret, held, peak = under(engine, budget, lambda: with_window(engine, X.WINDOW, 0, call))
            assert _bytes(a) == _bytes(b), which
            assert ret == (whole.num_keys, whole.num_entries, 0)
            assert engine.join_files_ranges() == [(lo, hi) for lo, hi, *_ in plan]
            st = engine.join_files_stats()
            assert st["passes"] == 3 * (1 + len(plan)) and st["shared_keys"] > 100 and st["range_peak_bytes"] <= X.worst_range_bytes(shards, plan, budget) <= budget
            assert dbfile.file_info(a)["positions_loaded"] == positions
    finally:
        whole.free()
