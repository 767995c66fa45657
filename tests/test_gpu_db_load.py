"""GPU suite: Engine.load_db (ipkgpu_db_load) -- a database file back onto the device.  Host-written files with the entry counts at
the unpack kernel's edges come back as the arrays they were written from and are written out again byte for byte; a built database
survives write + load array for array; damaged files are refused before a kernel sees them; the device budget is obeyed."""
import numpy as np
import pytest

import ipk_amd
from ipk_amd import dbfile
from ipk_amd import distributed as D
from ipk_amd.synth import synth_matrices
from oracle import ipk_oracle as co
from tests import db_files as F

pytestmark = pytest.mark.gpu


def same_as_arrays(db, want, positioned):
    assert db.num_keys == len(want["keys"]) and db.num_entries == int(want["off"][-1])
    assert np.array_equal(db.keys(), want["keys"])
    assert np.array_equal(db.key_offsets(), want["off"])
    br, sc = db.entries()
    assert np.array_equal(br, want["br"]) and np.array_equal(sc.view(np.uint32), want["sc"].view(np.uint32))
    assert np.array_equal(db.filter_values().view(np.uint32), want["fv"].view(np.uint32))
    assert np.array_equal(db.filter_values(f64=True), want["fv"].astype(np.float64))
    assert np.array_equal(db.filter_order(), want["order"])
    if positioned:
        assert np.array_equal(db.positions(), want["pos"])
    else:
        assert db.positions() is None


def round_trip(engine, tmp_path, want, positioned, header=F.HEADER):
    src = F.write(tmp_path / "src.ipk", want, positioned, header)
    db = engine.load_db(src)
    try:
        same_as_arrays(db, want, positioned)
        assert db.header == dbfile.file_info(src)
        back = tmp_path / "back.ipk"
        n = dbfile.write_db_device(engine, db, back, **dbfile.header_args(db.header))
        assert n == src.stat().st_size and back.read_bytes() == src.read_bytes()
    finally:
        db.free()


CASES = {
    "edges": lambda: F.synthetic(200, seed=5),                                            # 1, 2, 63, 64, 65, 255, 256, 257, 3000 entries
    "single": lambda: F.synthetic(keys=[201], counts=[3], seed=6),
    "empty": lambda: F.synthetic(keys=[], counts=[], seed=7),
    "top_key": lambda: F.synthetic(keys=[0, 5, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], counts=[2, 65, 1, 256, 7], seed=8),
    "zero_count": lambda: F.synthetic(keys=[1, 2, 3, 4], counts=[0, 5, 0, 0], seed=9),   # a record without entries is a legal record
}


@pytest.mark.parametrize("chunk", [0, 4096])
@pytest.mark.parametrize("positioned", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_round_trip_of_host_written_files(engine, tmp_path, case, positioned, chunk):
    """chunk = 4096: records, heads and single entries straddle the pinned buffers' boundaries (a 3000-entry record spans six)."""
    want = CASES[case]()
    header = dict(F.HEADER, kmer_size=16) if case == "top_key" else F.HEADER
    engine.set_option("db_load_chunk_bytes", chunk)
    try:
        assert engine.get_option("db_load_chunk_bytes") == chunk
        round_trip(engine, tmp_path, want, positioned, header)
    finally:
        engine.set_option("db_load_chunk_bytes", 0)


def test_positioned_records_start_at_every_phase(tmp_path):
    """The positioned file of the edge counts has records at every 2-byte phase mod 8 (what the funnel-shifted loads must cope with)."""
    starts, _ = F.record_starts(F.synthetic(200, seed=5), positioned=True)
    assert set(int(s) % 8 for s in starts) == {0, 2, 4, 6}


@pytest.mark.parametrize("sigma,k,n_groups,positions", [(4, 6, 2, False), (20, 3, 1, False), (20, 3, 2, True)])
def test_built_database_survives_write_and_load(engine, tmp_path, sigma, k, n_groups, positions):
    mats = synth_matrices(n_groups * 2, 40, sigma, 0.1, 77 + k)
    groups = np.repeat(np.arange(n_groups, dtype=np.uint32) + 3, 2)
    eps = co.log_threshold(1.5, sigma, k)
    built, parts = D.build_db_shard(engine, mats, groups, k, eps, sigma, positions=positions)
    built.filter_mif0(engine, n_groups + 1, ipk_amd.score_threshold(1.5, sigma, k))
    path = tmp_path / "built.ipk"
    head = dict(sequence_type="DNA" if sigma == 4 else "AA", tree_index=[(3, 1.0), (1, 0.5), (1, 0.25)], newick="(a:0.5,b:0.25)r;", kmer_size=k, omega=1.5)
    dbfile.write_db_device(engine, built, path, **head)
    assert built.num_keys > 0
    loaded = engine.load_db(path)
    try:
        br, sc = built.entries()
        # (the file keeps the filter value as a float: the loaded double is its widening, the built one the MIF0 double itself)
        want = dict(keys=built.keys(), off=built.key_offsets(), br=br, sc=sc, fv=built.filter_values(), order=built.filter_order(),
                    pos=built.positions())
        same_as_arrays(loaded, want, positions)
        for name, value in head.items():
            assert loaded.header[name] == value
        assert loaded.header["positions_loaded"] is positions
    finally:
        loaded.free(); built.free(); parts.free()


def scores_a_small_call(engine):
    mats = synth_matrices(2, 30, 4, 0.1, 5)
    eps = co.log_threshold(1.5, 4, 5)
    res = engine.score_groups(mats, np.array([1, 1], np.uint32), 5, eps)
    keys, scores, emitted = co.explore_group(mats, 5, eps)
    gk, gs = res.group(0)
    assert np.array_equal(gk, keys) and np.array_equal(gs.view(np.uint32), scores.view(np.uint32)) and res.emitted == emitted
    res.free()


@pytest.mark.parametrize("positioned", [False, True])
def test_damaged_files_are_refused(engine, tmp_path, positioned):
    want = F.synthetic(200, seed=11)
    good, bad = F.damaged(tmp_path, want, positioned)
    held = engine.mem_stats()[0]
    for name, (path, record) in bad.items():
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            engine.load_db(path)
        assert ei.value.code == 1, name
        if record is not None:
            assert f"record {record} at byte offset " in str(ei.value), (name, str(ei.value))
    assert engine.mem_stats()[0] <= held                     # the images are gone
    scores_a_small_call(engine)
    engine.load_db(good).free()


def test_duplicate_key_is_refused(engine, tmp_path):
    want = F.synthetic(50, seed=12)
    want["keys"][31] = want["keys"][30]                      # two records of one k-mer: a whole file, as far as the walk can tell
    path = F.write(tmp_path / "dup.ipk", want)
    assert dbfile.check_file(path) == (50, int(want["off"][-1]))
    with pytest.raises(ipk_amd.IpkGpuError, match="more than one record") as ei:
        engine.load_db(path)
    assert ei.value.code == 1
    scores_a_small_call(engine)


def test_device_budget_is_obeyed(engine, tmp_path):
    path = F.write(tmp_path / "a.ipk", F.synthetic(200, seed=5))
    engine.set_option("release_workspaces", 1)
    held = engine.mem_stats()[0]
    budget = engine.get_option("device_budget_bytes")
    engine.set_option("device_budget_bytes", held + path.stat().st_size // 2)        # the image of the file's body does not fit
    try:
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            engine.load_db(path)
        assert ei.value.code == 3
        assert engine.mem_stats()[0] == held
    finally:
        engine.set_option("device_budget_bytes", budget)
    engine.load_db(path).free()
    scores_a_small_call(engine)
