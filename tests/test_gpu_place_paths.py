"""GPU suite: the parts of Engine.place (ipkgpu_db_place) that tests/test_gpu_place.py leaves unexecuted or undecided -- a workgroup's
second and third query, both sides of the LDS bound, the prefix table at every code width, an inexact threshold on long queries, the
duplicate check's later passes, the slices and the batches under a device budget, the index rebuild, Engine.place_packed.

Every comparison is po.check's (tests/place_oracle.py): branches, order, score bits, counts and the per-query figures exactly, lwr
within po.lwr_tolerance.  The inputs are tests/place_cases.py from reuse_pool() on; tests/test_place_paths_inputs.py proves on the host
that they have the properties the tests here rely on."""
import numpy as np
import pytest

import ipk_amd
from ipk_amd import dbfile
from ipk_amd.engine import PLACE_NONE
from tests import place_cases as pc
from tests import place_oracle as po
from tests.test_gpu_place import default_options, loaded, same_bits          # noqa: F401  (fixtures of this module too)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def on_device(engine, tmp_path_factory):
    """(name, case) -> the case's database on the device (loaded once)."""
    d = tmp_path_factory.mktemp("place_paths")
    dbs = {}

    def get(name, case):
        if name not in dbs:
            dbs[name] = engine.load_db(pc.write_case_db(d / f"{name}.ipk", case))
        return dbs[name]
    yield get
    for db in dbs.values():
        db.free()


def place(engine, db, case, keep=7, queries=None, log_eps=pc.LOG_EPS):
    return engine.place(db, case.queries if queries is None else queries, keep_at_most=keep, sigma=case.sigma, k=case.k, log_eps=log_eps)


def compute_units(engine):
    import torch
    return int(torch.cuda.get_device_properties(engine.device_id).multi_processor_count)


# ---- 1. many queries per workgroup ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["lds", "global", "global_batches"])
def test_a_workgroup_places_three_queries(engine, loaded, path):
    """N = 2 G + G / 2 + 37 queries on a grid G wide: every workgroup places a second query, half of them a third, on tables that the
    previous query's epilogue cleared through its touched list.  Each query is a fixed-seed draw from the 72 distinct queries of the
    main and the order case and ""; every copy must equal the oracle's result for its text."""
    c = pc.reuse_pool()
    G = compute_units(engine) * (32 if path == "lds" else 4)
    draw = pc.reuse_draw(G)
    N = len(draw)
    assert N > 2 * G and N == 2 * G + G // 2 + 37
    once = pc.expected_at(c, pc.LOG_EPS, 7)                                  # computed once per distinct query
    want = [once[d] for d in draw]
    # the draw on THIS grid: a workgroup's consecutive queries mostly differ and share branches; empty ones follow full tables
    sets = pc.reuse_branch_sets()
    pairs = [(int(draw[i - G]), int(draw[i])) for i in range(G, N)]
    assert sum(a != b and bool(sets[a] & sets[b]) for a, b in pairs) >= 0.5 * len(pairs)
    assert any(len(sets[a]) == 300 and c.queries[b] == "" for a, b in pairs)
    if path != "lds":
        engine.set_option("place_lds_branches", 16)
    if path == "global_batches":
        engine.set_option("place_batch_queries", 2 * G)                      # two turns of the grid, then a batch narrower than the grid
        assert 0 < N - 2 * G < G
    res = place(engine, loaded("main_case"), c, queries=[c.queries[d] for d in draw])
    po.check(res, want)
    none = np.array([w["n_branches"] == 0 for w in want])
    assert none.sum() > N // 8
    assert (res.branches[none] == PLACE_NONE).all() and (res.scores[none] == 0).all() and (res.counts[none] == 0).all() and (res.lwr[none] == 0).all()


# ---- 2. table bounds -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("top", [4095, 4096, 63, 64])
def test_both_sides_of_the_table_bounds(engine, on_device, top):
    """B = 4096: the largest LDS tables (256 + 12 x 4096 bytes of dynamic LDS); B = 4097: the global tables by default; B = 64 and 65:
    b_pad 64 and 128.  The last branch is among the best of several queries.  Where the default is the LDS tables (B = 4096, 64, 65),
    the global tables give the same bits."""
    c = pc.bound_case(top)
    db = on_device(f"bound_{top}", c)
    res = place(engine, db, c)
    po.check(res, c.expected(7))
    assert any(top in row for row in res.branches.tolist())
    res64 = place(engine, db, c, keep=64)
    po.check(res64, c.expected(64))
    if top + 1 <= 4096:
        engine.set_option("place_lds_branches", 16)
        same_bits(res, place(engine, db, c))
        same_bits(res64, place(engine, db, c, keep=64))


# ---- 3. lookup -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tail", [False, True], ids=["top_key", "tail"])
@pytest.mark.parametrize("sigma,k", pc.LOOKUP_SHAPES)
def test_lookup_at_every_shift(engine, on_device, sigma, k, tail):
    """DNA k = 9, 12, 13, 15 and AA k = 3, 4, 5 (place_kernel<5, *> below k = 6; shifts 0, 2, 4, 8, 9, 10, 14): slots of 0, 1, 2 and up
    to 1025 keys, code 0 and the largest code, absent codes beside keys, in empty slots, above a full slot and (tail) above the
    database's last key, in windows that straddle the 64-window tiles."""
    c = pc.lookup_case(sigma, k, tail)
    db = on_device(f"lookup_{sigma}_{k}_{int(tail)}", c)
    res = place(engine, db, c)
    po.check(res, c.expected(7))
    engine.set_option("place_lds_branches", 16)
    same_bits(res, place(engine, db, c))


# ---- 4. long query, inexact threshold -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["order_case", "main_case", "long_case"])
def test_inexact_threshold(engine, loaded, name):
    """log_eps = f32(8 log10(1.5 / 4)): the penalty's product and its sum with S both round (a fused multiply-add changes a tenth of
    the scores: tests/test_place_paths_inputs.py); the long case has one query of 70 000 symbols, counts beyond 4000."""
    c = getattr(pc, name)()
    for keep in (7, 64):
        res = place(engine, loaded("main_case"), c, keep=keep, log_eps=pc.EPS_INEXACT)
        po.check(res, pc.expected_at(c, pc.EPS_INEXACT, keep))
    if name == "long_case":
        assert res.n_kmers[0] == 69993 and res.counts[0].max() > 3500
    engine.set_option("place_lds_branches", 16)
    same_bits(res, place(engine, loaded("main_case"), c, keep=64, log_eps=pc.EPS_INEXACT))


# ---- 5. duplicate check beyond the first pass ---------------------------------------------------------------------------------------------

def write_arrays(path, keys, off, br, sc):
    dbfile.write_db(path, "DNA", [(1, 0.0)], "(a:1,b:1)r;", 8, 1.5, keys, off, br, sc, np.zeros(len(keys), np.float32), np.arange(len(keys), dtype=np.uint32))
    return path


@pytest.mark.parametrize("which", ["tile", "apart", "last"])
def test_a_duplicate_beyond_branch_32768_is_refused(engine, loaded, tmp_path, which):
    """Branch 40 000 (the check's second bitmap pass) twice in one 64-entry tile and 200 entries apart, branch 70 000 (the third pass)
    twice in the last key: refused by the key's number; the engine places the main case afterwards."""
    keys, off, br, sc, bad_key = pc.dup_db(which)
    bad = engine.load_db(write_arrays(tmp_path / "dup.ipk", keys, off, br, sc))
    try:
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            engine.place(bad, [pc.decode(int(keys[0]), 4, 8)])
        assert ei.value.code == 1 and f"key {bad_key} " in str(ei.value) and "more than once" in str(ei.value)
    finally:
        bad.free()
    m = pc.main_case()
    po.check(place(engine, loaded("main_case"), m), m.expected(7))


def test_the_duplicate_check_accepts_the_control(engine, on_device):
    """Branches 32 767, 32 768, 65 535, 65 536 under one key and 40 000 under two DIFFERENT keys: accepted, placed as the oracle does."""
    c = pc.dup_control_case()
    res = place(engine, on_device("dup_control", c), c, keep=64)
    po.check(res, c.expected(64))
    assert {32767, 32768, 65535, 65536, 40000} <= set(res.branches[0].tolist())


# ---- 6. host paths -----------------------------------------------------------------------------------------------------------------------

def test_budgeted_slices(tmp_path):
    """200 queries on the global tables (B = 70 001) under device_budget_bytes = held + 64 MB: half of what is free holds 39 of the 200
    slices of 12 x 70 016 bytes, so the launch is narrower than the batch and its workgroups place several queries each.  The result
    is the oracle's and, bit for bit, that of the run without a budget; the peak stays within the budget.  (The 200 short queries are
    one batch: test_budgeted_batches_split has the batches.)"""
    c = pc.big_branch_case()
    rng = np.random.default_rng(200)
    draw = rng.integers(0, len(c.queries), 200)
    queries = [c.queries[d] for d in draw]
    want = [c.expected(7)[d] for d in draw]
    eng = ipk_amd.Engine(0)
    try:
        db = eng.load_db(pc.write_case_db(tmp_path / "big.ipk", c))
        held, _ = eng.mem_stats(reset_peak=True)
        budget = held + (64 << 20)
        eng.set_option("device_budget_bytes", budget)
        try:
            tight = place(eng, db, c, queries=queries)
            peak = eng.mem_stats()[1]
        finally:
            eng.set_option("device_budget_bytes", 0)
        po.check(tight, want)
        assert held < peak <= budget and peak - held < 200 * 12 * 70016
        free = place(eng, db, c, queries=queries)                            # no budget: a slice per query
        po.check(free, want)
        same_bits(tight, free)
        assert eng.mem_stats()[0] - held >= 200 * 12 * 70016
    finally:
        eng.close()


@pytest.mark.parametrize("path", ["lds", "global"])
def test_budgeted_batches_split(tmp_path, path):
    """1500 queries of the reuse pool (295 KB of sequence, 240 KB of results) under device_budget_bytes = held + 256 KB: more than
    twice what the budget leaves, so the call takes three batches or more, each sized from what is free at its turn and from what
    the workspaces of the batch before already hold.  The result is the oracle's and, bit for bit, that of the run without a budget;
    the peak stays within the budget.  On the global tables (B = 300 forced off the LDS) the slices share the same 256 KB: some 20
    of them, so a workgroup places twenty queries of a batch."""
    c = pc.reuse_pool()
    draw = pc.budget_draw()
    queries = [c.queries[d] for d in draw]
    once = pc.expected_at(c, pc.LOG_EPS, 7)
    want = [once[d] for d in draw]
    whole = sum(len(q) for q in queries) + len(queries) * pc.PLACE_QUERY_BYTES_7
    assert whole > 2 * pc.BUDGET_ROOM
    eng = ipk_amd.Engine(0)
    try:
        if path == "global":
            eng.set_option("place_lds_branches", 16)
        db = eng.load_db(pc.write_case_db(tmp_path / "main.ipk", c))
        po.check(place(eng, db, c, queries=queries[:1]), want[:1])           # the index is built and kept outside the budget
        held, _ = eng.mem_stats(reset_peak=True)
        budget = held + pc.BUDGET_ROOM
        eng.set_option("device_budget_bytes", budget)
        try:
            tight = place(eng, db, c, queries=queries)
            peak = eng.mem_stats()[1]
        finally:
            eng.set_option("device_budget_bytes", 0)
        po.check(tight, want)
        assert held < peak <= budget and 2 * (peak - held) < whole            # no batch held half of the call
        free = place(eng, db, c, queries=queries)                            # no budget: one batch
        same_bits(tight, free)
        assert eng.mem_stats()[0] - held >= whole
    finally:
        eng.close()


def valid_names(keys, sigma, k):
    return [pc.decode(int(c), sigma, k) for c in keys if pc.rank_of_code(int(c), sigma, k) is not None]


def test_another_code_width_rebuilds_the_index(engine):
    """A database from db_from_parts at DNA k = 8 placed on at k = 8, 9, amino acids k = 4 (its 16-bit keys read as 18- and 20-bit
    codes: another shift of the prefix table each time) and k = 8 again -- every call the oracle's on the same arrays; k = 7 is refused
    (the database holds a key of more than 14 bits) and leaves the k = 8 index right."""
    from ipk_amd.synth import synth_matrices
    k, sigma, n_groups, sites = 8, 4, 12, 200
    mats = synth_matrices(2 * n_groups, sites, sigma, 0.05, 4242)
    groups = np.repeat(np.arange(n_groups, dtype=np.uint32) * 3 + 5, 2)
    eps = ipk_amd.log_threshold(1.5, sigma, k)
    parts = engine.score_groups_keymajor(mats, groups, k, eps, n_owners=1)
    db = engine.db_from_parts(parts, sigma, k)
    try:
        keys = db.keys()
        br, sc = db.entries()
        view = po.DbView(keys, db.key_offsets(), br, sc)
        assert int(keys[-1]) >> 14 != 0
        rng = np.random.default_rng(89)

        def run(sigma, k):
            names = valid_names(keys, sigma, k)
            assert len(names) > 100
            letters = list(po.ALPHABET[sigma][0])
            q = ["".join(rng.choice(names, m)) for m in (1, 3, 9, 30)] + ["".join(rng.choice(letters, 150)), names[0], names[-1]]
            want = po.place(view, q, sigma, k, eps, 7)
            assert sum(w["n_found"] for w in want) >= 40
            po.check(engine.place(db, q, sigma=sigma, k=k, log_eps=eps), want)
        run(4, 8)
        run(4, 9)
        run(20, 4)
        run(4, 8)
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            engine.place(db, ["ACGTACGTAC"], sigma=4, k=7, log_eps=eps)
        assert ei.value.code == 1 and "holds key" in str(ei.value)
        run(4, 8)
    finally:
        db.free(); parts.free()


def test_place_packed(engine, loaded):
    """Engine.place_packed on a blob with 13 bytes before offsets[0], queries with the bytes 0x00, 0x80 and 0xFF between valid runs and
    an empty last query: the result of Engine.place on the same byte strings, which is the oracle's."""
    m = pc.main_case()
    names = [pc.decode(int(c), m.sigma, m.k) for c in m.db[0][:40]]
    run = lambda a, b: "".join(names[a:b]).encode()
    queries = [run(0, 5), run(5, 9) + b"\x00" + run(9, 12), run(12, 14) + b"\x80" + run(14, 20) + b"\xff" + run(20, 21), b"\xff" + run(21, 30) + b"\x00\x80",
               bytes(range(256)) + run(30, 33), run(33, 40).lower(), b""]
    blob = b"ACGTACGTACGTA" + b"".join(queries)
    assert len(blob) - len(b"".join(queries)) == 13
    off = 13 + np.concatenate([[0], np.cumsum([len(q) for q in queries])])
    want = po.place(m.view, queries, m.sigma, m.k, pc.LOG_EPS, 7)
    assert [w["n_found"] > 0 for w in want] == [True] * 6 + [False]
    db = loaded("main_case")
    packed = engine.place_packed(db, blob, off, keep_at_most=7, sigma=m.sigma, k=m.k, log_eps=pc.LOG_EPS)
    same_bits(packed, engine.place(db, queries, keep_at_most=7, sigma=m.sigma, k=m.k, log_eps=pc.LOG_EPS))
    po.check(packed, want)
    same_bits(packed, engine.place_packed(db, np.frombuffer(blob, np.uint8), off.tolist(), keep_at_most=7, sigma=m.sigma, k=m.k, log_eps=pc.LOG_EPS))
