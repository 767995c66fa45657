"""GPU suite: the parts of Engine.place with options (ipkgpu_db_place_opts: place_ext_kernel and the host side of db_place.hpp) that
tests/test_gpu_place_ext.py leaves unexecuted -- the lookup of an ambiguous window's resolutions at every code width, both sides of
the LDS bound under ambiguous windows, a 70 000-symbol query on both strands, an inexact threshold, bytes that alias an ambiguous
letter, keep_at_most = 1 with both strands, a strand tie between two branches, batches narrower than the grid, the window tables
under a device budget -- and the rounding ladder, which measures how close to a binary32 rounding midpoint an ambiguous contribution
may come before the device's exp10 / log10 round it the other way.

Every comparison is xo.check's (tests/place_ext_oracle.py): branches, order, score bits, counts, n_kmers, n_found, n_branches, strand
and n_ambiguous exactly, lwr within po.lwr_tolerance.  The inputs are tests/place_ext_cases.py from expected_ext_at() on;
tests/test_place_ext_paths_inputs.py proves on the host that they have the properties the tests here rely on."""
import numpy as np
import pytest

import ipk_amd
from tests import place_cases as pc
from tests import place_ext_cases as xc
from tests import place_ext_oracle as xo
from tests.test_gpu_place import default_options, same_bits                  # noqa: F401  (the fixture resets the options)
from tests.test_gpu_place_ext import same_ext_bits
from tests.test_gpu_place_paths import compute_units

pytestmark = pytest.mark.gpu

CASES = dict(xc.ALL_CASES, **xc.NEW_CASES)
GENERIC = [(n, a, s) for n, modes in xc.NEW_MODES.items() if n not in ("alias_case", "ladder_case") for a, s in modes]


@pytest.fixture(scope="module")
def loaded(engine, tmp_path_factory):
    """case name -> the case's database on the device (loaded once)."""
    d = tmp_path_factory.mktemp("place_ext_paths")
    dbs = {}

    def get(name):
        if name not in dbs:
            dbs[name] = engine.load_db(pc.write_case_db(d / f"{name}.ipk", CASES[name]()))
        return dbs[name]
    yield get
    for db in dbs.values():
        db.free()


def place(engine, db, case, ambiguity, strands, keep=7, queries=None, log_eps=xc.LOG_EPS):
    return engine.place(db, case.queries if queries is None else queries, keep_at_most=keep, sigma=case.sigma, k=case.k, log_eps=log_eps,
                        ambiguity=ambiguity, strands=strands)


def on_every_path(engine, run, want, one_query_batches=True):
    """run() on the LDS tables, on the global tables and with one query a batch: the oracle's results, the same bits on each."""
    lds = run()
    xo.check(lds, want)
    engine.set_option("place_lds_branches", 16)
    glob = run()
    xo.check(glob, want)
    same_ext_bits(lds, glob)
    engine.set_option("place_lds_branches", 0)
    if one_query_batches:
        engine.set_option("place_batch_queries", 1)
        same_ext_bits(lds, run())
        engine.set_option("place_batch_queries", 0)
    return lds


# ---- 1a, 1b, 1c, 1f: every new case on every path ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,ambiguity,strands", GENERIC)
def test_cases_on_every_path(engine, loaded, name, ambiguity, strands):
    """lookup_ext_*: the resolutions of an ambiguous window through place_lookup at shifts 0 .. 16 (a key, an empty slot, after a slot's
    last key, before its first, above the database's last key; 0xFFFFFFFF at k = 16).  bound_ext_*: B = 4096 (768 + 12 x 4096 bytes of
    dynamic LDS), 4097 (the global tables by default), 64 and 65 with the last branch under ambiguous windows.  long_ext_case: 70 000
    symbols on both strands, the text and its reverse complement (one query each: no one-query batches).  tie_case: equal scores on
    the two strands for different branches."""
    c = CASES[name]()
    want = c.expected(7, ambiguity, strands)
    res = on_every_path(engine, lambda: place(engine, loaded(name), c, ambiguity, strands), want, one_query_batches=name != "long_ext_case")
    if ambiguity and name != "tie_case":
        assert int(res.n_ambiguous.sum()) > 0
    if name == "long_ext_case":
        assert res.strand.tolist() == [0, 1] and res.n_kmers[0] == res.n_kmers[1] > 69000
        assert np.array_equal(res.scores[0].view(np.uint32), res.scores[1].view(np.uint32)) and np.array_equal(res.branches[0], res.branches[1])
    if name == "tie_case":
        assert res.strand[:2].tolist() == [0, 0] and res.branches[:2, 0].tolist() == [3, 9]
    if name.startswith("bound_ext_"):
        top = int(name.rsplit("_", 1)[1])
        assert any(top in row for row in res.branches.tolist())
        xo.check(place(engine, loaded(name), c, ambiguity, strands, keep=64), c.expected(64, ambiguity, strands))


# ---- 1d: an inexact threshold ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,ambiguity,strands", [(n, a, s) for n in ("main_ext_case", "strand_case") for a, s in xc.MODES[n]])
def test_inexact_threshold(engine, loaded, name, ambiguity, strands):
    """log_eps = pc.EPS_INEXACT: E = 10^log_eps is no round number, the penalty's product rounds and so does its sum with S."""
    c = CASES[name]()
    want = xc.expected_ext_at(c, pc.EPS_INEXACT, 7, ambiguity, strands)
    on_every_path(engine, lambda: place(engine, loaded(name), c, ambiguity, strands, log_eps=pc.EPS_INEXACT), want)
    xo.check(place(engine, loaded(name), c, ambiguity, strands, keep=64, log_eps=pc.EPS_INEXACT),
             xc.expected_ext_at(c, pc.EPS_INEXACT, 64, ambiguity, strands))


# ---- 1e: alias bytes -----------------------------------------------------------------------------------------------------------------------

def test_alias_bytes_through_place_packed(engine, loaded):
    """Engine.place_packed with ambiguity and both strands over queries that hold every byte equal to an ambiguous letter in its low five
    bits (masktab is indexed by byte & 31; only the symbol table keeps such a byte invalid), 0x00, 0x80, 0xFF, and U / u."""
    c = xc.alias_case()
    raw = [q.encode("latin-1") for q in c.queries]
    assert all(len(r) == len(q) for r, q in zip(raw, c.queries))
    blob = b"ACGTN" + b"".join(raw)
    off = 5 + np.concatenate([[0], np.cumsum([len(r) for r in raw])])
    want = c.expected(7, True, "both")
    db = loaded("main_ext_case")
    run = lambda: engine.place_packed(db, blob, off, keep_at_most=7, sigma=4, k=xc.K, log_eps=xc.LOG_EPS, ambiguity=True, strands="both")
    res = on_every_path(engine, run, want)
    assert set(res.strand.tolist()) == {0, 1} and int(res.n_ambiguous.sum()) == sum(w["n_ambiguous"] for w in want) > 0
    same_ext_bits(res, engine.place(db, raw, keep_at_most=7, sigma=4, k=xc.K, log_eps=xc.LOG_EPS, ambiguity=True, strands="both"))


# ---- 1f: keep_at_most = 1 with both strands ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ambiguity", [False, True], ids=["plain", "ambiguity"])
def test_keep_one_with_both_strands(engine, loaded, ambiguity):
    """One lane holds a result: where the given strand wins, its lane registers are restored after the reverse strand's pass."""
    c = xc.strand_case()
    want = c.expected(1, ambiguity, "both")
    res = on_every_path(engine, lambda: place(engine, loaded("strand_case"), c, ambiguity, "both", keep=1), want)
    assert res.branches.shape == (len(want), 1) and set(res.strand.tolist()) == {0, 1}
    seven = place(engine, loaded("strand_case"), c, ambiguity, "both")
    assert np.array_equal(res.branches[:, 0], seven.branches[:, 0]) and np.array_equal(res.scores[:, 0].view(np.uint32), seven.scores[:, 0].view(np.uint32))
    assert np.array_equal(res.lwr[:, 0], seven.lwr[:, 0]) and np.array_equal(res.strand, seven.strand)


# ---- three queries a workgroup, batches narrower than the grid -------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["lds", "global", "global_batches"])
def test_a_workgroup_places_three_queries_with_options(engine, loaded, path):
    """N = 2 G + G / 2 + 37 draws of reuse_ext_pool, ambiguity and both strands: every workgroup places a second query and half of them
    a third on tables (S, C, P, c) that the passes before must have left zero; "global_batches": batches G / 2 wide -- every launch
    narrower than the grid, a workgroup's slices carried from launch to launch."""
    c = xc.reuse_ext_pool()
    G = compute_units(engine) * (32 if path == "lds" else 4)
    draw = xc.reuse_ext_draw3(G)
    N = len(draw)
    assert N == 2 * G + G // 2 + 37
    once = c.expected(7, True, "both")
    want = [once[d] for d in draw]
    step = G // 2 if path == "global_batches" else G                          # queries i - step and i are one workgroup's
    before = [once[int(draw[i - step])] for i in range(step, N)]
    assert sum(w["n_ambiguous"] > 0 for w in before) > len(before) // 2 and sum(w["strand"] == 1 for w in before) > len(before) // 16
    if path != "lds":
        engine.set_option("place_lds_branches", 16)
    if path == "global_batches":
        engine.set_option("place_batch_queries", G // 2)
        assert 0 < N % (G // 2) < G // 2
    res = place(engine, loaded("main_ext_case"), c, True, "both", queries=[c.queries[d] for d in draw])
    xo.check(res, want)


# ---- the host side with the window tables under a budget ---------------------------------------------------------------------------------------

def test_budgeted_slices_ext(tmp_path):
    """200 queries on the global tables (B = 70 001, b_pad = 70 016) with ambiguity and both strands under device_budget_bytes = held +
    64 MB.  A workgroup's slice of S, C and the touched list is 12 x 70 016 = 840 192 bytes, its slice of P, c and the window's list
    16 x 70 016 = 1 120 256 bytes.  The rule of db_place.hpp: a batch grows while the growth of the window tables (a sixteenth on top)
    stays within half of what is free -- 28 queries; then 28 slices of S / C (half of 64 MB holds 39), then half of what is left holds
    19 slices of P / c: 19 workgroups place the first 28 queries (tests/test_place_ext_paths_inputs.py::test_budget_ext_arithmetic
    restates the rule for every batch).  The launch is narrower than the batch, the results are the oracle's and, bit for bit, those
    of the run without a budget, and the peak stays within the budget."""
    c = xc.big_branch_ext_case()
    draw = xc.big_branch_ext_draw()
    queries = [c.queries[d] for d in draw]
    once = c.expected(7, True, "both")
    want = [once[d] for d in draw]
    eng = ipk_amd.Engine(0)
    try:
        db = eng.load_db(pc.write_case_db(tmp_path / "big_ext.ipk", c))
        held, _ = eng.mem_stats(reset_peak=True)
        budget = held + (64 << 20)
        eng.set_option("device_budget_bytes", budget)
        try:
            tight = place(eng, db, c, True, "both", queries=queries)
            peak = eng.mem_stats()[1]
        finally:
            eng.set_option("device_budget_bytes", 0)
        xo.check(tight, want)
        print(f"budgeted slices: held {held}, peak {peak}, budget {budget}")
        assert held < peak <= budget and peak - held < 200 * 28 * 70016
        free = place(eng, db, c, True, "both", queries=queries)              # no budget: a slice of each table per query
        xo.check(free, want)
        same_ext_bits(tight, free)
        assert eng.mem_stats()[0] - held >= 200 * 28 * 70016
    finally:
        eng.close()


@pytest.mark.parametrize("path", ["lds", "global"])
def test_budgeted_batches_split_ext(tmp_path, path):
    """The 1500 queries of pc.budget_draw() mapped onto reuse_ext_pool, ambiguity and both strands, under device_budget_bytes = held +
    256 KB: the window tables (5120 bytes a workgroup) are sized with every batch, and on the global tables the slices of S and C share
    the same room.  No refusal for a call that fits; the oracle's results and, bit for bit, those of the run without a budget."""
    c = xc.reuse_ext_pool()
    draw = xc.budget_ext_draw()
    queries = [c.queries[d] for d in draw]
    once = c.expected(7, True, "both")
    want = [once[d] for d in draw]
    eng = ipk_amd.Engine(0)
    try:
        if path == "global":
            eng.set_option("place_lds_branches", 16)
        db = eng.load_db(pc.write_case_db(tmp_path / "main_ext.ipk", c))
        xo.check(place(eng, db, c, True, "both", queries=queries[:1]), want[:1])      # the index is built and kept outside the budget
        held, _ = eng.mem_stats(reset_peak=True)
        budget = held + pc.BUDGET_ROOM
        eng.set_option("device_budget_bytes", budget)
        try:
            tight = place(eng, db, c, True, "both", queries=queries)         # (IpkGpuError code 3 here: a refusal of a call that fits)
            peak = eng.mem_stats()[1]
        finally:
            eng.set_option("device_budget_bytes", 0)
        xo.check(tight, want)
        print(f"budgeted batches ({path}): held {held}, peak {peak}, budget {budget}")
        assert held < peak <= budget
        free = place(eng, db, c, True, "both", queries=queries)              # no budget: one batch
        same_ext_bits(tight, free)
    finally:
        eng.close()


# ---- the rounding ladder ---------------------------------------------------------------------------------------------------------------------

def test_rounding_ladder(engine, loaded):
    """One window, one resolution a key with the one score x: the placement's score is (float)log10((10^x + (R - 1) E) / R) and nothing
    else.  x from xc.LADDER: y lies 2^rung .. 2^(rung + 1) from a binary32 rounding midpoint.  The expected bits are the 60-digit
    value's.  Rungs -36 .. -44 (d >= 2^-44, the margin tests/test_place_ext_inputs.py keeps every other input at) are asserted on
    both table paths; the finer ones are placed and reported (profiles/place_ext_paths.txt has the table)."""
    c = xc.ladder_case()
    inputs = xc.ladder_inputs()
    got = {}
    for path in ("lds", "global"):
        engine.set_option("place_lds_branches", 16 if path == "global" else 0)
        res = place(engine, loaded("ladder_case"), c, True, "given", keep=1)
        assert res.n_branches.tolist() == [1] * len(inputs) and res.branches[:, 0].tolist() == [i % 50 for i in range(len(inputs))]
        assert res.n_ambiguous.tolist() == [1] * len(inputs) and res.counts[:, 0].tolist() == [1] * len(inputs)
        got[path] = res.scores[:, 0].view(np.uint32) == c.want_bits
    print("rung  R  inputs  correctly rounded (lds)  (global)")
    wrong = []
    for R in sorted(xc.LADDER):
        for rung in sorted(xc.LADDER[R], reverse=True):
            at = [i for i, (r, g, _) in enumerate(inputs) if (r, g) == (R, rung)]
            print(f"{rung:4d}  {R}  {len(at):6d}  {int(got['lds'][at].sum()):23d}  {int(got['global'][at].sum()):8d}")
            if rung >= xc.LADDER_ASSERTED_FROM:
                wrong += [(path, R, rung, hex(int(inputs[i][2].view(np.uint32)))) for path in got for i in at if not got[path][i]]
    assert not wrong, wrong
