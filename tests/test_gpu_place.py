"""GPU suite: Engine.place (ipkgpu_db_place) against the host restatement of its definition (tests/place_oracle.py).

Compared in every case: branches, their order, score bits and counts bit for bit; n_kmers, n_found, n_branches exactly; lwr within a
relative error of 64 (T + 1) 2^-53 for a query with T scored branches: the denominator is a sum, in any order, of T non-negative
doubles that is at least 1 ((T - 1) 2^-53); a term 10^x, x <= 0, is within 16 ulp of the device's function plus the rounding of its
argument (3.4 |x| 2^-53 relative, and 10^x |x| <= 0.16), so 64 covers term, sum and quotient with room to spare.

Databases are fabricated (tests/place_cases.py), written with dbfile.write_db and loaded with Engine.load_db unless a test says
otherwise."""
import numpy as np
import pytest

import ipk_amd
from ipk_amd import dbfile
from ipk_amd.engine import PLACE_NONE
from tests import place_cases as pc
from tests import place_oracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def loaded(engine, tmp_path_factory):
    """case name -> the case's database on the device (loaded once)."""
    d = tmp_path_factory.mktemp("place")
    dbs = {}

    def get(name):
        if name not in dbs:
            dbs[name] = engine.load_db(pc.write_case_db(d / f"{name}.ipk", getattr(pc, name)()))
        return dbs[name]
    yield get
    for db in dbs.values():
        db.free()


@pytest.fixture(autouse=True)
def default_options(engine):
    yield
    engine.set_option("place_lds_branches", 0)
    engine.set_option("place_batch_queries", 0)


def place(engine, db, case, keep=7, queries=None):
    return engine.place(db, case.queries if queries is None else queries, keep_at_most=keep, sigma=case.sigma, k=case.k, log_eps=pc.LOG_EPS)


def same_bits(a, b):
    for name in ("branches", "counts", "n_kmers", "n_found", "n_branches"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(a.scores.view(np.uint32), b.scores.view(np.uint32))
    assert np.array_equal(a.lwr, b.lwr)                       # (both paths walk the touched branches in one order)


def test_main_case(engine, loaded):
    """DNA k = 8, 64 queries: 0, 1, 2, 63, 64, 65, 66 and more windows, lower case and U, runs of N, repeated and absent k-mers, the
    first and the last key; keys of 63, 64, 65 and 129 entries."""
    c = pc.main_case()
    res = place(engine, loaded("main_case"), c)
    assert res.keep == 7 and res.branches.shape == (64, 7) and res.lwr.dtype == np.float64
    po.check(res, c.expected(7))
    assert res.time_ms["place"] > 0 and res.time_ms["total"] >= res.time_ms["place"]


def test_window_order_not_another(engine, loaded):
    """The order-sensitivity case (tests/test_place_inputs.py proves on the host that reversed window order changes its sums)."""
    c = pc.order_case()
    po.check(place(engine, loaded("main_case"), c), c.expected(7))


@pytest.mark.parametrize("name", ["aa_case", "k16_case", "k2_case", "one_key_case", "empty_case"])
def test_other_alphabets_and_sizes(engine, loaded, name):
    """AA k = 6 (30-bit codes, a key of the last letter throughout), DNA k = 16 (keys 0, 0x80000000, 0xFFFFFFFF), DNA k = 2 (all 16
    keys), one key, no key (every query then has no placement)."""
    c = getattr(pc, name)()
    res = place(engine, loaded(name), c)
    po.check(res, c.expected(7))
    if name == "empty_case":
        assert (res.branches == PLACE_NONE).all() and (res.n_found == 0).all() and res.n_kmers.tolist() == [1, 93, 0, 0]
    if name == "k16_case":
        assert {0, 0x80000000, 0xFFFFFFFF} <= set(c.db[0].tolist()) and res.n_found[:3].tolist() == [1, 1, 1]


def test_no_queries(engine, loaded):
    res = place(engine, loaded("main_case"), pc.main_case(), queries=[])
    assert res.n == 0 and res.branches.shape == (0, 7) and res.n_kmers.shape == (0,)


def test_defaults_come_from_the_loaded_file(engine, loaded):
    """sigma, k and the threshold of a loaded database: its header's (omega 1.5 -> log_threshold(1.5, 4, 8))."""
    c = pc.one_key_case()
    res = engine.place(loaded("one_key_case"), c.queries)
    po.check(res, po.place(c.view, c.queries, 4, 8, ipk_amd.log_threshold(1.5, 4, 8), 7))


def test_branch_id_70000_uses_the_global_tables(engine, loaded):
    c = pc.big_branch_case()
    assert c.db[2].max() == 70000
    res = place(engine, loaded("big_branch_case"), c)
    po.check(res, c.expected(7))
    assert any(70000 in [p[0] for p in po.place_one(c.view, q, 4, 8, pc.LOG_EPS, 64)["placements"]] for q in c.queries)
    po.check(place(engine, loaded("big_branch_case"), c, keep=64), c.expected(64))


def test_global_tables_give_the_lds_path_its_bits(engine, loaded):
    """The main case again with "place_lds_branches" = 16: 300 branches then live in the global tables."""
    c = pc.main_case()
    lds = place(engine, loaded("main_case"), c)
    engine.set_option("place_lds_branches", 16)
    assert engine.get_option("place_lds_branches") == 16
    glob = place(engine, loaded("main_case"), c)
    po.check(glob, c.expected(7))
    same_bits(lds, glob)
    o = pc.order_case()
    po.check(place(engine, loaded("main_case"), o), o.expected(7))


@pytest.mark.parametrize("keep", [1, 7, 64])
def test_top_n(engine, loaded, keep):
    """A query touching 100 branches, branches 11 and 57 with identical entries (equal scores: 11 first); queries with fewer
    branches than keep_at_most end in 0xFFFFFFFF."""
    c = pc.topn_case()
    want = c.expected(keep)
    assert want[0]["n_branches"] == 100
    res = place(engine, loaded("topn_case"), c, keep=keep)
    po.check(res, want)
    if keep == 64:
        row = res.branches[0].tolist()
        i = row.index(11)
        assert row[i + 1] == 57 and res.scores[0, i].view(np.uint32) == res.scores[0, i + 1].view(np.uint32)
        assert res.n_branches[2] == 37 and (res.branches[2, 37:] == PLACE_NONE).all() and (res.lwr[2, 37:] == 0).all()
    for path in (16,):                                            # the same selection over the global tables
        engine.set_option("place_lds_branches", path)
        same_bits(res, place(engine, loaded("topn_case"), c, keep=keep))


def test_batches_give_identical_results(engine, loaded):
    c = pc.main_case()
    auto = place(engine, loaded("main_case"), c)
    for n in (1, 5):
        engine.set_option("place_batch_queries", n)
        same_bits(auto, place(engine, loaded("main_case"), c))
    engine.set_option("place_lds_branches", 16)
    same_bits(auto, place(engine, loaded("main_case"), c))       # five queries a batch over the global tables


def test_refusals(engine, loaded, tmp_path):
    c = pc.main_case()
    good = loaded("main_case")
    # one branch twice under one key
    keys, off = np.array([3, 77, 4000], np.uint32), np.array([0, 2, 70, 73], np.uint64)
    br = np.concatenate([[5, 9], np.arange(68), [1, 2, 3]]).astype(np.uint32)
    br[2 + 66] = br[2 + 1]                                           # key 77: branch 1 at places 1 and 66 (two lanes' tiles apart)
    path = tmp_path / "dup.ipk"
    dbfile.write_db(path, "DNA", [(1, 0.0)], "(a:1,b:1)r;", 8, 1.5, keys, off, br, np.full(len(br), -1.0, np.float32), np.zeros(3, np.float32),
                    np.arange(3, dtype=np.uint32))
    bad = engine.load_db(path)
    try:
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            engine.place(bad, ["ACGTACGTAC"])
        assert ei.value.code == 1 and "key 77" in str(ei.value) and "more than once" in str(ei.value)
        with pytest.raises(ipk_amd.IpkGpuError):                     # and again: the refused database got no index
            engine.place(bad, ["ACGTACGTAC"])
    finally:
        bad.free()
    for keep in (0, 65):
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            place(engine, good, c, keep=keep)
        assert ei.value.code == 1 and "keep_at_most" in str(ei.value)
    for sigma, k in ((20, 8), (20, 6), (4, 7), (5, 8)):
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            engine.place(good, c.queries, sigma=sigma, k=k, log_eps=pc.LOG_EPS)
        assert ei.value.code == 1
    with pytest.raises(ipk_amd.IpkGpuError):
        engine.set_option("place_lds_branches", 4097)
    # the context and the good database are as usable as before
    po.check(place(engine, good, c), c.expected(7))


def test_a_database_built_here_without_a_file(engine):
    """synth -> score_groups_keymajor -> db_from_parts -> place: 24 reads of 60 symbols, each cut from the most probable sequence of a
    group's first matrix, land on their group's branch."""
    from ipk_amd.synth import synth_matrices
    k, sigma, n_groups, sites = 8, 4, 12, 200
    mats = synth_matrices(2 * n_groups, sites, sigma, 0.05, 4242)
    groups = np.repeat(np.arange(n_groups, dtype=np.uint32) * 3 + 5, 2)
    eps = ipk_amd.log_threshold(1.5, sigma, k)
    parts = engine.score_groups_keymajor(mats, groups, k, eps, n_owners=1)
    db = engine.db_from_parts(parts, sigma, k)
    try:
        rng = np.random.default_rng(9)
        reads, origin = [], []
        for i in range(24):
            g = i % n_groups
            best = "".join("ACGT"[j] for j in mats[2 * g].argmax(axis=1))
            s = int(rng.integers(0, sites - 60 + 1))
            reads.append(best[s:s + 60]); origin.append(int(groups[2 * g]))
        br, sc = db.entries()
        view = po.DbView(db.keys(), db.key_offsets(), br, sc)
        want = po.place(view, reads, sigma, k, eps, 7)
        # the oracle first: the synthetic columns are concentrated enough that a read's own branch wins
        assert [w["placements"][0][0] for w in want] == origin
        res = engine.place(db, reads, sigma=sigma, k=k, log_eps=eps)
        po.check(res, want)
        assert res.branches[:, 0].tolist() == origin
        with pytest.raises(ValueError):
            engine.place(db, reads)                                  # no file, no defaults
    finally:
        db.free(); parts.free()
