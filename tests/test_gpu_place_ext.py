"""GPU suite: Engine.place with ambiguity=True and / or strands="both" (ipkgpu_db_place_opts) against the host restatement of its
definition (tests/place_ext_oracle.py).  Compared as tests/test_gpu_place.py compares: branches, order, score bits, counts and the
per-query figures exactly, lwr within po.lwr_tolerance -- and strand and n_ambiguous exactly.  tests/test_place_ext_inputs.py proves
on the host that the inputs (tests/place_ext_cases.py) have the properties named here, that four wrong implementations change their
expected results, and that every ambiguous contribution is far enough from a rounding midpoint for exp10 and log10 of the device."""
import numpy as np
import pytest

import ipk_amd
from tests import place_cases as pc
from tests import place_ext_cases as xc
from tests import place_ext_oracle as xo
from tests.test_gpu_place import default_options, same_bits                  # noqa: F401  (the fixture resets the options)
from tests.test_gpu_place_paths import compute_units

pytestmark = pytest.mark.gpu

CASE_MODES = [(n, a, s) for n, modes in xc.MODES.items() for a, s in modes]


@pytest.fixture(scope="module")
def loaded(engine, tmp_path_factory):
    """case name -> the case's database on the device (loaded once)."""
    d = tmp_path_factory.mktemp("place_ext")
    dbs = {}

    def get(name):
        if name not in dbs:
            dbs[name] = engine.load_db(pc.write_case_db(d / f"{name}.ipk", xc.ALL_CASES[name]()))
        return dbs[name]
    yield get
    for db in dbs.values():
        db.free()


def place(engine, db, case, ambiguity, strands, keep=7, queries=None):
    return engine.place(db, case.queries if queries is None else queries, keep_at_most=keep, sigma=case.sigma, k=case.k, log_eps=xc.LOG_EPS,
                        ambiguity=ambiguity, strands=strands)


def same_ext_bits(a, b):
    same_bits(a, b)
    assert np.array_equal(a.strand, b.strand) and np.array_equal(a.n_ambiguous, b.n_ambiguous)


@pytest.mark.parametrize("name,ambiguity,strands", CASE_MODES)
def test_cases_on_every_path(engine, loaded, name, ambiguity, strands):
    """Every case and mode on the LDS tables, on the global tables ("place_lds_branches" = 16: the same bits) and one query a batch."""
    c = xc.ALL_CASES[name]()
    want = c.expected(7, ambiguity, strands)
    lds = place(engine, loaded(name), c, ambiguity, strands)
    assert lds.strand.dtype == np.uint8 and lds.n_ambiguous.dtype == np.uint32 and lds.strand.shape == (len(want),)
    xo.check(lds, want)
    engine.set_option("place_lds_branches", 16)
    glob = place(engine, loaded(name), c, ambiguity, strands)
    xo.check(glob, want)
    same_ext_bits(lds, glob)
    engine.set_option("place_lds_branches", 0)
    engine.set_option("place_batch_queries", 1)
    same_ext_bits(lds, place(engine, loaded(name), c, ambiguity, strands))
    if ambiguity:
        assert int(lds.n_ambiguous.sum()) > 0
    if name == "strand_case":
        assert set(lds.strand.tolist()) == {0, 1}


def test_all_placements_of_the_main_case(engine, loaded):
    """keep_at_most = 64: every planted branch's score and count, not only the best seven."""
    c = xc.main_ext_case()
    xo.check(place(engine, loaded("main_ext_case"), c, True, "both", keep=64), c.expected(64, True, "both"))
    c = xc.strand_case()
    xo.check(place(engine, loaded("strand_case"), c, True, "both", keep=64), c.expected(64, True, "both"))


def test_branch_id_70000_under_ambiguous_windows(engine, loaded):
    c = xc.big_branch_ext_case()
    assert c.db[2].max() == 70000
    want = c.expected(64, True, "given")
    assert any(70000 in [p[0] for p in w["placements"]] for w in want) and want[0]["n_ambiguous"] == xc.K
    xo.check(place(engine, loaded("big_branch_ext_case"), c, True, "given", keep=64), want)


@pytest.mark.parametrize("path", ["lds", "global"])
def test_a_workgroup_places_queries_after_ambiguous_and_reverse_passes(engine, loaded, path):
    """2 G + 37 short queries on a grid G wide: every workgroup places a second query and some a third on the tables (S, C, P, c) that
    an ambiguous window and a reverse-strand pass before them must have left zero."""
    c = xc.reuse_ext_pool()
    G = compute_units(engine) * (32 if path == "lds" else 4)
    draw = xc.reuse_ext_draw(G)
    assert len(draw) == 2 * G + 37
    once = c.expected(7, True, "both")
    want = [once[d] for d in draw]
    later = [once[int(draw[i - G])] for i in range(G, len(draw))]
    assert sum(w["n_ambiguous"] > 0 for w in later) > G // 2 and sum(w["strand"] == 1 for w in later) > G // 16
    if path != "lds":
        engine.set_option("place_lds_branches", 16)
    res = place(engine, loaded("main_ext_case"), c, True, "both", queries=[c.queries[d] for d in draw])
    xo.check(res, want)


def test_no_options_is_engine_place(engine, loaded):
    """{0, 0} through ipkgpu_db_place_opts (ctypes, the options given as zeros and as NULL) equals Engine.place array for array."""
    import ctypes as C
    from ipk_amd import engine as E
    c = xc.main_ext_case()
    db = loaded("main_ext_case")
    plain = engine.place(db, c.queries, sigma=4, k=xc.K, log_eps=xc.LOG_EPS)
    assert not plain.strand.any() and not plain.n_ambiguous.any()
    raw = [s.encode() for s in c.queries]
    off = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.uint64)
    data = np.frombuffer(b"".join(raw), np.uint8)
    for opts in (C.byref(E._PlaceOptions(0, 0)), None):
        out = C.c_void_p()
        rc = engine._lib.ipkgpu_db_place_opts(engine._h, db._h, 4, xc.K, C.c_float(xc.LOG_EPS), data.ctypes.data, off.ctypes.data, len(raw), 7,
                                              opts, C.byref(out))
        assert rc == 0
        try:
            res = E.Placements(engine._lib, out)
        finally:
            engine._lib.ipkgpu_placements_free(out)
        same_ext_bits(plain, res)
    # and the options change what they are for: N is no longer an invalid byte
    assert place(engine, db, c, True, "given").n_kmers.sum() > plain.n_kmers.sum()


def test_the_reverse_strand_is_the_placement_of_the_reversed_string(engine, loaded):
    c = xc.strand_case()
    db = loaded("strand_case")
    for ambiguity in (False, True):
        both = place(engine, db, c, ambiguity, "both")
        given = place(engine, db, c, ambiguity, "given")
        rev = place(engine, db, c, ambiguity, "given", queries=[xo.revcomp(s) for s in c.queries])
        assert both.strand.sum() >= 6
        for i in range(both.n):
            src = rev if both.strand[i] else given
            for name in ("branches", "counts", "lwr"):
                assert np.array_equal(getattr(both, name)[i], getattr(src, name)[i]), (i, name)
            assert np.array_equal(both.scores[i].view(np.uint32), src.scores[i].view(np.uint32))
            assert (both.n_kmers[i], both.n_found[i], both.n_branches[i], both.n_ambiguous[i]) == \
                   (src.n_kmers[i], src.n_found[i], src.n_branches[i], src.n_ambiguous[i])


def test_refusals(engine, loaded):
    import ctypes as C
    from ipk_amd import engine as E
    c = xc.aa_ext_case(3)
    with pytest.raises(ipk_amd.IpkGpuError) as ei:
        place(engine, loaded("aa3_ext_case"), c, True, "both")
    assert ei.value.code == 1 and "DNA" in str(ei.value)
    with pytest.raises(ValueError):
        place(engine, loaded("aa3_ext_case"), c, True, "reverse")
    m = xc.main_ext_case()
    db = loaded("main_ext_case")
    data = np.frombuffer(b"ACGTACGTAC", np.uint8)
    off = np.array([0, 10], np.uint64)
    for a, s in ((2, 0), (0, 2), (1, 7)):
        out = C.c_void_p()
        opts = E._PlaceOptions(a, s)
        rc = engine._lib.ipkgpu_db_place_opts(engine._h, db._h, 4, xc.K, C.c_float(xc.LOG_EPS), data.ctypes.data, off.ctypes.data, 1, 7, C.byref(opts),
                                              C.byref(out))
        assert rc == 1 and not out.value
    for keep in (0, 65):                                          # the refusals of ipkgpu_db_place carry over
        with pytest.raises(ipk_amd.IpkGpuError):
            place(engine, db, m, True, "both", keep=keep)
    with pytest.raises(ipk_amd.IpkGpuError):
        engine.place(db, m.queries, sigma=4, k=7, log_eps=xc.LOG_EPS, ambiguity=True)
    xo.check(place(engine, db, m, True, "both"), m.expected(7, True, "both"))
