"""Host checks of the selection's test inputs (tests/select_cases.py): every case has the property it is named for, the numpy
restatement does what the definition says on inputs small enough to check by hand, ipkgpu_db_mu_kmers agrees with its formula, and
the definition's reason for being -- raising omega without a rebuild -- holds for the CPU oracle on the build-equivalence input."""
import math

import numpy as np
import pytest

from ipk_amd import engine as E
from oracle import ipk_oracle as co
from tests import db_files as F
from tests import select_cases as S


def counts_of(db):
    return (db["off"][1:] - db["off"][:-1]).astype(np.int64)


def test_restatement_by_hand():
    """Four keys; record order 2, 0, 3, 1.  M = 3 leaves key 1 out; t = -2 drops key 0's second entry and all of key 3."""
    db = dict(keys=np.array([10, 20, 30, 40], np.uint32), off=np.array([0, 2, 3, 5, 6], np.uint64), br=np.array([1, 2, 3, 4, 5, 6], np.uint32),
              sc=np.array([-1.0, -2.0, -0.5, -1.5, -np.nan, -2.5], np.float32), pos=np.array([7, 8, 9, 10, 11, 12], np.uint32),
              fv=np.array([0.5, 0.75, 0.25, 0.625], np.float32), order=np.array([2, 0, 3, 1], np.uint32))
    v = S.restate(db, 3, -2.0)
    assert v["keys"].tolist() == [10, 30] and v["off"].tolist() == [0, 1, 2]
    assert v["br"].tolist() == [1, 4] and v["sc"].tolist() == [-1.0, -1.5] and v["pos"].tolist() == [7, 10]      # (the NaN score fails, -2.0 > -2.0 fails)
    assert v["fv"].tolist() == [0.5, 0.25] and v["order"].tolist() == [1, 0]
    everything = S.restate(db, 1 << 40, -np.inf)
    assert everything["keys"].tolist() == [10, 20, 30, 40] and everything["br"].tolist() == [1, 2, 3, 4, 6]     # (only the NaN entry fails > -inf)
    assert S.restate(db, 0, -np.inf)["keys"].size == 0 and S.restate(db, 4, np.inf)["off"].tolist() == [0]
    one = S.restate(db, 1, -np.inf)
    assert one["keys"].tolist() == [30] and one["order"].tolist() == [0] and one["br"].tolist() == [4]          # M counts before the entries are looked at


def test_identity_on_the_edge_case():
    db = S.edges()
    assert S.same_arrays(S.restate(db, 200, -np.inf), db)
    assert S.same_arrays(S.restate(db, 1 << 40, S.T_LOW), db)                    # -7 is below every score
    assert db["sc"].min() > S.T_LOW


def test_edges_have_their_properties():
    db = S.edges()
    cnt, off, sc = counts_of(db), db["off"], db["sc"]
    assert sorted(cnt[np.isin(cnt, F.EDGE_COUNTS)].tolist())[-1] == 3000 and set(F.EDGE_COUNTS) <= set(cnt.tolist())
    j = S.long_key(db)
    assert cnt[j] == 3000 and int(off[j]) % S.TILE != 0 and int(off[j]) // S.TILE + 2 <= (int(off[j + 1]) - 1) // S.TILE   # starts inside a tile, spans whole ones
    assert int(off[-1]) > 3 * S.TILE                                              # several workgroups
    # the all-fail key between two all-pass keys
    lo, mid, hi = (sc[int(off[k]):int(off[k + 1])] for k in (S.SANDWICH - 1, S.SANDWICH, S.SANDWICH + 1))
    assert len(lo) and len(mid) and len(hi) and (lo > S.T_MID).all() and (hi > S.T_MID).all() and not (mid > S.T_MID).any()
    v = S.restate(db, 200, S.T_MID)
    assert db["keys"][S.SANDWICH] not in v["keys"] and db["keys"][S.SANDWICH - 1] in v["keys"] and db["keys"][S.SANDWICH + 1] in v["keys"]
    # the score whose bits equal t fails, the next float passes
    a, t = S.exact_entry(db), S.t_exact(db)
    assert sc[a].view(np.uint32) == t.view(np.uint32) and sc[a + 1].view(np.uint32) == t.view(np.uint32) - 1 and sc[a + 1] > t
    ve = S.restate(db, 200, t)
    kept = set(zip(ve["br"].tolist(), ve["sc"].view(np.uint32).tolist()))
    assert (int(db["br"][a + 1]), int(sc[a + 1].view(np.uint32))) in kept and (int(db["br"][a]), int(sc[a].view(np.uint32))) not in kept
    # every threshold of the grid changes the result, and some keys are dropped only for M
    sizes = [len(S.restate(db, 200, t)["br"]) for t in S.t_grid(db)]
    assert sizes[0] == sizes[1] == len(sc) and sizes[1] > sizes[2] > 0 and sizes[2] != sizes[3] and sizes[4] == 0
    assert [len(S.restate(db, m, -np.inf)["keys"]) for m in S.M_GRID] == [0, 1, 2, 199, 200, 200, 200]
    assert len(S.restate(db, 199, S.T_MID)["keys"]) < 199


def test_heavy_single_and_equal_filter_values():
    db, t = S.heavy()
    cnt = counts_of(db)
    assert sorted(cnt.tolist())[-2:] == [1, 5000] and len(cnt) == 3001 and len(set(db["br"][int(db["off"][1700]):int(db["off"][1701])].tolist())) == 5000
    v = S.restate(db, 3001, t)
    assert 0.4 < len(v["br"]) / len(db["br"]) < 0.6 and len(v["keys"]) < 3001
    assert S.single()["keys"].tolist() == [201] and counts_of(S.single()).tolist() == [3]
    eq = S.equal_fv()
    assert len(set(eq["fv"].tolist())) == 3 and len(eq["fv"]) == 50
    for a, b in zip(eq["order"][:-1], eq["order"][1:]):                           # ascending (filter value, key): ties by key
        assert (eq["fv"][a], eq["keys"][a]) < (eq["fv"][b], eq["keys"][b])
    v = S.restate(eq, 25, -np.inf)
    assert len(v["keys"]) == 25 and sorted(v["order"].tolist()) == list(range(25)) and np.array_equal(v["keys"][v["order"]], eq["keys"][eq["order"][:25]])


@pytest.mark.parametrize("n", [1, 7, 200, 10 ** 9 + 7, (1 << 32) - 1])
def test_mu_kmers(n):
    for mu in (0.0, 1.0 / n, 0.5, 1.0 - 1.0 / n, 1.0):
        assert E.mu_kmers(mu, n) == min(n, int(math.ceil(mu * float(n)))), (mu, n)
    assert E.mu_kmers(0.0, n) == 0 and E.mu_kmers(1.0, n) == n and E.mu_kmers(1.0 / n, n) >= 1
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            E.mu_kmers(bad, n)


def test_oracle_at_a_higher_omega_is_the_selection_of_the_lower_one():
    """oracle(omega2) == restatement(oracle(omega1), all, log_eps(omega2)): key for key, score bit for score bit, entry order included."""
    mats = S.build_mats()
    e1, e2 = (co.log_threshold(w, S.BUILD_SIGMA, S.BUILD_K) for w in S.BUILD_OMEGAS)
    d1, d2 = S.oracle_db(mats, e1), S.oracle_db(mats, e2)
    assert 0 < len(d2["br"]) < len(d1["br"]) and 0 < len(d2["keys"]) < len(d1["keys"])
    v = S.restate(d1, len(d1["keys"]), e2, positioned=False)
    assert np.array_equal(v["keys"], d2["keys"]) and np.array_equal(v["off"], d2["off"])
    assert np.array_equal(v["br"], d2["br"]) and np.array_equal(v["sc"].view(np.uint32), d2["sc"].view(np.uint32))
    assert S.entry_sets(v) == S.entry_sets(d2)


@pytest.mark.parametrize("omega", [1.1, 1.3, 1.6, 1.7, 1.5, 1.8])
def test_the_files_own_omega_is_not_below_it(tmp_path, omega):
    """The file keeps omega as binary32; 1.1, 1.6 and 1.7 round UP there (1.7 -> 1.70000005), 1.3 and 1.8 down, 1.5 is exact.  The build's own decimal is the
    file's omega, not a value below it: both refusals compare in binary32.  One float32 step lower is refused."""
    import click
    from ipk_amd import cli, dbfile
    if omega in (1.1, 1.6, 1.7):
        assert float(np.float32(omega)) > omega
    path = F.write(tmp_path / "w.ipk", F.synthetic(20, seed=3), header=dict(F.HEADER, omega=omega))
    head = dbfile.file_info(path)
    assert head["omega"] == float(np.float32(omega))
    m, t = E._selection_args(head, 20, None, 0.5, None, omega)
    assert m == 10 and np.float32(t) == np.float32(E.log_threshold(omega, 4, F.HEADER["kmer_size"]))
    cli._check_selection(path, 0.5, omega)
    cli._check_selection(path, None, omega + 0.25)
    below = float(np.nextafter(np.float32(omega), np.float32(0)))
    with pytest.raises(ValueError, match="below the file's omega"):
        E._selection_args(head, 20, None, None, None, below)
    with pytest.raises(click.UsageError, match="below the file's omega"):
        cli._check_selection(path, None, below)
