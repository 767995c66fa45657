"""GPU suite: the positioned key-major database (ipkgpu_score_groups_keymajor_positions_device) -- one scoring pass on the device,
every entry carrying the start of the first window that reached its score -- against oracle/ipk_oracle.py::explore_group_pos.
All comparisons are exact: keys, offsets, branch ids, raw score bits, positions."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ipk_amd
from ipk_amd import dbfile
from ipk_amd import engine as E
from ipk_amd.synth import synth_matrices
from oracle import ipk_oracle as co

pytestmark = pytest.mark.gpu


def oracle_positions_db(mats, groups, k, eps, threads=1):
    """Key-major database of explore_group_pos per group: (keys, offsets, branches, score bits, positions, emitted)."""
    groups = np.asarray(groups, dtype=np.uint32)
    order = list(dict.fromkeys(groups.tolist()))

    def one(gid):
        return co.explore_group_pos(mats[groups == gid], k, eps)
    if threads > 1:
        with ThreadPoolExecutor(max_workers=min(16, threads)) as ex:
            res = list(ex.map(one, order))
    else:
        res = [one(g) for g in order]
    keys = np.concatenate([r[0] for r in res]) if res else np.zeros(0, np.uint32)
    bits = np.concatenate([r[1].view(np.uint32) for r in res])
    pos = np.concatenate([r[2] for r in res])
    br = np.concatenate([np.full(len(r[0]), gid, dtype=np.uint32) for gid, r in zip(order, res)])
    idx = np.argsort(keys, kind="stable")                       # key-major, groups in first-seen order inside a key
    ukeys, counts = np.unique(keys, return_counts=True)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return ukeys.astype(np.uint32), off, br[idx], bits[idx], pos[idx], sum(r[3] for r in res)


def positioned(engine, mats, groups, k, eps):
    """The new call's database as host arrays: (keys, offsets, branches, score bits, positions, emitted, launches)."""
    sigma = mats.shape[2]
    parts = engine.score_groups_keymajor_positions(mats, np.asarray(groups, dtype=np.uint32), k, eps)
    from_parts = parts.positions_tensor().cpu().numpy().view(np.uint32).copy()
    launches = parts.time_ms(E.T_SCORE_LAUNCHES)
    db = engine.db_from_parts(parts, sigma, k)
    br, sc = db.entries()
    pos = db.positions().copy()
    assert np.array_equal(pos, from_parts), "the positions did not move into the database with the entries"
    out = (db.keys().copy(), db.key_offsets().copy(), br, sc.view(np.uint32), pos, parts.emitted, launches)
    db.free(); parts.free()
    return out


def plain(engine, mats, groups, k, eps):
    sigma = mats.shape[2]
    parts = engine.score_groups_keymajor(mats, np.asarray(groups, dtype=np.uint32), k, eps)
    db = engine.db_from_parts(parts, sigma, k)
    br, sc = db.entries()
    assert db.positions() is None
    out = (db.keys().copy(), db.key_offsets().copy(), br, sc.view(np.uint32))
    db.free(); parts.free()
    return out


def assert_same(got, want, what=("keys", "offsets", "branches", "score bits", "positions")):
    for g, w, name in zip(got, want, what):
        assert len(g) == len(w), f"{name}: {len(g)} against {len(w)}"
        assert np.array_equal(g, w), f"{name} differ (first at {int(np.flatnonzero(np.asarray(g) != np.asarray(w))[0])})"


def check(engine, mats, groups, k, eps, threads=1):
    want = oracle_positions_db(mats, groups, k, eps, threads)
    got = positioned(engine, mats, groups, k, eps)
    assert_same(got[:5], want[:5])
    assert got[5] == want[5], "scored phylo-k-mer count differs"
    return got


GEOMETRIES = [(20, 6, 14), (20, 5, 20), (20, 3, 30), (4, 8, 90), (4, 4, 60), (4, 10, 150), (4, 12, 40), (4, 13, 30), (4, 14, 24)]


@pytest.mark.parametrize("sigma,k,sites", GEOMETRIES)
def test_oracle_parity(engine, sigma, k, sites):
    """1. every variant of the key geometry; interleaved matrices, one single-matrix group."""
    mats = synth_matrices(5, sites, sigma, 0.1, 70 + k)
    groups = np.array([4, 9, 4, 9, 2], dtype=np.uint32)
    check(engine, mats, groups, k, co.log_threshold(1.5, sigma, k))


@pytest.mark.parametrize("sigma,k,sites", GEOMETRIES)
def test_same_set_as_the_plain_call(engine, sigma, k, sites):
    """2. keys, offsets and entries bit-equal to score_groups_keymajor + db_from_parts: the position only rides along."""
    mats = synth_matrices(5, sites, sigma, 0.1, 70 + k)
    groups = np.array([4, 9, 4, 9, 2], dtype=np.uint32)
    eps = co.log_threshold(1.5, sigma, k)
    assert_same(positioned(engine, mats, groups, k, eps)[:4], plain(engine, mats, groups, k, eps))


def test_ties_and_order(engine):
    """3. equal score bits keep the window processed first; a strictly larger score in the second matrix takes its start."""
    col = np.log10(np.array([0.4, 0.3, 0.2, 0.1], dtype=np.float32))
    flat = np.tile(col, (2, 25, 1)).astype(np.float32)           # identical columns in both matrices of the group
    got = check(engine, flat, [0, 0], 6, co.log_threshold(1.0, 4, 6))
    assert len(got[4]) > 0 and np.all(got[4] == 0)
    # second matrix: one window (start 7) of sharper columns -- the k-mers it scores higher carry start 7, the rest stay at 0
    k, sigma = 6, 4
    second = flat[0].copy()
    second[7:7 + k] = np.log10(np.array([0.7, 0.15, 0.1, 0.05], dtype=np.float32))
    mats = np.stack([flat[0], second]).astype(np.float32)
    eps = co.log_threshold(1.0, sigma, k)
    got = check(engine, mats, [5, 5], k, eps)
    first_only = positioned(engine, mats[:1], [5], k, eps)
    larger = ~np.isin(got[0], first_only[0]) | (got[3] != first_only[3][np.searchsorted(first_only[0], got[0]).clip(0, len(first_only[0]) - 1)])
    assert larger.any() and not larger.all()
    assert np.all(got[4][larger] > 0) and np.all(got[4][~larger] == 0)
    # equal bits in both matrices: the first matrix's start
    got = check(engine, np.stack([second, second]).astype(np.float32), [5, 5], k, eps)
    one = positioned(engine, second[None], [5], k, eps)
    assert np.array_equal(got[4], one[4])


@pytest.mark.parametrize("case", ["dna", "dna2", "aa", "aa2"])
def test_big_list_windows(engine, case):
    """4. windows whose half lists exceed the fast path: their positions come through score_overflow_xp_kernel."""
    if case.startswith("dna"):
        mats, k, eps = synth_matrices(2, 14, 4, 1.0, 9), 10, -9.0
        groups = [0, 0] if case == "dna2" else [0, 1]
    else:
        mats, k, eps = synth_matrices(2 if case == "aa2" else 1, 8, 20, 0.3, 11), 6, -9.5
        groups = [0, 0] if case == "aa2" else [0]
    check(engine, mats, groups, k, eps)


def test_batching_does_not_show():
    """5. several batches (merged) and several writer passes (more than 256 groups in a batch) give the one-batch result."""
    eng = ipk_amd.Engine(0)
    try:
        mats = synth_matrices(12, 40, 20, 0.05, 515)
        groups = np.repeat(np.arange(6, dtype=np.uint32) + 3, 2)
        eps = co.log_threshold(1.5, 20, 4)
        whole = check(eng, mats, groups, 4, eps)
        eng.set_option("workspace_bytes", 1 << 20)
        split = positioned(eng, mats, groups, 4, eps)
        assert split[6] > 1, "the small workspace did not split the call into batches"
        assert_same(split[:5], whole[:5])
        eng.set_option("workspace_bytes", 8 << 30)
        mats = synth_matrices(300, 10, 20, 0.03, 516)
        got = check(eng, mats, np.arange(300, dtype=np.uint32) + 11, 6, co.log_threshold(1.5, 20, 6))
        assert got[6] == 1
    finally:
        eng.close()


def test_no_dense_tables_and_shared_workspaces():
    """6. the input of test_positions_tables_fit_the_workspace (>= 3 launches on the dense 8-byte tables) takes ONE scoring launch;
    plain and positioned calls alternating on one context do not disturb each other, with every wait restored (debug_flags bit 6) too."""
    sigma, k = 20, 6
    mats = synth_matrices(12, 14, sigma, 0.03, 606)
    groups = np.repeat(np.arange(6, dtype=np.uint32) + 40, 2)
    eps = co.log_threshold(1.5, sigma, k)
    eng = ipk_amd.Engine(0)
    try:
        eng.set_option("workspace_bytes", int(1.2e9))
        got = check(eng, mats, groups, k, eps)
        assert got[6] == 1, f"{got[6]:.0f} scoring launches"
        a = plain(eng, mats, groups, k, eps)
        b = positioned(eng, mats, groups, k, eps)
        c = plain(eng, mats, groups, k, eps)
        d = positioned(eng, mats, groups, k, eps)
        assert_same(c, a); assert_same(d[:5], b[:5]); assert_same(b[:5], got[:5])
        eng.set_option("debug_flags", 64)
        assert_same(plain(eng, mats, groups, k, eps), a)
        assert_same(positioned(eng, mats, groups, k, eps)[:5], b[:5])
    finally:
        eng.close()


def cfg_share(name, n_groups):
    """The first n_groups groups of ipk_amd.synth.CONFIGS[name], matrices as bench.py builds them (matrix index = group * mats_per_group + i)."""
    from ipk_amd.synth import CONFIGS
    cfg = CONFIGS[name]
    mpg = cfg["mats_per_group"]
    mats = synth_matrices(n_groups * mpg, cfg["sites"], cfg["sigma"], cfg["alpha"], cfg["seed"], first_mat=0)
    groups = np.repeat(np.arange(n_groups, dtype=np.uint32), mpg)
    return mats, groups, cfg["k"], co.log_threshold(cfg["omega"], cfg["sigma"], cfg["k"])


@pytest.mark.parametrize("name", ["cfg4", "cfg3"])
def test_scale_share(engine, name):
    """7. a 4-group share at the benchmarked shapes (4 x 2 x 3000 sites AA k = 6; 4 x 2 x 10 000 sites DNA k = 12), full comparison."""
    mats, groups, k, eps = cfg_share(name, 4)
    check(engine, mats, groups, k, eps, threads=min(16, len(os.sched_getaffinity(0))))


def header_args(k):
    return ("AA", [(1, 0.0), (3, 0.5)], "(a,b);", k, 1.5)


def test_device_writer_matches_the_host_serialiser(engine, tmp_path):
    """8. ipkgpu_db_write on a positioned database == write_db_positions over its host arrays == the file of the earlier route
    (score_groups_positions joined to the plain database on the host)."""
    sigma, k = 20, 4
    mats = synth_matrices(6, 30, sigma, 0.05, 808)
    groups = np.array([4, 4, 5, 5, 6, 6], dtype=np.uint32)
    eps = co.log_threshold(1.5, sigma, k)
    parts = engine.score_groups_keymajor_positions(mats, groups, k, eps)
    db = engine.db_from_parts(parts, sigma, k)
    db.filter_mif0(engine, 7, ipk_amd.score_threshold(1.5, sigma, k))
    seq, tree_index, newick, kk, omega = header_args(k)
    dev = tmp_path / "dev.ipk"
    dbfile.write_db_device(engine, db, dev, seq, tree_index, newick, kk, omega)
    br, sc = db.entries()
    host = tmp_path / "host.ipk"
    dbfile.write_db_positions(host, seq, tree_index, newick, kk, omega, db.keys(), db.key_offsets(), br, sc, db.positions(),
                              db.filter_values(), db.filter_order())
    assert dev.read_bytes() == host.read_bytes()
    # the earlier route: a second, group-major scoring call with positions, joined entry by entry
    res = engine.score_groups_positions(mats, groups, k, eps)
    keys_db, off_db = db.keys(), db.key_offsets().astype(np.int64)
    entry_key = np.repeat(keys_db, np.diff(off_db))
    pos_old = np.empty(len(br), dtype=np.uint32)
    rk, rp = res.keys(), res.positions()
    for gi, gid in enumerate(res.group_ids.tolist()):
        a, b = int(res.offsets[gi]), int(res.offsets[gi + 1])
        sel = np.flatnonzero(br == gid)
        pos_old[sel] = rp[a:b][np.searchsorted(rk[a:b], entry_key[sel])]
    res.free()
    old = tmp_path / "old.ipk"
    dbfile.write_db_positions(old, seq, tree_index, newick, kk, omega, keys_db, db.key_offsets(), br, sc, pos_old, db.filter_values(),
                              db.filter_order())
    assert dev.read_bytes() == old.read_bytes()
    db.free(); parts.free()


def test_device_writer_refuses_positions_beyond_u16(engine, tmp_path):
    sigma, k = 4, 8
    mats = synth_matrices(1, 65700, sigma, 0.1, 809)
    parts = engine.score_groups_keymajor_positions(mats, [1], k, co.log_threshold(1.5, sigma, k))
    db = engine.db_from_parts(parts, sigma, k)
    assert int(db.positions().max()) > 65535
    db.filter_mif0(engine, 3, ipk_amd.score_threshold(1.5, sigma, k))
    out = tmp_path / "far.ipk"
    with pytest.raises(ipk_amd.IpkGpuError, match="65535"):
        dbfile.write_db_device(engine, db, out, "DNA", [(1, 0.0)], "(a);", k, 1.5)
    assert not out.exists()
    db.free(); parts.free()


def test_refusals(engine):
    """10. several owners, and a key space without an exact partition, are refused; the capped big lists of k = 13 fail loudly and the
    context stays right."""
    mats = synth_matrices(2, 40, 4, 0.1, 77)
    with pytest.raises(ipk_amd.IpkGpuError) as ei:
        engine.score_groups_keymajor_positions(mats, [3, 3], 8, co.log_threshold(1.5, 4, 8), n_owners=2)
    assert ei.value.code == 1
    with pytest.raises(ipk_amd.IpkGpuError) as ei:
        engine.score_groups_keymajor_positions(mats, [3, 3], 3, co.log_threshold(1.5, 4, 3))
    assert ei.value.code == 1
    flat = np.full((2, 14, 4), np.log10(0.25), dtype=np.float32)
    with pytest.raises(ipk_amd.IpkGpuError):
        engine.score_groups_keymajor_positions(flat, [1, 1], 13, np.float32(-8.0))
    check(engine, mats, [3, 3], 13, co.log_threshold(1.5, 4, 13))


@pytest.mark.parametrize("k,extra", [(6, []), (4, ["--filter", "random"])])
def test_cli_keep_positions_through_the_new_call(tmp_path, k, extra):
    """9. `build --keep-positions -s amino`: one scoring pass, MIF0 and the streamed writer on the device (`--filter random`: host
    arrays with Db.positions()), every record against the oracle pipeline on the same file."""
    from click.testing import CliRunner
    from ipk_amd import cli
    from oracle import ar_oracle
    from tests.test_loader import write_probs
    ar_dir = tmp_path / "AR"; ar_dir.mkdir()
    labels = [f"{i}_X{j}" for i in range(3) for j in range(2)]
    write_probs(ar_dir / "ar.raxml.ancestralProbs", 20, labels, 30, 5, extras=False)
    with open(tmp_path / "map.tsv", "w") as fh:
        for i, lab in enumerate(labels):
            fh.write(f"{lab}\t{4 + i // 2}\n")
    out = tmp_path / "DBpos.ipk"
    res = CliRunner().invoke(cli.ipk, ["build", "-w", str(tmp_path), "--ar-dir", str(ar_dir), "--mapping", str(tmp_path / "map.tsv"), "-s", "amino",
                                       "-k", str(k), "--omega", "1.5", "-o", str(out), "--num-tree-nodes", "7", "--keep-positions"] + extra)
    assert res.exit_code == 0, (res.output, res.exception)
    hdr, recs = dbfile.read_db(out)
    assert hdr["positions_loaded"] is True and hdr["sequence_type"] == "AA" and hdr["kmer_size"] == k
    mats, _ = ar_oracle.read_file(ar_dir / "ar.raxml.ancestralProbs", 20)
    eps = co.log_threshold(1.5, 20, k)
    full = {}
    for g in range(3):
        keys, scores, pos, _ = co.explore_group_pos(np.stack([mats[labels[2 * g]], mats[labels[2 * g + 1]]]), k, eps)
        for kk, sc, pp in zip(keys.tolist(), scores.view(np.uint32).tolist(), pos.tolist()):
            full.setdefault(kk, []).append((4 + g, sc, pp))
    assert hdr["total_num_kmers"] == len(full) == len(recs) and hdr["total_num_entries"] == sum(len(v) for v in full.values())
    for key, fv, br, sc, pos in recs:
        assert [(int(b), int(s), int(p)) for b, s, p in zip(br, sc.view(np.uint32), pos)] == full[key]
    assert all(recs[i][1] <= recs[i + 1][1] for i in range(len(recs) - 1))
