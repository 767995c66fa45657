"""GPU suite: the random filter on the device (ipkgpu_db_filter_random, random_filter_kernel) and the one filter-and-write stage of
the build paths (dbfile.filter_and_write_device).  The yardstick is always the host path: dbfile.splitmix_unit, filter_sort_code,
write_db and write_db_positions.  Every comparison is bit for bit or byte for byte."""
import numpy as np
import pytest
from click.testing import CliRunner

import ipk_amd
from ipk_amd import cli, dbfile, keyrange, ondisk
from ipk_amd import distributed as D
from ipk_amd.loader import AncestralProbs
from ipk_amd.synth import synth_matrices
from oracle import ipk_oracle as co
from tests.test_loader import write_probs

pytestmark = pytest.mark.gpu

GROUPS = np.array([5, 5, 9, 9], dtype=np.uint32)
TREE_INDEX, NEWICK, OMEGA = [(1, 0.0), (3, 0.5), (5, 1.0)], "((a:1,b:1):1,c:1);", 1.5

# the host functions, kept beside the names the build paths could reach them by (7. patches those)
HOST_WRITE_DB, HOST_WRITE_DB_POSITIONS = dbfile.write_db, dbfile.write_db_positions


def host_draw(keys):
    """(doubles, floats, order) of the host path for a shard's ascending keys."""
    fv64 = dbfile.splitmix_unit(keys) if len(keys) else np.zeros(0)
    fv32 = fv64.astype(np.float32)
    return fv64, fv32, np.argsort(dbfile.filter_sort_code(fv32, keys), kind="stable").astype(np.uint32)


def check_values_and_order(db):
    keys = db.keys().copy()
    fv64, fv32, order = host_draw(keys)
    assert np.array_equal(db.filter_values().view(np.uint32), fv32.view(np.uint32))
    assert np.array_equal(db.filter_values(f64=True), fv64)
    assert np.array_equal(db.filter_order(), order)
    return keys, fv32, order


def host_file(path, db, seq, k, tree_index=TREE_INDEX, newick=NEWICK):
    """The yardstick file of a database: host draw and order, host arrays, host serialiser."""
    keys = db.keys().copy()
    _, fv32, order = host_draw(keys)
    br, sc = db.entries()
    pos = db.positions()
    if pos is None:
        HOST_WRITE_DB(path, seq, tree_index, newick, k, OMEGA, keys, db.key_offsets(), br, sc, fv32, order)
    else:
        HOST_WRITE_DB_POSITIONS(path, seq, tree_index, newick, k, OMEGA, keys, db.key_offsets(), br, sc, pos, fv32, order)
    return path.read_bytes()


def test_values_and_order_with_ties(engine):
    """1. every DNA 6-mer present (flat columns under a threshold all of them pass): over keys 0..4095 the draw has equal values,
    so the order's tie rule (ascending key) is exercised."""
    k = 6
    mats = np.full((2, 8, 4), np.log10(0.25), np.float32)
    db, parts = D.build_db_shard(engine, mats, np.array([5, 5], dtype=np.uint32), k, np.float32(k * np.log10(0.25) - 0.5), 4)
    assert db.num_keys == 4096 and np.array_equal(db.keys(), np.arange(4096, dtype=np.uint32))
    _, fv32, _ = host_draw(np.arange(4096, dtype=np.uint32))
    assert len(np.unique(fv32)) < 4096, "the host draw has no ties over these keys: the tie rule is not exercised"
    db.filter_random(engine)
    check_values_and_order(db)
    assert db.filter_time_ms() > 0
    db.free(); parts.free()


def test_partial_workgroup_and_empty(engine, tmp_path):
    """2. a few dozen keys (no multiple of the workgroup), and a database without a k-mer."""
    k = 4
    mats = synth_matrices(2, 6, 4, 0.1, 46)
    groups = np.array([5, 5], dtype=np.uint32)
    db, parts = D.build_db_shard(engine, mats, groups, k, co.log_threshold(OMEGA, 4, k), 4)
    assert 0 < db.num_keys < 256
    db.filter_random(engine)
    check_values_and_order(db)
    db.free(); parts.free()
    db, parts = D.build_db_shard(engine, mats, groups, k, np.float32(0.0), 4)
    assert db.num_keys == 0
    db.filter_random(engine)
    assert len(db.filter_values()) == 0 and len(db.filter_order()) == 0
    dev, host = tmp_path / "dev.ipk", tmp_path / "host.ipk"
    dbfile.write_db_device(engine, db, dev, "DNA", TREE_INDEX, NEWICK, k, OMEGA)
    HOST_WRITE_DB(host, "DNA", TREE_INDEX, NEWICK, k, OMEGA, np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint32),
                  np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint32))
    assert dev.read_bytes() == host.read_bytes()
    db.free(); parts.free()


def test_high_keys(engine):
    """3. DNA k = 16: keys at and above 2^31 and 0xFFFFFFFF are ordinary keys (first and last key-range pass of 16)."""
    p = np.full((40, 4), 0.01, np.float32)
    a, t = p.copy(), p.copy()
    a[:, 0] = 0.97
    t[:, 3] = 0.97
    mats = np.concatenate([np.log10(np.stack([a, t])).astype(np.float32), synth_matrices(2, 40, 4, 0.1, 77)])
    groups = np.array([5, 9, 5, 9], dtype=np.uint32)
    eps = co.log_threshold(OMEGA, 4, 16)
    seen = []
    for cls in (0, 15):
        parts = engine.score_groups_keyrange(mats, groups, 16, eps, 2, cls)
        db = engine.db_from_parts(parts, 4, 16)
        db.filter_random(engine)
        keys, _, _ = check_values_and_order(db)
        seen.append(keys)
        db.free(); parts.free()
    assert seen[0][0] == 0 and seen[1][-1] == 0xFFFFFFFF and seen[1][0] >= 2 ** 31


def plain_db(engine):
    k = 8
    return D.build_db_shard(engine, synth_matrices(4, 60, 4, 0.1, 808), GROUPS, k, co.log_threshold(OMEGA, 4, k), 4) + (k,)


def test_file_bytes_plain(engine, tmp_path):
    """4. filter_random + the device writer == write_db over the host arrays with the host draw and order."""
    db, parts, k = plain_db(engine)
    assert db.num_keys > 256
    want = host_file(tmp_path / "host.ipk", db, "DNA", k)
    db.filter_random(engine)
    dbfile.write_db_device(engine, db, tmp_path / "dev.ipk", "DNA", TREE_INDEX, NEWICK, k, OMEGA)
    assert (tmp_path / "dev.ipk").read_bytes() == want
    db.free(); parts.free()


def test_file_bytes_positioned(engine, tmp_path):
    """5. a positioned database (amino acids): the device writer's positioned records in the random order == write_db_positions."""
    sigma, k = 20, 3
    mats = synth_matrices(4, 30, sigma, 0.05, 303)
    parts = engine.score_groups_keymajor_positions(mats, np.array([4, 4, 5, 5], dtype=np.uint32), k, co.log_threshold(OMEGA, sigma, k))
    db = engine.db_from_parts(parts, sigma, k)
    assert db.num_keys > 0 and db.positions() is not None
    want = host_file(tmp_path / "host.ipk", db, "AA", k)
    db.filter_random(engine)
    check_values_and_order(db)
    dbfile.write_db_device(engine, db, tmp_path / "dev.ipk", "AA", TREE_INDEX, NEWICK, k, OMEGA)
    assert (tmp_path / "dev.ipk").read_bytes() == want
    assert dbfile.read_db(tmp_path / "dev.ipk")[0]["positions_loaded"] is True
    db.free(); parts.free()


def test_filtering_again(engine, tmp_path):
    """6. a filter call replaces what the other left: MIF0 then random writes 4.'s file, random then MIF0 the file of MIF0 alone."""
    thr = ipk_amd.score_threshold(OMEGA, 4, 8)
    db, parts, k = plain_db(engine)
    want_random = host_file(tmp_path / "host.ipk", db, "DNA", k)
    db.filter_mif0(engine, 11, thr)
    dbfile.write_db_device(engine, db, tmp_path / "mif0.ipk", "DNA", TREE_INDEX, NEWICK, k, OMEGA)
    want_mif0 = (tmp_path / "mif0.ipk").read_bytes()
    assert want_mif0 != want_random
    db.filter_random(engine)
    dbfile.write_db_device(engine, db, tmp_path / "a.ipk", "DNA", TREE_INDEX, NEWICK, k, OMEGA)
    assert (tmp_path / "a.ipk").read_bytes() == want_random
    db.free(); parts.free()
    db, parts, k = plain_db(engine)
    db.filter_random(engine)
    db.filter_mif0(engine, 11, thr)
    dbfile.write_db_device(engine, db, tmp_path / "b.ipk", "DNA", TREE_INDEX, NEWICK, k, OMEGA)
    assert (tmp_path / "b.ipk").read_bytes() == want_mif0
    db.free(); parts.free()


# ---- 7. the build paths use the device filter and the device writer ----------------------------------------------------------------

def no_host_writer(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("a build path called the host serialiser")
    monkeypatch.setattr(dbfile, "write_db", refuse)
    monkeypatch.setattr(dbfile, "write_db_positions", refuse)


def cli_inputs(tmp_path, sigma, n_groups, sites, seed, first_branch):
    ar_dir = tmp_path / "AR"; ar_dir.mkdir()
    labels = [f"{i}_X{j}" for i in range(n_groups) for j in range(2)]
    write_probs(ar_dir / "ar.raxml.ancestralProbs", sigma, labels, sites, seed, extras=False)
    branches = [first_branch + i // 2 for i in range(len(labels))]
    with open(tmp_path / "map.tsv", "w") as fh:
        for lab, b in zip(labels, branches):
            fh.write(f"{lab}\t{b}\n")
    arp = AncestralProbs(str(ar_dir / "ar.raxml.ancestralProbs"), sigma)
    mats = arp.read(labels)
    arp.close()
    return ar_dir, mats, np.array(branches, dtype=np.uint32)


@pytest.mark.parametrize("sigma,k,keep", [(4, 6, False), (20, 3, True)])
def test_cli_build_random_on_the_device(engine, tmp_path, monkeypatch, sigma, k, keep):
    """`build --filter random` (k = 6, 8 nodes x 40 sites), and `-s amino -k 3 --keep-positions`: the host writer is never called."""
    ar_dir, mats, branches = cli_inputs(tmp_path, sigma, 4 if sigma == 4 else 3, 40 if sigma == 4 else 30, 11 if sigma == 4 else 5, 7)
    db, parts = D.build_db_shard(engine, mats, branches, k, ipk_amd.log_threshold(OMEGA, sigma, k), sigma, positions=keep)
    assert db.num_keys > 0 and (db.positions() is not None) == keep
    want = host_file(tmp_path / "host.ipk", db, "DNA" if sigma == 4 else "AA", k, [], "")
    db.free(); parts.free()
    no_host_writer(monkeypatch)
    out = tmp_path / "DB.ipk"
    args = ["build", "-w", str(tmp_path), "--ar-dir", str(ar_dir), "--mapping", str(tmp_path / "map.tsv"), "-k", str(k), "--omega", "1.5",
            "-o", str(out), "--num-tree-nodes", "9", "--filter", "random"]
    res = CliRunner().invoke(cli.ipk, args + (["-s", "amino", "--keep-positions"] if keep else []))
    assert res.exit_code == 0, (res.output, res.exception)
    assert "Filtering time" in res.output and "Merge time" in res.output
    assert out.read_bytes() == want


def test_key_passes_random_on_the_device(engine, tmp_path, monkeypatch):
    k = 14
    mats = synth_matrices(4, 200, 4, 0.1, 1414)
    eps = co.log_threshold(OMEGA, 4, k)
    db, parts = D.build_db_shard(engine, mats, GROUPS, k, eps, 4)
    want = host_file(tmp_path / "host.ipk", db, "DNA", k)
    totals = (db.num_keys, db.num_entries)
    db.free(); parts.free()
    no_host_writer(monkeypatch)
    out = tmp_path / "passes.ipk"
    r = keyrange.build_db_file(engine, mats, GROUPS, k, eps, 4, str(out), str(tmp_path / "w"), "DNA", TREE_INDEX, NEWICK, OMEGA,
                               filter_="random", total_num_groups=11, passes=4)
    assert r["passes"] == 4 and r["totals"] == totals and r["filter_s"] > 0 and r["write_s"] > 0
    assert out.read_bytes() == want


def test_on_disk_random_on_the_device(engine, tmp_path, monkeypatch):
    k = 6
    groups = np.repeat(np.arange(5, 9, dtype=np.uint32), 2)
    mats = synth_matrices(len(groups), 40, 4, 0.1, 606)
    eps = co.log_threshold(OMEGA, 4, k)
    db, parts = D.build_db_shard(engine, mats, groups, k, eps, 4)
    want = host_file(tmp_path / "host.ipk", db, "DNA", k)
    totals = (db.num_keys, db.num_entries)
    db.free(); parts.free()
    no_host_writer(monkeypatch)
    out = tmp_path / "ondisk.ipk"
    r = ondisk.build_db_file(engine, mats, groups, k, eps, 4, str(out), str(tmp_path / "w"), "DNA", TREE_INDEX, NEWICK, OMEGA,
                             filter_="random", total_num_groups=9, batches=4, budget_bytes=8 << 30, piece_sizes=[2])
    assert r["pieces"] == 2 and tuple(r["totals"]) == totals and r["filter_s"] > 0
    assert out.read_bytes() == want
