"""GPU suite: DNA k = 14..16 databases built in key-range passes (ipkgpu_score_groups_keyrange_device, ipk_amd/keyrange.py),
checked against the oracle per pass, byte for byte against the one-call path at k = 14, and through the command line."""
import numpy as np
import pytest
from click.testing import CliRunner

import ipk_amd
from ipk_amd import cli, dbfile, keyrange
from ipk_amd import distributed as D
from ipk_amd.synth import synth_matrices
from oracle import db_oracle as dbo
from oracle import ipk_oracle as co

pytestmark = pytest.mark.gpu

GROUPS = np.array([5, 5, 9, 9], dtype=np.uint32)


def oracle_full(mats, groups, k, eps):
    """The whole database as sorted arrays (keys, key_offsets, branches, score bits) and the scored count (entries-sized only)."""
    res, emitted = [], 0
    for gid in dict.fromkeys(groups.tolist()):
        keys, scores, e = co.explore_group(mats[groups == gid], k, eps)
        res.append((gid, keys, scores))
        emitted += e
    return dbo.db_shard_arrays(dbo.build_db(res), 4, k, 0, 1), emitted


def check_passes(engine, mats, groups, k, lead):
    eps = co.log_threshold(1.5, 4, k)
    (ok, ooff, obr, osc), emitted = oracle_full(mats, groups, k, eps)
    ooff = ooff.astype(np.int64)
    total, seen = 0, 0
    for j, cls, base, span in keyrange.plan(4, k, 4 ** lead):
        parts = engine.score_groups_keyrange(mats, groups, k, eps, j, cls)
        assert parts.key_base == base and parts.slots == span
        total += parts.emitted
        db = engine.db_from_parts(parts, 4, k)
        a, b = np.searchsorted(ok, [base, base + span]) if base + span < 2 ** 32 else (np.searchsorted(ok, base), len(ok))
        keys, off = db.keys(), db.key_offsets().astype(np.int64)
        br, sc = db.entries()
        assert np.array_equal(keys, ok[a:b]), (k, lead, cls)
        assert np.array_equal(off, ooff[a:b + 1] - ooff[a])
        assert np.array_equal(br, obr[ooff[a]:ooff[b]]) and np.array_equal(sc.view(np.uint32), osc[ooff[a]:ooff[b]])
        seen += len(keys)
        db.free(); parts.free()
    assert seen == len(ok) and total == emitted
    return ok


@pytest.mark.parametrize("k,lead,sites", [(15, 1, 120), (15, 2, 120), (16, 2, 100), (16, 3, 60)])
def test_pass_databases_match_oracle(engine, k, lead, sites):
    mats = synth_matrices(4, sites, 4, 0.1, 1500 + k)
    check_passes(engine, mats, GROUPS, k, lead)


def test_k16_edge_keys(engine):
    """All A and all T are legal k = 16 k-mers: keys 0 and 0xFFFFFFFF, no full key serves as a sentinel."""
    p = np.full((40, 4), 0.01, np.float32)
    a, t = p.copy(), p.copy()
    a[:, 0] = 0.97
    t[:, 3] = 0.97
    mats = np.concatenate([np.log10(np.stack([a, t])).astype(np.float32), synth_matrices(2, 40, 4, 0.1, 77)])
    ok = check_passes(engine, mats, np.array([5, 9, 5, 9], dtype=np.uint32), 16, 2)
    assert ok[0] == 0 and ok[-1] == 0xFFFFFFFF


def test_batches_inside_a_pass(engine):
    """A small workspace: several batches of groups inside one pass, merged in the library; nothing changes."""
    mats = synth_matrices(6, 80, 4, 0.1, 1515)
    engine.set_option("workspace_bytes", 1 << 20)
    try:
        check_passes(engine, mats, np.array([1, 1, 2, 2, 3, 3], dtype=np.uint32), 15, 1)
    finally:
        engine.set_option("workspace_bytes", 8 << 30)


def test_flat_columns_fail_loudly(engine):
    """Flat columns under a threshold every k-mer passes (15 log10(0.25) = -9.03): the 8-symbol half lists (4^8 entries) exceed the
    big-list cap, and the pass fails; it never returns fewer k-mers.  The context stays usable."""
    mats = np.full((4, 40, 4), np.log10(0.25), np.float32)
    with pytest.raises(ipk_amd.IpkGpuError):
        engine.score_groups_keyrange(mats, GROUPS, 15, np.float32(-9.5), 1, 0)
    check_passes(engine, synth_matrices(4, 50, 4, 0.1, 78), GROUPS, 15, 1)


def test_unsupported_ranges_refused(engine):
    mats = synth_matrices(4, 60, 4, 0.1, 3)
    for k, lead, cls in [(15, 3, 0), (16, 1, 0), (13, 1, 0), (14, 1, 4)]:
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            engine.score_groups_keyrange(mats, GROUPS, k, -3.0, lead, cls)
        assert ei.value.code == 1


def _file_bytes(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("filt", ["mif0", "random"])
def test_k14_passes_write_the_one_call_bytes(engine, tmp_path, filt):
    k, sites = 14, 200
    mats = synth_matrices(4, sites, 4, 0.1, 1414)
    eps = co.log_threshold(1.5, 4, k)
    tree_index = [(1, 0.0), (3, 0.5), (5, 1.0)]
    newick, omega = "((a:1,b:1):1,c:1);", 1.5
    one = tmp_path / "one.ipk"
    db, parts = D.build_db_shard(engine, mats, GROUPS, k, eps, 4)
    if filt == "mif0":
        db.filter_mif0(engine, 11, ipk_amd.score_threshold(omega, 4, k))
        dbfile.write_db_device(engine, db, one, "DNA", tree_index, newick, k, omega)
    else:
        keys = db.keys()
        fv = dbfile.splitmix_unit(keys).astype(np.float32)
        order = np.argsort(dbfile.filter_sort_code(fv, keys), kind="stable")
        br, sc = db.entries()
        dbfile.write_db(one, "DNA", tree_index, newick, k, omega, keys, db.key_offsets(), br, sc, fv, order)
    n_keys, n_entries, emitted = db.num_keys, db.num_entries, parts.emitted
    db.free(); parts.free()
    out = tmp_path / "passes.ipk"
    r = keyrange.build_db_file(engine, mats, GROUPS, k, eps, 4, str(out), str(tmp_path / "w"), "DNA", tree_index, newick, omega,
                               filt, 11, passes=4)
    assert r["passes"] == 4 and r["totals"] == (n_keys, n_entries) and r["emitted"] == emitted
    assert _file_bytes(out) == _file_bytes(one)
    assert not (tmp_path / "w" / "passes").exists()


def test_k15_same_bytes_for_any_split(engine, tmp_path):
    k = 15
    mats = synth_matrices(4, 150, 4, 0.1, 1616)
    eps = co.log_threshold(1.5, 4, k)
    files = []
    for passes in (4, 16):
        out = tmp_path / f"db{passes}.ipk"
        r = keyrange.build_db_file(engine, mats, GROUPS, k, eps, 4, str(out), str(tmp_path / f"w{passes}"), "DNA", [(1, 0.0)], "a;",
                                   1.5, "mif0", 11, passes=passes)
        assert r["passes"] == passes
        files.append(_file_bytes(out))
    assert files[0] == files[1]


@pytest.mark.parametrize("k", [15, 16])
def test_cli_builds_k15_k16(tmp_path, k):
    """`ipk.py build -k 15 / 16` from reference-format inputs, checked against the oracle pipeline; --key-passes 16 at k = 15
    writes the same bytes as the default split."""
    from oracle import ar_oracle, tree_oracle as to
    from tests.test_cli import _reference_workdir
    tree_file, ar_dir, (root, eroot, mapping, relabel) = _reference_workdir(tmp_path, 6, 60, 300 + k)
    out = tmp_path / "DB.ipk"
    base = ["build", "-t", str(tree_file), "-w", str(tmp_path / "work"), "-k", str(k), "--ar-dir", str(ar_dir)]
    res = CliRunner().invoke(cli.ipk, base + ["-o", str(out)])
    assert res.exit_code == 0, (res.output, res.exception)
    assert "key-range passes" in res.output
    hdr, (keys, fvs, counts, eoff, br, sc) = dbfile.read_db(out, as_arrays=True)
    post = to.postorder(root)
    assert hdr["kmer_size"] == k and hdr["sequence_type"] == "DNA" and len(hdr["tree_index"]) == len(post)
    ar_root = to.reroot(to.parse(to.to_unrooted_ar(eroot, relabel)))
    amap = to.map_nodes(eroot, ar_root)
    mats, _ = ar_oracle.read_file(ar_dir / "extended_align.phylip.raxml.ancestralProbs", 4)
    eps = co.log_threshold(1.5, 4, k)
    res_g = []
    for branch, labs in to.ghost_groups(root, eroot, mapping, "both"):
        gk, gs, _ = co.explore_group(np.stack([mats[amap[lab]] for lab in labs]), k, eps)
        res_g.append((branch, gk, gs))
    ok, ooff, obr, osc = dbo.db_shard_arrays(dbo.build_db(res_g), 4, k, 0, 1)
    ooff = ooff.astype(np.int64)
    assert hdr["total_num_kmers"] == len(ok) and hdr["total_num_entries"] == len(obr)
    assert np.all(np.diff(fvs) >= 0) and len(np.unique(keys)) == len(keys)
    pos = np.searchsorted(ok, keys)
    assert np.array_equal(ok[pos], keys)
    assert np.array_equal(counts, (ooff[pos + 1] - ooff[pos]).astype(np.uint64))
    src = np.concatenate([np.arange(ooff[p], ooff[p + 1]) for p in pos]) if len(pos) else np.zeros(0, np.int64)
    assert np.array_equal(br, obr[src]) and np.array_equal(sc.view(np.uint32), osc[src])
    thr = co.score_threshold(1.5, 4, k)
    for i in np.linspace(0, len(keys) - 1, 100).astype(np.int64):
        p = pos[i]
        ref = co.mif0(osc[ooff[p]:ooff[p + 1]].view(np.float32), len(post), thr)
        assert abs(fvs[i] - ref) <= 1e-6 * max(1.0, abs(ref))
    if k == 15:
        out16 = tmp_path / "DB16.ipk"
        res = CliRunner().invoke(cli.ipk, base + ["-o", str(out16), "--key-passes", "16"])
        assert res.exit_code == 0, (res.output, res.exception)
        assert _file_bytes(out16) == _file_bytes(out)
