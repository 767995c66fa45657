"""CPU suite: the key-range split of DNA k = 14..16 (ipk_amd/keyrange.py), the merge of pass files, and the command line's
refusals -- no GPU needed."""
import numpy as np
import pytest
from click.testing import CliRunner

import ipk_amd
from ipk_amd import cli, dbfile, keyrange
from ipk_amd.synth import synth_matrices
from oracle import db_oracle as dbo
from oracle import ipk_oracle as co


def test_max_k_keyrange():
    assert ipk_amd.max_k_keyrange(4) == 16 and ipk_amd.max_k_keyrange(20) == 6 and ipk_amd.max_k_keyrange(7) == 0
    assert ipk_amd.max_k(4) == 14


ALLOWED = {(14, 1), (15, 1), (15, 2), (16, 2), (16, 3)}


def test_plan_covers_the_key_space():
    for k, j in sorted(ALLOWED):
        steps = keyrange.plan(4, k, 4 ** j)
        assert len(steps) == 4 ** j
        span = 4 ** (k - j)
        assert all(s[0] == j and s[1] == c and s[2] == c * span and s[3] == span for c, s in enumerate(steps))
        assert steps[0][2] == 0 and steps[-1][2] + steps[-1][3] == 4 ** k          # contiguous, disjoint, covering 4^k
    assert [len(keyrange.plan(4, k)) for k in (15, 16)] == [4, 16]                   # default: j = k - 14


def test_plan_rejects_everything_else():
    for k in range(2, 20):
        for j in range(0, 6):
            if (k, j) in ALLOWED:
                continue
            with pytest.raises(ValueError):
                keyrange.plan(4, k, 4 ** j)
    for k in (2, 13, 14, 17):
        with pytest.raises(ValueError):
            keyrange.plan(4, k)
    with pytest.raises(ValueError):
        keyrange.plan(4, 15, 8)                                                     # not a power of 4
    with pytest.raises(ValueError):
        keyrange.plan(20, 6, 20)                                                    # amino acids: no passes


def test_pass_files_merge_to_the_whole_file(tmp_path):
    """Shards of a k = 15 database cut at the pass boundaries, each written as a file of its own and merged, equal byte for byte
    the database written in one go (the mechanism of keyrange.build_db_file; host writers and oracle results)."""
    k = 15
    mats = synth_matrices(4, 60, 4, 0.1, 1507)
    groups = [(5, mats[:2]), (9, mats[2:])]
    eps = co.log_threshold(1.5, 4, k)
    res = []
    for gid, m in groups:
        keys, scores, _ = co.explore_group(m, k, eps)
        res.append((gid, keys, scores))
    keys, off, br, sc = dbo.db_shard_arrays(dbo.build_db(res), 4, k, 0, 1)
    off = off.astype(np.int64)
    assert len(keys) > 100
    thr = co.score_threshold(1.5, 4, k)
    fv = np.array([co.mif0(sc[off[i]:off[i + 1]].view(np.float32), 11, thr) for i in range(len(keys))], dtype=np.float32)
    tree_index, newick = [(1, 0.0), (3, 0.5), (5, 1.0)], "((a:1,b:1):1,c:1);"

    def write(path, a, b):
        o = off[a:b + 1] - off[a]
        kk, ff = keys[a:b], fv[a:b]
        order = np.argsort(dbfile.filter_sort_code(ff, kk), kind="stable")
        hdr = (tree_index, newick) if path.name == "whole.ipk" else ([], "")
        dbfile.write_db(path, "DNA", hdr[0], hdr[1], k, 1.5, kk, o, br[off[a]:off[b]], sc[off[a]:off[b]].view(np.float32), ff, order)

    whole = tmp_path / "whole.ipk"
    write(whole, 0, len(keys))
    for passes in (4, 16):
        paths = []
        for j, c, base, span in keyrange.plan(4, k, passes):
            a, b = np.searchsorted(keys, [base, base + span])
            p = tmp_path / f"pass{passes}_{c}.ipk"
            write(p, a, b)
            paths.append(p)
        merged = tmp_path / f"merged{passes}.ipk"
        assert dbfile.merge_shard_files(merged, "DNA", tree_index, newick, k, 1.5, paths) == (len(keys), len(br))
        assert merged.read_bytes() == whole.read_bytes()


def _build_args(tmp_path, k, extra=()):
    (tmp_path / "m.tsv").write_text("")
    return ["build", "-w", str(tmp_path / "w"), "--ar-dir", str(tmp_path), "-k", str(k), "--mapping", str(tmp_path / "m.tsv")] + list(extra)


def test_cli_refuses_k17(tmp_path):
    res = CliRunner().invoke(cli.ipk, _build_args(tmp_path, 17))
    assert res.exit_code == 2 and "[2, 16]" in res.output


def test_cli_refuses_passes_on_several_ranks(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    res = CliRunner().invoke(cli.ipk, _build_args(tmp_path, 15))
    assert res.exit_code == 2 and "ONE GPU" in res.output
    res = CliRunner().invoke(cli.ipk, _build_args(tmp_path, 12, ["--key-passes", "4"]))
    assert res.exit_code == 2


def test_cli_refuses_impossible_pass_counts(tmp_path):
    for k, n in [(15, 8), (13, 4), (16, 4), (14, 16)]:
        res = CliRunner().invoke(cli.ipk, _build_args(tmp_path, k, ["--key-passes", str(n)]))
        assert res.exit_code == 2 and "--key-passes" in res.output, (k, n, res.output)
