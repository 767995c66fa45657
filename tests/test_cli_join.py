"""`ipk.py build --group-range`, `merge --shared-keys`, `place --shared-keys`: the option surface and every usage error that needs no
GPU -- each is raised before an engine is created.  The runs themselves are in tests/test_gpu_cli_join.py."""
import click
import pytest
from click.testing import CliRunner

from ipk_amd import cli
from tests import db_files as F

TREELESS = dict(F.HEADER, tree_index=[], newick="", kmer_size=8)


def run(args, env=None):
    return CliRunner().invoke(cli.ipk, args, env=env)


def usage_error(res, *words):
    assert res.exit_code == 2, (res.exit_code, res.output, res.exception)
    for w in words:
        assert w in res.output, (w, res.output)


@pytest.fixture()
def shards(tmp_path):
    """Two plain shard files and a positioned one, all without a tree; one with the tests' tree; one of another k."""
    a = F.write(tmp_path / "a.ipk", F.synthetic(20, seed=1, k=8), False, TREELESS)
    b = F.write(tmp_path / "b.ipk", F.synthetic(20, seed=2, k=8), False, TREELESS)
    p = F.write(tmp_path / "p.ipk", F.synthetic(20, seed=3, k=8), True, TREELESS)
    t = F.write(tmp_path / "t.ipk", F.synthetic(20, seed=4, k=8), False, dict(F.HEADER, kmer_size=8))
    k4 = F.write(tmp_path / "k4.ipk", F.synthetic(20, seed=5, k=4), False, dict(TREELESS, kmer_size=4))
    return dict(a=str(a), b=str(b), p=str(p), t=str(t), k4=str(k4))


def test_group_range_parsing():
    assert cli._parse_group_range("0:5") == (0, 5) and cli._parse_group_range("5:6") == (5, 6) and cli._parse_group_range(" 6 : 12 ") == (6, 12)
    for bad in ("5", "a:b", "1:2:3", "", "0x1:2", "1.5:3"):
        with pytest.raises(click.UsageError, match="two integers"):
            cli._parse_group_range(bad)
    for bad in ("5:5", "6:5", "-1:3"):
        with pytest.raises(click.UsageError, match="0 <= LO < HI"):
            cli._parse_group_range(bad)


def test_new_options_exist_and_defaults_are_unchanged():
    names = lambda cmd: {o for p in cmd.params for o in p.opts}
    assert "--group-range" in names(cli.build)
    assert {"--shared-keys", "--filter", "--num-tree-nodes"} <= names(cli.merge)
    assert {"--shared-keys", "--num-tree-nodes"} <= names(cli.place)
    d = {p.name: p.default for p in cli.merge.params}
    assert d["on"] == "device" and d["shared_keys"] is False and d["filter_"] == "mif0" and d["num_tree_nodes"] == 0
    assert {p.name: p.default for p in cli.build.params}["group_range"] is None
    assert {p.name: p.default for p in cli.place.params}["shared_keys"] is False


def build_args(tmp_path, *extra):
    return ["build", "-w", str(tmp_path), "--ar-dir", str(tmp_path), "-k", "8"] + list(extra)


def test_group_range_usage_errors(tmp_path):
    usage_error(run(build_args(tmp_path, "--group-range", "3")), "--group-range takes LO:HI")
    usage_error(run(build_args(tmp_path, "--group-range", "4:4")), "0 <= LO < HI")
    usage_error(run(build_args(tmp_path, "--group-range", "0:2"), env={"WORLD_SIZE": "2"}), "--group-range runs on ONE GPU")
    usage_error(run(build_args(tmp_path, "--group-range", "0:2", "--on-disk")), "--group-range is not combined with --on-disk")
    usage_error(run(["build", "-w", str(tmp_path), "--ar-dir", str(tmp_path), "-k", "14", "--group-range", "0:2", "--key-passes", "4"]),
                "--group-range is not combined with key-range passes")
    usage_error(run(["build", "-w", str(tmp_path), "--ar-dir", str(tmp_path), "-k", "15", "--group-range", "0:2"]), "--group-range is not combined with key-range passes")
    # --keep-positions is allowed with it: the next refusal is about the inputs, which this directory does not hold
    res = run(["build", "-w", str(tmp_path), "--ar-dir", str(tmp_path), "-s", "amino", "-k", "3", "--keep-positions", "--group-range", "0:2"])
    usage_error(res, "Could not find")


def test_merge_shared_keys_usage_errors(shards, tmp_path):
    out = str(tmp_path / "out.ipk")
    usage_error(run(["merge", "--shared-keys", "--on", "host", "-o", out, shards["a"], shards["b"]]), "--shared-keys goes with --on device only")
    usage_error(run(["merge", "--shared-keys", "-o", out, shards["a"], shards["b"]]), "give --num-tree-nodes", "no tree index")
    usage_error(run(["merge", "--shared-keys", "--num-tree-nodes", "-3", "-o", out, shards["a"], shards["b"]]), "--num-tree-nodes must be positive")
    usage_error(run(["merge", "--shared-keys", "--num-tree-nodes", "9", "-o", out, shards["a"], shards["p"]]), "positions flag")
    usage_error(run(["merge", "--shared-keys", "--num-tree-nodes", "9", "-o", out, shards["a"], shards["k4"]]), "k 4 differs")
    usage_error(run(["merge", "--filter", "random", "-o", out, shards["a"], shards["b"]]), "go with --shared-keys")
    usage_error(run(["merge", "--num-tree-nodes", "9", "-o", out, shards["a"], shards["b"]]), "go with --shared-keys")


def test_place_shared_keys_usage_errors(shards, tmp_path):
    q = tmp_path / "q.fasta"
    q.write_text(">r\nACGTACGTACGT\n")
    usage_error(run(["place", "--shared-keys", "-i", shards["a"], "-i", shards["b"], "-q", str(q)]), "give --num-tree-nodes")
    usage_error(run(["place", "--shared-keys", "--stream-db", "-i", shards["t"], "-q", str(q)]), "--shared-keys does not go with --stream-db")
    usage_error(run(["place", "--shared-keys", "--num-tree-nodes", "9", "-i", shards["a"], "-i", shards["p"], "-q", str(q)]), "positions flag")
    usage_error(run(["place", "--shared-keys", "--num-tree-nodes", "9", "--mu", "1.5", "-i", shards["a"], "-i", shards["b"], "-q", str(q)]), "--mu must be in [0, 1]")
