"""`ipk.py merge --shared-keys --stream [--budget-mib N] [--tmp-dir DIR]`: the option surface and the usage errors, each raised before an
engine is created.  The runs themselves are in tests/test_gpu_cli_join_files.py."""
import pytest
from click.testing import CliRunner

from ipk_amd import cli
from tests import db_files as F

TREELESS = dict(F.HEADER, tree_index=[], newick="", kmer_size=8)


def run(args):
    return CliRunner().invoke(cli.ipk, args)


def usage_error(res, *words):
    assert res.exit_code == 2, (res.exit_code, res.output, res.exception)
    for w in words:
        assert w in res.output, (w, res.output)


@pytest.fixture()
def shards(tmp_path):
    a = F.write(tmp_path / "a.ipk", F.synthetic(20, seed=1, k=8), False, TREELESS)
    b = F.write(tmp_path / "b.ipk", F.synthetic(20, seed=2, k=8), False, TREELESS)
    p = F.write(tmp_path / "p.ipk", F.synthetic(20, seed=3, k=8), True, TREELESS)
    return [str(a), str(b)], str(p)


def test_the_options_exist_and_default_to_the_in_memory_route():
    names = {o for p in cli.merge.params for o in p.opts}
    assert {"--stream", "--budget-mib", "--tmp-dir"} <= names
    d = {p.name: p.default for p in cli.merge.params}
    assert d["stream"] is False and d["budget_mib"] is None and d["tmp_dir"] is None
    assert d["on"] == "device" and d["shared_keys"] is False and d["filter_"] == "mif0" and d["num_tree_nodes"] == 0
    assert "--stream-db" in {o for p in cli.place.params for o in p.opts} and "--stream" not in {o for p in cli.place.params for o in p.opts}


def test_stream_usage_errors(shards, tmp_path):
    (a, b), p = shards
    out = str(tmp_path / "out.ipk")
    usage_error(run(["merge", "--stream", "-o", out, a, b]), "--stream goes with --shared-keys")
    usage_error(run(["merge", "--stream", "--on", "host", "-o", out, a, b]), "--stream goes with --shared-keys")
    usage_error(run(["merge", "--shared-keys", "--budget-mib", "64", "--num-tree-nodes", "9", "-o", out, a, b]), "--budget-mib and --tmp-dir go with --stream")
    usage_error(run(["merge", "--shared-keys", "--tmp-dir", str(tmp_path / "r"), "--num-tree-nodes", "9", "-o", out, a, b]), "--budget-mib and --tmp-dir go with --stream")
    usage_error(run(["merge", "--budget-mib", "64", "-o", out, a, b]), "--budget-mib and --tmp-dir go with --stream")
    usage_error(run(["merge", "--shared-keys", "--stream", "--budget-mib", "0", "--num-tree-nodes", "9", "-o", out, a, b]), "--budget-mib must be positive")
    usage_error(run(["merge", "--shared-keys", "--stream", "--budget-mib", "-2", "--num-tree-nodes", "9", "-o", out, a, b]), "--budget-mib must be positive")
    # the refusals of --shared-keys stay those of the in-memory route
    usage_error(run(["merge", "--shared-keys", "--stream", "--on", "host", "-o", out, a, b]), "--shared-keys goes with --on device only")
    usage_error(run(["merge", "--shared-keys", "--stream", "-o", out, a, b]), "give --num-tree-nodes", "no tree index")
    usage_error(run(["merge", "--shared-keys", "--stream", "--num-tree-nodes", "9", "-o", out, a, p]), "positions flag")
    usage_error(run(["merge", "--shared-keys", "--stream", "--tmp-dir", a, "--num-tree-nodes", "9", "-o", out, a, b]), "--tmp-dir")   # a file is no directory
    assert not (tmp_path / "out.ipk").exists() and not (tmp_path / "out.ipk.ranges").exists()
