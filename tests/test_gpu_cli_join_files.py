"""GPU suite of the command line over branch shards that do not fit: `ipk.py build --group-range` three times and
`ipk.py merge --shared-keys --stream --budget-mib N`, under a budget that plans several key ranges, give the plain build's file byte for
byte; --tmp-dir is where the range files live, and it is left empty."""
import os

import pytest
from click.testing import CliRunner

from ipk_amd import cli, dbfile
from tests import diff_files_cases as D
from tests import join_files_cases as X
from tests.test_gpu_cli_join import N_GROUPS, RANGES, _bytes, inputs, invoke

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dna(tmp_path_factory):
    """The DNA k = 8 MIF0 build of tests/test_gpu_cli_join.py: the plain build's file and the three branch shards."""
    d = tmp_path_factory.mktemp("cli_join_files")
    base = inputs(d, 4, 64, 71) + ["-k", "8"]
    invoke(base + ["-o", str(d / "whole.ipk")])
    shards = []
    for i, r in enumerate(RANGES):
        invoke(base + ["--group-range", r, "-o", str(d / f"shard{i}.ipk")])
        shards.append(str(d / f"shard{i}.ipk"))
    return d, str(d / "whole.ipk"), shards, planned(shards)


def planned(shards):
    """(MiB, ranges): the first budget in steps of 1/64 MiB under which the restated plan accepts the shards, at the window the library
    derives from it -- there it cuts them into several ranges."""
    header = dbfile.file_info(shards[0])
    files = [dbfile.read_db(p)[1] for p in shards]
    for step in range(128, 1024):
        avail = step << 14
        sides = [X.Shard([r[0] for r in recs], [len(r[2]) for r in recs], False, window=D.default_window(avail)) for recs in files]
        try:
            return step / 64.0, X.plan(sides, avail, header)
        except X.NoRoom:
            continue
    raise AssertionError("no budget below 16 MiB takes the shards")


def test_streamed_merge_of_group_range_builds_is_the_plain_build(dna):
    d, whole, shards, (mib, plan) = dna
    assert len(plan) >= 2
    out = d / "streamed.ipk"
    res = invoke(["merge", "--shared-keys", "--stream", "--budget-mib", str(mib), "--num-tree-nodes", str(N_GROUPS + 1), "-o", str(out)] + shards)
    info = dbfile.file_info(whole)
    assert f"Output: {out} ({info['total_num_kmers']} k-mers, {info['total_num_entries']} entries; merged on the device; 0 entries joined by put; " in res.output, res.output
    assert f"joined in {len(plan)} key ranges)" in res.output, res.output
    assert _bytes(out) == _bytes(whole)
    assert not os.path.exists(str(out) + ".ranges")
    # without a budget: one range, the same bytes
    res = invoke(["merge", "--shared-keys", "--stream", "--num-tree-nodes", str(N_GROUPS + 1), "-o", str(d / "one.ipk")] + shards)
    assert "joined in 1 key ranges)" in res.output and _bytes(d / "one.ipk") == _bytes(whole)


def test_tmp_dir_is_honoured_and_emptied(dna, tmp_path):
    d, whole, shards, (mib, _) = dna
    args = ["merge", "--shared-keys", "--stream", "--budget-mib", str(mib), "--num-tree-nodes", str(N_GROUPS + 1)]
    mine = tmp_path / "mine"
    mine.mkdir()
    out = tmp_path / "a.ipk"
    invoke(args + ["--tmp-dir", str(mine), "-o", str(out)] + shards)
    assert _bytes(out) == _bytes(whole)
    assert os.listdir(mine) == [] and sorted(os.listdir(tmp_path)) == ["a.ipk", "mine"]       # a directory that was there stays, empty; no a.ipk.ranges
    # it is there the range files go: a directory that cannot be made stops the call, which names it and leaves no output
    nowhere = tmp_path / "missing" / "ranges"
    res = CliRunner().invoke(cli.ipk, args + ["--tmp-dir", str(nowhere), "-o", str(tmp_path / "c.ipk")] + shards)
    assert res.exit_code != 0 and str(nowhere) in res.output + str(res.exception)
    assert sorted(os.listdir(tmp_path)) == ["a.ipk", "mine"]
