"""GPU suite of the command line over branch shards: `ipk.py build --group-range` three times and `ipk.py merge --shared-keys` give the
plain build's file byte for byte; `place --shared-keys` places as on that file; `merge` without --shared-keys refuses the shards as
ever."""
import numpy as np
import pytest
from click.testing import CliRunner

from ipk_amd import cli, dbfile
from ipk_amd.cli import decode_kmer
from tests.test_loader import write_probs

pytestmark = pytest.mark.gpu

N_GROUPS, RANGES = 12, ["0:5", "5:6", "6:12"]


def _bytes(path):
    with open(path, "rb") as fh:
        return fh.read()


def inputs(tmp_path, sigma, sites, seed):
    ar_dir = tmp_path / "AR"; ar_dir.mkdir()
    labels = [f"{i}_X{j}" for i in range(N_GROUPS) for j in range(2)]
    write_probs(ar_dir / "ar.raxml.ancestralProbs", sigma, labels, sites, seed, extras=False)
    with open(tmp_path / "map.tsv", "w") as fh:
        for i, lab in enumerate(labels):
            fh.write(f"{lab}\t{20 + i // 2}\n")
    return ["build", "-w", str(tmp_path), "--ar-dir", str(ar_dir), "--mapping", str(tmp_path / "map.tsv"), "--omega", "1.5"]


def invoke(args):
    res = CliRunner().invoke(cli.ipk, args)
    assert res.exit_code == 0, (args, res.output, res.exception)
    return res


@pytest.fixture(scope="module")
def dna(tmp_path_factory):
    """The DNA k = 8 MIF0 build: the plain build's file and the three branch shards (--mapping and no tree: N = 12 groups + 1)."""
    d = tmp_path_factory.mktemp("cli_join_dna")
    base = inputs(d, 4, 64, 71) + ["-k", "8"]
    invoke(base + ["-o", str(d / "whole.ipk")])
    shards = []
    for i, r in enumerate(RANGES):
        invoke(base + ["--group-range", r, "-o", str(d / f"shard{i}.ipk")])
        shards.append(str(d / f"shard{i}.ipk"))
    return d, str(d / "whole.ipk"), shards


def test_group_range_builds_merged_are_the_plain_build_dna_mif0(dna):
    d, whole, shards = dna
    infos = [dbfile.file_info(p) for p in shards]
    assert sum(i["total_num_entries"] for i in infos) == dbfile.file_info(whole)["total_num_entries"]
    assert sum(i["total_num_kmers"] for i in infos) > dbfile.file_info(whole)["total_num_kmers"]          # the shards share k-mers
    out = d / "joined.ipk"
    res = invoke(["merge", "--shared-keys", "--num-tree-nodes", str(N_GROUPS + 1), "-o", str(out)] + shards)
    assert "merged on the device" in res.output and "0 entries joined by put" in res.output
    assert f"({dbfile.file_info(whole)['total_num_kmers']} k-mers, {dbfile.file_info(whole)['total_num_entries']} entries" in res.output
    assert _bytes(out) == _bytes(whole)


def test_group_range_builds_merged_are_the_plain_build_aa_positions_random(tmp_path):
    base = inputs(tmp_path, 20, 40, 72) + ["-k", "3", "-s", "amino", "--keep-positions", "--filter", "random"]
    invoke(base + ["-o", str(tmp_path / "whole.ipk")])
    shards = []
    for i, r in enumerate(RANGES):
        invoke(base + ["--group-range", r, "-o", str(tmp_path / f"shard{i}.ipk")])
        shards.append(str(tmp_path / f"shard{i}.ipk"))
    assert dbfile.file_info(shards[0])["positions_loaded"]
    out = tmp_path / "joined.ipk"
    invoke(["merge", "--shared-keys", "--filter", "random", "-o", str(out)] + shards)
    assert _bytes(out) == _bytes(tmp_path / "whole.ipk")
    # the same shard twice: every entry of the second copy is a duplicate, and the file is the shard's own
    res = invoke(["merge", "--shared-keys", "--filter", "random", "-o", str(tmp_path / "twice.ipk"), shards[1], shards[1]])
    n = dbfile.file_info(shards[1])["total_num_entries"]
    assert f"{n} entries joined by put" in res.output and _bytes(tmp_path / "twice.ipk") == _bytes(shards[1])


def test_merge_without_shared_keys_refuses_as_ever(dna):
    d, _, shards = dna
    res = CliRunner().invoke(cli.ipk, ["merge", "-o", str(d / "refused.ipk")] + shards)
    assert res.exit_code != 0
    text = res.output + str(res.exception)
    assert "is in source" in text and "a union takes disjoint key sets" in text


def test_group_range_beyond_the_groups_is_a_usage_error(dna, tmp_path):
    d, _, _ = dna
    res = CliRunner().invoke(cli.ipk, ["build", "-w", str(d), "--ar-dir", str(d / "AR"), "--mapping", str(d / "map.tsv"), "-k", "8", "--group-range", "6:13",
                                       "-o", str(tmp_path / "x.ipk")])
    assert res.exit_code == 2 and "there are 12 branch groups" in res.output


def test_place_on_branch_shards(dna, tmp_path):
    d, whole, shards = dna
    hdr, recs = dbfile.read_db(whole)
    rng = np.random.default_rng(5)
    keys = [r[0] for r in recs]
    reads = ["".join(decode_kmer(int(x), 8, "DNA") for x in rng.choice(keys, size=4, replace=False)) for _ in range(12)]
    q = tmp_path / "reads.fasta"
    q.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(reads)))
    for extra in ([], ["--mu", "0.5"], ["--omega", "1.75"]):
        one = CliRunner().invoke(cli.ipk, ["place", "-i", whole, "-q", str(q)] + extra)
        many = CliRunner().invoke(cli.ipk, ["place", "--shared-keys", "--num-tree-nodes", str(N_GROUPS + 1), "-q", str(q)] + [x for p in shards for x in ("-i", p)] + extra)
        assert one.exit_code == 0 and many.exit_code == 0, (one.output, many.output, many.exception)
        assert many.output == one.output and one.output.count("\n") >= 12
