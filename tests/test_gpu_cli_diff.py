"""GPU suite: `ipk.py diff` and `ipk.py dump` (the reference's ipkdiff / ipkdump) over files built by `ipk.py build` from a
reference-format workdir (the input helpers of tests/test_cli.py)."""
import numpy as np
import pytest
from click.testing import CliRunner

from ipk_amd import cli, dbfile
from oracle import tree_oracle as to
from tests.test_cli import _reference_workdir

pytestmark = pytest.mark.gpu

K = 7
LINES = ["Sequence type", "Position support", "Protocol version", "k-mer size", "Omega", "Threshold", "Reference tree", "Tree index",
         "Number of k-mers", "Number of phylo-k-mers", "Phylo-k-mer scores"]


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_diff")
    tree_file, ar_dir, _ = _reference_workdir(d, 7, 60, 321)
    out = {}
    for name, extra in (("mif0", ["--filter", "mif0"]), ("random", ["--filter", "random"]), ("omega", ["--omega", "1.25"])):
        out[name] = d / f"{name}.ipk"
        res = CliRunner().invoke(cli.ipk, ["build", "-t", str(tree_file), "-w", str(d / f"work_{name}"), "-k", str(K), "--ar-dir", str(ar_dir),
                                           "-o", str(out[name]), "-v", "0"] + extra)
        assert res.exit_code == 0, (res.output, res.exception)
    return out


def lines_of(output):
    """{line name: [status, values...]} of the tab-separated report"""
    rep = {}
    for ln in output.splitlines():
        if ln and not ln.startswith("\t") and ":\t" in ln:
            name, rest = ln.split(":\t", 1)
            rep[name] = rest.split("\t")
    return rep


def test_same_inputs_two_filters_are_equal(builds):
    """--filter mif0 and --filter random write the same k-mers in another order, with other filter values: no difference."""
    assert builds["mif0"].read_bytes() != builds["random"].read_bytes()
    for args in ([], ["--exact"], ["-v"]):
        res = CliRunner().invoke(cli.ipk, ["diff"] + args + [str(builds["mif0"]), str(builds["random"])])
        assert res.exit_code == 0, (res.output, res.exception)
        rep = lines_of(res.output)
        assert list(rep) == LINES                                # the reference's lines, in its order (plus Position support)
        assert all(v[0] == "OK" for v in rep.values()), res.output
        assert rep["k-mer size"][1:] == [str(K), str(K)] and rep["Sequence type"][1:] == ["DNA", "DNA"]
        assert rep["Omega"][1:] == ["1.5", "1.5"] and rep["Phylo-k-mer scores"][1] == "0"
        hdr = dbfile.file_info(builds["mif0"])
        assert rep["Number of k-mers"][1:] == [str(hdr["total_num_kmers"])] * 2
        assert rep["Number of phylo-k-mers"][1:] == [str(hdr["total_num_entries"])] * 2


def test_another_omega_differs(builds):
    res = CliRunner().invoke(cli.ipk, ["diff", "-v", "--max-records", "7", str(builds["mif0"]), str(builds["omega"])])
    assert res.exit_code == 1, (res.output, res.exception)
    rep = lines_of(res.output)
    assert list(rep) == LINES
    for name in ("Omega", "Threshold", "Number of k-mers", "Number of phylo-k-mers", "Phylo-k-mer scores"):
        assert rep[name][0] == "DIFF", name
    for name in ("Sequence type", "Position support", "Protocol version", "k-mer size", "Reference tree", "Tree index"):
        assert rep[name][0] == "OK", name
    assert rep["Omega"][1:] == ["1.5", "1.25"]
    a, b = dbfile.file_info(builds["mif0"]), dbfile.file_info(builds["omega"])
    # a lower omega is a lower threshold (omega / 4)^k: more k-mers pass
    assert b["total_num_entries"] > a["total_num_entries"]
    # every entry of A is one of B's with the same score, so the differences are B's surplus
    assert int(rep["Phylo-k-mer scores"][1]) == b["total_num_entries"] - a["total_num_entries"]
    body = res.output.split("\t\tcode\tk-mer\tbranch\tA score\tB score\n", 1)[1]
    recs = [ln.split("\t") for ln in body.splitlines() if ln.startswith("\t\t")]
    assert len(recs) == 7                                        # --max-records
    codes = [int(r[2]) for r in recs]
    assert codes == sorted(codes)
    for r in recs:
        assert r[3] == "".join("ACGT"[(int(r[2]) >> (2 * (K - 1 - i))) & 3] for i in range(K))
        assert r[5] == "-" and 0.0 < float(r[6]) <= 1.0          # scored in B only
    # without -v no records, the same status
    quiet = CliRunner().invoke(cli.ipk, ["diff", str(builds["mif0"]), str(builds["omega"])])
    assert quiet.exit_code == 1 and "\t\tcode" not in quiet.output


def test_dump_prints_the_file_in_record_order(builds):
    res = CliRunner().invoke(cli.ipk, ["dump", "--limit", "3", str(builds["mif0"])])
    assert res.exit_code == 0, (res.output, res.exception)
    hdr, recs = dbfile.read_db(builds["mif0"])
    # pre-order ids of the header's tree, restated: root 0, children in file order
    pre, stack = {}, [to.postorder(to.parse(hdr["newick"]))[-1]]
    while stack:
        n = stack.pop()
        pre[n.postorder] = len(pre)
        stack.extend(reversed(n.children))
    lines = res.output.splitlines()
    at = 0
    for key, fv, br, sc in recs[:3]:
        assert lines[at] == "".join("ACGT"[(key >> (2 * (K - 1 - i))) & 3] for i in range(K))
        assert lines[at + 1] == "\t%g\t%d" % (10.0 ** float(sc[0]), pre[int(br[0])])      # 10^score as the command documents: %g
        for j in range(len(br)):
            assert lines[at + 1 + j].split("\t")[2] == str(pre[int(br[j])])
        at += 1 + len(br)
    assert at == len(lines)
