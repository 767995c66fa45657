"""GPU suite: `ipk.py place --stream-db` and `ipk.py subset --queries` over the file of a placement case (tests/stream_cases.py): the
streamed placement prints the TSV `place` prints, byte for byte, and the subset file is the restriction."""
import pytest
from click.testing import CliRunner

import ipk_amd
from ipk_amd import cli
from tests import db_files as F
from tests import place_ext_cases as xc
from tests import select_cases as S
from tests import stream_cases as T
from tests.test_gpu_db_select import check

pytestmark = pytest.mark.gpu

MU, OMEGA = 0.7, 1.75


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_stream")
    case = xc.main_ext_case()
    db = T.case_db_dict(case)
    path = F.write(d / "db.ipk", db, False, T.case_header(case))
    fasta = d / "reads.fasta"
    fasta.write_text("".join(f">q{i}\n{q}\n" for i, q in enumerate(case.queries[:9])))
    return d, case, db, path, fasta


def run(args):
    res = CliRunner().invoke(cli.ipk, [str(a) for a in args])
    assert res.exit_code == 0, (res.output, res.exception)
    return res.output


@pytest.mark.parametrize("options", [[], ["--mu", MU, "--omega", OMEGA], ["--expand-ambiguous", "--strands", "both"],
                                     ["--mu", MU, "--omega", OMEGA, "--expand-ambiguous", "--strands", "both"]], ids=["plain", "selection", "ext", "both"])
def test_streamed_place_prints_the_same_tsv(files, options):
    _, _, _, path, fasta = files
    want = run(["place", "-i", path, "-q", fasta] + options)
    assert any(ln.split("\t")[1] != "-" for ln in want.splitlines())
    assert run(["place", "-i", path, "-q", fasta, "--stream-db", "--query-batch", 2] + options) == want
    assert run(["place", "-i", path, "-q", fasta, "--stream-db"] + options) == want


def test_subset_with_queries_writes_the_restriction(engine, files):
    d, case, db, path, fasta = files
    queries = case.queries[:9]
    for name, options, (ambiguity, strands), (mu, omega) in (("plain", [], (False, "given"), (None, None)),
                                                             ("ext", ["--expand-ambiguous", "--strands", "both", "--mu", MU, "--omega", OMEGA],
                                                              (True, "both"), (MU, OMEGA))):
        out = d / f"sub_{name}.ipk"
        run(["subset", "-i", path, "-o", out, "--queries", fasta] + options)
        codes = T.kmer_codes(queries, case.sigma, case.k, ambiguity, strands)
        m = len(db["keys"]) if mu is None else ipk_amd.engine.mu_kmers(mu, len(db["keys"]))
        t = S.NEG_INF if omega is None else ipk_amd.log_threshold(omega, case.sigma, case.k)
        want = T.expected(db, codes, m, t, positioned=False)
        assert 0 < len(want["keys"]) < len(db["keys"])
        back = engine.load_db(out)
        try:
            check(back, want, False, dict(back.header))
            assert back.header["omega"] == (F.HEADER["omega"] if omega is None else OMEGA)
        finally:
            back.free()
        # the subset places its reads as the file does
        assert run(["place", "-i", out, "-q", fasta] + options[:3]) == run(["place", "-i", path, "-q", fasta] + options)
