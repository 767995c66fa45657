"""GPU suite: `ipk.py place --expand-ambiguous --strands both` end to end on a written database file (the strand case of
tests/place_ext_cases.py): the seven-column TSV equals what the oracle (tests/place_ext_oracle.py) and the keep-factor rule give;
without the flags the output is the six columns it was."""
import pytest
from click.testing import CliRunner

from ipk_amd import cli
from tests import place_cases as pc
from tests import place_ext_cases as xc
from tests import place_ext_oracle as xo
from tests import place_oracle as po

pytestmark = pytest.mark.gpu

KEEP_FACTOR = 0.01


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_place_ext")
    c = xc.strand_case()
    db = pc.write_case_db(d / "strand.ipk", c)
    fasta = d / "reads.fasta"
    fasta.write_text("".join(f">q{i} text\n{s[:40]}\n{s[40:]}\n" for i, s in enumerate(c.queries)))
    return d, db, fasta, c


def expected_lines(c, ambiguity, strands):
    """The first five columns and the strand sign per line, and (lwr, scored branches) or None per line."""
    import ipk_amd
    log_eps = ipk_amd.log_threshold(1.5, c.sigma, c.k)               # write_case_db writes omega = 1.5
    lines, lwrs = [], []
    for i, s in enumerate(c.queries):
        r = xo.place_one(c.view, s.replace("-", ""), c.sigma, c.k, log_eps, 7, ambiguity, strands)      # (read_fasta drops gaps)
        sign = "-" if r["strand"] else "+"
        kept = [p for p in r["placements"] if p[3] >= KEEP_FACTOR * r["placements"][0][3]]
        for b, score, count, lwr in kept:
            lines.append([f"q{i}", str(b), "%.9g" % float(score), str(count), str(r["n_kmers"]), sign])
            lwrs.append((lwr, r["n_branches"]))
        if not kept:
            lines.append([f"q{i}", "-", "-", "-", str(r["n_kmers"]), sign])
            lwrs.append(None)
    return lines, lwrs


def run(files, flags, to_file):
    d, db, fasta, _ = files
    out = d / "out.tsv"
    res = CliRunner().invoke(cli.ipk, ["place", "-i", str(db), "-q", str(fasta)] + flags + (["-o", str(out)] if to_file else []))
    assert res.exit_code == 0, (res.output, res.exception)
    return [ln.split("\t") for ln in (out.read_text() if to_file else res.output).splitlines()]


def check(got, want, lwrs, columns):
    assert all(len(g) == columns for g in got)
    assert [g[:5] + g[6:] for g in got] == [w[:5] + (w[5:] if columns == 7 else []) for w in want]
    for g, w in zip(got, lwrs):
        if w is None:
            assert g[5] == "-"
        else:
            assert abs(float(g[5]) - w[0]) <= po.lwr_tolerance(w[1]) * w[0]


@pytest.mark.parametrize("ambiguity,to_file", [(True, True), (False, False)])
def test_both_strands_write_seven_columns(files, ambiguity, to_file):
    c = files[3]
    got = run(files, (["--expand-ambiguous"] if ambiguity else []) + ["--strands", "both"], to_file)
    want, lwrs = expected_lines(c, ambiguity, "both")
    check(got, want, lwrs, 7)
    signs = {g[0]: g[6] for g in got}
    assert signs[f"q{xc.STRAND['reverse_wins']}"] == "-" and signs[f"q{xc.STRAND['given_wins']}"] == "+" and signs[f"q{xc.STRAND['neither']}"] == "+"
    assert signs[f"q{xc.STRAND['codes']}"] == ("-" if ambiguity else "+")


def test_expand_ambiguous_alone_and_no_flags_write_six_columns(files):
    c = files[3]
    want, lwrs = expected_lines(c, True, "given")
    check(run(files, ["--expand-ambiguous"], True), want, lwrs, 6)
    plain, plain_lwrs = expected_lines(c, False, "given")
    assert plain != want
    got = run(files, [], False)
    check(got, plain, plain_lwrs, 6)
    assert got == run(files, ["--strands", "given"], False)
