"""GPU suite: `ipk.py place` over a file written by `ipk.py build` from a reference-format workdir (the input helpers of
tests/test_cli.py): the TSV equals what the oracle (tests/place_oracle.py) and the keep-factor rule give."""
import numpy as np
import pytest
from click.testing import CliRunner

import ipk_amd
from ipk_amd import cli, dbfile
from tests import place_oracle as po
from tests.test_cli import _reference_workdir

pytestmark = pytest.mark.gpu

K = 7


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_place")
    tree_file, ar_dir, _ = _reference_workdir(d, 7, 60, 321)
    out = d / "DB.ipk"
    res = CliRunner().invoke(cli.ipk, ["build", "-t", str(tree_file), "-w", str(d / "work"), "-k", str(K), "--ar-dir", str(ar_dir), "-o", str(out),
                                       "-v", "0"])
    assert res.exit_code == 0, (res.output, res.exception)
    return d, out


def expected_lines(db_file, records, keep_at_most, keep_factor):
    hdr, (keys, fvs, counts, eoff, br, sc) = dbfile.read_db(db_file, as_arrays=True)
    view = po.DbView(keys, eoff, br, sc)
    log_eps = ipk_amd.log_threshold(hdr["omega"], 4, hdr["kmer_size"])
    lines, lwrs, dropped = [], [], 0
    for name, seq in records:
        r = po.place_one(view, seq, 4, hdr["kmer_size"], log_eps, keep_at_most)
        kept = [p for p in r["placements"] if p[3] >= keep_factor * r["placements"][0][3]]
        dropped += len(r["placements"]) - len(kept)
        for b, score, count, lwr in kept:
            lines.append([name, str(b), "%.9g" % float(score), str(count), str(r["n_kmers"])])
            lwrs.append((lwr, r["n_branches"]))
        if not kept:
            lines.append([name, "-", "-", "-", str(r["n_kmers"])])
            lwrs.append(None)
    return lines, lwrs, dropped


@pytest.mark.parametrize("keep_at_most,keep_factor,to_file", [(7, 0.01, True), (3, 0.5, False), (64, 0.0, True)])
def test_place_writes_what_the_oracle_gives(built, keep_at_most, keep_factor, to_file):
    d, db_file = built
    hdr, recs = dbfile.read_db(db_file)
    rng = np.random.default_rng(5)
    kmers = [cli.decode_kmer(recs[i][0], K, "DNA") for i in rng.choice(len(recs), 40)]
    records = [("hits", "".join(kmers[:12])), ("lower", "".join(kmers[12:20]).lower().replace("t", "u")), ("random", "".join(rng.choice(list("ACGT"), 150))),
               ("none", "NNNNNNNNNN"), ("short", "ACG"), ("gapped", "".join(kmers[20:30]))]
    fasta = d / "reads.fasta"
    gapped = records[5][1]
    fasta.write_text("".join(f">{n} some description\n{s[:50]}\n{s[50:]}\n" for n, s in records[:5])
                     + f">gapped\n{gapped[:11]}-{gapped[11:30]}.. \n{gapped[30:]}\n")
    args = ["place", "-i", str(db_file), "-q", str(fasta), "--keep-at-most", str(keep_at_most), "--keep-factor", str(keep_factor)]
    out = d / f"out_{keep_at_most}.tsv"
    res = CliRunner().invoke(cli.ipk, args + (["-o", str(out)] if to_file else []))
    assert res.exit_code == 0, (res.output, res.exception)
    text = out.read_text() if to_file else res.output
    got = [ln.split("\t") for ln in text.splitlines()]
    want, lwrs, dropped = expected_lines(db_file, records, keep_at_most, keep_factor)
    assert [g[:5] for g in got] == want and all(len(g) == 6 for g in got)
    # the inputs do what they are for: queries without a placement, the three made of the file's k-mers placed, and the keep-factor
    # rule cutting placements off wherever it is not 0
    assert any(w is None for w in lwrs) and sum(w is not None for w in lwrs) >= 3
    assert {"hits", "lower", "gapped"} <= {g[0] for g in got if g[1] != "-"} and (dropped > 0) == (keep_factor > 0)
    for g, w in zip(got, lwrs):
        if w is None:
            assert g[5] == "-"
        else:
            assert abs(float(g[5]) - w[0]) <= po.lwr_tolerance(w[1]) * w[0]
