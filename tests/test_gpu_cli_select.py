"""GPU suite: `ipk.py subset` and `ipk.py place --mu --omega` over a file written by `ipk.py build` (the input helpers of
tests/test_cli.py): the subset file equals the one written from the numpy restatement of the selection (tests/select_cases.py), and
placing with the options equals placing on the subset file."""
import numpy as np
import pytest
from click.testing import CliRunner

import ipk_amd
from ipk_amd import cli, dbfile
from tests import select_cases as S
from tests.test_cli import _reference_workdir

pytestmark = pytest.mark.gpu

K, MU, OMEGA = 7, 0.5, 1.8


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_select")
    tree_file, ar_dir, _ = _reference_workdir(d, 7, 60, 321)
    out = d / "DB.ipk"
    res = CliRunner().invoke(cli.ipk, ["build", "-t", str(tree_file), "-w", str(d / "work"), "-k", str(K), "--ar-dir", str(ar_dir), "-o", str(out),
                                       "-v", "0"])
    assert res.exit_code == 0, (res.output, res.exception)
    sub = d / "sub.ipk"
    res = CliRunner().invoke(cli.ipk, ["subset", "-i", str(out), "-o", str(sub), "--mu", str(MU), "--omega", str(OMEGA)])
    assert res.exit_code == 0, (res.output, res.exception)
    return d, out, sub


def file_as_arrays(path):
    """(header, the file's database as a dictionary of tests/select_cases.restate: keys ascending, order = the file's record order)."""
    hdr, (keys_f, fv_f, counts, eoff, br_f, sc_f) = dbfile.read_db(path, as_arrays=True)
    perm = np.argsort(keys_f, kind="stable")
    order = np.empty(len(perm), np.uint32)
    order[perm] = np.arange(len(perm), dtype=np.uint32)
    cnt = np.asarray(counts, np.int64)[perm]
    take = np.concatenate([np.arange(int(eoff[r]), int(eoff[r]) + int(counts[r])) for r in perm] + [np.zeros(0, np.int64)]).astype(np.int64)
    return hdr, dict(keys=np.asarray(keys_f, np.uint32)[perm], off=np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64), br=np.asarray(br_f, np.uint32)[take],
                     sc=np.asarray(sc_f, np.float32)[take], fv=np.asarray(fv_f, np.float32)[perm], order=order)


def test_subset_writes_the_restated_selection(built):
    d, db_file, sub = built
    hdr, db = file_as_arrays(db_file)
    assert hdr["omega"] == 1.5
    m = ipk_amd.engine.mu_kmers(MU, len(db["keys"]))
    v = S.restate(db, m, ipk_amd.log_threshold(OMEGA, 4, K), positioned=False)
    # the input does what it is for: mu leaves k-mers out, and omega leaves out entries of the k-mers that stay
    assert 0 < len(v["keys"]) <= m < len(db["keys"]) and 0 < len(v["br"]) < len(S.restate(db, m, -np.inf, positioned=False)["br"])
    want = d / "want.ipk"
    dbfile.write_db(want, hdr["sequence_type"], hdr["tree_index"], hdr["newick"], K, OMEGA, v["keys"], v["off"], v["br"], v["sc"], v["fv"], v["order"])
    res = CliRunner().invoke(cli.ipk, ["diff", "--exact", str(sub), str(want)])
    assert res.exit_code == 0, res.output
    assert sub.read_bytes() == want.read_bytes()
    info = dbfile.file_info(sub)
    assert info["omega"] == np.float32(OMEGA) and info["total_num_kmers"] == len(v["keys"])
    # without options: the file itself
    same = d / "same.ipk"
    res = CliRunner().invoke(cli.ipk, ["subset", "-i", str(db_file), "-o", str(same)])
    assert res.exit_code == 0 and same.read_bytes() == db_file.read_bytes()


def test_place_with_the_options_is_place_on_the_subset(built):
    d, db_file, sub = built
    _, recs = dbfile.read_db(db_file)
    rng = np.random.default_rng(8)
    kmers = [cli.decode_kmer(recs[i][0], K, "DNA") for i in rng.choice(len(recs), 60)]
    fasta = d / "reads.fasta"
    fasta.write_text("".join(f">q{i}\n{''.join(kmers[10 * i:10 * i + 10])}\n" for i in range(6)) + ">none\nNNNNNNNNN\n")
    a = CliRunner().invoke(cli.ipk, ["place", "-i", str(db_file), "-q", str(fasta), "--mu", str(MU), "--omega", str(OMEGA)])
    b = CliRunner().invoke(cli.ipk, ["place", "-i", str(sub), "-q", str(fasta)])
    whole = CliRunner().invoke(cli.ipk, ["place", "-i", str(db_file), "-q", str(fasta)])
    assert a.exit_code == 0 and b.exit_code == 0 and whole.exit_code == 0, (a.output, b.output)
    assert a.output == b.output and a.output != whole.output
    assert any(ln.split("\t")[1] != "-" for ln in a.output.splitlines())


@pytest.mark.parametrize("command", ["subset", "place"])
def test_an_omega_below_the_files_is_refused(built, command):
    d, db_file, _ = built
    fasta = d / "one.fasta"
    fasta.write_text(">q\nACGTACGTACGT\n")
    args = ["subset", "-i", str(db_file), "-o", str(d / "no.ipk")] if command == "subset" else ["place", "-i", str(db_file), "-q", str(fasta)]
    res = CliRunner().invoke(cli.ipk, args + ["--omega", "1.25"])
    assert res.exit_code != 0 and "below the file's omega" in res.output
    assert not (d / "no.ipk").exists()
    res = CliRunner().invoke(cli.ipk, args + ["--mu", "1.5"])
    assert res.exit_code != 0 and "--mu" in res.output


@pytest.mark.parametrize("omega", [1.7, 1.1])
def test_the_builds_own_omega_is_accepted(engine, tmp_path, omega):
    """A file whose omega rounds up in binary32 (1.7 -> 1.70000005): --omega equal to the build's is the file's omega, not below it.
    The synthetic file's scores do not all lie above its omega's threshold as a build's do, so the expectation is the restatement at
    that threshold: `subset` writes it, `place` with the option places as on it, Engine.load_db / select_db give its totals."""
    from tests import db_files as F
    assert float(np.float32(omega)) > omega
    header = dict(F.HEADER, omega=omega)
    db = S.edges()
    path = F.write(tmp_path / "w.ipk", db, header=header)
    v = S.restate(db, len(db["keys"]), ipk_amd.log_threshold(omega, 4, F.HEADER["kmer_size"]), positioned=False)
    assert 0 < len(v["keys"])
    want = F.write(tmp_path / "want.ipk", v, header=header)
    out = tmp_path / "out.ipk"
    res = CliRunner().invoke(cli.ipk, ["subset", "-i", str(path), "-o", str(out), "--omega", str(omega)])
    assert res.exit_code == 0, res.output
    assert out.read_bytes() == want.read_bytes()
    fasta = tmp_path / "q.fasta"
    fasta.write_text("".join(f">q{i}\n{q}\n" for i, q in enumerate(S.queries_of(db, F.HEADER["kmer_size"])[:4])))
    a = CliRunner().invoke(cli.ipk, ["place", "-i", str(path), "-q", str(fasta), "--omega", str(omega)])
    b = CliRunner().invoke(cli.ipk, ["place", "-i", str(want), "-q", str(fasta)])
    assert a.exit_code == 0 and b.exit_code == 0 and a.output == b.output, (a.output, b.output)
    assert any(ln.split("\t")[1] != "-" for ln in a.output.splitlines())
    loaded = engine.load_db(path, omega=omega)
    try:
        again = engine.select_db(loaded, omega=omega)
        assert again.num_entries == loaded.num_entries == len(v["br"]) and again.num_keys == loaded.num_keys == len(v["keys"])
        again.free()
    finally:
        loaded.free()
    res = CliRunner().invoke(cli.ipk, ["subset", "-i", str(path), "-o", str(tmp_path / "no.ipk"), "--omega", str(float(np.nextafter(np.float32(omega), np.float32(0))))])
    assert res.exit_code != 0 and "below the file's omega" in res.output
