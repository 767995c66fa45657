"""GPU suite: `ipk.py diff --stream [--budget-mib N]` prints what `ipk.py diff` prints and returns its status, on a built pair that
differs (another omega) and on an equal pair, also under a budget small enough to split the comparison into key ranges;
`ipk.py dump --key-range` and `ipk.py subset --key-range` against the records of the file read on the host."""
import numpy as np
import pytest
from click.testing import CliRunner

from ipk_amd import cli, dbfile
from oracle import tree_oracle as to
from tests import diff_files_cases as D
from tests.test_cli import _reference_workdir

pytestmark = pytest.mark.gpu

K = 7


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_diff_files")
    tree_file, ar_dir, _ = _reference_workdir(d, 7, 60, 321)
    out = {"dir": d}
    for name, extra in (("mif0", ["--filter", "mif0"]), ("random", ["--filter", "random"]), ("omega", ["--omega", "1.25"])):
        out[name] = d / f"{name}.ipk"
        res = CliRunner().invoke(cli.ipk, ["build", "-t", str(tree_file), "-w", str(d / f"work_{name}"), "-k", str(K), "--ar-dir", str(ar_dir),
                                           "-o", str(out[name]), "-v", "0"] + extra)
        assert res.exit_code == 0, (res.output, res.exception)
    return out


def side_of(path, window):
    """The file as tests/diff_files_cases.Side: its lists, and its arrays in the file's own record order."""
    hdr, recs = dbfile.read_db(path)
    lists = {int(key): [[int(b), np.float32(s), 0] for b, s in zip(br, sc)] for key, fv, br, sc in recs}
    keys = np.array(sorted(lists), np.uint32)
    index = {int(k): i for i, k in enumerate(keys)}
    counts = np.array([len(lists[int(k)]) for k in keys], np.int64)
    db = dict(keys=keys, off=np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), order=np.array([index[int(key)] for key, *_ in recs], np.uint32))
    return hdr, D.Side(lists, False, window, lambda _: db)


def splitting_budget(path_a, path_b, max_records):
    """KiB of a budget under which the restated plan (window by the default rule) has at least two ranges."""
    for kib in (4096, 2048, 1024, 512, 256, 128, 64):
        window = D.default_window(kib << 10)
        (ha, a), (hb, b) = side_of(path_a, window), side_of(path_b, window)
        try:
            if len(D.plan(a, b, kib << 10, max_records, ha, hb)) >= 2:
                return kib
        except D.NoRoom:
            break
    raise AssertionError("no budget splits this pair")


@pytest.mark.parametrize("pair,status", [(("mif0", "omega"), 1), (("mif0", "random"), 0), (("omega", "mif0"), 1)])
def test_stream_prints_what_diff_prints(builds, pair, status):
    a, b = str(builds[pair[0]]), str(builds[pair[1]])
    for args, m in (([], 0), (["-v", "--max-records", "7"], 7), (["--exact", "-v"], 100)):
        plain = CliRunner().invoke(cli.ipk, ["diff"] + args + [a, b])
        assert plain.exit_code == status, (plain.output, plain.exception)
        kib = splitting_budget(a, b, m)
        for extra in (["--stream"], ["--stream", "--budget-mib", repr(kib / 1024)]):
            got = CliRunner().invoke(cli.ipk, ["diff"] + args + extra + [a, b])
            assert got.exit_code == status, (got.output, got.exception)
            assert got.output == plain.output, extra
    alone = CliRunner().invoke(cli.ipk, ["diff", "--budget-mib", "8", a, b])
    assert alone.exit_code == 2 and "--stream" in alone.output


def lines_for(hdr, recs):
    pre, stack = {}, [to.postorder(to.parse(hdr["newick"]))[-1]]
    while stack:
        n = stack.pop()
        pre[n.postorder] = len(pre)
        stack.extend(reversed(n.children))
    out = []
    for key, fv, br, sc in recs:
        out.append("".join("ACGT"[(key >> (2 * (K - 1 - i))) & 3] for i in range(K)))
        out += ["\t%g\t%d" % (10.0 ** float(s), pre[int(x)]) for x, s in zip(br, sc)]
    return out


def test_dump_and_subset_of_a_key_range(builds):
    path = builds["mif0"]
    hdr, recs = dbfile.read_db(path)
    keys = sorted(int(r[0]) for r in recs)
    lo, hi = keys[len(keys) // 3], keys[2 * len(keys) // 3]
    inside = [r for r in recs if lo <= int(r[0]) < hi]                    # file order among themselves
    assert 0 < len(inside) < len(recs) and [int(r[0]) for r in inside] != sorted(int(r[0]) for r in inside)
    res = CliRunner().invoke(cli.ipk, ["dump", "--key-range", f"{lo}:{hi}", str(path)])
    assert res.exit_code == 0, (res.output, res.exception)
    assert res.output.splitlines() == lines_for(hdr, inside)
    res = CliRunner().invoke(cli.ipk, ["dump", "--key-range", f"{lo}:{hi}", "--limit", "2", str(path)])
    assert res.exit_code == 0 and res.output.splitlines() == lines_for(hdr, inside[:2])
    out = builds["dir"] / "range.ipk"
    res = CliRunner().invoke(cli.ipk, ["subset", "-i", str(path), "-o", str(out), "--key-range", f"{lo}:{hex(hi)}"])
    assert res.exit_code == 0, (res.output, res.exception)
    hdr2, recs2 = dbfile.read_db(out)
    assert hdr2 == dict(hdr, total_num_kmers=len(inside), total_num_entries=sum(len(r[2]) for r in inside))
    assert len(recs2) == len(inside)
    for (k1, f1, b1, s1), (k2, f2, b2, s2) in zip(recs2, inside):
        assert k1 == k2 and np.float32(f1).view(np.uint32) == np.float32(f2).view(np.uint32)
        assert np.array_equal(b1, b2) and np.array_equal(np.asarray(s1, np.float32).view(np.uint32), np.asarray(s2, np.float32).view(np.uint32))
    for bad in ("5", "7:3", "a:b", f"0:{(1 << 32) + 1}"):
        assert CliRunner().invoke(cli.ipk, ["dump", "--key-range", bad, str(path)]).exit_code == 2
    assert CliRunner().invoke(cli.ipk, ["subset", "-i", str(path), "-o", str(out), "--key-range", "0:5", "--mu", "0.5"]).exit_code == 2
