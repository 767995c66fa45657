"""The inputs of the union suite, checked without a GPU: for every case of tests/union_cases.py the HOST merge of the shards' files
(ipkgpu_db_merge_files, the oracle of ipkgpu_db_union) equals the numpy restatement array for array, and the properties the cases
claim hold.  Also without a device: ipkgpu_db_union_bytes against its documented formula, `ipk.py merge --on host`, and the usage
errors of `merge`, `place -i A -i B` and `build --union-on-device`."""
import numpy as np
import pytest
from click.testing import CliRunner

import ipk_amd
from ipk_amd import cli, dbfile
from tests import db_files as F
from tests import union_cases as U

KINDS = [False, True]                                # plain, positioned


def test_case_list_is_complete():
    assert [c["name"] for c in U.all_cases()] == U.CASE_NAMES


def test_entryless_records_round_trip_on_the_host(tmp_path):
    """What the `entryless` case rests on: write_db -> read_db gives a record without entries back."""
    c = U.case("entryless")
    s = c["shards"][0]
    assert (s["off"][1:] == s["off"][:-1]).any()
    _, (keys, fvs, counts, eoff, br, sc) = dbfile.read_db(F.write(tmp_path / "s.ipk", s, False, c["header"]), as_arrays=True)
    o = s["order"]
    assert np.array_equal(keys, s["keys"][o]) and np.array_equal(counts, (s["off"][1:] - s["off"][:-1])[o]) and len(br) == len(s["br"])
    _, recs = dbfile.read_db(F.write(tmp_path / "p.ipk", s, True, c["header"]))
    assert [len(r[2]) for r in recs] == list((s["off"][1:] - s["off"][:-1])[o].astype(int))


@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_host_merge_is_the_restatement(tmp_path, name, positioned):
    c = U.case(name)
    want = c["want"]
    merged, _ = U.host_merged(tmp_path, c, positioned)
    off = want["off"].astype(np.int64)
    o = want["order"]
    if positioned:
        hdr, recs = dbfile.read_db(merged)
        assert hdr["positions_loaded"]
        assert np.array_equal(np.array([r[0] for r in recs], np.uint32), want["keys"][o])
        assert np.array_equal(np.array([r[1] for r in recs], np.float32).view(np.uint32), want["fv"][o].view(np.uint32))
        for r, i in zip(recs, o):
            a, b = off[i], off[i + 1]
            assert np.array_equal(r[2], want["br"][a:b]) and np.array_equal(r[3].view(np.uint32), want["sc"][a:b].view(np.uint32))
            assert np.array_equal(r[4], want["pos"][a:b])
    else:
        hdr, (keys, fvs, counts, eoff, br, sc) = dbfile.read_db(merged, as_arrays=True)
        assert np.array_equal(keys, want["keys"][o])
        assert np.array_equal(fvs.view(np.uint32), want["fv"][o].view(np.uint32))
        assert np.array_equal(counts.astype(np.int64), (off[1:] - off[:-1])[o])
        ent = np.concatenate([np.arange(off[i], off[i + 1]) for i in o] + [np.zeros(0, np.int64)]).astype(np.int64)
        assert np.array_equal(br, want["br"][ent]) and np.array_equal(sc.view(np.uint32), want["sc"][ent].view(np.uint32))
    assert hdr["kmer_size"] == c["header"]["kmer_size"] and hdr["newick"] == c["header"]["newick"]
    assert hdr["total_num_kmers"] == len(want["keys"]) and hdr["total_num_entries"] == int(off[-1])
    assert np.all(np.diff(want["keys"].astype(np.int64)) > 0)


def test_the_cases_hold_what_they_claim():
    sizes = lambda name: [len(s["keys"]) for s in U.case(name)["shards"]]
    for p in (1, 2, 3, 8):
        assert len(sizes(f"owners{p}")) == p and sum(sizes(f"owners{p}")) == 600 and min(sizes(f"owners{p}")) > 0
    cnt = np.diff(U.case("owners8")["want"]["off"].astype(np.int64))
    assert set(F.EDGE_COUNTS) <= set(cnt.tolist())
    assert sizes("owners5_one_empty")[4] == 0 and min(sizes("owners5_one_empty")[:4]) > 0
    r = U.case("ranges")
    assert sizes("ranges")[2] == 0 and all(n > 0 for i, n in enumerate(sizes("ranges")) if i != 2)
    edges = [(int(s["keys"][0]), int(s["keys"][-1])) for s in r["shards"] if len(s["keys"])]
    assert all(a[1] < b[0] for a, b in zip(edges, edges[1:]))
    # tiles: from the cumulative counts
    t = U.case("tiles")["want"]
    off = t["off"].astype(np.int64)
    cnt = np.diff(off)
    assert cnt[0] == U.TILE and off[1] % U.TILE == 0                                   # the second record starts at a tile boundary
    big = int(np.argmax(cnt))
    assert cnt[big] == 5000
    first_tile = -(-off[big] // U.TILE)
    assert (first_tile + 2) * U.TILE <= off[big + 1]                                   # two whole tiles inside the one record
    assert off[-1] % U.TILE != 0                                                       # the last tile is partial
    ones = np.nonzero(cnt == 1)[0]
    assert len(ones) >= U.TILES_RUN and np.array_equal(ones[:U.TILES_RUN], np.arange(ones[0], ones[0] + U.TILES_RUN))
    run_tiles = off[ones[0]:ones[0] + U.TILES_RUN] // U.TILE
    assert np.bincount(run_tiles - run_tiles[0]).max() > 256                           # more keys than lanes fall in one tile
    a, b = (s["keys"] for s in U.case("tiles")["shards"])
    src = np.zeros(len(t["keys"]), np.int64)
    src[np.searchsorted(t["keys"], b)] = 1
    assert np.all(src[1:] != src[:-1])                                                 # neighbouring keys from different shards throughout
    m = sizes("many_sources")
    assert len(m) == 65 and m[0] >= 400 and all(1 <= n <= 3 for n in m[1:])
    ft = U.case("filter_ties")
    bits = [set(s["fv"].view(np.uint32).tolist()) for s in ft["shards"]]
    for v in (np.float32(-0.0), np.float32(0.0), np.float32(-1.5), np.float32(1.5), U.F32_MAX, np.float32(0.25)):
        assert all(int(v.view(np.uint32)) in b for b in bits)                          # in every shard: equal values across shards
    w = ft["want"]
    code = dbfile.filter_sort_code(w["fv"], w["keys"])[w["order"]]
    assert np.all(np.diff(code.astype(object)) > 0)
    tie = w["fv"][w["order"]].view(np.uint32)
    same = np.nonzero(tie[1:] == tie[:-1])[0]
    assert len(same) and np.all(w["keys"][w["order"]][same + 1] > w["keys"][w["order"]][same])   # ties in ascending key order
    zeros = w["fv"][w["order"]].view(np.uint32)
    assert zeros.tolist().index(0x80000000) < zeros.tolist().index(0)                  # -0.0 sorts before +0.0
    kb = U.case("key_bounds")
    assert kb["header"]["kmer_size"] == 16 and kb["shards"][0]["keys"][0] == 0 and kb["shards"][1]["keys"][-1] == 0xFFFFFFFF
    el = U.case("entryless")["want"]
    cnt = np.diff(el["off"].astype(np.int64))
    assert cnt[0] == 0 and cnt[len(cnt) // 2] == 0 and cnt[-1] == 0 and (cnt > 0).sum() == len(cnt) - 3


# ---- ipkgpu_db_union_bytes -----------------------------------------------------------------------------------------------------------

def test_union_bytes_is_the_documented_formula():
    """Five points computed by hand from the formula of include/ipkgpu.h (r: rounded up to 256, 256 at least; m: 256 at least;
    sort(n) = 9 n + 32768; scan(n) = n / 8 + 4096)."""
    f = ipk_amd.Engine.union_bytes
    # (0, 0, 1, plain): result 6 x 256; table 256, 3 + 2 blocks of 256, sort 32768, scan 4096, 256
    assert f(0, 0, 1, False) == 1536 + 256 + 768 + 512 + 32768 + 4096 + 256 == 40192
    # (1000, 5000, 8, plain): result 3 x 4096 + 8192 + 8192 + 40192; table 504, 24000, 8000, sort 41768, scan 125 + 4096, 256
    assert f(1000, 5000, 8, False) == 68864 + 504 + 24000 + 8000 + 41768 + 4221 + 256 == 147613
    # positioned: + r(20000) = 20224
    assert f(1000, 5000, 8, True) == 147613 + 20224
    # (64, 64, 2, positioned): result 768 + 768 + 512 + 512 + 256; table 256, 1536, 512, sort 33344, scan 8 + 4096, 256
    assert f(64, 64, 2, True) == 2816 + 256 + 1536 + 512 + 33344 + 4104 + 256 == 42824
    # (2^20, 2^24, 64, plain): result 3 x 4 MiB + (8 MiB + 256) + 8 MiB + 128 MiB; table 3640, 3 x 8 MiB, 2 x 4 MiB, sort, scan, 256
    assert f(1 << 20, 1 << 24, 64, False) == 163578112 + 3640 + 25165824 + 8388608 + 9469952 + 135168 + 256 == 206741560


def test_union_bytes_is_monotone():
    f = ipk_amd.Engine.union_bytes
    base = (1000, 5000, 8, False)
    grid = [0, 1, 63, 64, 65, 1000, 1001, 4096, 100000]
    for a, b in zip(grid, grid[1:]):
        assert f(a, base[1], base[2], False) <= f(b, base[1], base[2], False)
        assert f(base[0], a, base[2], True) <= f(base[0], b, base[2], True)
        assert f(base[0], base[1], a + 1, False) <= f(base[0], base[1], b + 1, False)
    assert f(100000, 5000, 8, False) > f(1000, 5000, 8, False) and f(1000, 500000, 8, False) > f(*base) and f(1000, 5000, 800, False) > f(*base)
    assert f(1000, 5000, 8, True) > f(*base)


# ---- the command line, as far as it needs no device ------------------------------------------------------------------------------------

def _bytes(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
def test_cli_merge_on_host_writes_the_host_merge(tmp_path, positioned):
    c = U.case("owners3")
    merged, paths = U.host_merged(tmp_path, c, positioned)
    out = tmp_path / "cli.ipk"
    res = CliRunner().invoke(cli.ipk, ["merge", "--on", "host", "-o", str(out)] + paths)
    assert res.exit_code == 0, (res.output, res.exception)
    assert _bytes(out) == _bytes(merged)
    assert f"{len(c['want']['keys'])} k-mers" in res.output and "on the host" in res.output


def test_cli_merge_takes_the_tree_of_the_first_shard_that_has_one(tmp_path):
    """Pass files carry an empty tree: the head is that of the one shard with a tree, wherever it stands."""
    c = U.case("owners3")
    bare = dict(c["header"], tree_index=[], newick="")
    paths = [str(F.write(tmp_path / f"s{i}.ipk", s, False, c["header"] if i == 1 else bare)) for i, s in enumerate(c["shards"])]
    merged, _ = U.host_merged(tmp_path, c, False)
    out = tmp_path / "cli.ipk"
    res = CliRunner().invoke(cli.ipk, ["merge", "--on", "host", "-o", str(out)] + paths)
    assert res.exit_code == 0, (res.output, res.exception)
    assert _bytes(out) == _bytes(merged)
    other = dict(c["header"], newick="(a:1,b:1)r:0;", tree_index=[(3, 2.0), (1, 1.0), (1, 1.0)])
    paths[2] = str(F.write(tmp_path / "other_tree.ipk", c["shards"][2], False, other))
    res = CliRunner().invoke(cli.ipk, ["merge", "--on", "host", "-o", str(out)] + paths)
    assert res.exit_code == 2 and "other_tree.ipk" in res.output and "tree" in res.output


@pytest.mark.parametrize("field,value", [("sequence_type", "AA"), ("kmer_size", 9), ("omega", 1.25), ("positions", True)])
def test_cli_merge_names_the_shard_that_disagrees(tmp_path, field, value):
    c = U.case("owners2")
    good = str(F.write(tmp_path / "good.ipk", c["shards"][0], False, c["header"]))
    if field == "positions":
        bad = str(F.write(tmp_path / "odd_one.ipk", c["shards"][1], True, c["header"]))
    else:
        bad = str(F.write(tmp_path / "odd_one.ipk", c["shards"][1], False, dict(c["header"], **{field: value})))
    for on in ("host", "device"):                      # refused from the heads, before any engine is made
        res = CliRunner().invoke(cli.ipk, ["merge", "--on", on, "-o", str(tmp_path / "out.ipk"), good, bad])
        assert res.exit_code == 2, (res.output, res.exception)
        assert "odd_one.ipk" in res.output
        assert not (tmp_path / "out.ipk").exists()


def test_cli_merge_needs_a_shard(tmp_path):
    res = CliRunner().invoke(cli.ipk, ["merge", "-o", str(tmp_path / "out.ipk")])
    assert res.exit_code == 2


def test_cli_place_refuses_stream_db_with_a_shard_set(tmp_path):
    c = U.case("owners2")
    paths = U.write_shards(tmp_path, c, False)
    q = tmp_path / "q.fasta"
    q.write_text(">r\nACGTACGTACGT\n")
    res = CliRunner().invoke(cli.ipk, ["place", "-i", paths[0], "-i", paths[1], "-q", str(q), "--stream-db"])
    assert res.exit_code == 2 and "--stream-db" in res.output
    odd = str(F.write(tmp_path / "odd_one.ipk", c["shards"][1], False, dict(c["header"], kmer_size=9)))
    res = CliRunner().invoke(cli.ipk, ["place", "-i", paths[0], "-i", odd, "-q", str(q)])
    assert res.exit_code == 2 and "odd_one.ipk" in res.output


def test_cli_build_union_on_device_is_for_key_range_builds(tmp_path):
    res = CliRunner().invoke(cli.ipk, ["build", "-w", str(tmp_path), "-k", "10", "--union-on-device"])
    assert res.exit_code == 2 and "--union-on-device" in res.output and "key-range" in res.output
    res = CliRunner().invoke(cli.ipk, ["build", "-w", str(tmp_path), "-k", "6", "-s", "amino", "--union-on-device"])
    assert res.exit_code == 2 and "--union-on-device" in res.output
