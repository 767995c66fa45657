"""The shard-file merge (ipkgpu_db_merge_files) on positioned shards: records of 16 + 10 n bytes, the positions flag read from the
shards' headers and written into the merged one.  Host code only; every comparison is on file bytes or exact values."""
import numpy as np
import pytest

import ipk_amd
from ipk_amd import dbfile

HEADER = ("AA", [(1, 0.0), (3, 0.5), (2, 0.25)], "((a,b),c);", 4, 1.5)


def synthetic_db(n_keys=3000, seed=11):
    """A positioned database of n_keys keys (AA k = 4 codes, ascending) with 1..5 entries each, positions <= 65535, filter values with
    ties (so that the key decides some of the order)."""
    rng = np.random.default_rng(seed)
    dense = np.sort(rng.choice(20 ** 4, size=n_keys, replace=False)).astype(np.uint64)
    keys = np.zeros(n_keys, np.uint64)
    for d in range(4):
        keys |= ((dense // 20 ** d) % 20) << np.uint64(5 * d)
    order = np.argsort(keys, kind="stable")
    keys = keys[order].astype(np.uint32)
    counts = rng.integers(1, 6, size=n_keys)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    n = int(off[-1])
    br = rng.integers(0, 500, size=n).astype(np.uint32)
    sc = (-rng.random(n) * 6).astype(np.float32)
    pos = rng.integers(0, 65536, size=n).astype(np.uint32)
    pos[:3] = (0, 65535, 1)
    fv = (rng.integers(0, 400, size=n_keys) / 400.0).astype(np.float32)
    return dict(keys=keys, off=off, br=br, sc=sc, pos=pos, fv=fv)


def subset(db, sel):
    """The records `sel` (boolean over keys) as a database of their own."""
    idx = np.flatnonzero(sel)
    a, b = db["off"][:-1].astype(np.int64)[idx], db["off"][1:].astype(np.int64)[idx]
    rows = np.concatenate([np.arange(x, y) for x, y in zip(a, b)]) if len(idx) else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum(b - a)]).astype(np.uint64)
    return dict(keys=db["keys"][idx], off=off, br=db["br"][rows], sc=db["sc"][rows], pos=db["pos"][rows],
                fv=db["fv"][idx])


def write(path, db, positioned=True, shard=False):
    seq, tree_index, newick, k, omega = HEADER
    order = np.argsort(dbfile.filter_sort_code(db["fv"], db["keys"]), kind="stable")
    ti, nw = ([], "") if shard else (tree_index, newick)          # (a shard's header carries only its totals)
    if positioned:
        dbfile.write_db_positions(path, seq, ti, nw, k, omega, db["keys"], db["off"], db["br"], db["sc"], db["pos"], db["fv"], order)
    else:
        dbfile.write_db(path, seq, ti, nw, k, omega, db["keys"], db["off"], db["br"], db["sc"], db["fv"], order)


def shards(tmp_path, db, P, positioned=True, tag="s"):
    paths = []
    for o in range(P):
        p = tmp_path / f"{tag}{P}_{o}.ipk"
        write(p, subset(db, db["keys"] % P == o), positioned, shard=True)
        paths.append(p)
    return paths


@pytest.mark.parametrize("P", [2, 3])
def test_positioned_shards_merge_to_the_one_file(tmp_path, P):
    db = synthetic_db()
    whole = tmp_path / "whole.ipk"
    write(whole, db)
    merged = tmp_path / f"merged{P}.ipk"
    nk, ne = dbfile.merge_shard_files(merged, *HEADER, shards(tmp_path, db, P))
    assert (nk, ne) == (len(db["keys"]), len(db["br"]))
    assert merged.read_bytes() == whole.read_bytes()
    hdr, recs = dbfile.read_db(merged)
    assert hdr["positions_loaded"] is True and hdr["total_num_kmers"] == nk and hdr["total_num_entries"] == ne
    got = {r[0]: r for r in recs}
    assert len(got) == nk
    off = db["off"].astype(np.int64)
    for i, key in enumerate(db["keys"].tolist()):
        _, fv, br, sc, pos = got[key]
        a, b = off[i], off[i + 1]
        assert np.float32(fv).view(np.uint32) == db["fv"][i].view(np.uint32)
        assert np.array_equal(br, db["br"][a:b]) and np.array_equal(sc.view(np.uint32), db["sc"][a:b].view(np.uint32))
        assert np.array_equal(pos, db["pos"][a:b])


def test_an_empty_positioned_shard_takes_part(tmp_path):
    db = synthetic_db(40, 5)
    whole = tmp_path / "whole.ipk"
    write(whole, db)
    none = np.zeros(len(db["keys"]), bool)
    a, b = tmp_path / "a.ipk", tmp_path / "b.ipk"
    write(a, subset(db, none), shard=True)
    write(b, db, shard=True)
    merged = tmp_path / "m.ipk"
    dbfile.merge_shard_files(merged, *HEADER, [a, b])
    assert merged.read_bytes() == whole.read_bytes()


def test_mixture_of_positioned_and_plain_shards_is_refused(tmp_path):
    db = synthetic_db(200, 3)
    pos = shards(tmp_path, db, 2, True, "p")
    plain = shards(tmp_path, db, 2, False, "q")
    for mix in ([pos[0], plain[1]], [plain[0], pos[1]]):
        with pytest.raises(ipk_amd.IpkGpuError, match="positioned and plain") as ei:
            dbfile.merge_shard_files(tmp_path / "mix.ipk", *HEADER, mix)
        assert ei.value.code == 1


def test_positioned_shards_under_protocol_version_0_are_refused(tmp_path, monkeypatch):
    """The layout of version 0 has neither protocol word nor positions flag: positioned shards cannot be told from plain ones, and are
    refused with a message that names the setting."""
    db = synthetic_db(200, 4)
    pos = shards(tmp_path, db, 2)
    monkeypatch.setenv("IPKGPU_IPK_PROTOCOL_VERSION", "0")
    with pytest.raises(ipk_amd.IpkGpuError, match="IPKGPU_IPK_PROTOCOL_VERSION=0") as ei:
        dbfile.merge_shard_files(tmp_path / "v0.ipk", *HEADER, pos)
    assert ei.value.code == 1
    monkeypatch.delenv("IPKGPU_IPK_PROTOCOL_VERSION")
    dbfile.merge_shard_files(tmp_path / "v7.ipk", *HEADER, pos)          # the same shards under the version they were written with


@pytest.mark.parametrize("protocol", [None, "0"])
def test_plain_shards_merge_as_before(tmp_path, monkeypatch, protocol):
    if protocol is not None:
        monkeypatch.setenv("IPKGPU_IPK_PROTOCOL_VERSION", protocol)
    db = synthetic_db(1500, 9)
    whole = tmp_path / "whole.ipk"
    write(whole, db, positioned=False)
    merged = tmp_path / "merged.ipk"
    dbfile.merge_shard_files(merged, *HEADER, shards(tmp_path, db, 3, positioned=False))
    assert merged.read_bytes() == whole.read_bytes()
    hdr, _ = dbfile.read_db(merged)
    assert hdr["positions_loaded"] is False
