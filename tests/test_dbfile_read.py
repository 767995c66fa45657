"""CPU suite: the reading side of the database file -- ipkgpu_db_file_open's description of the head and ipkgpu_db_file_check's walk
over the records (dbfile.file_info / check_file), against files written by the host serialisers and the same files damaged."""
import os
import subprocess
import sys

import pytest

import ipk_amd
from ipk_amd import dbfile
from tests import db_files as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def db():
    return F.synthetic(200, seed=11)


@pytest.mark.parametrize("positioned", [False, True])
def test_header_fields_and_totals(tmp_path, db, positioned):
    path = F.write(tmp_path / "a.ipk", db, positioned)
    info = dbfile.file_info(path)
    want = dict(F.HEADER)
    for name, value in want.items():
        assert info[name] == value, name
    assert info["positions_loaded"] is positioned
    assert info["protocol_version"] == dbfile.protocol_version() == 7
    assert info["library_version"] == 19
    assert info["total_num_kmers"] == len(db["keys"]) and info["total_num_entries"] == int(db["off"][-1])
    assert info["file_bytes"] == os.path.getsize(path)
    assert info["file_bytes"] - info["body_offset"] == F.record_starts(db, positioned)[1]
    # the tests' own parser reads the same head
    hdr, _ = dbfile.read_db(path)
    for name, value in hdr.items():
        assert info[name] == value, name
    assert dbfile.check_file(path) == (len(db["keys"]), int(db["off"][-1]))


def test_empty_and_single_record(tmp_path):
    empty = F.synthetic(keys=[], counts=[])
    p = F.write(tmp_path / "empty.ipk", empty)
    assert dbfile.check_file(p) == (0, 0)
    assert dbfile.file_info(p)["total_num_kmers"] == 0
    one = F.synthetic(keys=[77], counts=[5])
    assert dbfile.check_file(F.write(tmp_path / "one.ipk", one, positioned=True)) == (1, 5)


@pytest.mark.parametrize("positioned", [False, True])
def test_damaged_files_are_refused(tmp_path, db, positioned):
    good, bad = F.damaged(tmp_path, db, positioned)
    assert dbfile.check_file(good) == (len(db["keys"]), int(db["off"][-1]))
    assert set(bad) == {"truncated", "truncated_head", "count_plus_one", "count_last_plus_one", "count_2_40", "count_zeroed", "total_kmers",
                        "total_entries"}
    for name, (path, record) in bad.items():
        dbfile.file_info(path)                                   # the head itself is whole
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            dbfile.check_file(path)
        assert ei.value.code == 1, name
        msg = str(ei.value)
        if record is not None:
            assert f"record {record} at byte offset " in msg, (name, msg)
        if name.startswith("total_"):
            assert "header's total" in msg, (name, msg)
    # the offset named is the record's place in the file
    path, record = bad["count_2_40"]
    at = dbfile.file_info(path)["body_offset"] + int(F.record_starts(db, positioned)[0][record])
    with pytest.raises(ipk_amd.IpkGpuError, match=f"record {record} at byte offset {at}:.*{1 << 40}"):
        dbfile.check_file(path)


def test_not_a_database_file(tmp_path):
    p = tmp_path / "junk.ipk"
    p.write_bytes(b"\x16" + b"\0" * 7 + b"serialization::archivX" + b"\0" * 64)
    with pytest.raises(ipk_amd.IpkGpuError, match="not a database file"):
        dbfile.file_info(p)
    with pytest.raises(ipk_amd.IpkGpuError, match="cannot open"):
        dbfile.file_info(tmp_path / "missing.ipk")
    good = F.write(tmp_path / "good.ipk", F.synthetic(20, seed=3))
    cut = tmp_path / "head_cut.ipk"
    cut.write_bytes(good.read_bytes()[:60])                      # inside the head
    with pytest.raises(ipk_amd.IpkGpuError, match="not a database file"):
        dbfile.file_info(cut)


def test_other_protocol_version_is_refused(tmp_path):
    """A file written under IPKGPU_IPK_PROTOCOL_VERSION=0 (no protocol word, no positions flag) by another process is refused by this
    one, which expects version 7 -- read_head's rule."""
    path = tmp_path / "v0.ipk"
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests import db_files as F\n"
            "F.write(%r, F.synthetic(20, seed=3))\n") % (ROOT, str(path))
    env = dict(os.environ, IPKGPU_IPK_PROTOCOL_VERSION="0")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=ROOT)
    assert dbfile.protocol_version() == 7
    with pytest.raises(ipk_amd.IpkGpuError, match="protocol version"):
        dbfile.file_info(path)
    hdr, recs = dbfile.read_db(path, protocol=0)                  # it is a whole file of the older layout
    assert hdr["protocol_version"] == 0 and len(recs) == 20
