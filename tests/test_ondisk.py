"""CPU suite: the on-disk build's command line, ABI and piece planner (ipk_amd/ondisk.py); the device side is tests/test_gpu_ondisk.py."""
import ctypes

import numpy as np
import pytest
from click.testing import CliRunner

import ipk_amd
from ipk_amd import cli, ondisk
from ipk_amd import engine as E

NEW = ["ipkgpu_parts_spill", "ipkgpu_spill_merge", "ipkgpu_mem_stats"]


def _build_args(tmp_path, k, extra=()):
    (tmp_path / "m.tsv").write_text("")
    return ["build", "-w", str(tmp_path / "w"), "--ar-dir", str(tmp_path), "-k", str(k), "--mapping", str(tmp_path / "m.tsv")] + list(extra)


def test_help_describes_on_disk():
    res = CliRunner().invoke(cli.ipk, ["build", "--help"])
    assert res.exit_code == 0
    text = " ".join(res.output.split())
    at = text.index("--on-disk")
    assert "ignored" not in text[at:at + 200]
    assert "hashmaps" in text[at:at + 600]


def test_cli_refuses_positions_on_disk(tmp_path):
    res = CliRunner().invoke(cli.ipk, _build_args(tmp_path, 4, ["--on-disk", "--keep-positions", "-s", "amino"]))
    assert res.exit_code == 2 and "--on-disk does not keep positions" in res.output


def test_cli_refuses_on_disk_on_several_ranks(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    res = CliRunner().invoke(cli.ipk, _build_args(tmp_path, 10, ["--on-disk"]))
    assert res.exit_code == 2 and "--on-disk runs on ONE GPU" in res.output


def test_cli_refuses_on_disk_with_key_passes(tmp_path):
    res = CliRunner().invoke(cli.ipk, _build_args(tmp_path, 15, ["--on-disk"]))
    assert res.exit_code == 2 and "--on-disk is not combined with key-range passes" in res.output
    res = CliRunner().invoke(cli.ipk, _build_args(tmp_path, 14, ["--on-disk", "--key-passes", "4"]))
    assert res.exit_code == 2 and "--on-disk is not combined with key-range passes" in res.output


def test_library_exports_the_calls():
    lib = ipk_amd.load_library()
    E._bind_keymajor(lib)
    for name in NEW:
        assert hasattr(lib, name), f"libipkgpu.so does not export {name}"
        assert name in E.ABI_SYMBOLS
    n = ctypes.c_uint64(0)
    out = ctypes.c_void_p()
    assert lib.ipkgpu_parts_spill(None, None, b"/nowhere", 0, ctypes.byref(n)) == 1
    assert lib.ipkgpu_mem_stats(None, ctypes.byref(n), ctypes.byref(n), 0) == 1
    assert lib.ipkgpu_spill_merge(None, 4, 8, 0, 32, None, 0, ctypes.byref(out)) == 1


def _spill_merge_null(lib, path, sigma=4, k=8, owner=0, n_owners=32):
    arr = (ctypes.c_char_p * 1)(str(path).encode())
    out = ctypes.c_void_p()
    rc = lib.ipkgpu_spill_merge(None, sigma, k, owner, n_owners, arr, 1, ctypes.byref(out))
    return rc, lib.ipkgpu_last_error(None).decode()


def test_spill_merge_checks_files_on_the_host(tmp_path):
    """A missing, an empty and a foreign file are refused by name before anything needs a device (there is none here)."""
    lib = ipk_amd.load_library()
    E._bind_keymajor(lib)
    missing = tmp_path / "p0_b0.blk"
    rc, msg = _spill_merge_null(lib, missing)
    assert rc == 1 and str(missing) in msg
    empty = tmp_path / "p1_b0.blk"
    empty.write_bytes(b"")
    rc, msg = _spill_merge_null(lib, empty)
    assert rc == 1 and str(empty) in msg
    foreign = tmp_path / "p2_b0.blk"
    foreign.write_bytes(b"NOTSPILL" + bytes(4096))
    rc, msg = _spill_merge_null(lib, foreign)
    assert rc == 1 and str(foreign) in msg and "magic" in msg


def test_read_block_parses_the_layout(tmp_path):
    """read_block against bytes laid out by hand from the documented layout."""
    row = np.zeros(100, dtype=np.uint32)
    row[[0, 63, 64, 99]] = [1, 2, 65535, 7]
    bits, counts = ondisk.pack_counts(row)
    assert bits.tolist() == [(1 << 0) | (1 << 63), (1 << 0) | (1 << 35)] and counts.tolist() == [1, 2, 65535, 7]
    n_entries = int(row.sum())
    entries = np.arange(2 * n_entries, dtype=np.uint32)
    head = b"IPKSPILL" + np.array([1, 4, 8, 32, 5, 3], dtype=np.uint32).tobytes() + np.array([100, 4, n_entries, 0], dtype=np.uint64).tobytes()
    path = tmp_path / "p3_b5.blk"
    path.write_bytes(head + bits.tobytes() + counts.tobytes() + entries.tobytes())
    blk = ondisk.read_block(path)
    assert (blk["sigma"], blk["k"], blk["n_owners"], blk["owner"], blk["piece"], blk["slots"]) == (4, 8, 32, 5, 3, 100)
    assert np.array_equal(blk["bits"], bits) and np.array_equal(blk["counts"], counts) and np.array_equal(blk["entries"].ravel(), entries)
    path.write_bytes(path.read_bytes()[:-8])
    with pytest.raises(ValueError):
        ondisk.read_block(path)


def _run(plan, fits):
    """Drives a planner: fits(n) says whether a piece of n groups fits; returns the pieces and the sizes that were tried."""
    tried = []
    while plan.next() is not None:
        g0, g1 = plan.next()
        tried.append(g1 - g0)
        if fits(g1 - g0):
            plan.done(1000 + 10 * (g1 - g0))
        else:
            plan.nomem(12345)
    return plan.pieces, tried


@pytest.mark.parametrize("n_groups,budget", [(1, 10 ** 6), (7, 10 ** 6), (1000, 10 ** 5), (200000, 10 ** 9), (70000, 10 ** 12)])
def test_planner_covers_every_group_once_in_order(n_groups, budget):
    pieces, tried = _run(ondisk.PiecePlanner(n_groups, budget), lambda n: True)
    assert pieces[0] == (0, 1)                                             # the first piece is one group
    assert pieces[-1][1] == n_groups
    assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))           # contiguous, in order, no group twice
    assert all(0 < g1 - g0 <= ondisk.MAX_PIECE_GROUPS for g0, g1 in pieces)
    if n_groups == 200000:
        assert max(g1 - g0 for g0, g1 in pieces) == ondisk.MAX_PIECE_GROUPS   # the u16 counts bound a piece, not the budget


def test_planner_halves_after_nomem():
    plan = ondisk.PiecePlanner(1000, 10 ** 9, first=64)
    pieces, tried = _run(plan, lambda n: n <= 10)
    assert tried[:4] == [64, 32, 16, 8]                                    # halved until it fits
    assert pieces[0] == (0, 8) and pieces[-1][1] == 1000
    assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))
    assert max(g1 - g0 for g0, g1 in pieces) <= 10
    assert tried.count(16) == 1                                            # a size that failed is not tried again


def test_planner_one_group_that_does_not_fit_raises():
    plan = ondisk.PiecePlanner(5, 4096)
    with pytest.raises(ondisk.OnDiskError) as ei:
        plan.nomem(123456)
    assert "123456 bytes" in str(ei.value) and "4096" in str(ei.value)


def test_fixed_pieces():
    pieces, _ = _run(ondisk.FixedPlanner(10, 1 << 30, [3, 1, 4]), lambda n: True)
    assert pieces == [(0, 3), (3, 4), (4, 8), (8, 10)]
