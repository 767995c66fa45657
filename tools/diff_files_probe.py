"""Measurements of Engine.diff_files (ipkgpu_db_diff_files) on one GPU, on the file of tools/db_load_probe.py: the 125-group share of
the benchmark config cfg2 written as a database file of about 0.96 GB, against a copy of it with every 1000th score moved by 0.5.

  python tools/diff_files_probe.py [--out profiles/diff_files_probe.txt]

Written: the resident path of the same run (two loads and Engine.diff_dbs), then the comparison by key ranges under budgets aimed at 1,
2, 4 and 8 ranges (the window by the library's rule, a sixteenth of the budget): the ranges the plan made, wall seconds, the passes over
each body, the seconds in the histogram passes, in the range loads and in the host's walk, the walk's share, the device ms of the diffs
and the peak of device memory against the budget.  Recorded, not gated: no figure here is asserted anywhere."""
import argparse
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ipk_amd                                                           # noqa: E402
from ipk_amd import dbfile                                               # noqa: E402
from ipk_amd import engine as E                                          # noqa: E402
from tools.ondisk_probe import in_memory, share                          # noqa: E402


def budget_for(n_ranges, a, b):
    """A budget under which about n_ranges ranges are expected: the formula's figure for the whole pair, the part that does not shrink
    with the range (the window, by the library's rule a sixteenth of the budget) kept whole, the rest divided."""
    def fixed(avail):
        w = min(max(avail // 16, 4096), 256 << 20)
        return max(E.stream_window_bytes(min(w, h["file_bytes"] - h["body_offset"]), min(h["total_num_kmers"], max(w // 16, 1)), 0) for h in (a, b))
    whole = E.diff_files_range_bytes(0, a["total_num_kmers"], a["total_num_entries"], a["positions_loaded"], b["total_num_kmers"], b["total_num_entries"],
                                     b["positions_loaded"], 100)
    avail = whole // n_ranges
    for _ in range(8):
        avail = int(fixed(avail) + whole * 1.03 / n_ranges)
    return avail


def probe(out_path, n_groups):
    import torch
    tmp = tempfile.mkdtemp(prefix="diff_files_probe_", dir=os.environ.get("IPK_PROBE_DIR"))
    cfg, mats, groups = share("cfg2", n_groups)
    eng = ipk_amd.Engine(0)
    path_a, path_b = os.path.join(tmp, "a.ipk"), os.path.join(tmp, "b.ipk")
    m = in_memory(eng, cfg, mats, groups, path_a)
    size = os.path.getsize(path_a)
    lines = [f"cfg2 share: {n_groups} groups, sigma={cfg['sigma']} k={cfg['k']} sites={cfg['sites']}: {m['keys']} k-mers, {m['entries']} entries, file {size} bytes"]
    c = eng.load_db(path_a)
    ent = E._device_tensor(c.entries_device_ptr(), (c.num_entries, 2), "int32", c).view(torch.float32)
    ent[::1000, 1] += 0.5
    torch.cuda.synchronize()
    del ent
    dbfile.write_db_device(eng, c, path_b, **dbfile.header_args(c.header))
    c.free()
    lines.append(f"B: a copy with every 1000th score moved by 0.5, {os.path.getsize(path_b)} bytes")

    for rep in range(2):                                                  # the resident path
        eng.set_option("release_workspaces", 1)
        eng.mem_stats(reset_peak=True)
        held = eng.mem_stats()[0]
        t0 = time.time()
        da = eng.load_db(path_a)
        ta = eng.load_times()
        db_ = eng.load_db(path_b)
        tb = eng.load_times()
        counts, rec = eng.diff_dbs(da, db_, eps=1e-2, max_records=100)
        wall = time.time() - t0
        lines.append(f"resident (run {rep + 1}): two loads + diff_dbs {wall:.3f} s wall: loads {ta['total_s']:.3f} + {tb['total_s']:.3f} s (host walk "
                     f"{ta['walk_s']:.3f} + {tb['walk_s']:.3f} s), diff {eng.diff_time_ms():.3f} ms on the device; scores_differ {counts['scores_differ']}, "
                     f"{len(rec)} records; device peak {(eng.mem_stats()[1] - held) / 2 ** 20:.0f} MiB")
        da.free(); db_.free()
    want = counts
    ha, hb = dbfile.file_info(path_a), dbfile.file_info(path_b)
    for target in (1, 2, 4, 8):
        for rep in range(2):
            eng.set_option("release_workspaces", 1)
            held = eng.mem_stats()[0]
            avail = None if target == 1 else budget_for(target, ha, hb)
            eng.set_option("device_budget_bytes", 0 if avail is None else held + avail)
            eng.mem_stats(reset_peak=True)
            t0 = time.time()
            try:
                got, rec, info = eng.diff_files(path_a, path_b, eps=1e-2, max_records=100)
            finally:
                eng.set_option("device_budget_bytes", 0)
            wall = time.time() - t0
            peak = eng.mem_stats()[1] - held
            same = "the resident counts" if got == want else "OTHER COUNTS THAN THE RESIDENT PATH"
            lines.append(f"aimed at {target} range(s) (run {rep + 1}): budget {'none' if avail is None else '%.0f MiB' % (avail / 2 ** 20)}, window "
                         f"{info['window_bytes'] / 2 ** 20:.1f} MiB, {len(info['ranges'])} ranges, passes {info['passes_a']} + {info['passes_b']}, "
                         f"{info['body_bytes_read'] / 1e9:.2f} GB read; {wall:.3f} s wall, inside the call {info['total_s']:.3f} s: histogram passes "
                         f"{info['hist_s']:.3f} s, range loads {info['loads_s']:.3f} s, host walk {info['walk_s']:.3f} s = {100 * info['walk_s'] / info['total_s']:.0f} %; "
                         f"diffs {info['diff_ms']:.3f} ms on the device; device peak {peak / 2 ** 20:.0f} MiB; {same}, {len(rec)} records")
    eng.close()
    shutil.rmtree(tmp, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--groups", type=int, default=125)
    a = ap.parse_args()
    probe(a.out, a.groups)
