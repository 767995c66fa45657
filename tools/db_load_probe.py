"""Measurements of Engine.load_db and Engine.diff_dbs on one GPU, on the workload of tools/ondisk_probe.py: the 125-group share of
the benchmark config cfg2, built in memory and written as a database file of about 0.96 GB.

  python tools/db_load_probe.py [--out profiles/db_load_probe.txt]

Written: the load's seconds split into file read, host walk and waiting for the device; the two unpack kernels' ms and GB/s (bytes
each must move, over its time); the diff's ms of the loaded database against a second load of the same file and against a copy with
every 1000th score moved by 0.5; and, in the same run, the seconds a plain chunked pread of the same file into pinned memory takes --
the yardstick for the load (same file, same page-cache state: it was written moments before either reads it)."""
import argparse
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ipk_amd                                                           # noqa: E402
from ipk_amd import engine as E                                          # noqa: E402
from tools.ondisk_probe import in_memory, share                          # noqa: E402

CHUNK = 64 << 20                                                         # the load's default pinned buffer


def plain_read(path):
    """The whole file through two pinned buffers with pread, nothing else: seconds."""
    import torch
    bufs = [torch.empty(CHUNK, dtype=torch.uint8).pin_memory().numpy() for _ in range(2)]
    size = os.path.getsize(path)
    fd = os.open(path, os.O_RDONLY)
    t0 = time.time()
    at, j = 0, 0
    while at < size:
        n = os.preadv(fd, [memoryview(bufs[j & 1])[:min(CHUNK, size - at)]], at)
        if n <= 0:
            raise IOError("short read")
        at += n
        j += 1
    t = time.time() - t0
    os.close(fd)
    return t


def probe(out_path, n_groups):
    import torch
    tmp = tempfile.mkdtemp(prefix="db_load_probe_", dir=os.environ.get("IPK_PROBE_DIR"))
    cfg, mats, groups = share("cfg2", n_groups)
    eng = ipk_amd.Engine(0)
    path = os.path.join(tmp, "cfg2.ipk")
    m = in_memory(eng, cfg, mats, groups, path)
    size = os.path.getsize(path)
    lines = [f"cfg2 share: {n_groups} groups, sigma={cfg['sigma']} k={cfg['k']} sites={cfg['sites']}: {m['keys']} k-mers, {m['entries']} entries, "
             f"file {size} bytes (built in memory: score {m['score_s']:.3f} s, filter {m['filter_s']:.3f} s, file {m['file_s']:.3f} s)"]
    reads = [plain_read(path)]
    loads = []
    dbs = []
    for _ in range(3):                                                   # (the first load allocates the pinned buffers and the workspaces)
        t0 = time.time()
        dbs.append(eng.load_db(path))
        loads.append((time.time() - t0, eng.load_times()))
        reads.append(plain_read(path))
    n, ne = dbs[0].num_keys, dbs[0].num_entries
    lines.append("plain chunked pread of the file into pinned memory (64 MiB chunks), before and after each load: "
                 + ", ".join(f"{t:.3f} s = {size / t / 1e9:.2f} GB/s" for t in reads))
    for i, (wall, t) in enumerate(loads):
        heads_b, entries_b = 40 * n, 16 * ne
        lines.append(f"load {i + 1}: {wall:.3f} s wall = {size / wall / 1e9:.2f} GB/s; inside the call {t['total_s']:.3f} s: file read {t['read_s']:.3f} s, host walk "
                     f"{t['walk_s']:.3f} s, waiting for the device {t['device_wait_s']:.3f} s; device work behind the last copy {t['device_ms']:.2f} ms: "
                     f"db_unpack_heads_kernel {t['heads_ms']:.3f} ms = {heads_b / t['heads_ms'] / 1e6:.0f} GB/s of {heads_b} bytes, "
                     f"db_unpack_entries_kernel {t['entries_ms']:.3f} ms = {entries_b / t['entries_ms'] / 1e6:.0f} GB/s of {entries_b} bytes")
    best_read = min(reads)
    best_load = min(w for w, _ in loads[1:])
    lines.append(f"load / plain read: {best_load:.3f} s / {best_read:.3f} s = {best_load / best_read:.2f}")
    a, b, c = dbs
    for rep in range(2):
        counts, _ = eng.diff_dbs(a, b, eps=1e-2, max_records=100)
        lines.append(f"diff against a second load of the same file (run {rep + 1}): {eng.diff_time_ms():.3f} ms on the device; differences "
                     f"{counts['entries_only_a'] + counts['entries_only_b'] + counts['scores_differ']}")
    ent = E._device_tensor(c.entries_device_ptr(), (ne, 2), "int32", c).view(torch.float32)
    ent[::1000, 1] += 0.5
    torch.cuda.synchronize()
    for rep in range(2):
        counts, rec = eng.diff_dbs(a, c, eps=1e-2, max_records=100)
        lines.append(f"diff against a copy with every 1000th score moved by 0.5 (run {rep + 1}): {eng.diff_time_ms():.3f} ms on the device; scores_differ "
                     f"{counts['scores_differ']} of {ne} entries, max_abs_diff {counts['max_abs_diff']:.6f}, {len(rec)} records returned")
    del ent
    for d in dbs:
        d.free()
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
