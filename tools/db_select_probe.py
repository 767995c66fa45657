"""Measurements of Engine.select_db and Engine.load_db(path, mu=, omega=) on one GPU, on the file tools/db_load_probe.py uses: the
125-group share of the benchmark config cfg2, built in memory and written as a database file of about 0.96 GB.

  python tools/db_select_probe.py [--out profiles/db_select_probe.txt]

Written, for mu in {1, 0.5, 0.1} at the file's omega and at a higher one: the device time of the selection alone on the loaded
database (ipkgpu_db_select_time_ms, the best of three after a first call that allocates the workspaces), the whole load_select's
seconds and the body bytes it read (ipkgpu_db_load_time(ctx, 7)); and, in the same run, the full ipkgpu_db_load of the same file with
its db_unpack_entries_kernel time -- the two yardsticks.  Both ratios are recorded.  The FLAT check of the kernels (tools/isa_flat.py) is
appended when hipcc is there."""
import argparse
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ipk_amd                                                           # noqa: E402
from tools.ondisk_probe import in_memory, share                          # noqa: E402

MUS = (1.0, 0.5, 0.1)


def flat_check():
    import importlib.util
    spec = importlib.util.spec_from_file_location("isa_flat", os.path.join(ROOT, "tools", "isa_flat.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        return "FLAT check: no hipcc here, not made"
    path = mod.listing()
    try:
        bad = mod.flat_by_kernel(path)
        text = open(path).read()
        mine = sorted(set(w.split("(")[0] for w in __import__("re").findall(r"; -- Begin function (\S*db_select\S*)", text)))
    finally:
        shutil.rmtree(os.path.dirname(path), ignore_errors=True)
    return (f"FLAT check (tools/isa_flat.py over the gfx950 listing): {len(bad)} kernel(s) of the library with FLAT memory instructions; "
            f"{len(mine)} db_select_* kernel symbols in the listing, {sum(1 for k in bad if 'db_select' in k)} of them with FLAT instructions")


def probe(out_path, n_groups):
    tmp = tempfile.mkdtemp(prefix="db_select_probe_", dir=os.environ.get("IPK_PROBE_DIR"))
    cfg, mats, groups = share("cfg2", n_groups)
    eng = ipk_amd.Engine(0)
    path = os.path.join(tmp, "cfg2.ipk")
    m = in_memory(eng, cfg, mats, groups, path)
    size = os.path.getsize(path)
    higher = cfg["omega"] + 0.25
    lines = [f"cfg2 share: {n_groups} groups, sigma={cfg['sigma']} k={cfg['k']} sites={cfg['sites']}: {m['keys']} k-mers, {m['entries']} entries, "
             f"file {size} bytes, omega {cfg['omega']}; the higher omega is {higher}"]
    full = []
    db = None
    for _ in range(3):                                                   # (the first load allocates the pinned buffers and the workspaces)
        if db is not None:
            db.free()
        t0 = time.time()
        db = eng.load_db(path)
        full.append((time.time() - t0, eng.load_times()))
    best_full = min(w for w, _ in full[1:])
    unpack_ms = min(t["entries_ms"] for _, t in full[1:])
    body = full[-1][1]["body_bytes_read"]
    lines.append(f"full load (ipkgpu_db_load), best of the 2nd and 3rd: {best_full:.3f} s wall, body bytes read {body:.0f}; db_unpack_entries_kernel "
                 f"{unpack_ms:.3f} ms for {db.num_entries} entries; inside the call: " + ", ".join(f"{k} {v:.3f}" for k, v in full[-1][1].items() if k.endswith("_s")))
    lines.append("mu    omega  | select on the loaded database: ms (best of 3), / unpack kernel, kept k-mers, kept entries | load_select: s wall (best of 2), / full load, "
                 "body bytes read, / body, read_s, walk_s")
    for omega in (cfg["omega"], higher):
        for mu in MUS:
            ms = []
            for rep in range(4):
                v = eng.select_db(db, mu=mu, omega=omega)
                if rep:
                    ms.append(eng.select_time_ms())
                kept = (v.num_keys, v.num_entries)
                v.free()
            walls = []
            for rep in range(3):
                t0 = time.time()
                v = eng.load_db(path, mu=mu, omega=omega)
                w = time.time() - t0
                t = eng.load_times()
                assert (v.num_keys, v.num_entries) == kept
                v.free()
                if rep:
                    walls.append((w, t))
            w, t = min(walls, key=lambda x: x[0])
            lines.append(f"{mu:<5} {omega:<6} | {min(ms):8.3f} ms  {min(ms) / unpack_ms:6.2f} x  {kept[0]:>10} {kept[1]:>11} | {w:.3f} s  {w / best_full:5.2f} x  "
                         f"{t['body_bytes_read']:>12.0f}  {t['body_bytes_read'] / body:5.3f}  {t['read_s']:.3f}  {t['walk_s']:.3f}")
    db.free()
    eng.close()
    shutil.rmtree(tmp, ignore_errors=True)
    lines.append(flat_check())
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
