"""DNA k = 14..16 in key-range passes at a cfg3-shaped share (16 groups x 2 matrices x 10 000 sites, alpha 0.05): per pass the
scoring, reduce and key-major writer times, keys and entries, the shard file's seconds; the merge of the pass files; device
memory in use after a pass' scoring.  k = 14 as one call beside its 4 passes gives the cost of rebuilding the right halves in
every pass.  slice = 1 sets the engine option "slice_long_lists" (windows whose half lists exceed the big-list cap are scored in
slices instead of failing the pass) and reports the windows sliced per case; cases: a comma-separated subset of
one14,14x4,15x4,15x16,16x16.  Usage: python tools/keyrange_probe.py [groups] [sites] [out.txt] [alpha] [slice] [cases]"""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import ipk_amd
from ipk_amd import dbfile, keyrange
from ipk_amd import distributed as D
from ipk_amd import engine as E
from ipk_amd.synth import synth_matrices

groups = int(sys.argv[1]) if len(sys.argv) > 1 else 16
sites = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
out_path = sys.argv[3] if len(sys.argv) > 3 else None
alpha = float(sys.argv[4]) if len(sys.argv) > 4 else 0.05
slice_on = int(sys.argv[5]) if len(sys.argv) > 5 else 0
only = sys.argv[6].split(",") if len(sys.argv) > 6 else None
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


mats = synth_matrices(2 * groups, sites, 4, alpha, 42)
mg = np.repeat(np.arange(groups, dtype=np.uint32), 2)
dev = torch.from_numpy(mats).cuda()
eng = ipk_amd.Engine(0)
if slice_on:
    eng.set_option("slice_long_lists", 1)
free0, total = torch.cuda.mem_get_info()
say(f"keyrange probe: {groups} groups x 2 matrices x {sites} sites, alpha {alpha}, omega 1.5, mif0 filter, device writer, slice_long_lists {slice_on}; "
    f"device memory in use before: {(total - free0) / 2**30:.2f} GiB")
work = tempfile.mkdtemp(prefix="kr_probe_")
hdr = ([(1, 0.0)] * (groups + 1), "a;")


def one_call(k):
    eps = ipk_amd.log_threshold(1.5, 4, k)
    for it in range(2):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        db, parts = D.build_db_shard(eng, dev, mg, k, eps, 4)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        used = total - torch.cuda.mem_get_info()[0]
        db.filter_mif0(eng, groups + 1, ipk_amd.score_threshold(1.5, 4, k))
        t2 = time.perf_counter()
        dbfile.write_db_device(eng, db, os.path.join(work, "one.ipk"), "DNA", hdr[0], hdr[1], k, 1.5)
        t3 = time.perf_counter()
        if it == 1:
            say(f"k={k} one call: {(t1 - t0) * 1e3:.1f} ms wall (device {parts.time_ms(E.T_TOTAL):.1f}: scoring {parts.time_ms(E.T_SCORE_MAIN):.1f}, "
                f"reduce {parts.time_ms(E.T_SCORE_REDUCE):.1f}, writer {parts.time_ms(E.T_KM_WRITE):.1f}); keys {db.num_keys}, entries {db.num_entries}; "
                f"filter {(t2 - t1) * 1e3:.1f} ms, file {t3 - t2:.3f} s; device memory in use {used / 2**30:.2f} GiB")
        db.free(); parts.free()


def passes(k, n):
    eps = ipk_amd.log_threshold(1.5, 4, k)
    peak = [0]
    orig = eng.score_groups_keyrange

    def scored(*a, **kw):                       # device memory in use right after a pass' scoring (its parts alive)
        p = orig(*a, **kw)
        torch.cuda.synchronize()
        peak[0] = max(peak[0], total - torch.cuda.mem_get_info()[0])
        return p
    eng.score_groups_keyrange = scored
    try:
        for it in range(2):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            r = keyrange.build_db_file(eng, dev, mg, k, eps, 4, os.path.join(work, f"k{k}.ipk"), work, "DNA", hdr[0], hdr[1], 1.5,
                                       "mif0", groups + 1, passes=n)
            wall = time.perf_counter() - t0
    finally:
        eng.score_groups_keyrange = orig
    pp = r["per_pass"]
    say(f"k={k} {n} passes (j={r['lead']}): {wall:.2f} s wall; scoring calls {r['score_s'] * 1e3:.1f} ms, filter {r['filter_s'] * 1e3:.1f} ms, "
        f"pass files {r['write_s']:.3f} s, merge {r['merge_s']:.3f} s; keys {r['totals'][0]}, entries {r['totals'][1]}, scored {r['emitted']}; "
        f"device memory in use after a pass' scoring, at most {peak[0] / 2**30:.2f} GiB")
    for name in ("call_ms", "score_ms", "reduce_ms", "writer_ms", "keys_ms"):
        v = np.array([p[name] for p in pp])
        say(f"    per pass {name:9s}: mean {v.mean():7.2f}  min {v.min():7.2f}  max {v.max():7.2f}  sum {v.sum():8.1f}")
    v = np.array([p["shard_file_s"] for p in pp])
    say(f"    per pass shard file s: mean {v.mean():.4f}  sum {v.sum():.3f};  keys per pass {min(p['keys'] for p in pp)}..{max(p['keys'] for p in pp)}, "
        f"entries per pass {min(p['entries'] for p in pp)}..{max(p['entries'] for p in pp)}")


def sliced_windows():
    try:
        return eng.get_option("debug_sliced_windows")
    except ipk_amd.IpkGpuError:
        return 0


for case in (("one", 14), ("passes", 14, 4), ("passes", 15, 4), ("passes", 15, 16), ("passes", 16, 16)):
    name = "one14" if case[0] == "one" else f"{case[1]}x{case[2]}"
    if only and name not in only:
        continue
    before = sliced_windows()
    try:
        one_call(case[1]) if case[0] == "one" else passes(case[1], case[2])
        if slice_on:
            # (every build of a case runs twice, and a window is counted once per pass that meets it)
            say(f"    windows scored in slices, summed over the case's {2 if case[0] == 'one' else 2 * case[2]} scoring calls: {sliced_windows() - before} "
                f"of {groups * 2 * (sites - case[1] + 1)} windows a call")
    except ipk_amd.IpkGpuError as e:
        say(f"{case}: {e}")
eng.close()
if out_path:
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
