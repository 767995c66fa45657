"""DNA databases of k = 15, 16 (and k = 14 on request) built in key-range passes.

A DNA k-mer's packed code holds its first symbol in the top bits (pk_compute.cpp:96-104), so the k-mers whose first j
symbols spell a class c are the contiguous keys [c * 4^(k-j), (c+1) * 4^(k-j)).  One pass scores one class
(ipkgpu_score_groups_keyrange_device: a key space of 4^(k-j) slots, the geometry of the k = 13 / 14 exact partition),
its shard is filtered and written as a database file of its own, and the pass files are merged by (filter value, key)
into the one file (ipkgpu_db_merge_files, the role of merge_stage2, db_builder.cpp:392-458).  Filtering per pass is valid
because MIF0's value and the random filter's draw are both per k-mer.  Device memory is bounded by one pass.
"""
import os
import time

import numpy as np

from . import dbfile
from .engine import ERR_NOMEM, IpkGpuError, T_KM_WRITE, T_SCORE_MAIN, T_SCORE_REDUCE, T_TOTAL, score_threshold

KEY_SYMBOLS = (13, 14)            # k - j of a pass: the key spaces of the exact partition's 32768-slot buckets
MAX_K = 16                        # u32 keys: 2 bits per DNA symbol


def allowed_leads(sigma, k):
    """Leading-symbol counts j a pass may fix at this (sigma, k): DNA, j >= 1, 13 <= k - j <= 14, k <= 16."""
    if sigma != 4 or k > MAX_K:
        return []
    return [j for j in range(1, k) if k - j in KEY_SYMBOLS]


def plan(sigma, k, passes=None):
    """[(lead, class, key_base, span)] of the passes, in key order (contiguous, disjoint, covering 4^k).
    passes=None: j = k - 14 (4 passes at k = 15, 16 at k = 16); otherwise passes must be 4^j for an allowed j."""
    leads = allowed_leads(sigma, k)
    if passes is None:
        j = k - 14
        if j not in leads:
            raise ValueError(f"no default key-range split for sigma={sigma}, k={k}")
    else:
        by_count = {sigma ** j: j for j in leads}
        if passes not in by_count:
            raise ValueError(f"{passes} key-range passes are not possible at sigma={sigma}, k={k} "
                             f"(allowed: {sorted(by_count) or 'none'})")
        j = by_count[passes]
    span = sigma ** (k - j)
    return [(j, c, c * span, span) for c in range(sigma ** j)]


def build_db_file(engine, mats, mat_group, k, log_eps, sigma, path, workdir, sequence_type, tree_index, newick, omega,
                  filter_="mif0", total_num_groups=None, passes=None, keep_pass_files=False, union_on_device=False):
    """Scores every pass, writes its filtered shard to workdir/passes/pass<c>.ipk and merges the pass files into `path`.
    mats: [n_mats, sites, sigma] float32 (numpy or CUDA tensor; uploaded once).  Returns a dict with the totals, `emitted`,
    the number of passes, stage times summed over the passes (seconds) and per-pass device timings (ms).
    union_on_device: every pass' filtered database stays on the device instead; after the last pass they are united there
    (Engine.union_dbs), written once under the real header and freed -- the same file byte for byte, no pass files, no host merge.
    On the first IPKGPU_ERR_NOMEM anywhere in that mode the held databases are written as pass files and freed, the failed step is
    repeated once, and the build goes on in the file mode.  "route" says which way the file came about: "files" (the default),
    "device" or "fallback"; "union_s" is the time in the union and its write."""
    import torch

    steps = plan(sigma, k, passes)
    if not hasattr(mats, "data_ptr"):
        mats = torch.from_numpy(np.ascontiguousarray(mats, dtype=np.float32)).cuda()
    mat_group = np.ascontiguousarray(mat_group, dtype=np.uint32)
    pdir = os.path.join(workdir, "passes")
    os.makedirs(pdir, exist_ok=True)
    thr = score_threshold(omega, sigma, k)
    n_nodes = total_num_groups or len(np.unique(mat_group)) + 1
    out = {"passes": len(steps), "lead": steps[0][0], "emitted": 0, "score_s": 0.0, "filter_s": 0.0, "write_s": 0.0,
           "merge_s": 0.0, "union_s": 0.0, "route": "device" if union_on_device else "files", "per_pass": []}
    paths = []
    held = []                         # union_on_device: (pass file's path, filtered database) of the passes so far

    def spill_held():
        # the device route has run out of memory: what it holds becomes pass files, and the build is the file mode's from here on
        t0 = time.time()
        for file, d in held:
            dbfile.write_db_device(engine, d, file, sequence_type, [], "", k, omega)
            d.free()
        del held[:]
        out["write_s"] += time.time() - t0
        out["route"] = "fallback"

    def on_device(step, again=True):
        # one step of the device route; IPKGPU_ERR_NOMEM: fall back, then the step once more (another failure stands) -- but for the
        # union itself, which the host merge of the pass files replaces
        try:
            return step()
        except IpkGpuError as e:
            if e.code != ERR_NOMEM or out["route"] != "device":
                raise
        spill_held()
        return step() if again else None

    def filter_db(d):
        t0 = time.time()
        if filter_ == "mif0":
            d.filter_mif0(engine, n_nodes, thr)
        elif filter_ == "random":
            d.filter_random(engine)
        else:
            raise ValueError(f"unknown filter {filter_!r} (mif0, random)")
        return time.time() - t0

    for lead, cls, base, span in steps:
        file = os.path.join(pdir, f"pass{cls}.ipk")
        paths.append(file)
        if out["route"] == "device":
            state = {}

            def score_pass():
                for key in ("db", "parts"):
                    if state.get(key) is not None:
                        state.pop(key).free()
                state["parts"] = engine.score_groups_keyrange(mats, mat_group, k, log_eps, lead, cls)
                state["db"] = engine.db_from_parts(state["parts"], sigma, k)
                state["t1"] = time.time()
                return filter_db(state["db"])
            t0 = time.time()
            try:
                filter_s = on_device(score_pass)
            except BaseException:
                for key in ("db", "parts"):
                    if state.get(key) is not None:
                        state[key].free()
                for _, d in held:
                    d.free()
                raise
            parts, db, t1, write_s = state["parts"], state["db"], state["t1"], 0.0
            if out["route"] == "device":
                held.append((file, db))
            else:
                t2 = time.time()
                dbfile.write_db_device(engine, db, file, sequence_type, [], "", k, omega)
                write_s = time.time() - t2
        else:
            t0 = time.time()
            parts = engine.score_groups_keyrange(mats, mat_group, k, log_eps, lead, cls)
            db = engine.db_from_parts(parts, sigma, k)
            t1 = time.time()
            filter_s, write_s = dbfile.filter_and_write_device(engine, db, file, filter_, sequence_type, [], "", k, omega, n_nodes, thr)
        out["emitted"] += parts.emitted
        out["score_s"] += t1 - t0
        out["filter_s"] += filter_s
        out["write_s"] += write_s
        out["per_pass"].append({"class": cls, "key_base": base, "keys": db.num_keys, "entries": db.num_entries,
                                "emitted": parts.emitted, "call_ms": parts.time_ms(T_TOTAL), "score_ms": parts.time_ms(T_SCORE_MAIN),
                                "reduce_ms": parts.time_ms(T_SCORE_REDUCE), "writer_ms": parts.time_ms(T_KM_WRITE),
                                "keys_ms": db.time_ms(), "shard_file_s": write_s})
        if not (held and held[-1][1] is db):
            db.free()
        parts.free()
    if out["route"] == "device":
        def union_and_write():
            u = engine.union_dbs([d for _, d in held])
            try:
                dbfile.write_db_device(engine, u, path, sequence_type, tree_index, newick, k, omega)
                return u.num_keys, u.num_entries
            finally:
                u.free()
        t0 = time.time()
        try:
            totals = on_device(union_and_write, again=False)
        except BaseException:
            for _, d in held:
                d.free()
            raise
        if out["route"] == "device":
            out["totals"] = totals
            out["union_s"] = time.time() - t0
            for _, d in held:
                d.free()
            del held[:]
            paths = []
    if out["route"] != "device":
        t0 = time.time()
        out["totals"] = dbfile.merge_shard_files(path, sequence_type, tree_index, newick, k, omega, paths)
        out["merge_s"] = time.time() - t0
    if not keep_pass_files:
        for p in paths:
            os.remove(p)
        try:
            os.rmdir(pdir)
        except OSError:
            pass
    return out
