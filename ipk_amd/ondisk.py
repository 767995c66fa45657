"""The on-disk build (`--on-disk`): a database that does not fit device memory, on one GPU, without positions.

The reference's on-disk mode (db_builder.cpp:137,340-458,673-681; branch_group.cpp:104-185) in three stages:

  1. the groups are scored in pieces -- contiguous ranges of the first-seen group order -- each split by owner = dense code % B
     (kmer_batch); every owner block of a piece leaves the device as workdir/hashmaps/p<piece>_b<batch>.blk (explore_group's spill);
  2. per batch b, the pieces' blocks come back in piece order (= group order = the reference's append order), are merged on the
     device, filtered and written as the shard file workdir/hashmaps/<b>.ipk (merge_stage1, get_batch_db_name);
  3. the B shard files are merged by (filter value, key) into the database file (merge_stage2).

MIF0's value and the random filter's draw are per k-mer and every k-mer lives in one batch, so filtering per batch is valid and the
file equals, byte for byte, the one the in-memory build writes.  The device never holds more than one piece's result or one batch of
the database; the engine's "device_budget_bytes" makes that a checked bound (Engine.mem_stats).  Nothing overlaps: the mode is
bound by the file system, as the reference's is ("slower but takes minimal RAM").
"""
import os
import shutil
import time

import numpy as np

from . import dbfile
from .engine import IpkGpuError, score_threshold

MAX_PIECE_GROUPS = 65535          # a spill block's counts are u16 and a key has at most one entry per group (spill_format.hpp)
HEAD_BYTES = 64
MAGIC = b"IPKSPILL"
ERR_NOMEM = 3


class OnDiskError(RuntimeError):
    pass


class PiecePlanner:
    """Cuts n_groups (first-seen order) into contiguous pieces against a budget of device bytes.

    next() gives the piece to score, [g0, g1); done(peak_bytes) reports what it held at most and moves on; nomem(need) reports that
    it did not fit: the same range is offered again cut in half, and one group that does not fit raises OnDiskError.  The first piece
    is one group.  Later ones are sized from the bytes seen so far -- the line through the peaks of the last two piece sizes (a
    piece's peak has a part that does not grow with its groups), before there are two sizes the bytes per group -- against the
    budget, at most 8 times the piece before, never above max_groups, and between the largest size that fitted and the smallest
    that did not by bisection."""

    def __init__(self, n_groups, budget_bytes, max_groups=MAX_PIECE_GROUPS, first=1, fill=0.5):
        self.n_groups, self.budget, self.max_groups, self.fill = int(n_groups), int(budget_bytes), int(max_groups), fill
        self.g0 = 0
        self.size = max(1, min(int(first), self.max_groups))
        self.good, self.bad = 0, self.max_groups + 1      # largest size that went through, smallest that did not fit
        self.last = None                                  # (groups, peak) of the piece before
        self.line = None                                  # (fixed bytes, bytes per group)
        self.pieces = []                                  # the (g0, g1) that went through

    def next(self):
        if self.g0 >= self.n_groups:
            return None
        return self.g0, min(self.n_groups, self.g0 + min(self.size, self.max_groups))

    def done(self, peak_bytes):
        g0, g1 = self.next()
        n = g1 - g0
        self.pieces.append((g0, g1))
        self.g0 = g1
        self.good = max(self.good, n)
        if self.last is not None and self.last[0] != n:
            per_group = max(1.0, (peak_bytes - self.last[1]) / (n - self.last[0]))
            self.line = (max(0.0, peak_bytes - per_group * n), per_group)
        self.last = (n, peak_bytes)
        if self.line is not None:
            want = int((0.9 * self.budget - self.line[0]) / self.line[1])
        else:
            want = int(self.budget * self.fill / max(1.0, float(peak_bytes) / n))
            if peak_bytes <= self.budget * self.fill:
                want = max(want, 2 * n)                   # (half the budget unused: twice the groups fit)
        cap = self.max_groups if self.bad > self.max_groups else max(self.good, (self.good + self.bad) // 2)
        self.size = max(1, min(want, 8 * n, cap, self.bad - 1))

    def nomem(self, need_bytes=None):
        g0, g1 = self.next()
        n = g1 - g0
        if n <= 1:
            need = f"at least {int(need_bytes)} bytes" if need_bytes else "more"
            raise OnDiskError(f"one branch group needs {need} of device memory, the budget is {self.budget} bytes: "
                              "the on-disk build cannot cut below one group")
        self.bad = min(self.bad, n)
        self.size = max(1, n // 2)


class FixedPlanner(PiecePlanner):
    """Pieces of given sizes (tests: the result must not depend on where the cuts fall); a piece that does not fit is still halved."""

    def __init__(self, n_groups, budget_bytes, sizes):
        super().__init__(n_groups, budget_bytes)
        self.sizes, self.i = list(sizes), 0
        self.size = self.sizes[0]

    def done(self, peak_bytes):
        g0, g1 = self.next()
        self.pieces.append((g0, g1))
        self.g0 = g1
        self.i += 1
        self.size = self.sizes[min(self.i, len(self.sizes) - 1)]


def block_path(hdir, piece, batch):
    return os.path.join(hdir, f"p{piece}_b{batch}.blk")


def read_block(path):
    """Parses a spill block (ipk_amd/csrc/spill_format.hpp) with numpy: a dict of the head's fields, `bits` u64 [ceil(slots / 64)],
    `counts` u16 [n_keys] and `entries` u32 [n_entries, 2] (branch, score bits).  The reader of the tests and of whoever looks at a
    kept workdir; the build itself reads blocks inside the library (ipkgpu_spill_merge)."""
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.size < HEAD_BYTES or raw[:8].tobytes() != MAGIC:
        raise ValueError(f"{path}: not a spill block")
    w = raw[8:32].view(np.uint32)
    q = raw[32:64].view(np.uint64)
    out = {"version": int(w[0]), "sigma": int(w[1]), "k": int(w[2]), "n_owners": int(w[3]), "owner": int(w[4]), "piece": int(w[5]),
           "slots": int(q[0]), "n_keys": int(q[1]), "n_entries": int(q[2])}
    words = (out["slots"] + 63) // 64
    at = HEAD_BYTES
    c_bytes = (out["n_keys"] * 2 + 7) // 8 * 8
    if raw.size != at + words * 8 + c_bytes + out["n_entries"] * 8:
        raise ValueError(f"{path}: the file size does not match its head")
    out["bits"] = raw[at:at + words * 8].view(np.uint64)
    at += words * 8
    out["counts"] = raw[at:at + out["n_keys"] * 2].view(np.uint16)
    at += c_bytes
    out["entries"] = raw[at:].view(np.uint32).reshape(-1, 2)
    return out


def pack_counts(row):
    """(bits u64, counts u16) of a dense counts row, as a block holds them -- what numpy derives, for the tests."""
    row = np.asarray(row)
    words = (row.size + 63) // 64
    occ = np.zeros(words * 64, dtype=np.uint8)
    occ[:row.size] = row != 0
    bits = np.packbits(occ.reshape(words, 64), axis=1, bitorder="little").view(np.uint64).reshape(words)
    return bits, row[row != 0].astype(np.uint16)


def _piece_matrices(mats, slot_of, g0, g1):
    """The matrices of groups [g0, g1) in input order, on the device, for one call."""
    import torch
    sel = np.flatnonzero((slot_of >= g0) & (slot_of < g1))
    lo, hi = (int(sel[0]), int(sel[-1]) + 1) if sel.size else (0, 0)
    whole = hi - lo == sel.size
    if hasattr(mats, "data_ptr"):
        return (mats[lo:hi] if whole else mats[torch.from_numpy(sel).to(mats.device)]).contiguous(), sel
    host = mats[lo:hi] if whole else mats[sel]
    return torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).cuda(), sel


def build_db_file(engine, mats, mat_group, k, log_eps, sigma, path, workdir, sequence_type, tree_index, newick, omega,
                  filter_="mif0", total_num_groups=None, batches=32, budget_bytes=None, keep_files=False, piece_sizes=None):
    """Builds the database file `path` through workdir/hashmaps with at most `budget_bytes` of device memory held by the engine
    (None: half of the free device memory, the rule of "workspace_bytes").  mats: [n_mats, sites, sigma] float32, numpy (the
    matrices may stay in host memory: a piece's are uploaded for its call) or a CUDA tensor.  piece_sizes: groups per piece instead
    of the planner's (tests).  Returns a dict: totals (k-mers, entries), emitted, pieces, batches, stage1_s / stage2_s / stage3_s,
    filter_s (inside stage 2), spilled_bytes, dense_bytes (what the blocks' dense form would have taken), held_peak (and its
    parts stage1_peak, stage2_peak), budget_bytes."""
    import torch

    B = int(batches)
    if B < 1:
        raise ValueError("batches must be >= 1")
    mat_group = np.ascontiguousarray(mat_group, dtype=np.uint32)
    order = list(dict.fromkeys(mat_group.tolist()))                      # first-seen order (db_builder.cpp:524-553)
    index = {g: i for i, g in enumerate(order)}
    slot_of = np.array([index[g] for g in mat_group.tolist()], dtype=np.int64)
    n_groups = len(order)
    n_nodes = total_num_groups or n_groups + 1
    thr = score_threshold(omega, sigma, k)
    slots = (sigma ** k + B - 1) // B
    if budget_bytes is None:
        budget_bytes = torch.cuda.mem_get_info()[0] // 2
    budget_bytes = int(budget_bytes)
    hdir = os.path.join(workdir, "hashmaps")
    os.makedirs(hdir, exist_ok=True)
    old = {name: engine.get_option(name) for name in ("device_budget_bytes", "workspace_bytes")}
    engine.set_option("release_workspaces", 1)                           # what earlier calls left on the device is not this build's
    engine.set_option("device_budget_bytes", budget_bytes)
    engine.set_option("workspace_bytes", max(1, budget_bytes // 2))
    out = {"batches": B, "budget_bytes": budget_bytes, "emitted": 0, "spilled_bytes": 0, "dense_bytes": 0, "filter_s": 0.0, "held_peak": 0}
    try:
        # ---- stage 1: pieces of groups, scored split by batch, every block to a file
        t0 = time.time()
        plan = FixedPlanner(n_groups, budget_bytes, piece_sizes) if piece_sizes else PiecePlanner(n_groups, budget_bytes)
        engine.mem_stats(reset_peak=True)
        while plan.next() is not None:
            g0, g1 = plan.next()
            piece = len(plan.pieces)
            parts = None
            try:
                dev, sel = _piece_matrices(mats, slot_of, g0, g1)
                parts = engine.score_groups_keymajor(dev, mat_group[sel], k, log_eps, n_owners=B)
                spilled = engine.parts_spill(parts, hdir, piece)
            except IpkGpuError as e:
                if e.code != ERR_NOMEM:
                    raise
                plan.nomem(engine.get_option("last_refused_bytes"))
                continue
            finally:
                if parts is not None:
                    emitted, entries = parts.emitted, parts.num_entries
                    parts.free()
                dev = None
            out["emitted"] += emitted
            out["spilled_bytes"] += spilled
            out["dense_bytes"] += B * slots * 4 + entries * 8
            peak = engine.mem_stats(reset_peak=True)[1]
            out["held_peak"] = max(out["held_peak"], peak)
            plan.done(peak)
        n_pieces = len(plan.pieces)
        out["pieces"] = n_pieces
        out["piece_ranges"] = list(plan.pieces)
        out["stage1_s"] = time.time() - t0
        out["stage1_peak"] = out["held_peak"]
        engine.set_option("release_workspaces", 1)                       # the scoring workspaces are not needed any more
        engine.mem_stats(reset_peak=True)

        # ---- stage 2: per batch, the pieces' blocks back in piece order -> merge, filter, shard file
        t0 = time.time()
        shard_paths, n_keys, n_entries, stage2_peak = [], 0, 0, 0
        for b in range(B):
            blocks = [block_path(hdir, p, b) for p in range(n_pieces)]
            shard = os.path.join(hdir, f"{b}.ipk")                       # get_batch_db_name (db_builder.cpp:460-464)
            db = None
            try:
                db = engine.spill_merge(sigma, k, b, B, blocks)
                out["filter_s"] += dbfile.filter_and_write_device(engine, db, shard, filter_, sequence_type, [], "", k, omega, n_nodes, thr)[0]
                n_keys += db.num_keys
                n_entries += db.num_entries
            except IpkGpuError as e:
                if e.code != ERR_NOMEM:
                    raise
                # (merged: the blocks' dense rows and their scan, 12 bytes per slot and block, the entries twice; then filter and writer)
                need = n_pieces * slots * 12 + 3 * sum(os.path.getsize(f) for f in blocks)
                fit = max(B + 1, -(-B * need // max(1, budget_bytes * 3 // 4)))
                raise OnDiskError(f"batch {b} of {B} does not fit the budget of {budget_bytes} bytes of device memory (about {need} bytes for "
                                  f"its {n_pieces} blocks, merged, filtered and written): {fit} batches would fit") from e
            finally:
                if db is not None:
                    db.free()
            shard_paths.append(shard)
            if not keep_files:
                for f in blocks:
                    os.remove(f)
            stage2_peak = max(stage2_peak, engine.mem_stats(reset_peak=True)[1])
            out["held_peak"] = max(out["held_peak"], stage2_peak)
        out["stage2_s"] = time.time() - t0
        out["stage2_peak"] = stage2_peak

        # ---- stage 3: the shard files merged by (filter value, key)
        t0 = time.time()
        out["totals"] = dbfile.merge_shard_files(path, sequence_type, tree_index, newick, k, omega, shard_paths)
        out["stage3_s"] = time.time() - t0
        if tuple(out["totals"]) != (n_keys, n_entries):
            raise OnDiskError(f"the merged file holds {out['totals']} (k-mers, entries), the batches {(n_keys, n_entries)}")
    finally:
        if not keep_files:
            shutil.rmtree(hdir, ignore_errors=True)                      # as the reference does (db_builder.cpp:213); after a failure too
        engine.set_option("release_workspaces", 1)
        for name, value in old.items():
            if name == "device_budget_bytes" or value > 0:
                engine.set_option(name, value)
    return out
