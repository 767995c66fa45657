"""The placement definition of include/ipkgpu.h (ipkgpu_db_place) restated on the host: the sequential loop, np.float32 arithmetic step
by step, the likelihood weight ratios in binary64 with math.fsum.  Test infrastructure only: nothing under ipk_amd/ imports it."""
import math

import numpy as np

ALPHABET = {4: ("ACGT", 2), 20: ("RHKDESTNQCGPAILMFWYV", 5)}          # the code order of ipk_amd.cli._ALPHABET
NONE = 0xFFFFFFFF


def symbol_codes(sigma):
    """byte -> symbol code, -1 for an invalid byte (case-insensitive; DNA: U = T)."""
    letters, _ = ALPHABET[sigma]
    t = np.full(256, -1, np.int64)
    for i, ch in enumerate(letters):
        t[ord(ch)] = i
        t[ord(ch.lower())] = i
    if sigma == 4:
        t[ord("U")] = t[ord("u")] = 3
    return t


def encode_kmer(kmer, sigma):
    """The packed code of a k-mer string, first symbol in the highest bits (the inverse of cli.decode_kmer)."""
    letters, bits = ALPHABET[sigma]
    code = 0
    for ch in kmer:
        code = (code << bits) | letters.index(ch)
    return code


def window_codes(seq, sigma, k):
    """[(start, code)] of the valid windows of `seq` (str or bytes), ascending start."""
    raw = seq.encode() if isinstance(seq, str) else bytes(seq)
    t, bits = symbol_codes(sigma), ALPHABET[sigma][1]
    sym = t[np.frombuffer(raw, np.uint8)] if raw else np.zeros(0, np.int64)
    out = []
    for s in range(0, len(raw) - k + 1):
        w = sym[s:s + k]
        if (w < 0).any():
            continue
        code = 0
        for c in w:
            code = (code << bits) | int(c)
        out.append((s, code))
    return out


class DbView:
    """key -> (branches, scores) of a database given as the arrays of dbfile.write_db / Db.keys() etc."""

    def __init__(self, keys, key_offsets, branches, scores):
        self.branches, self.scores = np.asarray(branches, np.uint32), np.asarray(scores, np.float32)
        self.range = {int(k): (int(key_offsets[i]), int(key_offsets[i + 1])) for i, k in enumerate(keys)}
        self.n_branches = int(self.branches.max()) + 1 if len(self.branches) else 0

    def entries(self, code):
        r = self.range.get(code)
        return None if r is None else (self.branches[r[0]:r[1]].astype(np.int64), self.scores[r[0]:r[1]])


def accumulate(db, seq, sigma, k, reverse=False):
    """(W, n_found, S f32 [B], C i64 [B]): the sequential loop over the valid windows in ascending start, S[b] = S[b] + x in np.float32
    for each entry of a window's key (a key names a branch once, so one vector statement per window is that loop).
    reverse: the windows walked in descending start (the order-sensitivity proof)."""
    wins = window_codes(seq, sigma, k)
    S, Cn, found = np.zeros(db.n_branches, np.float32), np.zeros(db.n_branches, np.int64), 0
    for _, code in (reversed(wins) if reverse else wins):
        e = db.entries(code)
        if e is None:
            continue
        found += 1
        assert len(np.unique(e[0])) == len(e[0]), "precondition: a key names a branch once"
        S[e[0]] = S[e[0]] + e[1]
        Cn[e[0]] += 1
    return len(wins), found, S, Cn


def place_one(db, seq, sigma, k, log_eps, keep_at_most):
    """dict(n_kmers, n_found, n_branches, placements = [(branch, score f32, count, lwr f64)] best first, at most keep_at_most)."""
    W, found, S, Cn = accumulate(db, seq, sigma, k)
    hit = np.nonzero(Cn)[0]
    pen = (W - Cn[hit]).astype(np.float32) * np.float32(log_eps)            # one rounding: the product
    score = S[hit] + pen                                                    # one rounding: the sum
    assert score.dtype == np.float32 and pen.dtype == np.float32
    order = sorted(range(len(hit)), key=lambda i: (-float(score[i]), int(hit[i])))
    pl = []
    if order:
        m = float(score[order[0]])
        terms = [10.0 ** (float(score[i]) - m) for i in order]
        den = math.fsum(terms)
        pl = [(int(hit[i]), score[i], int(Cn[hit[i]]), terms[r] / den) for r, i in enumerate(order[:keep_at_most])]
    return dict(n_kmers=W, n_found=found, n_branches=len(order), placements=pl)


def place(db, seqs, sigma, k, log_eps, keep_at_most):
    return [place_one(db, s, sigma, k, log_eps, keep_at_most) for s in seqs]


def lwr_tolerance(n_branches):
    """Relative error allowed on an lwr of a query with T scored branches: 64 (T + 1) 2^-53 (derivation: tests/test_gpu_place.py)."""
    return 64.0 * (n_branches + 1) * 2.0 ** -53


def check(res, want, q=None):
    """Asserts that query i of an ipk_amd Placements equals want[i] (place()): branches, order, score bits and counts exactly, the three
    per-query figures exactly, lwr within lwr_tolerance."""
    idx = range(len(want)) if q is None else [q]
    assert res.n == len(want)
    for i in idx:
        w = want[i]
        assert (int(res.n_kmers[i]), int(res.n_found[i]), int(res.n_branches[i])) == (w["n_kmers"], w["n_found"], w["n_branches"]), i
        pl = w["placements"]
        n = len(pl)
        assert res.branches[i, :n].tolist() == [p[0] for p in pl], i
        assert (res.branches[i, n:] == NONE).all(), i
        assert res.scores[i, :n].view(np.uint32).tolist() == [int(np.float32(p[1]).view(np.uint32)) for p in pl], i
        assert res.counts[i, :n].tolist() == [p[2] for p in pl], i
        tol = lwr_tolerance(w["n_branches"])
        for j, p in enumerate(pl):
            assert abs(float(res.lwr[i, j]) - p[3]) <= tol * p[3], (i, j, float(res.lwr[i, j]), p[3])
