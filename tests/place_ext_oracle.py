"""The definition of ipkgpu_db_place_opts (include/ipkgpu.h) restated on the host, on top of tests/place_oracle.py: windows with one
ambiguous symbol expanded into their resolutions, both strands placed.  y of an ambiguous window is computed with plain Python floats
(10.0 ** x, math.log10); the strands are the same placement of the Python-reversed, complemented string.  `variant` names a WRONG
implementation (tests/test_place_ext_inputs.py proves that the cases tell each from the definition).  Test infrastructure only."""
import math

import numpy as np

from tests import place_oracle as po

AMBIGUOUS = {4: {"R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"},
             20: {"B": "DN", "Z": "EQ", "J": "IL", "X": po.ALPHABET[20][0]}}
COMPLEMENT = dict(zip("ACGTURYKMBVDHacgturykmbvdh", "TGCAAYRMKVBHDtgcaayrmkvbhd"))      # S, W, N and every other byte: themselves
COMPLEMENT_PLAIN_ONLY = dict(zip("ACGTUacgtu", "TGCAAtgcaa"))                              # the variant "no_complement_codes"
VARIANTS = ("no_threshold", "amb_after_tile", "no_complement_codes", "mean_of_logs")


def revcomp(seq, table=COMPLEMENT):
    return "".join(table.get(ch, ch) for ch in reversed(seq))


def windows(seq, sigma, k):
    """[(start, [codes])] of the exact (one code) and ambiguous (R codes, ascending symbol code) windows of `seq`, ascending start."""
    letters, bits = po.ALPHABET[sigma]
    plain = {ch: i for i, ch in enumerate(letters)}
    if sigma == 4:
        plain["U"] = 3
    res = {a: sorted(plain[ch] for ch in r) for a, r in AMBIGUOUS[sigma].items()}
    s = seq.upper()
    out = []
    for st in range(0, len(s) - k + 1):
        w = s[st:st + k]
        amb = [i for i, ch in enumerate(w) if ch in res]
        if any(ch not in plain and ch not in res for ch in w) or len(amb) > 1:
            continue
        codes = []
        for sym in (res[w[amb[0]]] if amb else [None]):
            code = 0
            for i, ch in enumerate(w):
                code = (code << bits) | (sym if amb and i == amb[0] else plain[ch])
            codes.append(code)
        out.append((st, codes))
    return out


def contribution(db, codes, E, variant=None):
    """(any resolution a key, {branch: y f32}) of an ambiguous window with the resolution codes `codes`."""
    R = len(codes)
    named = {}                                             # branch -> its scores, resolutions in ascending order
    found = False
    for code in codes:
        e = db.entries(code)
        if e is None:
            continue
        found = True
        for b, x in zip(e[0].tolist(), e[1]):
            named.setdefault(b, []).append(float(x))
    ys = {}
    for b, xs in named.items():
        c = len(xs)
        if variant == "mean_of_logs":
            ys[b] = np.float32((math.fsum(xs) + (R - c) * math.log10(E)) / R)
            continue
        P = 0.0
        for x in xs:
            P = P + 10.0 ** x
        if variant != "no_threshold":
            P = P + float(R - c) * E
        ys[b] = np.float32(math.log10(P / float(R)))
    return found, ys


def accumulate(db, seq, sigma, k, log_eps, variant=None):
    """(W, n_found, n_ambiguous, S f32 [B], C i64 [B]): po.accumulate's loop with the ambiguous windows at their own places."""
    E = 10.0 ** float(np.float32(log_eps))
    wins = windows(seq, sigma, k)
    if variant == "amb_after_tile":                        # a tile's ambiguous windows after its exact ones
        wins = sorted(wins, key=lambda w: (w[0] // 64, len(w[1]) > 1, w[0]))
    S, Cn, found, n_amb = np.zeros(db.n_branches, np.float32), np.zeros(db.n_branches, np.int64), 0, 0
    for _, codes in wins:
        if len(codes) == 1:
            e = db.entries(codes[0])
            if e is None:
                continue
            found += 1
            S[e[0]] = S[e[0]] + e[1]
            Cn[e[0]] += 1
            continue
        n_amb += 1
        any_key, ys = contribution(db, codes, E, variant)
        found += int(any_key)
        for b, y in ys.items():
            S[b] = S[b] + y
            Cn[b] += 1
    return len(wins), found, n_amb, S, Cn


def place_strand(db, seq, sigma, k, log_eps, keep_at_most, ambiguity, variant=None):
    """po.place_one's dict plus n_ambiguous, of one strand."""
    if not ambiguity:
        return dict(po.place_one(db, seq, sigma, k, log_eps, keep_at_most), n_ambiguous=0)
    W, found, n_amb, S, Cn = accumulate(db, seq, sigma, k, log_eps, variant)
    hit = np.nonzero(Cn)[0]
    pen = (W - Cn[hit]).astype(np.float32) * np.float32(log_eps)
    score = S[hit] + pen
    assert score.dtype == np.float32
    order = sorted(range(len(hit)), key=lambda i: (-float(score[i]), int(hit[i])))
    pl = []
    if order:
        m = float(score[order[0]])
        terms = [10.0 ** (float(score[i]) - m) for i in order]
        den = math.fsum(terms)
        pl = [(int(hit[i]), score[i], int(Cn[hit[i]]), terms[r] / den) for r, i in enumerate(order[:keep_at_most])]
    return dict(n_kmers=W, n_found=found, n_branches=len(order), placements=pl, n_ambiguous=n_amb)


def place_one(db, seq, sigma, k, log_eps, keep_at_most, ambiguity=False, strands="given", variant=None):
    seq = seq.decode() if isinstance(seq, bytes) else seq
    given = dict(place_strand(db, seq, sigma, k, log_eps, keep_at_most, ambiguity, variant), strand=0)
    if strands != "both":
        return given
    rc = revcomp(seq, COMPLEMENT_PLAIN_ONLY if variant == "no_complement_codes" else COMPLEMENT)
    rev = dict(place_strand(db, rc, sigma, k, log_eps, keep_at_most, ambiguity, variant), strand=1)
    if rev["placements"] and (not given["placements"] or float(rev["placements"][0][1]) > float(given["placements"][0][1])):
        return rev
    return given


def place(db, seqs, sigma, k, log_eps, keep_at_most, ambiguity=False, strands="given", variant=None):
    return [place_one(db, s, sigma, k, log_eps, keep_at_most, ambiguity, strands, variant) for s in seqs]


def check(res, want, q=None):
    """po.check, and strand and n_ambiguous exactly."""
    po.check(res, want, q)
    for i in (range(len(want)) if q is None else [q]):
        assert (int(res.strand[i]), int(res.n_ambiguous[i])) == (want[i]["strand"], want[i]["n_ambiguous"]), i
