"""CPU suite: the inputs of tests/test_gpu_place_ext.py do what they are for.  The properties of tests/place_ext_cases.py by
hand-written counts; four wrong implementations (place_ext_oracle.VARIANTS) each change an expected score bit or count; every
ambiguous contribution of every case lies at least 2^-44 from a binary32 rounding midpoint and the oracle's y is the correctly
rounded one -- so a device whose binary64 exp10 and log10 are within 3 ulp (OpenCL's bounds, taken as the bound and not measured
on the device) rounds to the same float: P is a sum of at most 21 positive terms, each within 3 ulp, so within (3 + 21) 2^-53
relative, which log10 turns into 24 x 2^-53 / ln 10 < 2^-49.6 absolute; log10's own 3 ulp at |y| < 16 (mixed_scores reaches
-10.5) are 3 x 2^-49 < 2^-47.4; together below 2^-47, an eighth of the margin."""
import decimal
import math

import numpy as np
import pytest

from tests import place_ext_cases as xc
from tests import place_ext_oracle as xo

K = xc.K
DNA_CODES = set("RYSWKMBDHVN")


def amb_at(s):
    return [i for i, ch in enumerate(s.upper()) if ch in DNA_CODES]


def n_windows(s, bad):
    """(W, ambiguous) of a DNA query counted from its characters: a window is lost to a byte of `bad` or to two ambiguous symbols."""
    W = amb = 0
    for st in range(len(s) - K + 1):
        w = s[st:st + K].upper()
        if any(ch in bad for ch in w):
            continue
        n = sum(ch in DNA_CODES for ch in w)
        W += n <= 1
        amb += n == 1
    return W, amb


def test_positions_of_the_ambiguous_symbol():
    c = xc.main_ext_case()
    q, want = c.queries, c.expected(7)
    assert amb_at(q[0]) == [7] and len(q[0]) == 2 * K - 1          # windows 0 .. 7 hold it at positions 7 .. 0
    assert (want[0]["n_kmers"], want[0]["n_ambiguous"], want[0]["n_found"]) == (K, K, K)
    assert [amb_at(q[i]) for i in (1, 2, 3, 4)] == [[0], [63], [64], [64 + K - 2]]
    assert amb_at(q[5]) == [len(q[5]) - 1]
    for i in (1, 2, 3, 4):
        assert want[i]["n_ambiguous"] == min(K, amb_at(q[i])[0] + 1) and want[i]["n_kmers"] == len(q[i]) - K + 1
    assert want[5]["n_ambiguous"] == 1
    # two symbols k apart: 2 k ambiguous windows, none lost; 4 apart: the 4 windows holding both are lost, 4 + 4 expanded; NN: 7 lost, 2 expanded
    assert np.diff(amb_at(q[6])).tolist() == [K] and (want[6]["n_kmers"], want[6]["n_ambiguous"]) == (len(q[6]) - K + 1, 2 * K)
    assert np.diff(amb_at(q[7])).tolist() == [4] and (want[7]["n_kmers"], want[7]["n_ambiguous"]) == (len(q[7]) - K + 1 - 4, 8)
    assert np.diff(amb_at(q[8])).tolist() == [1] and (want[8]["n_kmers"], want[8]["n_ambiguous"]) == (len(q[8]) - K + 1 - 7, 2)
    for i, s in enumerate(q):
        assert (want[i]["n_kmers"], want[i]["n_ambiguous"]) == n_windows(s, "X*?-"), i
    # queries of several tiles with ambiguous windows in a later tile
    assert len(q[19]) > 200 and max(amb_at(q[19])) > 128


def test_resolutions_and_case():
    c = xc.main_ext_case()
    q, want = c.queries, c.expected(64)
    sizes = {len(codes) for _, codes in xo.windows(q[9], 4, K)}
    assert sizes == {1, 2, 3, 4}
    assert {ch for ch in q[9] if ch in DNA_CODES} == DNA_CODES
    assert q[10] == q[9].lower() and q[10] != q[9]
    assert want[10] == want[9] or all(str(a) == str(b) for a, b in zip(want[10]["placements"], want[9]["placements"]))
    assert want[9]["n_found"] > 0 and want[9]["n_ambiguous"] == 11 * K
    # -, *, ? and X stay invalid: the query places as it does with '#' in their places, and an X is not an N
    inv = q[11]
    for ch in "-*?X":
        assert ch in inv
        assert str(xo.place_one(c.view, inv.replace(ch, "#"), 4, K, xc.LOG_EPS, 64, True)) == str(want[11])
    assert str(xo.place_one(c.view, inv.replace("X", "N"), 4, K, xc.LOG_EPS, 64, True)) != str(want[11])
    assert want[11]["n_ambiguous"] > 0


def test_planted_groups():
    c = xc.main_ext_case()
    for name, (w, counts, shares) in xc.GROUPS.items():
        codes = xc._codes(w, 4)
        assert len(codes) == len(counts)
        ent = [c.view.entries(code) for code in codes]
        assert [0 if e is None else len(e[0]) for e in ent] == counts, name
        for b, rs in shares.items():
            assert [r for r, e in enumerate(ent) if e is not None and b in e[0]] == rs, (name, b)
    assert sorted(len(v[2]) and sorted(len(rs) for rs in v[2].values()) for v in xc.GROUPS.values() if v[2]) == [[1, 2], [1, 2, 3], [1, 2, 3, 4]]
    assert xc.GROUPS["all4"][1] == [63, 64, 65, 129]
    want = c.expected(64)
    found = {n: want[12 + i]["n_found"] for i, n in enumerate(("all4", "all3", "all2", "one", "none"))}
    assert found == {"all4": 1, "all3": 1, "all2": 1, "one": 1, "none": 0}
    assert want[16]["placements"] == [] and want[16]["n_kmers"] == 1 and want[15]["n_branches"] == 17
    # one window each: every branch of queries 12 .. 15 is touched by an ambiguous window only
    assert all(want[i]["n_kmers"] == want[i]["n_ambiguous"] == 1 and want[i]["n_branches"] > 0 for i in (12, 13, 14, 15))


def first_touch(c, s):
    """branch -> (kind of the first window that scores it, kinds of all windows that score it); kind: True = ambiguous."""
    seen = {}
    for _, codes in xo.windows(s, c.sigma, c.k):
        named = set()
        for code in codes:
            e = c.view.entries(code)
            if e is not None:
                named |= set(e[0].tolist())
        for b in named:
            seen.setdefault(b, []).append(len(codes) > 1)
    return seen


def test_branches_first_touched_by_ambiguous_windows_and_shared_by_consecutive_ones():
    c = xc.main_ext_case()
    seen = first_touch(c, c.queries[18])                        # an ambiguous window first, exact windows after it
    assert any(v[0] and not all(v) for v in seen.values())      # first touched by the ambiguous window, then by exact ones
    seen = first_touch(c, c.queries[17])
    assert any(v[0] and not all(v) for v in seen.values()) and any(not v[0] and any(v) for v in seen.values()) and any(all(v) for v in seen.values())
    seen = first_touch(c, c.queries[0])                         # 8 consecutive ambiguous windows
    assert max(len(v) for v in seen.values()) == K and sum(len(v) >= 2 for v in seen.values()) > 50


def test_amino_acid_cases():
    for k in (3, 6):
        c = xc.aa_ext_case(k)
        want = c.expected(7)
        sizes = set()
        for s in c.queries:
            sizes |= {len(codes) for _, codes in xo.windows(s, 20, k)}
        assert sizes == {1, 2, 20}
        assert len(xc._codes(c.queries[0], 20)) == 20 and all(c.view.entries(code) is not None for code in xc._codes(c.queries[0], 20))
        for ch in "BZJX":
            assert any(ch in s for s in c.queries)
        assert want[0]["n_found"] == 1 and want[0]["n_ambiguous"] == 1 and sum(w["n_ambiguous"] for w in want) > 30
        assert want[4]["n_ambiguous"] == 2                      # XX
        assert all(w["placements"] for w in want[:4])


def test_strand_cases():
    c = xc.strand_case()
    q, S = c.queries, xc.STRAND
    plain = c.expected(7, False, "both")
    given = c.expected(7, False, "given")
    rev = xo.place(c.view, [xo.revcomp(s) for s in q], 4, K, xc.LOG_EPS, 7)
    assert xo.revcomp("ACGTURYKMBVDHSWNacgt-x") == "x-acgtNWSDHBVKMRYAACGT"
    assert plain[S["reverse_wins"]]["strand"] == 1 and plain[S["given_wins"]]["strand"] == 0
    assert rev[S["given_wins"]]["placements"] == [] or float(rev[S["given_wins"]]["placements"][0][1]) < float(given[S["given_wins"]]["placements"][0][1])
    p = S["palindrome"]
    assert xo.revcomp(q[p]) == q[p] and plain[p]["strand"] == 0 and plain[p]["placements"]
    assert plain[S["neither"]]["placements"] == [] and rev[S["neither"]]["placements"] == [] and plain[S["neither"]]["strand"] == 0
    o = S["only_reverse"]
    assert given[o]["placements"] == [] and plain[o]["strand"] == 1 and plain[o]["placements"]
    first = S["len_first"]
    assert [len(q[first + i]) for i in range(5)] == [K - 1, K, K + 63, K + 64, K + 65]
    assert [plain[first + i]["strand"] for i in range(5)] == [0, 1, 1, 1, 1] and plain[first]["n_kmers"] == 0
    assert [plain[first + i]["n_found"] for i in range(1, 5)] == [1, 64, 65, 66]
    # R, K, B and D: the reverse strand wins only with the codes complemented
    both = c.expected(7, True, "both")
    wrong = c.expected(7, True, "both", "no_complement_codes")
    i = S["codes"]
    assert set("RKBD") <= set(q[i]) and both[i]["strand"] == 1 and both[i]["n_ambiguous"] == both[i]["n_kmers"] == len(q[i]) - K + 1
    assert wrong[i]["strand"] == 0 and wrong[i]["placements"] and plain[i]["placements"] == []
    # strands and ambiguity together: a query with an N whose reverse wins
    assert any(w["strand"] == 1 and w["n_ambiguous"] > 0 and w["n_found"] > w["n_ambiguous"] for w in both)


def differences(variant):
    """(queries whose expected placements differ, queries) over every case and mode, the variant against the definition."""
    diff = total = 0
    for name, make in xc.ALL_CASES.items():
        c = make()
        for ambiguity, strands in xc.MODES[name]:
            a, b = c.expected(64, ambiguity, strands), c.expected(64, ambiguity, strands, variant)
            diff += sum(str(x) != str(y) for x, y in zip(a, b))
            total += len(a)
    return diff, total


@pytest.mark.parametrize("variant", xo.VARIANTS)
def test_wrong_implementations_are_told_apart(variant):
    diff, total = differences(variant)
    print(f"variant {variant}: {diff} of {total} expected query results differ")
    assert diff > 0


def contributions(cases=None, modes=None):
    """{(scores of the resolutions naming a branch, R)} over every ambiguous window of every case, on every strand a mode places."""
    cases, modes = (xc.ALL_CASES, xc.MODES) if cases is None else (cases, modes)
    out = set()
    for name, make in cases.items():
        c = make()
        both = any(s == "both" for a, s in modes[name] if a)
        for s in c.queries:
            for seq in ([s, xo.revcomp(s)] if both else [s]):
                for _, codes in xo.windows(seq, c.sigma, c.k):
                    if len(codes) == 1:
                        continue
                    named = {}
                    for code in codes:
                        e = c.view.entries(code)
                        if e is not None:
                            for b, x in zip(e[0].tolist(), e[1]):
                                named.setdefault(b, []).append(float(x))
                    out |= {(tuple(xs), len(codes)) for xs in named.values()}
    return out


def rounding_margin(cases, modes, log_eps, at_least, but=()):
    """Every ambiguous contribution of `cases` under the threshold `log_eps`: the oracle's y is the correctly rounded one and the
    60-digit value lies at least 2^-44 from a binary32 rounding midpoint (`but`: contributions the caller checks by itself).
    -> (contributions, the closest distance)."""
    D = decimal.Decimal
    margin = D(2) ** -44
    E32 = float(np.float32(log_eps))
    E = 10.0 ** E32
    seen = contributions(cases, modes)
    assert set(but) <= seen
    seen -= set(but)
    closest = D(1)
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        pow10 = {}
        for xs, R in seen:
            for x in xs + (E32,):
                if x not in pow10:
                    pow10[x] = D(10) ** D(x)
            y = ((sum((pow10[x] for x in xs), D(0)) + (R - len(xs)) * pow10[E32]) / R).log10()
            P = 0.0
            for x in xs:
                P = P + 10.0 ** x
            P = P + float(R - len(xs)) * E
            got = np.float32(math.log10(P / float(R)))
            f = np.float32(float(y))
            cand = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
            right = min(cand, key=lambda v: abs(D(float(v)) - y))
            assert got.view(np.uint32) == np.float32(right).view(np.uint32), (xs, R)
            d = min(abs(y - (D(float(cand[0])) + D(float(cand[1]))) / 2), abs(y - (D(float(cand[1])) + D(float(cand[2]))) / 2))
            closest = min(closest, d)
            assert d >= margin, (xs, R, float(d))
            assert abs(y) <= 10.5                               # (mixed_scores: at most 7 x 1.5 in magnitude)
    print(f"log_eps {float(E32)!r}: {len(seen)} distinct ambiguous contributions; the closest to a binary32 rounding midpoint: {float(closest):.3e} "
          f"(margin {float(margin):.3e})")
    assert len(seen) > at_least
    return len(seen), closest


def test_rounding_margin_of_every_ambiguous_contribution():
    rounding_margin(xc.ALL_CASES, xc.MODES, xc.LOG_EPS, 1000)
