"""CPU suite: the properties of the inputs of tests/test_gpu_place_ext_paths.py (tests/place_ext_cases.py, from expected_ext_at() on),
counted with the host oracle (tests/place_ext_oracle.py).  Conditions on inputs, no measurement of the engine: where each planted
resolution lands in the prefix table, the last branch under ambiguous windows, the strand flips, the alias bytes, the inexact
threshold, the strand tie, the draws of the reuse and budget tests, the rule of db_place.hpp restated for the budget tests -- and
the rounding margin of tests/test_place_ext_inputs.py over the new cases at both thresholds, and the ladder's recorded distances.

Every test prints the counts it asserts on (pytest -s); profiles/place_ext_paths.txt records them."""
import math

import numpy as np
import pytest

from tests import place_cases as pc
from tests import place_ext_cases as xc
from tests import place_ext_oracle as xo
from tests import place_oracle as po
from tests.test_place_ext_inputs import rounding_margin

K = xc.K


def note(line):
    print("| " + line)


# ---- 1a. lookup -------------------------------------------------------------------------------------------------------------------------

LOOKUPS = [(s, k, t) for s, k in xc.LOOKUP_EXT_SHAPES for t in (False, True)]


@pytest.mark.parametrize("sigma,k,tail", LOOKUPS)
def test_lookup_ext_cases(sigma, k, tail):
    """Per shape: planted windows with the ambiguous symbol at position 0 (each resolution in a slot of its own), at k - 1 (one slot
    wherever the shift is at least a symbol wide) and, for amino acids k = 4, 5, 6, at the position whose 5 bits straddle the shift (X:
    more than one slot, fewer than 20); at every position a resolution that is a key, one in an empty slot, and where a slot holds more
    than a code one after its slot's last key and one before its first key, with `tail` one above the database's last key; R = 2, 3, 4
    (DNA) and 2, 20 (amino acids).  The oracle finds a planted window alone exactly when a resolution of it is a key."""
    c = xc.lookup_ext_case(sigma, k, tail)
    keys, table, shift = xc.lookup_table(c)
    bits = po.ALPHABET[sigma][1]
    assert shift == {(4, 9): 2, (4, 12): 8, (4, 13): 10, (4, 15): 14, (4, 16): 16, (20, 3): 0, (20, 4): 4, (20, 5): 9, (20, 6): 14}[(sigma, k)]
    positions = xc.lookup_positions(sigma, k)
    assert positions["first"] == 0 and positions["last"] == k - 1
    assert positions.get("straddle") == {(20, 4): 3, (20, 5): 3, (20, 6): 3}.get((sigma, k))
    if "straddle" in positions:
        low = bits * (k - 1 - positions["straddle"])
        assert low < shift < low + bits
    need = {"key", "empty_slot"} | ({"after_last", "before_first"} if shift else set()) | ({"above_last"} if tail else set())
    want = c.expected(7, True, "given")
    kinds = {p: {} for p in positions}
    sizes = set()
    for i, (pname, kind, letter, w) in enumerate(c.planted):
        pos = positions[pname]
        assert c.queries[i] == w and w[pos] == letter and len(w) == k and sum(ch in xo.AMBIGUOUS[sigma] for ch in w) == 1
        codes = xc._codes(w, sigma)
        sizes.add(len(codes))
        got = [xc.resolution_kind(keys, table, shift, code) for code in codes]
        assert kind in got, (pname, kind, w, got)
        for g in got:
            kinds[pname][g] = kinds[pname].get(g, 0) + 1
        slots = {code >> shift for code in codes}
        if pname == "first":
            assert len(slots) == len(codes)                              # another slot than its siblings
        elif pname == "last" and shift >= bits:
            assert len(slots) == 1                                       # neighbours inside one slot's search
        elif pname == "straddle" and letter == "X":
            assert 1 < len(slots) < 20
        assert (want[i]["n_kmers"], want[i]["n_ambiguous"], want[i]["n_found"]) == (1, 1, int("key" in got)), (i, w)
    for pname in positions:
        assert need <= set(kinds[pname]), (pname, kinds[pname])
    assert sizes == ({2, 3, 4} if sigma == 4 else {2, 20})
    # the runs: ambiguous windows in later tiles, between found exact windows
    runs = range(len(c.planted), len(c.queries))
    assert all(want[i]["n_found"] >= 2 and want[i]["n_ambiguous"] >= 1 for i in runs if len(c.queries[i]) > 3 * k)
    assert any(st >= 64 and len(codes) > 1 for i in runs for st, codes in xo.windows(c.queries[i], sigma, k))
    if (sigma, k) == (4, 16):
        top_is_key = 0xFFFFFFFF in set(keys.tolist())
        assert top_is_key == (not tail)
        at = {q: i for i, q in enumerate(c.queries)}
        for q in ("T" * 15 + "N", "N" + "T" * 15):
            codes = xc._codes(q, 4)
            assert codes[-1] == 0xFFFFFFFF and xc.resolution_kind(keys, table, shift, codes[-1]) == ("above_last" if tail else "key")
            assert want[at[q]]["n_found"] == int(any(code in set(keys.tolist()) for code in codes))
    note(f"lookup_ext sigma {sigma} k {k}{' tail' if tail else ''}: shift {shift}, {len(c.planted)} planted windows, {len(c.queries)} queries; "
         f"resolution kinds by position {kinds}; windows found {sum(w['n_found'] for w in want)} of {sum(w['n_kmers'] for w in want)}, "
         f"{sum(w['n_ambiguous'] for w in want)} ambiguous")


# ---- 1b. table bounds -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("top", [4095, 4096, 63, 64])
def test_bound_ext_cases_name_the_last_branch_under_ambiguous_windows(top):
    c = xc.bound_ext_case(top)
    assert c.db is pc.bound_case(top).db and c.view.n_branches == top + 1
    letters, places = set(), set()
    for w in c.windows:
        amb = [i for i, ch in enumerate(w) if ch in xo.AMBIGUOUS[4]]
        assert len(amb) == 1
        letters.add(w[amb[0]]); places.add(amb[0])
        named = set()
        for code in xc._codes(w, 4):
            e = c.view.entries(code)
            named |= set() if e is None else set(e[0].tolist())
        assert top in named, w
    assert places == set(range(8)) and {len(xo.AMBIGUOUS[4][ch]) for ch in letters} == {2, 3, 4}
    for strands in ("given", "both"):
        want = c.expected(7, True, strands)
        best7 = [q for q, w in enumerate(want) if top in [p[0] for p in w["placements"]]]
        assert len(best7) >= 3 and all(w["n_ambiguous"] >= 1 for w in want)
    note(f"bound_ext top = {top}: {len(c.windows)} ambiguous windows name branch {top}; it is in the best 7 of queries {best7}; "
         f"most branches a query scores: {max(w['n_branches'] for w in want)}")


# ---- 1c. the long query -----------------------------------------------------------------------------------------------------------------

def test_long_ext_case_flips_the_strand():
    c = xc.long_ext_case()
    s, r = c.queries
    assert len(s) == 70000 and r == xo.revcomp(s) and xo.revcomp(r) == s
    amb = np.array([i for i, ch in enumerate(s) if ch in xo.AMBIGUOUS[4]])
    gaps = np.diff(amb)
    invalid = [i for i, ch in enumerate(s) if ch in xc.LONG_EXT_INVALID]
    assert 1300 <= len(amb) <= 1800 and (gaps < K).sum() >= 15 and np.median(gaps) in range(40, 61) and amb.max() > 69900
    assert 14 <= len(invalid) <= 24 and set(s) <= set("ACGT") | set(xo.AMBIGUOUS[4]) | set(xc.LONG_EXT_INVALID)
    a, b = c.expected(7, True, "both")
    assert (a["strand"], b["strand"]) == (0, 1)
    assert str({**a, "strand": None}) == str({**b, "strand": None})     # everything else equal
    assert a["n_ambiguous"] > 9000 and a["n_found"] > 8000 and a["n_branches"] == 60 and a["n_kmers"] > 69000
    given = c.expected(7, True, "given")
    assert given[0]["placements"][0][1] == a["placements"][0][1] and float(given[1]["placements"][0][1]) < float(a["placements"][0][1])
    note(f"long_ext: {len(s)} symbols, {len(amb)} ambiguity codes ({int((gaps < K).sum())} fewer than k after another), {len(invalid)} invalid bytes; "
         f"W = {a['n_kmers']}, {a['n_ambiguous']} ambiguous windows, {a['n_found']} found; best score {float(a['placements'][0][1])!r} against "
         f"{float(given[1]['placements'][0][1])!r} on the other strand; {math.ceil((len(s) - K + 1) / 64)} tiles a pass")


# ---- 1d. the inexact threshold --------------------------------------------------------------------------------------------------------

def fused_ext_changes(case, log_eps, strands):
    """pc.fused_penalty_changes over xo.accumulate (ambiguous windows expanded), on every strand placed: (changed, scored pairs)."""
    changed = pairs = 0
    eps = np.float32(log_eps)
    for q in case.queries:
        for seq in ([q, xo.revcomp(q)] if strands == "both" else [q]):
            W, _, _, S, Cn = xo.accumulate(case.view, seq, case.sigma, case.k, log_eps)
            hit = np.nonzero(Cn)[0]
            two = S[hit] + (W - Cn[hit]).astype(np.float32) * eps
            one = (S[hit].astype(np.float64) + (W - Cn[hit]).astype(np.float64) * np.float64(eps)).astype(np.float32)
            pairs += len(hit); changed += int((two.view(np.uint32) != one.view(np.uint32)).sum())
    return changed, pairs


@pytest.mark.parametrize("name", ["main_ext_case", "strand_case"])
def test_the_inexact_threshold_decides(name):
    c = xc.ALL_CASES[name]()
    for ambiguity, strands in xc.MODES[name]:
        a, b = c.expected(7, ambiguity, strands), xc.expected_ext_at(c, pc.EPS_INEXACT, 7, ambiguity, strands)
        bits = lambda w: [int(np.float32(p[1]).view(np.uint32)) for p in w["placements"]]
        differ = sum(bits(x) != bits(y) for x, y in zip(a, b))
        placed = sum(bool(x["placements"]) for x in a)
        assert differ >= 0.8 * placed and [x["n_kmers"] for x in a] == [y["n_kmers"] for y in b]
        if ambiguity:
            changed, pairs = fused_ext_changes(c, pc.EPS_INEXACT, strands)
            exact = fused_ext_changes(c, xc.LOG_EPS, strands)
            note(f"inexact threshold, {name} {strands}: {differ} of {placed} placed queries change score bits against -4.5; a fused penalty changes "
                 f"{changed} of {pairs} scored pairs (at -4.5: {exact[0]} of {exact[1]})")
            assert changed >= 0.05 * pairs and exact[0] == 0


# ---- 1e. alias bytes ----------------------------------------------------------------------------------------------------------------------

def test_alias_bytes_are_invalid():
    odd = xc.alias_bytes()
    low = {ord(ch) & 31: ch for ch in xc.ALIAS_LETTERS}
    assert len(odd) == 6 * 11 and [b for b in odd if b & 31 == ord("N") & 31] == [0x0E, 0x2E, 0x8E, 0xAE, 0xCE, 0xEE]
    c = xc.alias_case()
    text = "".join(c.queries)
    for b in odd + [0x00, 0x80, 0xFF]:
        ch = chr(b)
        assert ch in text and not (b < 128 and ch.isalpha())
        probe = "ACGTACG" + ch + "CGTACGTA"
        assert [st for st, _ in xo.windows(probe, 4, K)] == [8]                    # the one window without the byte
        if b & 31 in low:                                                         # the letter it aliases is expanded in its place
            assert len(xo.windows(probe.replace(ch, low[b & 31]), 4, K)) == 9
        assert xo.revcomp(ch) == ch
    for q in c.queries:
        assert len(q.upper()) == len(q) and len(q.encode("latin-1")) == len(q)
    want = c.expected(7, True, "both")
    n = len(c.queries)
    real, fake = want[n - 5], want[n - 4]
    assert real["n_ambiguous"] == 2 * K and fake["n_ambiguous"] == 0 and fake["n_kmers"] == real["n_kmers"] - 2 * K
    assert want[n - 7]["n_kmers"] == 0 and want[n - 6]["n_kmers"] == 1            # only such bytes; 7 valid symbols between two of them
    # U is T: the same windows, and its complement is A
    u = c.queries[n - 3]
    assert "U" in u and "T" not in u and xo.windows(u, 4, K) == xo.windows(u.replace("U", "T"), 4, K)
    assert xo.revcomp("Uu") == "aA" and want[n - 3]["strand"] == 0 and want[n - 1]["strand"] == 1 and want[n - 1]["n_found"] == want[n - 3]["n_found"]
    assert "u" in c.queries[n - 2] and want[n - 2]["n_ambiguous"] == K
    note(f"alias: {len(odd)} bytes alias an ambiguous letter in their low five bits; {n} queries, {sum(w['n_found'] for w in want)} windows found, "
         f"strands {[w['strand'] for w in want]}")


# ---- 1f. keep = 1 and a strand tie ----------------------------------------------------------------------------------------------------

def test_keep_one_and_the_strand_tie():
    s = xc.strand_case()
    for ambiguity in (False, True):
        one, seven = s.expected(1, ambiguity, "both"), s.expected(7, ambiguity, "both")
        assert {w["strand"] for w in one} == {0, 1} and all(len(w["placements"]) <= 1 for w in one)
        assert [w["strand"] for w in one] == [w["strand"] for w in seven] and any(w["strand"] == 0 and w["n_branches"] > 1 for w in one)
    c = xc.tie_case()
    T, U = c.T, c.U
    assert len(xo.windows(T, 4, K)) == len(xo.windows(U, 4, K)) == xc.TIE_WINDOWS
    assert c.queries[0] == T + "-" + xo.revcomp(U) and c.queries[1] == xo.revcomp(T) + "-" + U and xo.revcomp(c.queries[0]) == U + "-" + xo.revcomp(T)
    for ambiguity in (False, True):
        want = c.expected(7, ambiguity, "both")
        for q, first, other in ((0, 3, 9), (1, 9, 3)):
            given = xo.place_strand(c.view, c.queries[q], 4, K, xc.LOG_EPS, 7, ambiguity)
            rev = xo.place_strand(c.view, xo.revcomp(c.queries[q]), 4, K, xc.LOG_EPS, 7, ambiguity)
            g, r = given["placements"][0], rev["placements"][0]
            assert (g[0], r[0]) == (first, other) and np.float32(g[1]).view(np.uint32) == np.float32(r[1]).view(np.uint32)
            assert float(g[1]) * 2 == int(float(g[1]) * 2)                      # a multiple of -0.5 (penalty -4.5 x 24 included): exact
            assert given["n_kmers"] == rev["n_kmers"] == 2 * xc.TIE_WINDOWS and g[2] == r[2] == xc.TIE_WINDOWS
            assert (want[q]["strand"], want[q]["placements"][0][0]) == (0, first)
        assert [w["strand"] for w in want[2:]] == [0, 1, 0, 1]                   # no tie: the longer side wins
    note(f"tie: T and U of {xc.TIE_WINDOWS} windows, score {float(g[1])!r} on both strands; the given strand's branch is kept")


# ---- reuse and budgets ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [8192, 1024, 512])
def test_later_queries_of_a_workgroup_follow_ambiguous_and_reverse_passes(G):
    c = xc.reuse_ext_pool()
    draw = xc.reuse_ext_draw3(G)
    once = c.expected(7, True, "both")
    assert len(draw) == 2 * G + G // 2 + 37
    before = [once[int(draw[i - G])] for i in range(G, len(draw))]
    amb = sum(w["n_ambiguous"] > 0 for w in before)
    rev = sum(w["strand"] == 1 for w in before)
    note(f"reuse_ext G = {G}: N = {len(draw)}; {amb} of {len(before)} later queries follow one with ambiguous windows, {rev} one whose reverse strand won")
    assert amb > len(before) // 2 and rev > len(before) // 16
    before = [once[int(draw[i - G // 2])] for i in range(G // 2, len(draw))]     # batches G / 2 wide: queries i - G / 2 and i share a workgroup
    assert sum(w["n_ambiguous"] > 0 for w in before) > len(before) // 2


class NoMem(Exception):
    pass


def simulate_budget(lengths, room, b_pad, max_grid, global_tables, per_query, most=1 << 18, caps=None):
    """The batch rule of ipkgpu_db_place_opts (ipk_amd/csrc/db_place.hpp) with ambiguity on, restated over byte counts: `room` is what
    the budget leaves above what the context held before the call; -> [(queries, table slices, window-table slices, launch width)] per
    batch and the peak held above the start.  NoMem where the engine would refuse."""
    cap = dict(seq=0, off=0, out=0, tables=0, amb=0) if caps is None else dict(caps)
    used = [0]                                                                   # (what `caps` hold is part of what was held before)
    peak = [0]
    free = lambda: room - used[0]
    grows = lambda name, need: 0 if need <= cap[name] else need + need // 16 - cap[name]

    def ensure(name, need):
        if cap[name] >= need and cap[name]:
            return
        regrow = cap[name] > 0
        used[0] -= cap[name]
        need = max(need, 16)
        want = need + need // 16 if regrow else need
        if want > free():
            want = need
        if want > free():
            raise NoMem(name)
        used[0] += want; cap[name] = want
        peak[0] = max(peak[0], used[0])
    off = np.concatenate([[0], np.cumsum(lengths)])
    slice_bytes, amb_bytes = 12 * b_pad, 16 * b_pad
    slices = amb_slices = 0
    out, q0, n_q = [], 0, len(lengths)
    while q0 < n_q:
        half = free() // 2
        q1 = q0 + 1
        while q1 < n_q and q1 - q0 < most:
            nbytes, n = int(off[q1 + 1] - off[q0]), q1 + 1 - q0
            if grows("seq", nbytes + 16) + grows("off", (n + 1) * 8) + grows("out", n * per_query + 64) + grows("amb", min(n, max_grid) * amb_bytes) > half:
                break
            q1 += 1
        nq = q1 - q0
        ensure("seq", int(off[q1] - off[q0]) + 16); ensure("off", (nq + 1) * 8); ensure("out", nq * per_query + 64)
        grid = min(nq, max_grid)
        if global_tables and grid > slices:
            want = grid
            if want * slice_bytes > cap["tables"]:
                want = max(1, min(want, (free() // 2 + cap["tables"]) // slice_bytes))
            ensure("tables", want * slice_bytes)
            slices = want
        if grid > amb_slices:
            want = grid
            if want * amb_bytes > cap["amb"]:
                want = max(1, min(want, (free() // 2 + cap["amb"]) // amb_bytes))
            ensure("amb", want * amb_bytes)
            amb_slices = want
        out.append((nq, slices, amb_slices, min(grid, slices, amb_slices) if global_tables else min(grid, amb_slices)))
        q0 = q1
    return out, peak[0]


def test_budget_ext_arithmetic():
    """test_budgeted_slices_ext: B = 70 001, b_pad = 70 016, a slice of S, C and the touched list 840 192 bytes, one of P, c and the
    window's list 1 120 256 bytes; 64 MB above the database.  The window tables join the batch sizing: a batch grows while their growth
    (a sixteenth on top) stays within half of what is free, 32 MiB: 28 queries.  Then the tables are clipped one after the other against
    half of what is free at their turn: 28 slices of S / C / touched (22.4 MiB; half of 64 MiB holds 39), then half of the 41.6 MiB left holds
    19 slices of P / c (20.3 MiB): the first launch is 19 workgroups for 28 queries.  Later batches grow both blocks; no launch is as
    wide as the 200 queries and the peak stays within the budget."""
    c = xc.big_branch_ext_case()
    b_pad = (c.view.n_branches + 63) & ~63
    assert b_pad == 70016
    lengths = [len(c.queries[d]) for d in xc.big_branch_ext_draw()]
    batches, peak = simulate_budget(lengths, 64 << 20, b_pad, 256 * 4, True, xc.PLACE_EXT_QUERY_BYTES_7 + 0)
    note(f"budget_ext slices: a slice is {12 * b_pad} + {16 * b_pad} bytes; batches (queries, S/C slices, P/c slices, launch width): {batches}; "
         f"peak {peak} of {64 << 20}")
    assert batches[0] == (28, 28, 19, 19)
    assert sum(b[0] for b in batches) == 200 and all(b[3] < b[0] or b[0] < 200 for b in batches) and max(b[3] for b in batches) < 200
    assert peak <= 64 << 20 and peak < 200 * 28 * b_pad


@pytest.mark.parametrize("path", ["lds", "global"])
def test_budgeted_ext_batches_cannot_be_one(path):
    """The 1500 queries of budget_ext_draw() under BUDGET_ROOM: sequences, offsets and results alone are more than the room, and the
    window tables (5120 bytes a workgroup at b_pad = 320) take most of each batch's half: the rule gives tens of batches and refuses
    none (the workspaces hold what a one-query call before left: nothing to speak of)."""
    c, draw = xc.reuse_ext_pool(), xc.budget_ext_draw()
    lengths = [len(c.queries[d]) for d in draw]
    whole = int(np.sum(lengths)) + len(draw) * xc.PLACE_EXT_QUERY_BYTES_7
    assert xc.PLACE_EXT_QUERY_BYTES_7 == 168 and len(draw) == 1500 and whole > pc.BUDGET_ROOM and c.view.n_branches == 300
    assert len(set(draw.tolist())) == len(c.queries)
    glob = path == "global"
    first = dict(seq=len(c.queries[draw[0]]) + 16, off=16, out=xc.PLACE_EXT_QUERY_BYTES_7 + 64, tables=12 * 320 if glob else 0, amb=16 * 320)
    batches, peak = simulate_budget(lengths, pc.BUDGET_ROOM, 320, 256 * (4 if glob else 32), glob, xc.PLACE_EXT_QUERY_BYTES_7, caps=first)
    note(f"budget_ext batches ({path}): {whole} bytes of sequences and results against a room of {pc.BUDGET_ROOM}; the rule gives {len(batches)} batches, "
         f"the first {batches[:3]}, the widest launch {max(b[3] for b in batches)}, peak {peak}")
    assert len(batches) >= 3 and peak <= pc.BUDGET_ROOM and sum(b[0] for b in batches) == 1500


# ---- the rounding margin over the new cases ------------------------------------------------------------------------------------------------

MARGIN_CASES = {n: f for n, f in xc.NEW_CASES.items() if n != "ladder_case"}      # (the ladder is the margin's own measurement)
# main_ext_case keeps its seed, and under the inexact threshold ONE of its contributions (query 9 and its lower-case copy, window 71: H
# with three keys, a branch that one of them names with x = -0.000791...) lies 2^-44.4 from a midpoint: inside the margin, outside the
# error bound of 2^-47.  It is named here, checked by itself against 2^-45, and the ladder's rung -45 measures what the device does there.
CLOSE_AT_INEXACT = {((float(np.float32(-0.0007914228481240571)),), 3)}


@pytest.mark.parametrize("log_eps", [xc.LOG_EPS, float(pc.EPS_INEXACT)], ids=["exact", "inexact"])
def test_rounding_margin_of_the_new_cases(log_eps):
    """The same 2^-44 and the same 60-digit arithmetic as tests/test_place_ext_inputs.py, over the cases added here and -- at the
    inexact threshold -- over the earlier cases placed with it."""
    rounding_margin(MARGIN_CASES, xc.NEW_MODES, log_eps, 1000)
    if log_eps != xc.LOG_EPS:
        old = {n: xc.ALL_CASES[n] for n in ("main_ext_case", "strand_case")}
        rounding_margin(old, xc.MODES, log_eps, 1000, but=CLOSE_AT_INEXACT)
        for xs, R in CLOSE_AT_INEXACT:
            y, right, d = xc.exact_contribution(xs, R, log_eps)
            host = np.float32(math.log10((10.0 ** xs[0] + float(R - 1) * 10.0 ** log_eps) / float(R)))
            note(f"main_ext_case at the inexact threshold: x = {xs[0]!r}, R = {R}: d = 2^{math.log2(float(d)):.2f}")
            assert 2.0 ** -45 <= float(d) < 2.0 ** -44 and host.view(np.uint32) == right.view(np.uint32)


# ---- the rounding ladder --------------------------------------------------------------------------------------------------------------------

def test_ladder_distances():
    """Every recorded x again at 60 digits: 2^rung <= d < 2^(rung + 1); rungs -36 .. -45 are all there for both R, eight inputs each down
    to -44; the expected bits are the 60-digit value's.  Where the binary64 oracle rounds the other way is counted, not asserted."""
    assert sorted(xc.LADDER) == [2, 4]
    off = 0
    for R, rungs in xc.LADDER.items():
        assert set(range(-45, -35)) <= set(rungs) and min(rungs) <= -48
        for rung, xs in rungs.items():
            assert 1 <= len(xs) <= 8 and len(set(xs)) == len(xs) and (len(xs) == 8 or rung < xc.LADDER_ASSERTED_FROM)
            for b in xs:
                x = np.uint32(b).view(np.float32)
                assert -6.0 <= float(x) < -1.0
                y, right, d = xc.exact_contribution((float(x),), R, xc.LOG_EPS)
                assert 2.0 ** rung <= float(d) < 2.0 ** (rung + 1), (R, rung, hex(b), math.log2(float(d)))
                host = np.float32(math.log10((10.0 ** float(x) + float(R - 1) * 10.0 ** -4.5) / float(R)))
                off += int(host.view(np.uint32) != right.view(np.uint32))
    c = xc.ladder_case()
    inputs = xc.ladder_inputs()
    assert len(inputs) == len(c.queries) == len(set(c.queries)) == sum(len(v) for r in xc.LADDER.values() for v in r.values())
    want = c.expected(1, True, "given")
    for i, (R, rung, x) in enumerate(inputs):
        assert len(xc._codes(c.queries[i], 4)) == R and (want[i]["n_kmers"], want[i]["n_found"], want[i]["n_branches"]) == (1, 1, 1)
        assert want[i]["placements"][0][0] == i % 50 and want[i]["placements"][0][2] == 1
        if rung >= xc.LADDER_ASSERTED_FROM:                                      # the binary64 oracle is right down to the margin
            assert int(np.float32(want[i]["placements"][0][1]).view(np.uint32)) == int(c.want_bits[i])
    note(f"ladder: {len(inputs)} inputs, rungs {sorted(xc.LADDER[2], reverse=True)} (R = 2) and {sorted(xc.LADDER[4], reverse=True)} (R = 4); "
         f"the host's binary64 arithmetic rounds {off} of them the other way")
