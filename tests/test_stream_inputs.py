"""CPU suite: the inputs of tests/test_gpu_stream.py.  The theorem the streamed load rests on, checked on the host -- the oracle's
placements on R(D, K) equal those on D in every field -- and the assertions that the streamed file reaches the hard spots of the window
cuts at the test's window size."""
import numpy as np
import pytest

from tests import db_files as F
from tests import place_cases as pc
from tests import place_ext_cases as xc
from tests import place_ext_oracle as xo
from tests import stream_cases as T

KEEP = 7
THEOREM = {
    "main_case": (pc.main_case, [(False, "given")]),
    "aa_case": (pc.aa_case, [(False, "given")]),
    "k2_case": (pc.k2_case, [(False, "given")]),
    "main_ext_case": (xc.main_ext_case, [(True, "both")]),
    "aa_ext_case": (lambda: xc.aa_ext_case(3), [(True, "given")]),
    "strand_case": (xc.strand_case, [(True, "both"), (False, "both")]),
    "alias_case": (xc.alias_case, [(True, "both")]),
}


def as_dict(case):
    keys, off, br, sc = case.db
    n = len(keys)
    return dict(keys=np.asarray(keys, np.uint32), off=np.asarray(off, np.uint64), br=np.asarray(br, np.uint32), sc=np.asarray(sc, np.float32),
                fv=np.zeros(n, np.float32), order=np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("name", sorted(THEOREM))
def test_placements_on_the_restriction_equal_those_on_the_database(name):
    make, modes = THEOREM[name]
    case = make()
    for ambiguity, strands in modes:
        codes = T.kmer_codes(case.queries, case.sigma, case.k, ambiguity, strands)
        r = T.restrict(as_dict(case), codes, positioned=False)
        if name == "k2_case":
            assert len(r["keys"]) == len(case.db[0]) == 16, "the 16 codes of k = 2: a set that holds every key"
        elif name == "strand_case":
            assert 0 < len(r["keys"]) <= len(case.db[0])                    # (its queries and their reverse complements name every key)
        else:
            assert 0 < len(r["keys"]) < len(case.db[0]), "K strictly between empty and all of D's keys"
        whole = xo.place(case.view, case.queries, case.sigma, case.k, pc.LOG_EPS, KEEP, ambiguity, strands)
        view = T.view_of(r)
        view.n_branches = case.view.n_branches                               # (S and C are sized by D's branch count in both)
        part = xo.place(view, case.queries, case.sigma, case.k, pc.LOG_EPS, KEEP, ambiguity, strands)
        assert len(whole) == len(part)
        for a, b in zip(whole, part):
            assert {x: a[x] for x in ("n_kmers", "n_found", "n_branches", "strand", "n_ambiguous")} == \
                   {x: b[x] for x in ("n_kmers", "n_found", "n_branches", "strand", "n_ambiguous")}
            assert len(a["placements"]) == len(b["placements"])
            for p, q in zip(a["placements"], b["placements"]):
                assert (p[0], np.float32(p[1]).view(np.uint32), p[2], p[3]) == (q[0], np.float32(q[1]).view(np.uint32), q[2], q[3])


def test_set_restatement_on_small_strings():
    assert T.kmer_codes(["ACGTA"], 4, 4) == {0b00011011, 0b01101100}
    assert T.kmer_codes(["ACGN"], 4, 4) == set()
    assert T.kmer_codes(["ACGN"], 4, 4, ambiguity=True) == {0b00011000 | s for s in range(4)}
    assert T.kmer_codes(["ANGN"], 4, 4, ambiguity=True) == set()             # two ambiguous symbols: nothing
    assert T.kmer_codes(["AAAC"], 4, 4, strands="both") == {0b00000001, 0b10111111}
    assert T.kmer_codes(["acgu"], 4, 4) == {0b00011011}
    w = T.words_of({0, 31, 32, 255}, 4, 4)
    assert w.tolist() == [0x80000001, 1, 0, 0, 0, 0, 0, 0x80000000]
    assert T.n_words(4, 2) == 2 and T.n_words(4, 16) == 1 << 27 and T.n_words(20, 6) == 1 << 25
    assert T.kmer_codes(["V" * 6], 20, 6) == {int("10011" * 6, 2)}           # the all-V code of the amino acids


@pytest.mark.parametrize("positioned", [False, True])
def test_the_streamed_file_reaches_the_hard_spots(positioned):
    db, want = T.stream_db(), T.stream_wanted(positioned)
    file_keys = db["keys"][db["order"]].tolist()
    sizes = T.record_sizes(db, positioned)
    cap = T.window_cap(positioned)
    wins = T.windows_of(sizes, cap)
    assert sum(sizes) == F.record_starts(db, positioned)[1] and wins[0][0] == 0 and wins[-1][1] == 200
    assert all(a[1] == b[0] for a, b in zip(wins, wins[1:])) and len(wins) > 20
    flags = [k in want for k in file_keys]
    per_window = [flags[a:b] for a, b in wins]
    assert any(not any(w) for w in per_window), "a window with no wanted record"
    assert any(all(w) and len(w) > 1 for w in per_window), "a window whose records are all wanted"
    assert flags[0] and flags[-1], "the file's first and last records"
    a, b = wins[0]
    assert sum(sizes[a:b]) == cap and flags[b - 1], "a wanted record that ends exactly at a window's end"
    assert max(sizes) > cap and flags[int(np.argmax(sizes))], "a wanted record longer than the window"
    assert any(sum(sizes[a:b]) > cap for a, b in wins) and sum(s > T.CHUNK for s in sizes) > 10, "records longer than a load chunk"
    assert {31, 32, 4 ** T.K4 - 1} <= want and {31, 32, 4 ** T.K4 - 1, T.OUTSIDE} <= set(file_keys)
    assert T.OUTSIDE not in want and T.OUTSIDE >> 5 == T.n_words(4, T.K4), "key 4^k: one word past the bitmap"
    assert T.ABSENT in want and T.ABSENT not in file_keys
    kept = len(T.restrict(db, want)["keys"])
    assert 0 < kept < 200 and kept == len(want) - 1
    assert T.kmer_codes(T.stream_queries(positioned), 4, T.K4) == want
    # the other two window sizes: one window, and cuts in front of and behind the longest record
    assert len(T.windows_of(sizes, sum(sizes))) == 1
    longest = T.windows_of(sizes, T.window_cap(positioned, "longest"))
    assert 1 < len(longest) < len(wins)


def test_restriction_follows_the_selection_rules():
    db, want = T.stream_db(), T.stream_wanted(False)
    r = T.restrict(db, want)
    assert np.array_equal(r["keys"], np.array(sorted(want - {T.ABSENT}), np.uint32))
    assert np.array_equal(r["keys"][r["order"]], np.array([k for k in db["keys"][db["order"]].tolist() if k in want], np.uint32))
    j = int(np.searchsorted(db["keys"], 31))
    i = int(np.searchsorted(r["keys"], 31))
    assert np.array_equal(r["br"][int(r["off"][i]):int(r["off"][i + 1])], db["br"][int(db["off"][j]):int(db["off"][j + 1])])
    assert r["fv"][i].view(np.uint32) == db["fv"][j].view(np.uint32)
    everything = T.restrict(db, set(range(4 ** T.K4 + 1)))
    assert all(np.array_equal(everything[x], db[x]) for x in ("keys", "off", "br", "sc", "pos", "fv", "order"))
    assert len(T.restrict(db, set())["keys"]) == 0
