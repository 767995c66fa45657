"""GPU suite: Engine.diff_dbs (ipkgpu_db_diff) -- the reference's ipkdiff comparison on the device.  Expected counts and records come
from `restate` below: a dictionary-based restatement of the rules in plain Python over the host arrays (include/ipkgpu.h,
tools/src/diff.cpp:210-295 of the reference)."""
import copy

import numpy as np
import pytest

import ipk_amd
from tests import db_files as F

pytestmark = pytest.mark.gpu

# list lengths: the unpack / diff kernels' edges twice over (one list to drop a branch from, one to add one to), and two lists longer
# than the LDS chunk of the diff's general path
COUNTS = F.EDGE_COUNTS + [1, 64, 65, 1500]
N_KEYS = 300


def as_lists(db):
    """{key: [[branch, score, position], ...]} of a database in arrays"""
    out = {}
    for i, key in enumerate(db["keys"]):
        a, b = int(db["off"][i]), int(db["off"][i + 1])
        out[int(key)] = [[int(db["br"][j]), np.float32(db["sc"][j]), int(db["pos"][j])] for j in range(a, b)]
    return out


def as_arrays(lists, seed=3):
    keys = np.array(sorted(lists), np.uint32)
    counts = [len(lists[int(k)]) for k in keys]
    flat = [e for k in keys for e in lists[int(k)]]
    db = F.synthetic(keys=keys, counts=counts, seed=seed)
    db["br"] = np.array([e[0] for e in flat], np.uint32)
    db["sc"] = np.array([e[1] for e in flat], np.float32)
    db["pos"] = np.array([e[2] for e in flat], np.uint32)
    return db


def restate(A, B, eps, positions):
    """(counts, records) of A against B by the rules: keys ascending; an entry is matched with the first entry of the same branch in
    the other list; scores match iff float |a - b|, as a double, < eps (eps 0: equal bits); records = A's entries in A's order that
    are unmatched or differ, then B's unmatched ones in B's order."""
    c = dict(keys_a=len(A), keys_b=len(B), keys_only_a=0, keys_only_b=0, entries_a=sum(map(len, A.values())), entries_b=sum(map(len, B.values())),
             entries_only_a=0, entries_only_b=0, scores_differ=0, positions_differ=0)
    dmax = np.float32(0)
    rec = []
    nan = np.float32(np.nan)
    for key in sorted(set(A) | set(B)):
        if key not in B:
            c["keys_only_a"] += 1
            c["entries_only_a"] += len(A[key])
            rec += [(key, br, sc, nan) for br, sc, _ in A[key]]
            continue
        if key not in A:
            c["keys_only_b"] += 1
            c["entries_only_b"] += len(B[key])
            rec += [(key, br, nan, sc) for br, sc, _ in B[key]]
            continue
        first_a, first_b = {}, {}
        for e in A[key]:
            first_a.setdefault(e[0], e)
        for e in B[key]:
            first_b.setdefault(e[0], e)
        for br, sc, pos in A[key]:
            other = first_b.get(br)
            if other is None:
                c["entries_only_a"] += 1
                rec.append((key, br, sc, nan))
                continue
            d = np.abs(np.float32(sc) - np.float32(other[1]))                     # float arithmetic
            assert d.dtype == np.float32
            dmax = max(dmax, d)
            same = (np.float32(sc).view(np.uint32) == np.float32(other[1]).view(np.uint32)) if eps == 0 else float(d) < eps
            if not same:
                c["scores_differ"] += 1
                rec.append((key, br, sc, other[1]))
            elif positions and pos != other[2]:
                c["positions_differ"] += 1
        for br, sc, _ in B[key]:
            if br not in first_a:
                c["entries_only_b"] += 1
                rec.append((key, br, nan, sc))
    c["max_abs_diff"] = float(dmax)
    return c, np.array(rec, dtype=ipk_amd.engine.DIFF_RECORD) if rec else np.zeros(0, ipk_amd.engine.DIFF_RECORD)


def same_records(got, want):
    assert len(got) == len(want)
    assert np.array_equal(got["key"], want["key"]) and np.array_equal(got["branch"], want["branch"])
    for f in ("a_score", "b_score"):
        assert np.array_equal(np.isnan(got[f]), np.isnan(want[f]))
        ok = ~np.isnan(want[f])
        assert np.array_equal(got[f][ok].view(np.uint32), want[f][ok].view(np.uint32))


@pytest.fixture(scope="module")
def base(engine, tmp_path_factory):
    rng = np.random.default_rng(21)
    keys = np.sort(rng.choice(np.arange(10, 1000), size=N_KEYS, replace=False))      # DNA k = 5; room in front of and behind the keys
    counts = rng.integers(1, 9, size=N_KEYS)
    at = rng.permutation(np.arange(1, N_KEYS - 1))[:len(COUNTS)]                     # (the first and the last key stay short lists)
    counts[at] = COUNTS
    db = F.synthetic(keys=keys, counts=counts, seed=22)
    lists = as_lists(db)
    by_len = {}
    for i, n in zip(at, COUNTS):
        by_len.setdefault(n, []).append(int(keys[i]))
    d = tmp_path_factory.mktemp("diff")
    loaded = {pos: engine.load_db(F.write(d / f"a{int(pos)}.ipk", db, positioned=pos)) for pos in (True, False)}
    assert ipk_amd.load_library().ipkgpu_db_diff_chunk() == 1024 and 1500 > 1024 and 3000 > 2 * 1024
    yield dict(lists=lists, by_len=by_len, db=loaded, dir=d)
    for x in loaded.values():
        x.free()


def p_first_key(B, base):
    del B[min(B)]


def p_last_key(B, base):
    del B[max(B)]


def p_added_keys(B, base):
    between = next(k for k in range(min(B) + 1, max(B)) if k not in B)
    B[3] = [[7, np.float32(-1.5), 9], [2, np.float32(-2.5), 11]]
    B[between] = [[b, np.float32(-0.001 * b), b] for b in range(70)]
    B[1010] = [[5, np.float32(-3.0), 0]]


def p_branch_dropped(B, base):
    for n in (1, 64, 65, 3000):
        lst = B[base["by_len"][n][0]]
        del lst[len(lst) // 2]


def p_branch_added(B, base):
    for n, which, where in ((1, 1, 0), (64, 1, 64), (65, 1, 30), (1500, 0, 1100)):
        B[base["by_len"][n][which]].insert(where, [5000 + n, np.float32(-4.25), 17])  # (the base's branches are below 4000)


def p_scores_moved(B, base):
    keys = sorted(B)
    B[keys[5]][0][1] = np.float32(B[keys[5]][0][1] + np.float32(0.005))               # inside eps = 1e-2
    B[keys[9]][-1][1] = np.float32(B[keys[9]][-1][1] - np.float32(0.02))              # beyond it
    lst = B[base["by_len"][3000][0]]
    lst[2500][1] = np.float32(lst[2500][1] + np.float32(0.5))


def p_reordered(B, base):
    B[base["by_len"][257][0]].reverse()                                               # no difference: the order carries no meaning
    lst = B[base["by_len"][1500][0]]
    lst.append(lst.pop(0))
    lst = B[base["by_len"][3000][0]]
    lst[:] = lst[2000:] + lst[:2000]


def p_positions(B, base):
    keys = sorted(B)
    B[keys[20]][0][2] ^= 1
    B[base["by_len"][256][0]][255][2] ^= 0x8000
    B[base["by_len"][1500][0]].reverse()                                              # (general path) ...
    B[base["by_len"][1500][0]][7][2] ^= 2                                             # ... one position changed there too


PERTURB = dict(first_key=p_first_key, last_key=p_last_key, added_keys=p_added_keys, branch_dropped=p_branch_dropped, branch_added=p_branch_added,
               scores_moved=p_scores_moved, reordered=p_reordered, positions=p_positions)


def perturbed(base, names):
    B = copy.deepcopy(base["lists"])
    for n in names:
        PERTURB[n](B, base)
    return B


def check(engine, base, B, eps, tag, b_positioned=True, max_records=(0, 5, None)):
    path = F.write(base["dir"] / f"{tag}.ipk", as_arrays(B), positioned=b_positioned)
    db_b = engine.load_db(path)
    try:
        want_c, want_r = restate(base["lists"], B, eps, b_positioned)
        for m in max_records:
            m = len(want_r) + 10 if m is None else m
            fwd, got_r = engine.diff_dbs(base["db"][True], db_b, eps=eps, max_records=m)
            assert fwd == want_c, (tag, m)
            assert np.float32(fwd["max_abs_diff"]).view(np.uint32) == np.float32(want_c["max_abs_diff"]).view(np.uint32)
            same_records(got_r, want_r[:m])
        # and the other way round: B against A
        want_c, want_r = restate(B, base["lists"], eps, b_positioned)
        got_c, got_r = engine.diff_dbs(db_b, base["db"][True], eps=eps, max_records=len(want_r) + 1)
        assert got_c == want_c, (tag, "reversed")
        same_records(got_r, want_r)
        return fwd
    finally:
        db_b.free()


@pytest.mark.parametrize("name", list(PERTURB) + ["all"])
def test_perturbed_copies(engine, base, name):
    names = list(PERTURB) if name == "all" else [name]
    got = check(engine, base, perturbed(base, names), 1e-2, name)
    if name == "reordered":
        assert all(got[f] == 0 for f in ("keys_only_a", "keys_only_b", "entries_only_a", "entries_only_b", "scores_differ", "positions_differ"))
        assert got["max_abs_diff"] == 0.0
    if name == "scores_moved":
        assert got["scores_differ"] == 2 and 0.49 < got["max_abs_diff"] < 0.51
    if name == "positions":
        assert got["positions_differ"] == 3 and got["scores_differ"] == 0
    if name == "branch_dropped":
        assert got["entries_only_a"] == 4 and got["entries_only_b"] == 0
    if name == "branch_added":
        assert got["entries_only_b"] == 4 and got["entries_only_a"] == 0
    if name == "added_keys":
        assert got["keys_only_b"] == 3 and got["entries_only_b"] == 73


def test_positions_count_only_when_both_have_them(engine, base):
    got = check(engine, base, perturbed(base, ["positions", "scores_moved"]), 1e-2, "plain_b", b_positioned=False, max_records=(None,))
    assert got["positions_differ"] == 0 and got["scores_differ"] == 2


def test_exact_comparison(engine, base):
    B = copy.deepcopy(base["lists"])
    e = B[base["by_len"][65][0]][64]
    e[1] = (np.float32(e[1]).view(np.uint32) ^ np.uint32(1)).view(np.float32)          # the last bit of one score
    got = check(engine, base, B, 0.0, "one_bit")
    assert got["scores_differ"] == 1 and got["max_abs_diff"] > 0
    got = check(engine, base, B, 1e-2, "one_bit_eps", max_records=(None,))
    assert got["scores_differ"] == 0


def test_a_against_itself_and_against_nothing(engine, base):
    a = base["db"][True]
    n_entries = sum(map(len, base["lists"].values()))
    for other in (a, base["db"][False]):
        got, rec = engine.diff_dbs(a, other, eps=0.0, max_records=10)
        assert got == dict(keys_a=N_KEYS, keys_b=N_KEYS, keys_only_a=0, keys_only_b=0, entries_a=n_entries, entries_b=n_entries, entries_only_a=0,
                           entries_only_b=0, scores_differ=0, positions_differ=0, max_abs_diff=0.0)
        assert len(rec) == 0
    got = check(engine, base, {}, 1e-2, "empty", max_records=(0, 5, None))
    assert got["keys_only_a"] == N_KEYS and got["entries_only_a"] == n_entries and got["keys_b"] == 0


def test_bad_arguments(engine, base):
    with pytest.raises(ipk_amd.IpkGpuError):
        engine.diff_dbs(base["db"][True], base["db"][False], eps=-1.0)
