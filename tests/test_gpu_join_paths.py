"""GPU suite: the cases of tests/join_paths.py through Engine.join_dbs (ipkgpu_db_join) against tests/join_cases.restate bit for bit --
chains of three and four occurrences with ties, signed zeros, one-ulp steps, NaN and infinities in the wavefront kernel, the LDS kernel
at every padded size and the sorted pass; branches that share a slot of the branch table and none that is equal; keys at and above
2^31; the refusal of "join_route" = 2 on a list beyond a wavefront whose first run has no entries.  The cases' properties are checked
on the CPU (tests/test_join_paths_inputs.py)."""
import numpy as np
import pytest

import ipk_amd
from tests import join_cases as J
from tests import join_paths as P
from tests.test_gpu_db_join import join_on_route, same_join
from tests.test_gpu_db_load import same_as_arrays

pytestmark = pytest.mark.gpu

KINDS = [False, True]                                # plain, positioned


@pytest.fixture(scope="module")
def shard_files(tmp_path_factory):
    """(case name, positioned) -> the case's shard files, written once."""
    d = tmp_path_factory.mktemp("join_paths")
    made = {}

    def get(name, positioned):
        if (name, positioned) not in made:
            made[name, positioned] = J.write_shards(d, P.case(name), positioned)
        return made[name, positioned]
    return get


def free_all(dbs):
    for d in dbs:
        d.free()


def arrays_of(j, positioned):
    br, sc = j.entries()
    return (j.keys().copy(), j.key_offsets().copy(), br.copy(), sc.view(np.uint32).copy(), None if not positioned else j.positions().copy())


def chain_rows_are_the_table(j, positioned):
    """per length and per row: the kept score bits and position are the table's (a failure names the resolver and the row)"""
    keys, off = j.keys(), j.key_offsets().astype(np.int64)
    br, sc = j.entries()
    pos = j.positions() if positioned else np.zeros(len(br), np.uint32)
    wrong = []
    for ki, (key, n) in enumerate(P.CHAIN_KEYS):
        i = int(np.searchsorted(keys, key))
        assert keys[i] == key
        got = P.kept_rows(br[off[i]:off[i + 1]], sc[off[i]:off[i + 1]], pos[off[i]:off[i + 1]])
        for r, want in enumerate(P.table_rows(ki)):
            if got[r] is None or got[r][0] != want[0] or (positioned and got[r][1] != want[1]):
                wrong.append((P.resolver(n), n, P.ROW_NAMES[r], "got", got[r] and (hex(got[r][0]), got[r][1]), "want", (hex(want[0]), want[1])))
    assert not wrong, wrong


@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
@pytest.mark.parametrize("name", ["chains", "slot_alias", "high_keys"])
def test_join_is_the_restatement_on_both_routes(engine, shard_files, name, positioned):
    c = P.case(name)
    want = c["want"]
    srcs = [engine.load_db(p) for p in shard_files(name, positioned)]
    try:
        got = {}
        for route in (0, 1):
            j = join_on_route(engine, srcs, route)
            try:
                if name == "chains":
                    chain_rows_are_the_table(j, positioned)
                same_join(j, want, positioned)
                st = engine.join_stats()
                assert st["shared_keys"] == want["shared_keys"] and st["entries_dropped"] == want["dropped"]
                assert st["route"] == want["route"] == 1
                got[route] = arrays_of(j, positioned)
            finally:
                j.free()
        for a, b in zip(got[0], got[1]):
            assert (a is None and b is None) or np.array_equal(a, b)
        for s, shard in zip(srcs, c["shards"]):                               # the sources are untouched
            same_as_arrays(s, shard, positioned)
    finally:
        free_all(srcs)


@pytest.mark.parametrize("positioned", KINDS, ids=["plain", "positioned"])
def test_chains_in_reversed_shard_order(engine, shard_files, positioned):
    """The first place moves and the winners change: the join of shards 3, 2, 1, 0 is the restatement of that order."""
    c = P.case("chains")
    want = c["want_reversed"]
    assert not np.array_equal(want["br"], c["want"]["br"]) and not np.array_equal(want["sc"].view(np.uint32), c["want"]["sc"].view(np.uint32))
    srcs = [engine.load_db(p) for p in shard_files("chains", positioned)[::-1]]
    try:
        for route in (0, 1):
            j = join_on_route(engine, srcs, route)
            try:
                same_join(j, want, positioned)
                assert engine.join_stats()["entries_dropped"] == want["dropped"]
            finally:
                j.free()
    finally:
        free_all(srcs)


def test_route_2_takes_slot_aliases_and_names_a_duplicate_beyond_a_wavefront(engine, shard_files):
    alias = [engine.load_db(p) for p in shard_files("slot_alias", True)]
    loc = [engine.load_db(p) for p in shard_files("locate", True)]
    try:
        # branches that share slots and none that is equal: the duplicate stage runs, drops nothing, and the call succeeds
        j = join_on_route(engine, alias, 2)
        try:
            same_join(j, P.case("slot_alias")["want"], True)
            st = engine.join_stats()
            assert st["route"] == 1 and st["entries_dropped"] == 0
        finally:
            j.free()
        with pytest.raises(ipk_amd.IpkGpuError) as ei:
            join_on_route(engine, loc, 2)
        assert ei.value.code == 1
        # the first dropped entry of the concatenated layout: key 300's last, first held by source 1 (source 0's run has no entries)
        for w in (f"k-mer {P.LOCATE_KEY} ", f"branch {P.LOCATE_BRANCH} ", "source 1", "source 3"):
            assert w in str(ei.value), (w, str(ei.value))
        want = P.case("locate")["want"]
        for route in (0, 1):                                                  # the engine joins the same sources afterwards
            j = join_on_route(engine, loc, route)
            try:
                same_join(j, want, True)
                assert engine.join_stats()["entries_dropped"] == want["dropped"] == 2
            finally:
                j.free()
    finally:
        free_all(alias + loc)


def test_join_bytes_bounds_the_chains(shard_files):
    """The held peak of the call on `chains` -- the branch table, the three duplicate kernels and the sorted pass -- stays within
    ipkgpu_db_join_bytes of the sources' keys and entries in all (include/ipkgpu.h)."""
    c = P.case("chains")
    eng = ipk_amd.Engine(0)
    try:
        srcs = [eng.load_db(p) for p in shard_files("chains", True)]
        eng.set_option("release_workspaces", 1)
        held = eng.mem_stats(reset_peak=True)[0]
        j = eng.join_dbs(srcs)
        assert eng.join_stats()["route"] == 1
        same_join(j, c["want"], True)
        j.free()
        peak = eng.mem_stats()[1]
        need = eng.join_bytes(sum(len(s["keys"]) for s in c["shards"]), sum(len(s["br"]) for s in c["shards"]), len(c["shards"]), True)
        print(f"join bytes, chains: held {held}, peak {peak}, join_bytes {need}")
        assert held < peak <= held + need
    finally:
        eng.close()
