"""Fabricated table slices for the compressed back half (LDS max-reduce -> compress_slice -> compressed key-major writers -> merge of
batches), shared by tests/test_comp_paths_inputs.py (CPU: the cases are what they claim, the expectation is the oracle's) and
tests/test_gpu_comp_paths.py (GPU: every entry point against the expectation, bit for bit).  Not a test file.

A *box* is a window of k sites whose site i admits a chosen set of symbols; every other entry of the matrix is NEG = -1000.0 and
the threshold is EPS = -100, so the k-mers a window scores are exactly the Cartesian product of its sites' admitted sets (a window
that holds one column without an admitted symbol scores nothing: a sum of k <= 14 scores of at most 2.5 and one -1000 is below
EPS at the window's first bound).  Admitted scores are float32 multiples of 0.25 in [-2.0, 2.5]: every sum is exact in float32 and
in float64, none is infinite.  Boxes stand in a matrix as *islands* separated by one all-NEG column.  `expect` enumerates the boxes
directly in float64 and never calls the oracle.

Geometry of the code under test, quoted from its sources (ipk_amd/csrc):
    slice size TBL, DNA k = 11..14      32 768     ipkgpu.hip:641 (stream_tbl), :840 (xp_tbl)
    slice size TBL, DNA k = 8..10       16 384     ipkgpu.hip:641 (stream_tbl), :841 (xp_tbl)
    slice size TBL, AA k = 6            16 000     ipkgpu.hip:839 (xp_tbl)
    workgroup, 128-KB table             16 wavefronts of 32 blocks of 64 slots    kernels_score.hpp:1088-1089 (comp_bpw, comp_padded_slots), NT = 1024 ipkgpu.hip:713, :903
    workgroup, 64-KB table              8 wavefronts of 32 blocks (250 or 256 real)   the same lines, NT = 512
    pairs per chunk at TBL 32 768       256        kernels_score.hpp:494 (chunk_pairs)
    chunks per trip D                   2          ipkgpu.hip:702 (IPK_RPIPE_D)
    KMC_CAP                             4224       kernels_keymajor.hpp:492 (IPK_KMC_CAP)
    first-trip slots of the positions reduce   TBL / 2   kernels_score.hpp:1912 (pos_sub_slots)
    value room of a slice               (min(pairs, slots) + 1) / 2 eight-byte units   kernels_score.hpp:1048 (comp_slice_room_kernel)
    slices of persistent workgroup w    w, w + G, ... of n_gb = groups * NB, G = min(n_gb, CUs)   kernels_reduce_pipe.hpp:39-41, ipkgpu.hip:732

Half-list rule: a DNA box admits at most 2^8 = 256 k-mer suffixes in its right half and 8 prefixes of one slice in its left half,
below the fast capacity of every DNA k >= 11 kernel family (tests/grid_paths.py `family`: 384, 6144): the scoring kernels' long-list
paths are not under test here.  Larger slot sets are cut into boxes of at most 256 keys (`boxes_of`; 64 at DNA k = 8..10, capacity
160), so a `dense` slice is 128 boxes in 32 matrices.  A slice of 32 768 slots spans the whole right half of a k <= 13 window, so no
single box of 4096 keys inside one slice obeys the rule; the `dups` pattern therefore takes its pairs from the WINDOWS of dups_m(k)
matrices whose every site admits the same two symbols: at least DUPS_CHUNKS = 640 chunks into a slice of 128 or 256 keys, 40 chunks and
DUPS_TRIPS = 20 trips of D = 2 per wavefront.  The `big_box` cases are the exception to the rule: one window whose low 15 key bits are
free, a dense slice out of the scoring kernels' long-list path (a right half list of 4096 at k = 12, of 16 384 at k = 13)."""
import collections
import functools

import numpy as np

NEG, EPS = np.float32(-1000.0), -100.0
BLOCK = 64                      # slots per occupancy block
BPW = 32                        # blocks per wavefront region
CH = 256                        # pairs per chunk at TBL = 32768
RPIPE_D = 2
KMC_CAP = 4224
ISLANDS = 4                     # boxes per matrix
SITES = 60                      # sites of every DNA k >= 11 matrix: 47..50 windows
DUPS_CHUNKS, DUPS_TRIPS = 640, 20   # what a `dups` slice brings the persistent reduce at least: chunks, trips of D chunks per wavefront
VALUES = np.array([0.0, -0.25, -0.5, -0.75, -1.0, -1.25, -1.5, -1.75, -2.0, 0.5], dtype=np.float32)


def geometry(sigma, k):
    """(TBL, wavefronts, slices per group NB) of the compressed reduce of (sigma, k)."""
    T = sigma ** k
    if sigma == 4 and 11 <= k <= 14:
        tbl, waves = 32768, 16
    elif sigma == 4 and 8 <= k <= 10:
        tbl, waves = 16384, 8
    elif sigma == 20 and k == 6:
        tbl, waves = 16000, 8
    else:
        raise ValueError((sigma, k))
    return tbl, waves, (T + tbl - 1) // tbl


def box_bits(k):
    """Free bits of a box at most: 256 keys from DNA k = 11 (fast capacities 384 and 6144), 64 at k = 8..10 (160)."""
    return 8 if k >= 11 else 6


def chunk_pairs(tbl):
    """kernels_score.hpp:494"""
    return 512 if tbl == 16384 else 256


def sites_of(k):
    return SITES if k >= 11 else ISLANDS * k + ISLANDS - 1


def dups_m(k, pair=(0, 1)):
    """Matrices of a `dups` pattern over the symbols `pair`: as many as bring each of its slices (128 or 256 keys) DUPS_CHUNKS chunks
    of CH pairs, and two more; 10 for the 64-KB families."""
    if k < 11:
        return 10
    per_slice = 2 ** k // len(dups_slices(k, pair))
    return -(-DUPS_CHUNKS * CH // (per_slice * (sites_of(k) - k + 1))) + 2


# ---- boxes (DNA: a key is 2 bits per symbol, first symbol most significant; slot = key % TBL, slice = key // TBL) -----------------

def _popcount(x):
    return bin(x).count("1")


def boxes_of(base, mask, limit=8):
    """The key set {base | m : m a subset of the bits `mask`} as (base, mask) pairs of at most 2^limit keys each.  Every such pair is a
    box: a site with both bits free admits four symbols, with one bit free two, with none one."""
    assert base & mask == 0
    if _popcount(mask) <= limit:
        return [(base, mask)]
    top = 1 << (mask.bit_length() - 1)
    return boxes_of(base, mask & ~top, limit) + boxes_of(base | top, mask & ~top, limit)


def range_boxes(key0, lo, n):
    """Slots [lo, lo + n) of the slice that starts at key `key0`, as aligned power-of-two ranges cut into boxes."""
    out = []
    while n:
        size = 1
        while size * 2 <= n and lo % (size * 2) == 0:
            size *= 2
        out += boxes_of(key0 + lo, size - 1)
        lo, n = lo + size, n - size
    return out


def box_columns(k, base, mask, rng, special=None):
    """[k, 4] float32: the box's window.  `special`: "zero" (every admitted score 0.0), "positive" (0.0 but 2.5 at the first site)."""
    cols = np.full((k, 4), NEG, dtype=np.float32)
    for i in range(k):
        sh = 2 * (k - 1 - i)
        fixed, free = (base >> sh) & 3, (mask >> sh) & 3
        for s in range(4):
            if (s & ~free) == fixed:
                cols[i, s] = 0.0 if special else rng.choice(VALUES)
    if special == "positive":
        cols[0][cols[0] == 0.0] = 2.5
    return cols


# ---- slice patterns: (key0 of the slice, slots of the slice, waves, rng) -> list of items -------------------------------------------
# An item is ("box", base, mask, special) -- packed ISLANDS to a matrix in order --, ("solo", base, mask, special) -- a matrix of its
# own -- or ("pair", base, mask) -- the same box with the same scores twice: second island of one matrix and first island of the
# next, so that (rank 0, start k + 1) meets (rank 1, start 0) on equal score bits.

def _single(key0, slot, special=None):
    return ("box", key0 + slot, 0, special)


def corners(key0, nslots, waves):
    """One key each at slots 0, 31, 32, 63, 64 and nslots - 1; slot 0 scores 0.0, slot 31 scores 2.5; the key at slot 63 comes as a
    `pair`."""
    return [_single(key0, 0, "zero"), _single(key0, 31, "positive"), _single(key0, 32), ("pair", key0 + 63, 0), _single(key0, 64),
            _single(key0, nslots - 1)]


def _five(key0, blk):
    """blocks blk .. blk + 4: full / empty / single key in lane 0 / single key in lane 63 / full"""
    return (range_boxes(key0, blk * BLOCK, BLOCK) + range_boxes(key0, (blk + 2) * BLOCK, 1) + range_boxes(key0, (blk + 3) * BLOCK + 63, 1) +
            range_boxes(key0, (blk + 4) * BLOCK, BLOCK))


def neighbours(key0, nslots, waves):
    """The five blocks inside wavefront 1's region (blocks 10..14 of it) and across the boundary of wavefronts 2 and 3 (blocks 30, 31 |
    0, 1, 2)."""
    return [("box", b, m, None) for b, m in _five(key0, BPW + 10) + _five(key0, 2 * BPW + 30)]


def alternate(key0, nslots, waves):
    """Even blocks of wavefront 4 full, odd ones empty; the complement in wavefront 5."""
    w = BPW * BLOCK
    return [("box", b, m, None) for b, m in boxes_of(key0 + 4 * w, (w - 1) & ~BLOCK) + boxes_of(key0 + 5 * w + BLOCK, (w - 1) & ~BLOCK)]


def one_wave(which):
    def pattern(key0, nslots, waves):
        w = BPW * BLOCK
        if which == "first":
            r = [(0, w)]
        elif which == "last":
            r = [((waves - 1) * w, nslots - (waves - 1) * w)]
        else:                                                    # everything but wavefront 0
            r = [(w, nslots - w)]
        return [("box", b, m, None) for lo, n in r for b, m in range_boxes(key0, lo, n)]
    pattern.__name__ = "one_wave_" + which
    return pattern


def dense(key0, nslots, waves):
    return [("box", b, m, None) for b, m in range_boxes(key0, 0, nslots)]


def odd(n):
    """n keys from slot 5 on: 1, 3 and 4095 leave the 4-byte hole of an odd count in the slice's value area"""
    def pattern(key0, nslots, waves):
        return [("box", b, m, None) for b, m in range_boxes(key0, 5, n)]
    pattern.__name__ = f"odd_{n}"
    return pattern


def few_chunks(n):
    """n single-box matrices of 128 keys each on the slots [128 (i % 8), + 128): at least n / 2 chunks, at most one per matrix"""
    def pattern(key0, nslots, waves):
        return [("solo", key0 + 128 * (i % 8), 127, None) for i in range(n)]
    pattern.__name__ = f"few_chunks_{n}"
    return pattern


def empty(key0, nslots, waves):
    return []


def block_3(key0, nslots, waves):
    return [("box", key0 + 3 * BLOCK, BLOCK - 1, None)]


PATTERNS = {p.__name__: p for p in (empty, block_3, corners, neighbours, alternate, one_wave("first"), one_wave("last"), one_wave("rest"), dense,
                                    odd(1), odd(3), odd(4095), few_chunks(1), few_chunks(2), few_chunks(15), few_chunks(16), few_chunks(17))}


# ---- dups: matrices whose every site admits the same two symbols --------------------------------------------------------------------
# Every one of the sites - k + 1 windows of such a matrix is a box of the same 2^k keys (the k-mers over the two symbols), 2^7 or 2^8
# of them in each slice they touch: dups_m(k) matrices bring every key dups_m(k) * windows pairs.  The first matrix scores the first
# symbol 0.0 and the second -1.0 at every site, the last matrix the other way round: a key of j second symbols scores -j in every
# window of the first and -(k - j) in every window of the last, so keys of mostly one symbol have their maximum there, tied between
# all of that matrix' windows; the matrices between are independent draws and take the keys in the middle.

def dups_slices(k, pair, tbl=32768):
    """The slices (key // tbl) of the k-mers over the symbols `pair`, ascending."""
    keys = dups_keys(k, pair)
    return sorted(set((keys // tbl).tolist()))


@functools.lru_cache(maxsize=None)
def dups_keys(k, pair):
    keys = np.zeros(1, dtype=np.int64)
    for _ in range(k):
        keys = (keys[:, None] * 4 + np.array(pair)[None, :]).ravel()
    return np.sort(keys)


def dups_matrices(k, pair, seed):
    rng = np.random.RandomState(seed)
    sites, m = sites_of(k), dups_m(k, pair)
    mats = np.full((m, sites, 4), NEG, dtype=np.float32)
    mats[:, :, list(pair)] = rng.choice(VALUES[:9], size=(m, sites, 2))             # (0.0 .. -2.0)
    mats[0][:, list(pair)] = (0.0, -1.0)
    mats[m - 1][:, list(pair)] = (-1.0, 0.0)
    return mats


# ---- cases ------------------------------------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "name sigma k groups mats slices sequences")
# groups: uint32 [n_mats] group id per matrix (matrices of a group contiguous, ids not ascending); slices: {(group index, slice): pattern
# name}, every other slice of the case is empty; sequences: {sequence name: (workgroup, first item, [(group index, slice), ...])}
SEQUENCES = collections.OrderedDict([
    ("dense_empty_corners", ("dense", "empty", "corners")),
    ("empty_empty_dups", ("empty", "empty", "dups")),
    ("dups_few1_empty", ("dups", "few_chunks_1", "empty")),
    ("few17_dense", ("few_chunks_17", "dense")),
    ("last_empty", ("empty",)),
    ("last_dups", ("dups",)),
])
DUPS_PAIRS = [(0, 1), (2, 3), (0, 2), (1, 3), (0, 3), (1, 2)]
CATALOGUE = ["corners", "neighbours", "alternate", "one_wave_first", "one_wave_last", "one_wave_rest", "odd_1", "odd_3", "odd_4095",
             "few_chunks_2", "few_chunks_15", "few_chunks_16"]


def workgroup_items(w, n_groups, nb, cus):
    """The (group index, slice) pairs persistent workgroup w reduces, in order."""
    n_gb = n_groups * nb
    G = min(n_gb, cus)
    return [divmod(gb, nb) for gb in range(w, n_gb, G)] if w < G else []


def place(k, n_groups, cus, catalogue):
    """{(group index, slice): pattern name or ("dups", symbol pair)} and the sequences met.  Every sequence of SEQUENCES goes to a
    workgroup of its own where one has enough slices (the `last_*` ones at a workgroup's last slice), one `dups` to a group; then the
    CATALOGUE patterns go to free slices of group 0 and `dense` gets `corners` in the slices before and after it and in the same slice of
    the next group where those are free."""
    tbl, waves, nb = geometry(4, k)
    G = min(n_groups * nb, cus)
    slices, met, dups_group = {}, {}, {}
    dset = {p: set(dups_slices(k, p, tbl)) for p in DUPS_PAIRS}

    def free(g, b):
        return (g, b) not in slices and not (g in dups_group and b in dset[dups_group[g]])

    def try_put(items, names):
        """the assignments that put `names` on `items`, or None"""
        new, pair_of = {}, {}
        for (g, b), name in zip(items, names):
            if (g, b) in new or (g, b) in slices:
                return None
            if name == "dups":
                if g in pair_of:
                    return None
                if g in dups_group:
                    return None
                fits = [p for p in DUPS_PAIRS if b in dset[p] and not any((g, x) in slices for x in dset[p])]
                if not fits:
                    return None
                pair_of[g] = fits[0]
                new[(g, b)] = ("dups", fits[0])
            else:
                if not free(g, b):
                    return None
                new[(g, b)] = name
        for (g, b), name in new.items():                               # a dups of this sequence must leave its other slices alone
            if name[0] != "dups" and g in pair_of and b in dset[pair_of[g]]:
                return None
        return new, pair_of

    used = set()
    # (a workgroup's last slice lies in the last group: `last_dups` takes that group's dups before another sequence does)
    for seq, names in sorted(SEQUENCES.items(), key=lambda kv: kv[0] != "last_dups"):
        for w in range(G):
            if w in used:
                continue
            items = workgroup_items(w, n_groups, nb, cus)
            if len(items) < len(names) or (seq.startswith("last_") and len(items) < 2):
                continue
            starts = [len(items) - 1] if seq.startswith("last_") else range(len(items) - len(names) + 1)
            done = False
            for j in starts:
                got = try_put(items[j:j + len(names)], names)
                if got:
                    slices.update(got[0]); dups_group.update(got[1])
                    met[seq] = (w, j, items[j:j + len(names)])
                    used.add(w); done = True
                    break
            if done:
                break
    for (g, b), name in list(slices.items()):
        if name == "dense":
            for gg, bb in ((g, b - 1), (g, b + 1), ((g + 1) % n_groups, b)):
                if 0 <= bb < nb and free(gg, bb) and (gg, bb) != (g, b):
                    slices[(gg, bb)] = "corners"
    if catalogue:                                                      # (pattern i goes to group i % n_groups)
        b = 0
        # (`one_wave_rest`, 30 matrices, goes with one group only: 200 matrices a case at most)
        names = [n for n in CATALOGUE if n_groups == 1 or n != "one_wave_rest"] + [n for n in ("few_chunks_1", "few_chunks_17", "dense") if n not in slices.values()] + ([] if dups_group else ["dups"])
        for i, name in enumerate(names):
            g = i % n_groups
            if name == "dups":
                dups_group[g] = next(p for p in DUPS_PAIRS if not any((g, x) in slices for x in dset[p]))
                continue
            if name in ("odd_3", "odd_4095"):                          # (placed with odd_1: three consecutive slices of a group)
                continue
            span = 3 if name == "odd_1" else 1
            while not all(free(g, x) for x in range(b, b + span + 2)):
                b += 1
            if name == "odd_1":
                slices[(g, b + 1)], slices[(g, b + 2)], slices[(g, b + 3)] = "odd_1", "odd_3", "odd_4095"
            else:
                slices[(g, b + 1)] = name
            if name == "dense":                                        # an overrun of its value area shows in a neighbour
                slices[(g, b)] = slices[(g, b + 2)] = "corners"
                if free((g + 1) % n_groups, b + 1):
                    slices[((g + 1) % n_groups, b + 1)] = "corners"
            b += span + 2
    if "corners" not in slices.values():                               # (its 0.0 and 2.5 scores: every case has one)
        slices[next((0, b) for b in range(nb) if all(free(0, x) for x in (b - 1, b, b + 1)))] = "corners"
    for g, p in dups_group.items():                                    # every slice a dups touches carries its name
        for b in dset[p]:
            slices[(g, b)] = ("dups", p)
    return slices, met


@functools.lru_cache(maxsize=None)
def build(k, n_groups, cus, catalogue=None):
    """The case of DNA k with `n_groups` groups for a device of `cus` compute units; the CATALOGUE patterns go in with one group and with
    the two groups of k = 11 (None; three groups carry the sequences alone: 200 matrices at most), always (True) or not at all (False)."""
    catalogue = (n_groups == 1 or (k == 11 and n_groups == 2)) if catalogue is None else catalogue
    slices, met = place(k, n_groups, cus, catalogue)
    return assemble(f"dna_k{k}_g{n_groups}_cu{cus}", k, n_groups, slices, met)


def assemble(label, k, n_groups, slices, met=None):
    """The case whose slices carry the patterns `slices` ({(group index, slice): pattern name or ("dups", symbol pair)})."""
    tbl, waves, nb = geometry(4, k)
    sites = sites_of(k)
    gids = [3 * (n_groups - g) + 1 if g % 2 else 3 * g + 2 for g in range(n_groups)]          # distinct, not ascending
    mats, groups = [], []
    for g in range(n_groups):
        rng = np.random.RandomState(1000 * k + g)
        queue, solo = [], []                                            # windows [k, 4] to pack ISLANDS per matrix | one per matrix
        group_mats = []

        def flush():
            while queue:
                m = np.full((sites, 4), NEG, dtype=np.float32)
                for i in range(min(ISLANDS, len(queue))):
                    cols = queue.pop(0)
                    if cols is not None:
                        m[i * (k + 1):i * (k + 1) + k] = cols
                group_mats.append(m)

        for (gg, b), name in sorted(slices.items(), key=lambda kv: kv[0]):
            if gg != g or name == "empty":
                continue
            if name[0] == "dups":
                if b == min(dups_slices(k, name[1], tbl)):
                    flush()
                    group_mats.extend(dups_matrices(k, name[1], 77 * k + g))
                continue
            key0 = b * tbl
            items = [it if len(it) == 4 else it + (None,) for it in PATTERNS[name](key0, min(tbl, 4 ** k - key0), waves)]
            for kind, base, mask, special in [(kind, b2, m2, sp) for kind, b1, m1, sp in items for b2, m2 in boxes_of(b1, m1, box_bits(k))]:
                cols = box_columns(k, base, mask, rng, special)
                if kind == "solo":
                    solo.append(cols)
                elif kind == "pair":
                    while len(queue) % ISLANDS != 1:                    # second island of a matrix, then first island of the next
                        queue.append(None)
                    queue.extend([cols, None, None, cols])
                else:
                    queue.append(cols)
        flush()
        for cols in solo:
            m = np.full((sites, 4), NEG, dtype=np.float32)
            m[:k] = cols
            group_mats.append(m)
        if not group_mats:                                              # a group needs a matrix: one that scores nothing
            group_mats.append(np.full((sites, 4), NEG, dtype=np.float32))
        mats += group_mats
        groups += [gids[g]] * len(group_mats)
    return Case(label, 4, k, np.array(groups, dtype=np.uint32), np.ascontiguousarray(np.stack(mats)), slices, met or {})


@functools.lru_cache(maxsize=None)
def nine_groups(k):
    """Nine groups, `neighbours` in slice 5 of the even ones and `dups` in the odd ones: batches of three groups, writer passes of 4, 4, 1."""
    slices = {}
    for g in range(9):
        if g % 2:
            slices.update({(g, b): ("dups", DUPS_PAIRS[g // 2]) for b in dups_slices(k, DUPS_PAIRS[g // 2])})
        else:
            slices[(g, 5)] = "neighbours"
    return assemble(f"dna_k{k}_nine", k, 9, slices)


@functools.lru_cache(maxsize=None)
def full_block(k, n_groups=130):
    """`n_groups` groups of one matrix, each holding the same full 64-key block (block 3 of slice 1) with scores of its own:
    64 * n_groups entries of one key block, 8320 against KMC_CAP = 4224 at 130."""
    slices = {(g, 1): "block_3" for g in range(n_groups)}
    return assemble(f"dna_k{k}_block", k, n_groups, slices)


@functools.lru_cache(maxsize=None)
def big_box(k):
    """One group: ONE window whose low 15 key bits are free -- slice 5, 32 768 keys, every slot -- in a matrix of its own, between
    `corners` in slices 4 and 6.  Its right half list holds 4096 (k = 12) or 16 384 (k = 13) suffixes: the long-list path."""
    case = assemble(f"dna_k{k}_big_box", k, 1, {(0, 4): "corners", (0, 6): "corners"})
    m = np.full((1, sites_of(k), 4), NEG, dtype=np.float32)
    m[0, :k] = box_columns(k, 5 * 32768, 32767, np.random.RandomState(500 + k))
    slices = dict(case.slices)
    slices[(0, 5)] = "big_box"
    return Case(case.name, 4, k, np.append(case.groups, case.groups[0]), np.ascontiguousarray(np.concatenate([case.mats, m])), slices, {})


@functools.lru_cache(maxsize=None)
def k14():
    """DNA k = 14, one group: `dense` between two `corners`, and `corners` in the last of the 8192 slices."""
    return assemble("dna_k14", 14, 1, {(0, 0): "corners", (0, 1): "dense", (0, 2): "corners", (0, 8191): "corners"})


@functools.lru_cache(maxsize=None)
def small_dna(k):
    """DNA k = 8, 10 (variant 6: 6-byte pairs, 64-KB slices, 8 wavefronts of 32 blocks): three groups; boxes of at most 64 keys."""
    pair = DUPS_PAIRS[0]
    d = dups_slices(k, pair, 16384)
    nb = geometry(4, k)[2]
    slices = {(0, 0): "corners", (0, 1): "neighbours", (0, 2): "alternate", (0, 3): "one_wave_first",
              (1, 0): "one_wave_last", (1, 1): "odd_1", (1, 2): "odd_3", (1, 3): "odd_4095"}
    if nb > 4:
        slices[(1, nb - 1)] = "corners"                                  # the last slice of the key space
    free = [b for b in range(nb) if b not in d]
    slices.update({(2, b): ("dups", pair) for b in d})
    slices.update({(2, free[0]): "dense", (2, free[1]): "few_chunks_17"})
    return assemble(f"dna_k{k}_small", k, 3, slices)


# ---- amino acids, k = 6: 16 000-slot slices (slice = key // 16000: two 8000-key suffix blocks), 250 real blocks of 256 ---------------------

def aa_columns(sets, rng, special=None):
    cols = np.full((len(sets), 20), NEG, dtype=np.float32)
    for i, syms in enumerate(sets):
        for sym in syms:
            cols[i, sym] = 0.0 if special else rng.choice(VALUES)
    if special == "positive":
        cols[0][cols[0] == 0.0] = 2.5
    return cols


def aa_digits(key, k=6):
    return [[(key // 20 ** (k - 1 - i)) % 20] for i in range(k)]


@functools.lru_cache(maxsize=None)
def aa_k6():
    """Two groups.  Group 0: `corners` in slice 0 (slots 0, 31, 32, 63, 64, 15 999; slot 63 as a `pair`); `last_block_partial` in slice 1
    (120 keys in slots 15 880..15 999: blocks 248 and 249, nothing in the padding blocks 250..255); a full block 0 and 16 keys of
    block 1 in slice 2; the first and the last slot of the last slice.  Group 1: dups_m(k) matrices whose every site admits symbols 0
    and 1 (64 keys, 16 in each of four slices, from every window)."""
    k, tbl = 6, 16000
    rng = np.random.RandomState(606)
    sites = sites_of(k)
    pair = aa_columns(aa_digits(63), rng)                              # the same box twice: (rank 1, start 7) and (rank 2, start 0)
    queue = [aa_columns(aa_digits(0), rng, "zero"), aa_columns(aa_digits(31), rng, "positive"), aa_columns(aa_digits(32), rng), aa_columns(aa_digits(64), rng),
             None, pair, None, None,
             pair, aa_columns(aa_digits(tbl - 1), rng), aa_columns([[0], [0], [3], [19], list(range(14, 20)), list(range(20))], rng),
             aa_columns([[0], [0], [4], [0], [0, 1, 2, 3], list(range(20))], rng),
             aa_columns(aa_digits(20 ** 6 - tbl), rng), aa_columns(aa_digits(20 ** 6 - 1), rng)]
    mats = []
    while queue:
        m = np.full((sites, 20), NEG, dtype=np.float32)
        for i in range(min(ISLANDS, len(queue))):
            cols = queue.pop(0)
            if cols is not None:
                m[i * (k + 1):i * (k + 1) + k] = cols
        mats.append(m)
    groups = [9] * len(mats)
    d = np.full((dups_m(k), sites, 20), NEG, dtype=np.float32)
    d[:, :, :2] = rng.choice(VALUES, size=(dups_m(k), sites, 2))
    d[0] = d[0][np.arange(sites) % (k + 1)]
    return Case("aa_k6", 20, k, np.array(groups + [4] * dups_m(k), dtype=np.uint32), np.ascontiguousarray(np.concatenate([np.stack(mats), d])), {}, {})


def pack_aa(keys, k=6):
    """Dense base-20 codes -> the group-major result's keys (5 bits per symbol, first symbol most significant)."""
    keys = np.asarray(keys, dtype=np.int64)
    out = np.zeros_like(keys)
    for i in range(k):
        out |= ((keys // 20 ** i) % 20) << (5 * i)
    return out.astype(np.uint32)


# ---- the expectation: direct enumeration, float64 ----------------------------------------------------------------------------------------

def window_pairs(m, k, sigma=4):
    """(keys int64, scores float64, starts int64) of every k-mer the windows of matrix m score: per window the Cartesian product of
    its sites' admitted sets; a window with a site that admits nothing scores nothing."""
    ok = m > NEG / 2
    ks, ss, ws = [], [], []
    for s in range(m.shape[0] - k + 1):
        if not ok[s:s + k].any(axis=1).all():
            continue
        keys, sums = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.float64)
        for i in range(s, s + k):
            sym = np.flatnonzero(ok[i])
            keys = (keys[:, None] * sigma + sym[None, :]).ravel()
            sums = (sums[:, None] + m[i, sym].astype(np.float64)[None, :]).ravel()
        assert (sums > EPS).all()
        ks.append(keys); ss.append(sums); ws.append(np.full(len(keys), s, dtype=np.int64))
    if not ks:
        return np.zeros(0, np.int64), np.zeros(0, np.float64), np.zeros(0, np.int64)
    return np.concatenate(ks), np.concatenate(ss), np.concatenate(ws)


def group_pairs(case, gid):
    """(keys, scores, starts, ranks) of every pair of a group, matrices in input order.  (Kept for the case asked last: a case's name
    names its content, the builders are pure.)"""
    if _PAIRS.get("case") != case.name:
        _PAIRS.clear()
        _PAIRS["case"] = case.name
    if gid not in _PAIRS:
        _PAIRS[gid] = _group_pairs(case, gid)
    return _PAIRS[gid]


_PAIRS = {}


def _group_pairs(case, gid):
    k = case.k
    out = [[], [], [], []]
    for rank, m in enumerate(case.mats[case.groups == gid]):
        keys, sums, starts = window_pairs(m, k, case.sigma)
        for o, a in zip(out, (keys, sums, starts, np.full(len(keys), rank, dtype=np.int64))):
            o.append(a)
    return tuple(np.concatenate(o) for o in out)


def reduce_pairs(keys, sums, starts, ranks, nwin, rule="max_first"):
    """Per key the winning pair: (keys ascending, float32 score bits, window starts).  rule "max_first" is the back half's: the maximum
    score, among equal scores the smallest rank * nwin + start.  The others are wrong back halves: "last_writer" (the pair processed
    last wins whatever its score), "max_last" (among equal scores the LARGEST rank * nwin + start)."""
    seq = ranks * nwin + starts
    if rule == "max_first":
        order = np.lexsort((seq, -sums, keys))
    elif rule == "max_last":
        order = np.lexsort((-seq, -sums, keys))
    else:
        order = np.lexsort((-np.arange(len(keys)), keys))
    k_sorted = keys[order]
    first = np.r_[True, k_sorted[1:] != k_sorted[:-1]] if len(keys) else np.zeros(0, bool)
    sel = order[first]
    s32 = sums[sel].astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), sums[sel])
    return keys[sel], s32.view(np.uint32), starts[sel].astype(np.uint32)


def group_order(case):
    return list(dict.fromkeys(case.groups.tolist()))


@functools.lru_cache(maxsize=None)
def expect(k, n_groups, cus, catalogue=None, rule="max_first"):
    """Per group in first-seen order: (gid, keys ascending, score bits, window starts, scored count)."""
    return case_expect(build(k, n_groups, cus, catalogue), rule)


def case_expect(case, rule="max_first"):
    """`expect` of any case: per group in first-seen order (gid, keys ascending, score bits, window starts, scored count)."""
    nwin = case.mats.shape[1] - case.k + 1
    out = []
    for gid in group_order(case):
        keys, sums, starts, ranks = group_pairs(case, gid)
        out.append((gid,) + reduce_pairs(keys, sums, starts, ranks, nwin, rule) + (len(keys),))
    return out


def shift_blocks(res, tbl=32768):
    """A wrong back half: every key's 64-slot block bits taken from the block before (keys 64 slots up inside their slice, the
    last block's lost)."""
    out = []
    for gid, keys, bits, pos, n in res:
        moved = keys + BLOCK
        keep = moved // tbl == keys // tbl
        out.append((gid, moved[keep], bits[keep], pos[keep], n))
    return out


def key_major(res, owners):
    """(scored count, per owner (slots with entries, their counts), entries [n, 2] uint32 (group id, score bits), positions [n], owner
    offsets): owner o holds the keys q * owners + o at slot q; owner-major, keys ascending, a key's entries in group order -- the
    shape of tests/test_gpu_dense_back_half.py::_expected with the counts rows kept sparse (4^13 and 4^14 slots)."""
    keys = np.concatenate([r[1] for r in res])
    gid = np.concatenate([np.full(len(r[1]), r[0], dtype=np.uint32) for r in res])
    rank = np.concatenate([np.full(len(r[1]), i, dtype=np.int64) for i, r in enumerate(res)])
    bits = np.concatenate([r[2] for r in res])
    pos = np.concatenate([r[3] for r in res])
    order = np.lexsort((rank, keys // owners, keys % owners))
    keys, gid, bits, pos = keys[order], gid[order], bits[order], pos[order]
    per_owner, offsets = [], [0]
    for o in range(owners):
        mine = keys[keys % owners == o] // owners
        slots, counts = np.unique(mine, return_counts=True)
        per_owner.append((slots, counts))
        offsets.append(offsets[-1] + len(mine))
    return sum(r[4] for r in res), per_owner, np.stack([gid, bits], axis=1), pos, offsets


# ---- what a case is: occupancy, pairs, room, chunks ------------------------------------------------------------------------------------

def slice_stats(case, g_index, b):
    """Of slice b of the group with index g_index: dict(keys, pairs, blocks: keys per 64-slot block, waves: keys per wavefront region,
    room: value room in 8-byte units, used: units its values fill, chunks_floor)."""
    tbl, waves, nb = geometry(case.sigma, case.k)
    gid = group_order(case)[g_index]
    keys = group_pairs(case, gid)[0]
    mine = keys[keys // tbl == b] % tbl
    nslots = min(tbl, case.sigma ** case.k - b * tbl)
    distinct = np.unique(mine)
    blocks = np.bincount(distinct // BLOCK, minlength=waves * BPW)
    return dict(keys=len(distinct), pairs=len(mine), blocks=blocks, waves=blocks.reshape(waves, BPW).sum(axis=1),
                room=(min(len(mine), nslots) + 1) // 2, used=(len(distinct) + 1) // 2, chunks_floor=-(-len(mine) // chunk_pairs(tbl)), slots=distinct)


def dups_stats(case, g_index):
    """Of the `dups` keys of a group: (share of keys whose kept score two or more pairs reach, keys whose winning pair lies in the first
    dups matrix, in one between, in the last)."""
    k = case.k
    nwin = case.mats.shape[1] - k + 1
    pair = next(v[1] for (g, b), v in case.slices.items() if g == g_index and v[0] == "dups")
    pk, ps, pw, pr = group_pairs(case, group_order(case)[g_index])
    sel = np.isin(pk, dups_keys(k, pair))
    pk, ps, pw, pr = pk[sel], ps[sel], pw[sel], pr[sel] - pr[sel].min()
    keys, bits, _ = reduce_pairs(pk, ps, pw, pr, nwin)
    at = np.searchsorted(keys, pk)
    win = ps.astype(np.float32).view(np.uint32) == bits[at]
    seq = np.full(len(keys), np.iinfo(np.int64).max)
    np.minimum.at(seq, at[win], (pr * nwin + pw)[win])
    by = np.bincount(seq // nwin, minlength=dups_m(k, pair))
    return float((np.bincount(at[win], minlength=len(keys)) >= 2).mean()), int(by[0]), int(by[1:-1].sum()), int(by[-1])
