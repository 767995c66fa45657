"""Fabricated slices for the dense reduce of 6-byte pairs (reduce_buckets_kernel<16384, 512, false, PAIR6>: DNA k = 8..10, 16 384-slot
slices, 8 wavefronts, 512 pairs a chunk), built with the helpers of tests/comp_paths.py; shared by tests/test_dense_reduce_inputs.py
(CPU: the cases are what they claim) and tests/test_gpu_dense_reduce.py.  Not a test file.

DNA k = 8 has NB = 4 slices a group; gb = group index * NB + slice."""
import functools

from tests import comp_paths as cp

K, TBL, WAVES, NB, CHUNK = 8, 16384, 8, 4, 512
COUNTS = (1, 2, 3, 4, 5, 511, 512)                     # pairs of the small slices: every count modulo 4, a chunk's last pair
PAIR = cp.DUPS_PAIRS[0]


def _slot(s):
    def pattern(key0, nslots, waves):
        return [("box", key0 + s, 0, None)]
    pattern.__name__ = f"slot_{s}"
    return pattern


# (further counts of comp_paths.odd and two single slots, under names of their own)
for _p in [cp.odd(n) for n in COUNTS] + [_slot(0), _slot(TBL - 1)]:
    cp.PATTERNS.setdefault(_p.__name__, _p)

CYCLE = ("empty", "odd_1", "odd_2", "empty", "empty", "odd_3", "odd_4", "block_3", "odd_5", "corners", "odd_511", "odd_512", "slot_0",
         f"slot_{TBL - 1}", "empty")
HEAVY = {0: ("dups", PAIR), 1: ("dups", PAIR), 2: "dense", 3: "few_chunks_2"}      # the slices of the group that holds the long ones


def layout(n_groups):
    """{(group index, slice): pattern}: one group: the heavy slices, the last one empty; three: slot 0 and slot 16 383 alone, a full
    block between empty ones, the heavy group in the middle; more: CYCLE over gb (15 patterns against NB = 4: every pattern meets
    every slice index), the heavy group in the middle."""
    assert cp.dups_slices(K, PAIR, TBL) == [0, 1]
    if n_groups == 1:
        s = {(0, b): v for b, v in HEAVY.items()}
        s[(0, 3)] = "empty"
        return s
    if n_groups == 3:
        s = {(0, 0): "empty", (0, 1): "slot_0", (0, 2): "empty", (0, 3): "empty",
             (2, 0): f"slot_{TBL - 1}", (2, 1): "empty", (2, 2): "block_3", (2, 3): "empty"}
        s.update({(1, b): v for b, v in HEAVY.items()})
        return s
    s = {divmod(gb, NB): CYCLE[gb % len(CYCLE)] for gb in range(n_groups * NB)}
    s.update({(n_groups // 2, b): v for b, v in HEAVY.items()})
    return s


@functools.lru_cache(maxsize=None)
def case(n_groups):
    return cp.assemble(f"dense_reduce_k{K}_g{n_groups}", K, n_groups, layout(n_groups))


@functools.lru_cache(maxsize=None)
def second_call_case():
    """What a call after `case(1)` must not inherit: slot 0 alone where the dups stood, nothing where `dense` stood."""
    return cp.assemble(f"dense_reduce_k{K}_second", K, 1, {(0, 0): "slot_0", (0, 1): "empty", (0, 2): "empty", (0, 3): f"slot_{TBL - 1}"})
