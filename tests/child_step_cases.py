"""Fabricated inputs for the child-node steps and the single-step half joins of the DNA k = 8..12 scoring kernel (kernels_quad.hpp),
shared by tests/test_child_step_inputs.py (CPU: the inputs contain every class listed in `required`) and
tests/test_gpu_child_step_paths.py (GPU: every entry point against the oracle).  Not a test file.

Every column's best entry is +0.0 and every other entry -0.25 * an integer, eps = -1.0: all sums are exact, every threshold of a
window whose columns all hold a zero is eps itself, and a candidate of a node, of a half or of the window survives exactly when its
entries sum to more than -1.0.  A window is laid out column by column from a table of node contents with a known number of
survivors (`node_columns`), so the list lengths of a designed window are chosen, not found; the windows that straddle two designed
ones are scored like any others.  `classify` counts the classes from the matrices with oracle/np_oracle.py alone."""
import collections
import functools
import itertools

import numpy as np

from oracle import np_oracle as no

SIGMA = 4
EPS = -1.0
TILE = {8: 40, 9: 40, 10: 40, 11: 32, 12: 32}           # windows per tile of the kernel that scores k
ONEWIN = {8: False, 9: False, 10: False, 11: True, 12: True}   # one window per wavefront step (its four nodes in the four slots)
FAST_CAP = {8: 160, 9: 160, 10: 160, 11: 384, 12: 384}   # half-list capacity of the fast path
GROUPS2 = (5, 2)                                         # two groups, ids not ascending: the count-only pre-pass samples both
KS = (8, 9, 10, 11, 12)
TAILS = (1, 3)                                           # windows in a matrix' last tile: one alone; an odd count (half a pair idles)

FLAT = (0.0, 0.0, 0.0, 0.0)
ONE = (0.0, -2.0, -2.0, -2.0)                            # one entry survives
DEAD = (-2.0, -2.0, -2.0, -2.0)                          # no window over this column scores above eps


def split(k):
    """(LA, LB, RA, RB): symbols of the four child nodes."""
    hl = k // 2
    hr = k - hl
    return hl // 2, hl - hl // 2, hr // 2, hr - hr // 2


def slots(k):
    """Per node 0..3: the 16-lane slots (0..3) its candidates can sit in.  k <= 10: slot = 2 * (odd window of the pair) + (second
    node of the step), the steps pairing the 2-symbol nodes in node order, then the 3-symbol nodes; k >= 11: the node's rank among
    the nodes of its size."""
    h = split(k)
    out = []
    for n in range(4):
        rank = sum(1 for m in range(n) if h[m] == h[n])
        out.append((rank,) if ONEWIN[k] else (rank % 2, 2 + rank % 2))
    return out


def slot_of(k, n, w):
    """The slot of node n of the window at offset w of its tile."""
    s = slots(k)[n]
    return s[0] if ONEWIN[k] else s[w % 2]


@functools.lru_cache(maxsize=None)
def node_columns(h):
    """n -> h columns (4 entries each, the first +0.0, descending) of which exactly n of the 4^h candidates sum to more than eps,
    for every n in 1..4^h: the first combination in lexicographic order of a fixed alphabet."""
    alpha = (0.0, -0.25, -0.5, -0.75, -2.0)
    cols = [(0.0,) + c for c in itertools.combinations_with_replacement(alpha, 3)]
    v = np.array(cols, dtype=np.float64)
    s = v[:, None, :, None] + v[None, :, None, :]                                    # [c0, c1, i, j]
    if h == 2:
        cnt = (s > EPS).sum(axis=(2, 3))
    else:
        s = s[:, :, None, :, :, None] + v[None, None, :, None, None, :]              # [c0, c1, c2, i, j, l]
        cnt = (s > EPS).sum(axis=(3, 4, 5))
    out = {}
    for idx in np.argwhere(cnt > 0):
        out.setdefault(int(cnt[tuple(idx)]), tuple(cols[i] for i in idx))
    assert sorted(out) == list(range(1, 4 ** h + 1)), f"{h}-symbol node: no columns for some list length"
    return out


def _node(h, n):
    return [ONE] * h if n == 1 else list(node_columns(h)[n])


def designs(k, full=True):
    """The designed windows of k: (name, parity or None, [k columns]).  `full`: with the sweep of second-child list lengths."""
    h = split(k)
    out = []

    def window(name, parity, contents):
        cols = []
        for n in range(4):
            cols += contents.get(n, [ONE] * h[n])
        out.append((name, parity, cols))

    for par in ((None,) if ONEWIN[k] else (0, 1)):
        for n in range(4):
            if h[n] == 2:
                window(f"all16 n{n}", par, {n: [FLAT, FLAT]})
            else:
                window(f"all64 n{n}", par, {n: [FLAT] * 3})
                for i in range(4):                                                   # sub-step i empty, the other three full
                    first = tuple(-2.0 if s == i else 0.0 for s in range(4))
                    window(f"sub{i}=0 n{n}", par, {n: [first, FLAT, FLAT]})
        dead = [ONE] * k
        dead[k // 2] = DEAD
        out.append(("dead", par, dead))
    fl, fr = 4 ** h[1], 4 ** h[3]
    # first child x second child list lengths with at most 64 candidates: 63 and 64 of them, and rows of every length
    pairs = [(a, b) for a in (1, 2, 3, 4, 5, 7, 9, 16) for b in (64 // a, 63 // a) if a * b in (63, 64) or a in (2, 3, 5)]
    for a, b in pairs:
        if a <= 4 ** h[0] and b <= fl:
            window(f"L {a}x{b}", None, {0: _node(h[0], a), 1: _node(h[1], b)})
        if a <= 4 ** h[2] and b <= fr:
            window(f"R {a}x{b}", None, {2: _node(h[2], a), 3: _node(h[3], b)})
    if full:
        for i in range(max(fl, fr)):
            window(f"sweep {i}", None, {1: _node(h[1], 1 + i % fl), 3: _node(h[3], 1 + i % fr)})
    return out


Case = collections.namedtuple("Case", "name k tail sites mats groups")


@functools.lru_cache(maxsize=None)
def case(k, tail):
    """The matrices of (k, tail): 4 tiles and `tail` windows a matrix, the designed windows k + 1 or k + 2 columns apart (an odd
    distance: both window parities), the entries of every column in an order of its own; the groups alternate over the matrices."""
    nwin = 4 * TILE[k] + tail
    sites = nwin + k - 1
    rng = np.random.default_rng(1000 * k + tail)
    step = k + 1 if k % 2 == 0 else k + 2
    mats, cur, pos = [], None, 0
    for name, parity, cols in designs(k, full=(tail == 1)):
        while True:
            if cur is None:
                cur = np.array([ONE] * sites, dtype=np.float32)
                pos = 0
            w = pos if parity is None or pos % 2 == parity else pos + 1
            if w + k <= sites - 2:
                break
            mats.append(cur)
            cur = None
        cur[w:w + k] = np.array(cols, dtype=np.float32)
        pos = w + step
    mats.append(cur)
    if len(mats) % 2:
        mats.append(np.array([ONE] * sites, dtype=np.float32))
    mats = np.stack(mats)
    for m in mats:
        for j in range(sites):
            if len(set(m[j])) > 2:                                                   # a column of node_columns: its entries in an order of its own
                m[j] = m[j, rng.permutation(4)]
            elif (m[j] == -2.0).sum() == 3:                                          # ONE: any entry survives  (the sub-step columns keep theirs)
                m[j] = np.roll(m[j], rng.integers(4))
    groups = np.array([GROUPS2[i % 2] for i in range(len(mats))], dtype=np.uint32)
    return Case(f"k{k}_tail{tail}", k, tail, sites, np.ascontiguousarray(mats, dtype=np.float32), groups)


def cases():
    return [(k, t) for k in KS for t in TAILS]


# ---- the classifier ------------------------------------------------------------------------------------------------------------------

def window_nodes(m, best, k, w, eps=EPS):
    """The survivor masks of the four child nodes of window w, and the two half-list lengths, by oracle/np_oracle.py's dense node
    (S(j, h, eps) with its own child thresholds)."""
    f32 = np.float32
    la, lb, ra, rb = split(k)
    hl = la + lb
    eps_l = f32(f32(eps) - f32(best[w + k] - best[w + hl]))                          # pk_compute.cpp:54-55 at (0, k)
    eps_r = f32(f32(eps) - f32(best[w + hl] - best[w]))
    e = [f32(eps_l - f32(best[w + hl] - best[w + la])), f32(eps_l - f32(best[w + la] - best[w])),
         f32(eps_r - f32(best[w + k] - best[w + hl + ra])), f32(eps_r - f32(best[w + hl + ra] - best[w + hl]))]
    j = [0, la, hl, hl + ra]
    masks = [no._node(m, best, w, j[n], (la, lb, ra, rb)[n], e[n], 2)[2] for n in range(4)]
    n_l = int(no._node(m, best, w, 0, hl, eps_l, 2)[2].sum())
    n_r = int(no._node(m, best, w, hl, k - hl, eps_r, 2)[2].sum())
    return masks, n_l, n_r


@functools.lru_cache(maxsize=None)
def classify(k, tail):
    """(set of classes the case's windows reach, windows whose half lists exceed the fast capacity as (matrix, window)).  Classes:
    ("n2", 0 | 16, slot), ("n3", 64, slot): a node's list length; ("sub", i, 0 | 16, slot): survivors of sub-step i of a 3-symbol
    node; ("sub_only0", i, slot): sub-step i empty and the other three full; ("tl" | "tr", 1 | 63 | 64) and ("nlb" | "nrb", n): a
    window whose half joins take the single step (both halves <= 64 candidates, no list empty); "empty_half"; ("tail", n): windows
    in the last tile."""
    c = case(k, tail)
    h = split(k)
    found, over = set(), []
    nwin = c.sites - k + 1
    found.add(("tail", nwin % TILE[k]))
    for mi, m in enumerate(c.mats):
        best = no.prefix_max(m)
        for w in range(nwin):
            masks, n_l, n_r = window_nodes(m, best, k, w)
            cnt = [int(x.sum()) for x in masks]
            for n in range(4):
                slot = slot_of(k, n, w % TILE[k])
                if h[n] == 2:
                    if cnt[n] in (0, 16):
                        found.add(("n2", cnt[n], slot))
                else:
                    if cnt[n] == 64:
                        found.add(("n3", 64, slot))
                    sub = masks[n].reshape(4, 16).sum(axis=1)
                    for i in range(4):
                        if sub[i] in (0, 16):
                            found.add(("sub", i, int(sub[i]), slot))
                        if sub[i] == 0 and sub.sum() == 48:
                            found.add(("sub_only0", i, slot))
            if min(cnt) == 0 or n_l == 0 or n_r == 0:
                found.add("empty_half")
                continue
            tl, tr = cnt[0] * cnt[1], cnt[2] * cnt[3]
            if tl <= 64 and tr <= 64:
                found.update({("tl", tl), ("tr", tr), ("nlb", cnt[1]), ("nrb", cnt[3])})
            if max(n_l, n_r) > FAST_CAP[k]:
                over.append((mi, w))
    return found, over


def required(k):
    """Every class the inputs of k (both tails together) must reach."""
    h = split(k)
    req = {("tail", 1), ("tail", 3), "empty_half"}
    for n in range(4):
        for slot in slots(k)[n]:
            if h[n] == 2:
                req |= {("n2", 0, slot), ("n2", 16, slot)}
            else:
                req.add(("n3", 64, slot))
                for i in range(4):
                    req |= {("sub", i, 0, slot), ("sub", i, 16, slot), ("sub_only0", i, slot)}
    for t in (1, 63, 64):
        req |= {("tl", t), ("tr", t)}
    req |= {("nlb", n) for n in range(1, 4 ** h[1] + 1)} | {("nrb", n) for n in range(1, 4 ** h[3] + 1)}
    return req
