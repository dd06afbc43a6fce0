"""The CPU model of gdx_pair_hits_many[_dev]: the definition of include/gdx_experimental.h "paired-end pairing", step by step on
numpy arrays of shape (n_pairs, 2, mate_slots), checked against a naive second implementation (a dict per locus, plain loops over
all combinations), hand-made pairs with the numbers written out, the generator of read pairs of the chain test, and the
declarations a binding looks for.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from genedex_amd import alphabet as alph
from test_best_hits_model import EDIT_INVALID, EDIT_TOO_LONG, best_hits_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gdx_pair_hits_many", "gdx_pair_hits_many_dev")
PAIR_NAMES = ("n_proper", "n_best", "pair_dist", "sub_dist", "mapq", "pair_span")
MATE_NAMES = ("mate_slot", "mate_dist", "win_query", "win_begin", "win_text_id", "win_position")
OUT_NAMES = PAIR_NAMES + MATE_NAMES
NONE = 0xFFFFFFFF            # GDX_CAND_NONE and GDX_PAIR_NONE
MAPQ_NONE = 255
MAX_MATE_SLOTS = 32
MAX_INSERT = (1 << 31) - 1


def kept_slots(cand_query, cand_begin, text_id, position, dist, end, n_mates, mate_slots, max_dist):
    """steps 1 and 2 -> bool[n_mates, mate_slots]: the slots still live after the duplicates of a locus are gone"""
    ms, k = int(mate_slots), int(max_dist)
    shape = lambda x: np.asarray(x).astype(np.int64).reshape(int(n_mates), ms)  # noqa: E731
    cq, cb, t, p, d = (shape(x) for x in (cand_query, cand_begin, text_id, position, dist))
    j = np.broadcast_to(np.arange(ms, dtype=np.int64), cq.shape)
    # 1. live
    live = (cq != NONE) & (d <= k)
    # 2. same locus, per mate: of the live slots with one key only the least (dist, j) stays
    e = shape(end) if end is not None else (p - cb) & 0xFFFFFFFF
    rank = d * ms + j
    keep = live.copy()
    for o in range(ms):
        same = live[:, o:o + 1] & (cq == cq[:, o:o + 1]) & (t == t[:, o:o + 1]) & (e == e[:, o:o + 1])
        keep &= ~(same & (rank[:, o:o + 1] < rank))
    return keep


def pair_hits_model(cand_query, cand_begin, text_id, position, dist, end, n_pairs, mate_slots, max_dist, min_insert, max_insert):
    """-> the twelve arrays of OUT_NAMES (six of n_pairs entries, six of 2 n_pairs; the winner's hit as two), u32 values in int64"""
    n, ms, k, lo, hi = int(n_pairs), int(mate_slots), int(max_dist), int(min_insert), int(max_insert)
    assert 1 <= ms <= MAX_MATE_SLOTS and k <= 1 << 30 and lo <= hi <= MAX_INSERT
    shape = lambda x: np.asarray(x).astype(np.int64).reshape(2 * n, ms)  # noqa: E731
    cq, cb, t, p, d = (shape(x) for x in (cand_query, cand_begin, text_id, position, dist))
    # per slot
    strand = cq & 1
    diag = p - cb                                       # not wrapped
    right = shape(end) if end is not None else diag
    keep = kept_slots(cand_query, cand_begin, text_id, position, dist, end, 2 * n, ms, k)
    # 3. proper combinations (i, j): mate 0 along axis 1, mate 1 along axis 2
    m0 = lambda x: x[0::2][:, :, None]  # noqa: E731
    m1 = lambda x: x[1::2][:, None, :]  # noqa: E731
    span = np.where(m0(strand) == 0, m1(right) - m0(diag), m0(right) - m1(diag))
    proper = m0(keep) & m1(keep) & (m0(t) == m1(t)) & (m0(strand) != m1(strand)) & (lo <= span) & (span <= hi)
    score = m0(d) + m1(d)
    # 4. pair results
    big = np.int64(1) << 62
    n_proper = proper.sum(axis=(1, 2))
    any_proper = n_proper > 0
    order = score * (ms * ms) + np.arange(ms * ms, dtype=np.int64).reshape(1, ms, ms)     # (score, i, j) as one number
    flat = np.where(proper, order, big).reshape(n, ms * ms)
    at = flat.argmin(axis=1)
    rows = np.arange(n)
    bi, bj = at // ms, at % ms
    pair_dist = np.where(any_proper, score.reshape(n, -1)[rows, at], 2 * k + 2)
    pair_span = np.where(any_proper, span.reshape(n, -1)[rows, at], 0) & 0xFFFFFFFF
    n_best = (proper & (score == pair_dist[:, None, None])).reshape(n, -1).sum(axis=1)
    others = np.where(proper, score, big).reshape(n, -1).copy()
    others[rows, at] = big
    others = others.min(axis=1)
    sub_dist = np.where(others == big, 2 * k + 2, others)
    mapq = np.where(any_proper, np.minimum(60, 60 * (sub_dist - pair_dist) // (2 * k + 2)), MAPQ_NONE)
    # 5. winners: the pair's slots, or each mate's single-end best (gdx_best_hits_many over 2 n_pairs groups of mate_slots)
    single = best_hits_model(cand_query, cand_begin, text_id, position, dist, end, 2 * n, ms, k)
    slot = np.where(single[0] == NONE, 0, single[0])
    paired = np.repeat(any_proper, 2)
    slot = np.where(paired, np.stack([bi, bj], axis=1).reshape(-1), slot)
    mapped = paired | (single[0] != NONE)
    mates = np.arange(2 * n)
    pick = lambda x, none: np.where(mapped, x[mates, slot], none)  # noqa: E731
    return (n_proper, n_best, pair_dist, sub_dist, mapq, pair_span,
            np.where(mapped, slot, NONE), pick(d, k + 1), pick(cq, NONE), pick(cb, 0), pick(t, 0), pick(p, 0))


def pair_hits_naive(cand_query, cand_begin, text_id, position, dist, end, n_pairs, mate_slots, max_dist, min_insert, max_insert):
    """the same results pair by pair: per mate a dict per locus, then plain loops over all (i, j)"""
    ms, k, lo, hi = int(mate_slots), int(max_dist), int(min_insert), int(max_insert)
    pairs, mates = [], []
    for p in range(int(n_pairs)):
        kept = []
        for s in (0, 1):
            first = (2 * p + s) * ms
            alive = sorted((int(dist[x]), x - first) for x in range(first, first + ms) if int(cand_query[x]) != NONE and int(dist[x]) <= k)
            loci = {}
            for d, j in alive:
                x = first + j
                e = int(end[x]) if end is not None else (int(position[x]) - int(cand_begin[x])) % (1 << 32)
                loci.setdefault((int(cand_query[x]), int(text_id[x]), e), (d, j))
            kept.append(sorted(loci.values()))
        combos = []
        for di, i in kept[0]:
            for dj, j in kept[1]:
                x, y = 2 * p * ms + i, (2 * p + 1) * ms + j
                if int(text_id[x]) != int(text_id[y]) or (int(cand_query[x]) & 1) == (int(cand_query[y]) & 1):
                    continue
                f, r = (x, y) if int(cand_query[x]) & 1 == 0 else (y, x)
                right = int(end[r]) if end is not None else int(position[r]) - int(cand_begin[r])
                span = right - (int(position[f]) - int(cand_begin[f]))
                if lo <= span <= hi:
                    combos.append((di + dj, i, j, span))
        combos.sort()
        if combos:
            pd, bi, bj, span = combos[0]
            sub = combos[1][0] if len(combos) > 1 else 2 * k + 2
            pairs.append((len(combos), sum(1 for c in combos if c[0] == pd), pd, sub, min(60, 60 * (sub - pd) // (2 * k + 2)), span))
            winners = (bi, bj)
        else:
            pairs.append((0, 0, 2 * k + 2, 2 * k + 2, MAPQ_NONE, 0))
            winners = tuple(kept[s][0][1] if kept[s] else None for s in (0, 1))
        for s in (0, 1):
            if winners[s] is None:
                mates.append((NONE, k + 1, NONE, 0, 0, 0))
            else:
                x = (2 * p + s) * ms + winners[s]
                mates.append((winners[s], int(dist[x]), int(cand_query[x]), int(cand_begin[x]), int(text_id[x]), int(position[x])))
    cols = lambda rows, width: tuple(np.array(c, dtype=np.int64).reshape(-1) for c in zip(*rows)) if rows \
        else tuple(np.zeros(0, np.int64) for _ in range(width))  # noqa: E731
    return cols(pairs, 6) + cols(mates, 6)


def assert_same(got, want, what):
    assert len(got) == len(want) == len(OUT_NAMES)
    for g, w, name in zip(got, want, OUT_NAMES):
        g, w = np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64)
        assert g.shape == w.shape, f"{what}: {name}: shape {g.shape} != {w.shape}"
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what}: {name} differs in {bad.size} entries, first at {bad[0]}: {g[bad[0]]} != {w[bad[0]]}"


LO, HI = 200, 500            # the insert bounds of the random tests


def random_pair_slots(rng, n_pairs, mate_slots, max_dist, with_end, min_insert=LO, max_insert=HI, pool=4, one_text=False,
                      negative=True):
    """slots of n_pairs pairs whose loci come from a pool of `pool` loci per mate, so that duplicates and ties are common.  A
    locus has a strand (mostly the mate's role, forward for mate 0 of an even pair and for mate 1 of an odd one: the roles are
    swapped in every second pair; one in seven on the other strand, which gives same-strand combinations), a text (one in seven on
    text 1 unless one_text) and a coordinate: a forward locus the diagonal F + {0, 0, 0, 1, 5000}, a reverse locus the right end
    F + {min_insert - 1, min_insert, the middle, max_insert, max_insert + 1}, so that spans below, at, inside, at and above the
    bounds occur.  F = 1000 + 13 p, and -7 in every fifth pair when `negative` (position < cand_begin on the forward strand).
    Distances as test_best_hits_model.random_slots draws them, but three mates in ten have one small distance in all their slots and
    a pair in eight exactly max_dist in all slots of both mates; some slots unused (some of them with distance 0), some mates dead.
    -> (cand_query, cand_begin, text_id, position, dist, end)"""
    n, ms, k, lo, hi = int(n_pairs), int(mate_slots), int(max_dist), int(min_insert), int(max_insert)
    assert not negative or lo >= 158
    m = 2 * n * ms
    mate = np.repeat(np.arange(2 * n, dtype=np.int64), ms)
    pair, s = mate >> 1, mate & 1
    locus = rng.integers(0, pool, m)
    role = (np.arange(2 * n) ^ (np.arange(2 * n) >> 1)) & 1                  # the strand a mate is expected on
    l_strand = np.where(rng.random((2 * n, pool)) < 0.15, 1 - role[:, None], role[:, None])
    l_text = np.zeros((2 * n, pool), dtype=np.int64) if one_text else (rng.random((2 * n, pool)) < 0.15).astype(np.int64)
    l_fwd = np.array([0, 0, 0, 1, 5000])[rng.integers(0, 5, (2 * n, pool))]
    l_rev = rng.choice([lo - 1, lo, (lo + hi) // 2, hi, hi + 1], (2 * n, pool), p=[0.1, 0.2, 0.4, 0.2, 0.1])
    base = np.where((np.arange(n) % 5 == 0) & negative, -7, 1000 + 13 * np.arange(n))
    strand, t = l_strand[mate, locus], l_text[mate, locus]
    length = 150 if with_end else 0                                         # what lies between a diagonal and its right end
    diag = base[pair] + np.where(strand == 0, l_fwd[mate, locus], l_rev[mate, locus] - length)
    cb = np.where(diag < 0, rng.integers(1, 3, m), rng.integers(0, 3, m)) * 7
    p = diag + cb
    assert (p >= 0).all() and (p < 1 << 32).all()
    end = diag + 150 if with_end else None
    cq = 4 * pair + 2 * s + strand
    near = rng.integers(0, min(k, 3) + 1, (2 * n, pool))                     # 0 .. min(k, 3): both mates must be live for a pair
    far = rng.integers(0, k + 2, (2 * n, pool))
    own = np.where(rng.random((2 * n, pool)) < 0.7, near, far)
    d = np.minimum(own[mate, locus] + np.array([0, 0, 0, 1, 2])[rng.integers(0, 5, m)], k + 1)
    # three mates in ten are level: all their slots carry one small distance, so that combinations tie at every k; in a pair
    # in eight both mates have exactly k in all slots: the largest score there is, 2k, occurs
    level = rng.random(2 * n) < 0.3
    d = np.where(level[mate], rng.integers(0, min(k, 3) + 1, 2 * n)[mate], d)
    d = np.where((rng.random(n) < 0.125)[pair], k, d)
    d = np.where(rng.random(m) < 0.1, rng.choice([k + 1, EDIT_INVALID, EDIT_TOO_LONG], m), d)
    d = np.where(np.repeat(rng.random(2 * n) < 0.08, ms), k + 1, d)          # a mate in twelve is dead
    unused = rng.random(m) < 0.15
    cq = np.where(unused, NONE, cq)
    d = np.where(unused & (rng.random(m) < 0.5), 0, d)                       # an unused slot may carry any distance
    return cq, cb, t, p, d, end


# ------------------------------------------------------------------------------------------------
# (a) the model against the naive implementation

@pytest.mark.parametrize("mate_slots", (1, 2, 3, 5, 8, 17, 32))
def test_model_equals_the_naive_implementation(mate_slots):
    rng = np.random.default_rng(17000 + mate_slots)
    n = 400
    for k in (0, 3, 11, 1 << 30):
        for with_end in (True, False):
            slots = random_pair_slots(rng, n, mate_slots, k, with_end)
            want = pair_hits_naive(*slots, n, mate_slots, k, LO, HI)
            assert_same(pair_hits_model(*slots, n, mate_slots, k, LO, HI), want, f"k = {k}, end = {with_end}")
            # the inputs show something: proper and non-proper pairs, unique ones, a mate without a live slot
            assert (want[0] > 0).any() and (want[0] == 0).any() and (want[1] == 1).any() and (want[6] == NONE).any()
            assert (want[1] >= 2).any() or mate_slots == 1     # (one slot per mate is one combination: it cannot tie)
            assert (want[2] == 2 * k).any()                    # the largest score there is: both winners at the limit


def test_the_generator_shows_every_kind_of_combination():
    rng = np.random.default_rng(17099)
    n, ms, k = 400, 5, 3
    for with_end in (True, False):
        cq, cb, t, p, d, end = random_pair_slots(rng, n, ms, k, with_end)
        sh = lambda x: np.asarray(x).reshape(n, 2, ms)  # noqa: E731
        cq3, t3, diag = sh(cq), sh(t), sh(p - cb)
        used = cq3 != NONE
        both = used[:, 0, :, None] & used[:, 1, None, :]
        s0, s1 = (cq3[:, 0] & 1)[:, :, None], (cq3[:, 1] & 1)[:, None, :]
        right = sh(end) if with_end else diag
        span = np.where(s0 == 0, right[:, 1][:, None, :] - diag[:, 0][:, :, None], right[:, 0][:, :, None] - diag[:, 1][:, None, :])
        opposite = both & (s0 != s1) & (t3[:, 0][:, :, None] == t3[:, 1][:, None, :])
        for value in (LO - 1, LO, (LO + HI) // 2, HI, HI + 1):
            assert (opposite & (span == value)).any(), value
        assert (both & (s0 == s1)).any() and (both & (t3[:, 0][:, :, None] != t3[:, 1][:, None, :])).any()
        assert (diag < 0).any() and (used & (sh(d) == 0)).any() and (~used & (sh(d) == 0)).any()
        assert (opposite & (s0 == 1)).any() and (opposite & (s0 == 0)).any()     # the roles of the mates both ways


# ------------------------------------------------------------------------------------------------
# (b) hand-made pairs, the expected numbers written out

UNUSED = (NONE, 0, 0, 0, 0, 0)


def one_pair(mate0, mate1, k, lo, hi, with_end=True):
    """mate0, mate1: lists of (cand_query, cand_begin, text_id, position, dist, end) per slot, padded here to one length with
    unused slots -> both implementations' record of the one pair: the six pair words, then per output of MATE_NAMES a 2-tuple"""
    ms = max(len(mate0), len(mate1))
    slots = list(mate0) + [UNUSED] * (ms - len(mate0)) + list(mate1) + [UNUSED] * (ms - len(mate1))
    cols = [np.array(c, dtype=np.int64) for c in zip(*slots)]
    args = (*cols[:5], cols[5] if with_end else None, 1, ms, k, lo, hi)
    got = pair_hits_model(*args)
    assert_same(pair_hits_naive(*args), got, "hand-made")
    return tuple(int(x[0]) for x in got[:6]) + tuple((int(x[0]), int(x[1])) for x in got[6:])


def fwd(pos, dist, query=0, begin=0, text=0, length=100):
    """a slot of a forward-strand query (an even number) whose alignment is text[pos - begin, pos - begin + length)"""
    assert query % 2 == 0
    return (query, begin, text, pos, dist, pos - begin + length)


def rev(pos, dist, query=3, begin=0, text=0, length=100):
    assert query % 2 == 1
    return (query, begin, text, pos, dist, pos - begin + length)


def test_mapq_table():
    # (pair_dist, sub_dist or None for a lone combination) -> mapq = min(60, 60 * (sub - best) // (2k + 2))
    table = {0: {(0, None): 60, (0, 0): 0},
             3: {(0, None): 60, (0, 0): 0, (0, 1): 7, (0, 2): 15, (0, 3): 22, (1, None): 52, (2, 4): 15, (3, 4): 7, (6, None): 15,
                 (6, 6): 0, (4, None): 30}}
    for k, rows in table.items():
        for (pd, sd), mapq in rows.items():
            a = (pd + 1) // 2                               # mate 0's distance; mate 1 has pd - a, and sd - a at another locus
            assert a <= k and pd - a <= k and (sd is None or sd - a <= k)
            mate1 = [rev(1200, pd - a)] + ([rev(1250, sd - a)] if sd is not None else [])
            r = one_pair([fwd(1000, a)], mate1, k, 100, 500)
            want = (1 if sd is None else 2, 2 if sd == pd else 1, pd, sd if sd is not None else 2 * k + 2, mapq, 300)
            assert r[:6] == want, (k, pd, sd, r)
            assert r[6] == (0, 0) and r[7] == (a, pd - a)


def test_both_distances_at_the_largest_max_dist():
    # k = 2^30, both slots at distance k: the score 2^31 is the largest there is; 2k + 2 = 2^31 + 2 still fits u32
    k = 1 << 30
    r = one_pair([fwd(1000, k)], [rev(1200, k)], k, 200, 500)
    assert r == (1, 1, 1 << 31, (1 << 31) + 2, 0, 300, (0, 0), (k, k), (0, 3), (0, 0), (0, 0), (1000, 1200))
    # several slots: mate 0's slot 0 is dead, its slot 2 pairs with mate 1's slot 0 (and ties with slot 1 there)
    mate0 = [fwd(1000, k + 1), UNUSED, fwd(1010, k)]
    mate1 = [rev(1200, k), rev(1250, k), rev(9000, 0)]
    r = one_pair(mate0, mate1, k, 200, 500)
    assert r == (2, 2, 1 << 31, 1 << 31, 0, 290, (2, 0), (k, k), (0, 3), (0, 0), (0, 0), (1010, 1200))
    # a lone combination one below the limit: mapq = 60 * 3 // (2^31 + 2) = 0 as well, but sub_dist is the none value
    r = one_pair(mate0, [rev(9000, 0), UNUSED, rev(1200, k - 1)], k, 200, 500)
    assert r[:8] == (1, 1, (1 << 31) - 1, (1 << 31) + 2, 0, 290, (2, 2), (k, k - 1))


def test_the_span_at_and_beyond_the_two_bounds():
    # forward diagonal 1000; the reverse mate ends at 1000 + span
    for span, proper in ((199, False), (200, True), (201, True), (499, True), (500, True), (501, False)):
        r = one_pair([fwd(1000, 1)], [rev(900 + span, 2)], 3, 200, 500)
        assert r[:6] == ((1, 1, 3, 8, 37, span) if proper else (0, 0, 8, 8, MAPQ_NONE, 0)), (span, r)
        assert r[6] == (0, 0) and r[7] == (1, 2) and r[8] == (0, 3)        # the winners are the two slots either way
    # without ends the span is the distance between the diagonals
    for span, proper in ((199, False), (200, True), (500, True), (501, False)):
        r = one_pair([fwd(1000, 0)], [rev(1000 + span, 0)], 3, 200, 500, with_end=False)
        assert r[:6] == ((1, 1, 0, 8, 60, span) if proper else (0, 0, 8, 8, MAPQ_NONE, 0)), (span, r)
    # min_insert = max_insert and the widest bounds
    assert one_pair([fwd(1000, 0)], [rev(1200, 0)], 3, 300, 300)[:6] == (1, 1, 0, 8, 60, 300)
    assert one_pair([fwd(0, 0)], [rev(MAX_INSERT - 100, 0)], 3, 0, MAX_INSERT)[:6] == (1, 1, 0, 8, 60, MAX_INSERT)
    assert one_pair([fwd(0, 0)], [rev(MAX_INSERT - 99, 0)], 3, 0, MAX_INSERT)[0] == 0
    # a reverse mate that ends left of the forward diagonal: a negative span, never proper, even at min_insert 0
    assert one_pair([fwd(1000, 0)], [rev(800, 0)], 3, 0, MAX_INSERT)[0] == 0
    assert one_pair([fwd(1000, 0)], [rev(900, 0)], 3, 0, MAX_INSERT)[:6] == (1, 1, 0, 8, 60, 0)


def test_a_negative_diagonal_of_the_forward_mate():
    # position 2 < cand_begin 9: the diagonal is -7, kept in 64 bits; the reverse mate ends at 293, the span is 300
    r = one_pair([fwd(2, 1, begin=9)], [rev(193, 0)], 3, 200, 500)
    assert r == (1, 1, 1, 8, 52, 300, (0, 0), (1, 0), (0, 3), (9, 0), (0, 0), (2, 193))
    # (wrapped to 32 bits the diagonal would be 2^32 - 7 and the span negative); one more than the span as the lower bound
    assert one_pair([fwd(2, 1, begin=9)], [rev(193, 0)], 3, 301, 500)[0] == 0
    # the same without ends: diagonals -7 and 293
    assert one_pair([fwd(2, 1, begin=9)], [rev(293, 0)], 3, 200, 500, with_end=False)[:6] == (1, 1, 1, 8, 52, 300)


def test_the_roles_of_the_mates_swapped():
    # mate 0 on the reverse strand (query 1), mate 1 forward (query 2): span = right of mate 0 - diagonal of mate 1
    r = one_pair([rev(1200, 2, query=1)], [fwd(1000, 1, query=2)], 3, 200, 500)
    assert r == (1, 1, 3, 8, 37, 300, (0, 0), (2, 1), (1, 2), (0, 0), (0, 0), (1200, 1000))
    # the other way round the same two loci are 300 apart in the wrong order
    assert one_pair([fwd(1200, 2)], [rev(1000, 1)], 3, 200, 500)[0] == 0


def test_two_slots_of_one_strand_are_never_proper():
    assert one_pair([fwd(1000, 0)], [fwd(1200, 0, query=2)], 3, 0, MAX_INSERT)[:6] == (0, 0, 8, 8, MAPQ_NONE, 0)
    assert one_pair([rev(1000, 0, query=1)], [rev(1200, 0)], 3, 0, MAX_INSERT)[:6] == (0, 0, 8, 8, MAPQ_NONE, 0)
    # and two texts neither
    assert one_pair([fwd(1000, 0)], [rev(1200, 0, text=1)], 3, 0, MAX_INSERT)[:6] == (0, 0, 8, 8, MAPQ_NONE, 0)


def test_the_rescue_case():
    # mate 0 has one live slot; mate 1 two slots of equal distance at two loci, the later one in range
    mate0, mate1 = [fwd(1000, 1)], [rev(5000, 1), rev(1200, 1)]
    cols = [np.array(c, dtype=np.int64) for c in zip(*(mate0 + [UNUSED] + mate1))]
    single = best_hits_model(*cols, 2, 2, 3)
    assert int(single[4][1]) == 2 and int(single[5][1]) == 0 and int(single[0][1]) == 0    # mate 1 alone: tied, mapq 0, slot 0
    r = one_pair(mate0, mate1, 3, 200, 500)
    assert r == (1, 1, 2, 8, 45, 300, (0, 1), (1, 1), (0, 3), (0, 0), (0, 0), (1000, 1200))


def test_a_duplicate_locus_in_mate_one_does_not_make_the_pair_look_tied():
    # slots 0 and 1 of mate 1 end at the same place of the same text: one locus, the copy of distance 1 stays
    r = one_pair([fwd(1000, 0)], [rev(1200, 2, begin=10), rev(1190, 1)], 3, 200, 500)
    assert r == (1, 1, 1, 8, 52, 290, (0, 1), (0, 1), (0, 3), (0, 0), (0, 0), (1000, 1190))
    # with equal distances the earlier slot stays
    r = one_pair([fwd(1000, 0)], [rev(1200, 1, begin=10), rev(1190, 1)], 3, 200, 500)
    assert r[:6] == (1, 1, 1, 8, 52, 290) and r[6] == (0, 0)
    # another end is another locus: then the pair is tied
    r = one_pair([fwd(1000, 0)], [rev(1201, 1, begin=10), rev(1190, 1)], 3, 200, 500)
    assert r[:6] == (2, 2, 1, 1, 0, 291) and r[6] == (0, 0)
    # the least (score, i, j): the tie goes to the earlier slot of mate 0 first
    r = one_pair([fwd(1000, 1), fwd(1010, 1)], [rev(1200, 1), rev(1190, 0)], 3, 200, 500)
    assert r[:6] == (4, 2, 1, 1, 0, 290) and r[6] == (0, 1)


def test_without_a_proper_combination_the_winners_are_the_single_end_bests():
    mate0 = [fwd(1000, 2), fwd(3000, 1), UNUSED]
    mate1 = [rev(9000, 3), (3, 0, 0, 9500, EDIT_INVALID, NONE), rev(9900, 0)]
    r = one_pair(mate0, mate1, 3, 200, 500)
    cols = [np.array(c, dtype=np.int64) for c in zip(*(mate0 + mate1))]
    single = best_hits_model(*cols, 2, 3, 3)
    assert r[:6] == (0, 0, 8, 8, MAPQ_NONE, 0)
    assert r[6] == (1, 2) == tuple(int(x) for x in single[0]) and r[7] == (1, 0) == tuple(int(x) for x in single[1])
    for mine, theirs in zip(r[8:], single[6:]):
        assert mine == tuple(int(x) for x in theirs)
    # a dead mate: the other keeps its single-end best, the dead one gets the none pattern
    r = one_pair([fwd(1000, 2)], [rev(1200, 4)], 3, 200, 500)
    assert r == (0, 0, 8, 8, MAPQ_NONE, 0, (0, NONE), (2, 4), (0, NONE), (0, 0), (0, 0), (1000, 0))
    assert one_pair([UNUSED], [UNUSED], 3, 200, 500) == (0, 0, 8, 8, MAPQ_NONE, 0, (NONE, NONE), (4, 4), (NONE, NONE), (0, 0), (0, 0), (0, 0))


# ------------------------------------------------------------------------------------------------
# (c) read pairs for the chain test

def edited(rng, seq, n_edits):
    """seq with n_edits edits (substitution, inserted symbol, dropped symbol) at distinct offsets in [5, len - 5)"""
    at = set(int(x) for x in rng.choice(np.arange(5, len(seq) - 5), size=n_edits, replace=False)) if n_edits else set()
    out = bytearray()
    for i, c in enumerate(seq):
        if i in at:
            kind = int(rng.integers(0, 3))
            if kind == 0:
                out.append(b"ACGT"[(b"ACGT".index(c) + 1 + int(rng.integers(0, 3))) % 4])
            elif kind == 1:
                out.append(b"ACGT"[int(rng.integers(0, 4))])
                out.append(c)
            continue
        out.append(c)
    return bytes(out)


def read_pairs(rng, texts, n_pairs, fragment=(200, 400), mate_len=(50, 120), max_edits=3):
    """n_pairs fragments of fragment[0] .. fragment[1] symbols of a random text; mate 0 = its first mate_len symbols, mate 1 = the
    reverse complement of its last mate_len symbols, each with 0 .. max_edits edits; in every second pair the two change places
    -> (reads, mates interleaved; per read (text_id, the diagonal its forward form was taken from, strand))"""
    reads, origin = [], []
    for p in range(n_pairs):
        text_id = int(rng.integers(0, len(texts)))
        t = texts[text_id]
        ln = int(rng.integers(fragment[0], fragment[1] + 1))
        start = int(rng.integers(0, len(t) - ln + 1))
        l0, l1 = (int(x) for x in rng.integers(mate_len[0], mate_len[1] + 1, 2))
        first = edited(rng, t[start:start + l0], int(rng.integers(0, max_edits + 1)))
        last = alph.reverse_complement(edited(rng, t[start + ln - l1:start + ln], int(rng.integers(0, max_edits + 1))))
        mates = [(first, (text_id, start, 0)), (last, (text_id, start + ln - l1, 1))]
        for read, where in (mates[::-1] if p % 2 else mates):
            reads.append(read), origin.append(where)
    return reads, origin


# the seeds: a combination of one mate with the WRONG copy of the other is out of range by construction, but with both mates
# inside the unit a pair can be proper as a whole in another copy (or text: the unit is in all of them), and where the candidates
# of the right copy were cut by max_candidates that is its only combination.  So "unique proper pairs lie at their origin" holds
# by the choice of these two seeds, not by construction: about one seed in two has such a pair (one of ~140), and whoever changes
# repeat_collection, read_pairs or the CHAIN knobs has to look for seeds again (the counts:
# test_the_chain_inputs_show_what_the_device_test_needs prints them)
PAIR_CHAIN = dict(n_pairs=150, min_insert=150, max_insert=450, seed={2: 17522, 6: 17546})
_PAIR_CHAIN = {}


def pair_chain_case(copies):
    """the inputs of the chain test on the device and the models' results on them, made once: texts of repeat_collection (the
    copies of the unit lie 450 or more apart: a combination with the wrong copy is out of range), 150 read pairs, the four
    queries of every pair as with_strands("both") makes them, and with the CHAIN knobs of test_candidates_model and max_edits =
    band + 3 the models' candidates, alignments of every slot, pair hits and single-end best hits"""
    from test_align_model import align_model
    from test_candidates_model import A, CHAIN, candidates_model, repeat_collection
    from test_smems_model import model_arrays, oracle_pair

    if copies not in _PAIR_CHAIN:
        rng = np.random.default_rng(PAIR_CHAIN["seed"][copies])
        texts = repeat_collection(rng, copies)
        reads, origin = read_pairs(rng, texts, PAIR_CHAIN["n_pairs"])
        qs = [q for r in reads for q in (r, alph.reverse_complement(r))]
        F, R = oracle_pair(texts, A)
        n_smems, _, begin, length, start, end, status = model_arrays(F, R, qs, CHAIN["max_smems"], CHAIN["min_length"])
        assert not status.any()
        cands = candidates_model(F.full_sa.astype(np.int64), F.sentinel_indices.astype(np.int64), n_smems, begin, length, start, end,
                                 CHAIN["max_smems"], CHAIN["max_occ"], CHAIN["band"], CHAIN["max_candidates"])
        _, _, _, cq, cb, ct, cp, _, _ = cands
        k, ms = CHAIN["band"] + 3, 2 * CHAIN["max_candidates"]
        aligned = align_model(texts, A, qs, cq, cb, np.stack([ct, cp], axis=1), k)
        slots = (cq, cb, ct, cp, aligned[0], aligned[2])
        pairs = pair_hits_model(*slots, len(reads) // 2, ms, k, PAIR_CHAIN["min_insert"], PAIR_CHAIN["max_insert"])
        single = best_hits_model(*slots, len(reads), ms, k)
        _PAIR_CHAIN[copies] = dict(texts=texts, reads=reads, origin=origin, qs=qs, cands=cands, k=k, mate_slots=ms, aligned=aligned,
                                   pairs=pairs, single=single)
    return _PAIR_CHAIN[copies]


def pair_chain_counts(c):
    """what the chain test asserts about its inputs -> (proper pairs, pairs with n_proper == 1 and a mate tied single-end, pairs
    not proper, unique proper pairs, those of them with both winners within band + 3 diagonals of where the mates were taken)"""
    from test_candidates_model import CHAIN

    n_proper, n_best = c["pairs"][0], c["pairs"][1]
    tied_single = (c["single"][4].reshape(-1, 2) >= 2).any(axis=1)
    unique = (n_proper > 0) & (n_best == 1)
    wq, wb, wt, wp = (c["pairs"][x].reshape(-1, 2) for x in (8, 9, 10, 11))
    where = np.array(c["origin"], dtype=np.int64).reshape(-1, 2, 3)
    near = ((wt == where[:, :, 0]) & (np.abs(wp - wb - where[:, :, 1]) <= CHAIN["band"] + 3) & ((wq & 1) == where[:, :, 2])).all(axis=1)
    return (int((n_proper > 0).sum()), int(((n_proper == 1) & tied_single).sum()), int((n_proper == 0).sum()), int(unique.sum()),
            int((unique & near).sum()))


@pytest.mark.parametrize("copies", (2, 6))
def test_the_chain_inputs_show_what_the_device_test_needs(copies):
    c = pair_chain_case(copies)
    n = PAIR_CHAIN["n_pairs"]
    proper, rescued, improper, unique, at_origin = pair_chain_counts(c)
    print(f"copies {copies}: {proper} proper, {rescued} with a tied mate and one proper combination, {improper} not proper, "
          f"{at_origin} of {unique} unique proper pairs at their origin")
    # copies 2: 148 proper, 3 rescued, 2 not proper, 148 of 148 at their origin; copies 6: 138, 7, 12, 138 of 138
    assert proper * 2 >= n and rescued >= 1 and improper >= 1 and at_origin == unique


def test_read_pairs_are_what_the_chain_test_takes_them_for():
    from test_candidates_model import repeat_collection

    rng = np.random.default_rng(17400)
    texts = repeat_collection(rng, 2)
    reads, origin = read_pairs(rng, texts, 40)
    assert len(reads) == 80 and all(47 <= len(r) <= 123 for r in reads)
    for p in range(40):
        (t0, d0, s0), (t1, d1, s1) = origin[2 * p], origin[2 * p + 1]
        assert t0 == t1 and {s0, s1} == {0, 1} and s0 == p % 2
        f, r = (0, 1) if s0 == 0 else (1, 0)
        df, dr = origin[2 * p + f][1], origin[2 * p + r][1]
        assert 200 - 120 <= dr - df <= 400 - 50                                 # the fragment from its start to the last mate's start
    exact = [i for i, r in enumerate(reads) if (r if origin[i][2] == 0 else alph.reverse_complement(r)) ==
             texts[origin[i][0]][origin[i][1]:origin[i][1] + len(r)]]
    assert 10 <= len(exact) <= 40                                               # a quarter of the mates has no edit


# ------------------------------------------------------------------------------------------------
# (d) the two calls are declared everywhere a binding looks for them

def test_header_library_stub_and_rust_binding_have_both_calls():
    from genedex_amd import _lib
    from test_candidates_model import _header_arg_counts

    counts = _header_arg_counts("gdx_experimental.h")
    assert counts.get("gdx_pair_hits_many") == 22 and counts.get("gdx_pair_hits_many_dev") == 23
    assert "gdx_pair_hits_many" not in _header_arg_counts("gdx.h")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    rust = open(os.path.join(ROOT, "bindings", "rust", "gdx.rs")).read()
    for name in NAMES:
        assert hasattr(lib, name), name + " is not exported by libgdx.so"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == counts[name], name
        assert re.search(r"pub fn " + name + r"\s*\(", rust), name
    assert re.search(r"pub fn pair_hits_many\b", rust)  # the safe wrapper of GpuFmIndex
    header = open(os.path.join(ROOT, "include", "gdx_experimental.h")).read()
    for name, text, value in (("GDX_PAIR_NONE", "0xFFFFFFFFu", NONE), ("GDX_PAIR_MAPQ_NONE", "255u", MAPQ_NONE),
                              ("GDX_PAIR_MAX_MATE_SLOTS", "32u", MAX_MATE_SLOTS)):
        assert re.search(r"#define\s+" + name + r"\s+" + text + r"\s", header), name
        assert getattr(_lib, name) == value, name
        assert re.search(r"pub const " + name + r": u\d+ = ", rust), name
