"""The CPU model of gdx_seed_candidates_many (seed slots -> ranked, de-duplicated verification candidates), written straight from
the definition in include/gdx_experimental.h on plain Python and numpy -- the oracle's full suffix array and sentinel indices for
(t, pos), a sort of tuples, a linear scan for the groups, the weight from a boolean coverage array over the read; nothing of
the library --, hand-worked cases with literal expected tuples, the chain property SMEMs -> candidates -> alignments on random
reads, and the ABI bookkeeping of the two new calls (header, library, ctypes stub, Rust declarations).
tests/test_gpu_candidates.py holds the GPU against this model."""
import ctypes
import os
import re

import numpy as np

from genedex_amd import alphabet as alph
from test_align_model import align_model
from test_edit_distance_model import NO_END
from test_smems_model import model_arrays, oracle_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gdx_seed_candidates_many", "gdx_seed_candidates_many_dev")
NONE, BAD_SEEDS, MAX_ANCHORS = 0xFFFFFFFF, 1, 1024
OUT_NAMES = ("n_candidates", "n_groups", "n_skipped", "cand_query", "cand_begin", "text_id", "position", "cand_weight", "status")
A = alph.ascii_dna()


def candidates_model(sa, sentinels, n_seeds, begin, length, start, end, max_seeds, max_occ, band, max_candidates):
    """-> (n_candidates, n_groups, n_skipped: u32[nq]; cand_query, cand_begin: u32[nq * max_candidates]; text_id, position:
    u64[..]; cand_weight: u32[..]; status: u8[nq]).  sa: the full suffix array of the concatenation, sentinels: the position
    of every text's sentinel in it.  Per query: the check; one anchor (t, d, begin, length, pos) per row of every seed on at
    most max_occ rows; sorted as tuples; a new group at the first anchor, at another t, or when d - d_first > band; weight =
    the set bits of a coverage array over the read; representative = the greatest length, the first among equals; groups by
    (-weight, t, d_first); the first max_candidates into the slots, the none pattern behind them."""
    sa = np.asarray(sa, dtype=np.int64)
    sentinels = np.asarray(sentinels, dtype=np.int64)
    n, nq, ms, mc = sa.size, len(n_seeds), int(max_seeds), int(max_candidates)
    assert ms >= 1 and max_occ >= 1 and 1 <= mc <= 1024 and ms * max_occ <= MAX_ANCHORS
    n_cand, n_groups, n_skipped = (np.zeros(nq, dtype=np.uint32) for _ in range(3))
    cq = np.full(nq * mc, NONE, dtype=np.uint32)
    cb, cw = np.zeros(nq * mc, dtype=np.uint32), np.zeros(nq * mc, dtype=np.uint32)
    ct, cp = np.zeros(nq * mc, dtype=np.uint64), np.zeros(nq * mc, dtype=np.uint64)
    status = np.zeros(nq, dtype=np.uint8)
    for i in range(nq):
        ns = int(n_seeds[i])
        if ns > ms:
            status[i] = BAD_SEEDS
            continue
        seeds = [tuple(int(x[i * ms + j]) for x in (begin, length, start, end)) for j in range(ns)]
        bad = any(ln == 0 or s > e or e > n for _, ln, s, e in seeds)
        bad |= any(not (b1 < b0 and b1 + l1 < b0 + l0) for (b0, l0, _, _), (b1, l1, _, _) in zip(seeds, seeds[1:]))
        if bad:
            status[i] = BAD_SEEDS
            continue
        anchors = []
        for b, ln, s, e in seeds:
            if e - s > max_occ:
                n_skipped[i] += 1
                continue
            for r in range(s, e):
                g = int(sa[r])
                t = int(np.searchsorted(sentinels, g, side="left"))       # the smallest t with g <= sentinels[t]
                pos = g if t == 0 else g - int(sentinels[t - 1]) - 1
                anchors.append((t, pos - b, b, ln, pos))
        anchors.sort()
        groups = []
        for an in anchors:
            if not groups or an[0] != groups[-1][0][0] or an[1] - groups[-1][0][1] > band:
                groups.append([])
            groups[-1].append(an)
        n_groups[i] = len(groups)
        ranked = []
        for grp in groups:
            covered = np.zeros(max(b + ln for _, _, b, ln, _ in grp), dtype=bool)
            for _, _, b, ln, _ in grp:
                covered[b:b + ln] = True
            rep = grp[0]
            for an in grp[1:]:
                if an[3] > rep[3]:
                    rep = an
            ranked.append((-int(covered.sum()), grp[0][0], grp[0][1], rep))
        ranked.sort(key=lambda x: x[:3])
        n_cand[i] = min(len(ranked), mc)
        for c, (neg_w, _, _, rep) in enumerate(ranked[:mc]):
            k = i * mc + c
            cq[k], cb[k], ct[k], cp[k], cw[k] = i, rep[2], rep[0], rep[4], -neg_w
    return n_cand, n_groups, n_skipped, cq, cb, ct, cp, cw, status


def concatenation(texts):
    """the texts as the index lays them out: every text followed by its sentinel (byte 0)"""
    return b"".join(bytes(t) + b"\x00" for t in texts)


def rows_of(texts, sa, pattern):
    """[start, end): the rows of the suffix array whose suffixes begin with `pattern`, by comparing bytes"""
    cat = concatenation(texts)
    rows = [r for r in range(len(sa)) if cat[int(sa[r]):int(sa[r]) + len(pattern)] == bytes(pattern)]
    assert rows and rows == list(range(rows[0], rows[-1] + 1)), pattern
    return rows[0], rows[-1] + 1


def seed_arrays(per_query, max_seeds):
    """per_query: per query a list of (begin, length, start, end) -> (n_seeds u32, begin, length u32, start, end u64); a list
    longer than max_seeds keeps its count and loses the seeds behind max_seeds"""
    nq = len(per_query)
    n_seeds = np.array([len(s) for s in per_query], dtype=np.uint32)
    begin, length = np.zeros(nq * max_seeds, dtype=np.uint32), np.zeros(nq * max_seeds, dtype=np.uint32)
    start, end = np.zeros(nq * max_seeds, dtype=np.uint64), np.zeros(nq * max_seeds, dtype=np.uint64)
    for i, seeds in enumerate(per_query):
        for j, (b, ln, s, e) in enumerate(seeds[:max_seeds]):
            k = i * max_seeds + j
            begin[k], length[k], start[k], end[k] = b, ln, s, e
    return n_seeds, begin, length, start, end


def expected_arrays(per_query, max_candidates):
    """per query (status, n_groups, n_skipped, [(cand_begin, text_id, position, weight), ...]) -> the nine output arrays"""
    nq, mc = len(per_query), max_candidates
    out = [np.zeros(nq, dtype=np.uint32) for _ in range(3)]
    cq = np.full(nq * mc, NONE, dtype=np.uint32)
    cb, cw = np.zeros(nq * mc, dtype=np.uint32), np.zeros(nq * mc, dtype=np.uint32)
    ct, cp = np.zeros(nq * mc, dtype=np.uint64), np.zeros(nq * mc, dtype=np.uint64)
    status = np.zeros(nq, dtype=np.uint8)
    for i, (st, groups, skipped, cands) in enumerate(per_query):
        assert len(cands) <= mc
        out[0][i], out[1][i], out[2][i], status[i] = len(cands), groups, skipped, st
        for c, (b, t, p, w) in enumerate(cands):
            k = i * mc + c
            cq[k], cb[k], ct[k], cp[k], cw[k] = i, b, t, p, w
    return out[0], out[1], out[2], cq, cb, ct, cp, cw, status


def assert_same(got, want, what):
    for g, w, name in zip(got, want, OUT_NAMES):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, name, len(bad), int(bad[0]), int(g[bad[0]]), int(w[bad[0]]))


_ORACLES = {}


def oracle_of(texts):
    """(sa, sentinels) of the oracle's index of `texts`"""
    key = tuple(bytes(t) for t in texts)
    if key not in _ORACLES:
        F, _ = oracle_pair(list(key), A)
        _ORACLES[key] = (F.full_sa.astype(np.int64), F.sentinel_indices.astype(np.int64))
    return _ORACLES[key]


# ------------------------------------------------------------------------------------------------
# (a) cases worked by hand.  A case: texts, per query its seeds as (begin, pattern) -- the rows are those of the pattern -- or
#     as raw (begin, length, start, end), the knobs, and per query the literal (status, n_groups, n_skipped, candidates).

T = b"ACGTTGCAAGGCTTAGCCATGATCGGA"                 # every 6-mer of it occurs once
U = b"ACGTTGCA"
THREE = U + b"TT" + U + b"TT" + U + b"GG"          # U at 0, 10 and 20
TANDEM = b"ACACACACACGGT"                          # ACAC at 0, 2, 4 and 6
WIDE = (0xFFFFFFF0, 0x20, 0, 0)                    # a seed that ends beyond 2^32, on no row


def _hand_cases():
    c = {}
    c["one seed, one row"] = ([T], [[(3, T[5:11])]], (4, 8, 0, 2), [(0, 1, 0, [(3, 0, 5, 6)])])
    # [2, 12) and [10, 16) on diagonal 2: one candidate of the union's 14 symbols, named by the longer seed
    c["two seeds on one diagonal"] = ([T], [[(10, T[12:18]), (2, T[4:14])]], (4, 8, 0, 2), [(0, 1, 0, [(2, 0, 4, 14)])])
    c["two rows band apart"] = ([U + b"TT" + U], [[(0, U)]], (4, 8, 10, 2), [(0, 1, 0, [(0, 0, 0, 8)])])
    c["two rows band + 1 apart"] = ([U + b"TT" + U], [[(0, U)]], (4, 8, 9, 2), [(0, 2, 0, [(0, 0, 0, 8), (0, 0, 10, 8)])])
    # diagonals 0, 10, 20 at band 10: 20 - 0 > 10, so the third opens a group although 20 - 10 <= 10
    c["the first diagonal rules"] = ([THREE], [[(0, U)]], (4, 8, 10, 4), [(0, 2, 0, [(0, 0, 0, 8), (0, 0, 20, 8)])])
    c["a negative diagonal"] = ([T], [[(5, T[0:6])]], (4, 8, 0, 2), [(0, 1, 0, [(5, 0, 0, 6)])])
    # ACGT$ $ ACGT$: positions 0 and 6 of the concatenation, both on diagonal 0 of their own text
    c["texts do not merge"] = ([b"ACGT", b"", b"ACGT"], [[(0, b"ACGT")]], (4, 8, 100, 3),
                               [(0, 2, 0, [(0, 0, 0, 4), (0, 2, 0, 4)])])
    c["a tandem repeat counts once"] = ([TANDEM], [[(0, b"ACAC")]], (4, 8, 6, 2), [(0, 1, 0, [(0, 0, 0, 4)])])
    c["a tandem repeat cut by the band"] = ([TANDEM], [[(0, b"ACAC")]], (4, 8, 3, 4), [(0, 2, 0, [(0, 0, 0, 4), (0, 0, 4, 4)])])
    c["a weight tie"] = ([b"GG" + U, U + b"TT"], [[(0, U)]], (4, 8, 0, 2), [(0, 2, 0, [(0, 0, 2, 8), (0, 1, 0, 8)])])
    # text 1 holds both seeds on diagonal 2 (weight 14), text 0 only the first: weight goes before (t, d_first)
    c["weight before order"] = ([b"GG" + U, b"TT" + U + b"AGCCATGA"], [[(10, b"CCATGA"), (0, U)]], (4, 8, 0, 2),
                                [(0, 2, 0, [(0, 1, 2, 14), (0, 0, 2, 8)])])
    # two seeds of 6 symbols in one group: the anchor on the smaller diagonal is the first in the order, whichever seed it is
    c["a representative tie, the later seed first"] = ([T], [[(10, T[13:19]), (2, T[4:10])]], (4, 8, 1, 2), [(0, 1, 0, [(2, 0, 4, 12)])])
    c["a representative tie, the earlier seed first"] = ([T], [[(10, T[12:18]), (2, T[5:11])]], (4, 8, 1, 2), [(0, 1, 0, [(10, 0, 12, 12)])])
    c["occ == max_occ"] = ([TANDEM], [[(0, b"ACAC")]], (4, 4, 6, 2), [(0, 1, 0, [(0, 0, 0, 4)])])
    c["occ == max_occ + 1"] = ([TANDEM], [[(7, b"GGT"), (0, b"ACAC")]], (4, 3, 6, 2), [(0, 1, 1, [(7, 0, 10, 3)])])
    c["n_groups == max_candidates"] = ([THREE], [[(0, U)]], (4, 8, 0, 3), [(0, 3, 0, [(0, 0, 0, 8), (0, 0, 10, 8), (0, 0, 20, 8)])])
    c["n_groups == max_candidates + 1"] = ([THREE], [[(0, U)]], (4, 8, 0, 2), [(0, 3, 0, [(0, 0, 0, 8), (0, 0, 10, 8)])])
    # the four causes, each beside a good query; n = 28 for T
    good, good_want = [(3, T[5:11])], (0, 1, 0, [(3, 0, 5, 6)])
    bad_want = (BAD_SEEDS, 0, 0, [])
    c["bad: n_seeds > max_seeds"] = ([T], [good, [(9, T[11:17]), (3, T[5:11])], good], (1, 8, 0, 2), [good_want, bad_want, good_want])
    c["bad: length == 0"] = ([T], [[(3, 0, 5, 6)], good], (4, 8, 0, 2), [bad_want, good_want])
    c["bad: start > end"] = ([T], [good, [(3, 6, 6, 5)]], (4, 8, 0, 2), [good_want, bad_want])
    c["bad: end > n"] = ([T], [[(3, 6, 27, 29)], good], (4, 8, 0, 2), [bad_want, good_want])
    c["good: end == n"] = ([T], [[(3, 6, 28, 28)], good], (4, 8, 0, 2), [(0, 0, 0, []), good_want])
    c["bad: begin does not descend"] = ([T], [[(3, 6, 0, 0), (3, 5, 0, 0)], good], (4, 8, 0, 2), [bad_want, good_want])
    c["bad: end does not descend"] = ([T], [[(5, 6, 0, 0), (3, 8, 0, 0)], good], (4, 8, 0, 2), [bad_want, good_want])
    # ... in 64 bits: [0xFFFFFFF0, 2^32 + 0x10) lies behind [5, 37), though its end is 0x10 in 32 bits
    c["good: descending in 64 bits"] = ([T], [[WIDE, (5, 0x20, 0, 0)], good], (4, 8, 0, 2), [(0, 0, 0, []), good_want])
    # ... and [8, 2^32 + 7) does not end in front of [0x10, 0x30), though its end is 7 in 32 bits
    c["bad: an end beyond 2^32"] = ([T], [[(0x10, 0x20, 0, 0), (8, 0xFFFFFFFF, 0, 0)], good], (4, 8, 0, 2), [bad_want, good_want])
    return c


HAND_CASES = _hand_cases()


def hand_case_inputs(name):
    """-> (texts, the five seed arrays, (max_seeds, max_occ, band, max_candidates), the nine expected arrays)"""
    texts, queries, knobs, want = HAND_CASES[name]
    sa, _ = oracle_of(texts)
    per_query = []
    for seeds in queries:
        per_query.append([s if len(s) == 4 else (s[0], len(s[1])) + rows_of(texts, sa, s[1]) for s in seeds])
    return texts, seed_arrays(per_query, knobs[0]), knobs, expected_arrays(want, knobs[3])


def test_hand_worked_cases():
    assert len(HAND_CASES) == 26
    for name in HAND_CASES:
        texts, seeds, (ms, occ, band, mc), want = hand_case_inputs(name)
        sa, sentinels = oracle_of(texts)
        assert_same(candidates_model(sa, sentinels, *seeds, ms, occ, band, mc), want, name)


def test_the_hand_worked_inputs_are_what_their_names_say():
    assert all(T.count(T[i:i + 6]) == 1 for i in range(len(T) - 5)) and len(concatenation([T])) == 28
    for name, rows in (("one seed, one row", 1), ("two rows band apart", 2), ("the first diagonal rules", 3),
                       ("texts do not merge", 2), ("a tandem repeat counts once", 4), ("occ == max_occ", 4)):
        _, (n_seeds, _, _, start, end), _, _ = hand_case_inputs(name)
        assert int(end[n_seeds[0] - 1] - start[n_seeds[0] - 1]) == rows, name
    assert HAND_CASES["occ == max_occ"][2][1] == 4 and HAND_CASES["occ == max_occ + 1"][2][1] == 3
    _, seeds, _, want = hand_case_inputs("bad: n_seeds > max_seeds")
    assert seeds[0].tolist() == [1, 2, 1] and want[8].tolist() == [0, BAD_SEEDS, 0]
    # the none pattern: every slot behind n_candidates, and every slot of a bad query
    _, _, _, want = hand_case_inputs("bad: end > n")
    assert want[3].tolist() == [NONE, NONE, 1, NONE] and not want[4][[0, 1, 3]].any() and not want[7][[0, 1, 3]].any()


# ------------------------------------------------------------------------------------------------
# (b) the chain SMEMs -> candidates -> alignments on random reads

def repeat_collection(rng, copies, n_texts=3, unit_len=300, gap=(150, 260)):
    """n_texts texts in which one unit of unit_len symbols stands `copies` times, each copy with 2..8 substitutions, random
    symbols in front, between and behind"""
    rand = lambda n: bytes(b"ACGT"[i] for i in rng.integers(0, 4, n))  # noqa: E731
    unit = rand(unit_len)
    texts = []
    for _ in range(n_texts):
        parts = [rand(int(rng.integers(*gap)))]
        for _ in range(copies):
            copy = bytearray(unit)
            for p in rng.choice(unit_len, size=int(rng.integers(2, 9)), replace=False):
                copy[p] = b"ACGT"[(b"ACGT".index(copy[p]) + 1 + int(rng.integers(0, 3))) % 4]
            parts += [bytes(copy), rand(int(rng.integers(*gap)))]
        texts.append(b"".join(parts))
    return texts


def edited_reads(rng, texts, n_reads, len_min=40, len_max=150, max_edits=3):
    """reads of len_min..len_max symbols that follow a text from a random start with 0..max_edits edits (substitution, inserted
    symbol, skipped text symbol) at distinct offsets in [5, L - 5) -> (reads, [(text_id, start)], edits per read)"""
    qs, origin, edits = [], [], []
    for _ in range(n_reads):
        text_id = int(rng.integers(0, len(texts)))
        t = texts[text_id]
        ln, k = int(rng.integers(len_min, len_max + 1)), int(rng.integers(0, max_edits + 1))
        start = int(rng.integers(0, len(t) - ln - k))
        at = set(int(x) for x in rng.choice(np.arange(5, ln - 5), size=k, replace=False)) if k else set()
        q, p = bytearray(), start
        while len(q) < ln:
            if len(q) in at:
                at.discard(len(q))
                kind = int(rng.integers(0, 3))
                if kind == 0:                                   # another symbol
                    q.append(b"ACGT"[(b"ACGT".index(t[p]) + 1 + int(rng.integers(0, 3))) % 4])
                    p += 1
                elif kind == 1:                                 # a symbol the text does not have
                    q.append(b"ACGT"[int(rng.integers(0, 4))])
                else:                                           # the read skips a text symbol
                    p += 1
                    q.append(t[p])
                    p += 1
                continue
            q.append(t[p])
            p += 1
        qs.append(bytes(q)), origin.append((text_id, start)), edits.append(k)
    return qs, origin, edits


CHAIN = dict(max_smems=16, min_length=12, max_occ=8, band=8, max_candidates=2, n_reads=300)
_CHAIN = {}


def chain_case(copies):
    """the inputs of the chain property and the model's results on them, made once: dict(texts, qs, origin, edits, seeds (the
    model's seven SMEM arrays), cands (the nine arrays at max_candidates 2), sa, sentinels)"""
    if copies not in _CHAIN:
        rng = np.random.default_rng(14000 + copies)
        texts = repeat_collection(rng, copies)
        qs, origin, edits = edited_reads(rng, texts, CHAIN["n_reads"])
        F, R = oracle_pair(texts, A)
        seeds = model_arrays(F, R, qs, CHAIN["max_smems"], CHAIN["min_length"])
        sa, sentinels = F.full_sa.astype(np.int64), F.sentinel_indices.astype(np.int64)
        n_smems, _, begin, length, start, end, status = seeds
        assert not status.any()
        cands = candidates_model(sa, sentinels, n_smems, begin, length, start, end, CHAIN["max_smems"], CHAIN["max_occ"],
                                 CHAIN["band"], CHAIN["max_candidates"])
        _CHAIN[copies] = dict(texts=texts, qs=qs, origin=origin, edits=edits, seeds=seeds, cands=cands, sa=sa, sentinels=sentinels)
    return _CHAIN[copies]


def chain_alignments(copies):
    """align_model on EVERY slot of chain_case(copies)'s candidates, used or not, with max_edits = band + the most edits of a
    read -> (max_edits, the model's five arrays); made once"""
    c = chain_case(copies)
    if "aligned" not in c:
        _, _, _, cq, cb, ct, cp, _, _ = c["cands"]
        k = CHAIN["band"] + 3
        c["aligned"] = (k, align_model(c["texts"], A, c["qs"], cq, cb, np.stack([ct, cp], axis=1), k))
    return c["aligned"]


def test_candidates_lead_the_alignment_to_the_origin_of_a_read():
    c = chain_case(2)
    texts, qs, origin, edits = c["texts"], c["qs"], c["origin"], c["edits"]
    assert 2000 <= sum(len(t) for t in texts) <= 5000 and set(edits) == {0, 1, 2, 3}
    n_cand, n_groups, n_skipped, cq, cb, ct, cp, cw, status = c["cands"]
    nq, mc, band = len(qs), CHAIN["max_candidates"], CHAIN["band"]
    assert not status.any() and (n_cand == np.minimum(n_groups, mc)).all()
    # the conditions on the inputs, so that a pass shows something
    several, cut = int((n_groups >= 2).sum()), int((n_groups > mc).sum())
    found = []
    for i in range(nq):
        near = [k for k in range(i * mc, i * mc + int(n_cand[i]))
                if int(ct[k]) == origin[i][0] and abs(int(cp[k]) - int(cb[k]) - origin[i][1]) <= band + 3]
        if near:
            found.append((i, near[0]))
    print(f"{nq} reads: {several} with >= 2 groups, {cut} cut by max_candidates = {mc}, {len(found)} with a candidate at their origin")
    assert several * 10 >= nq and cut * 10 >= nq and len(found) * 10 >= 9 * nq
    # every slot, used or not, through the alignment model with max_edits = band + the most edits of a read
    k, (dist, _, a_end, n_cigar, _) = chain_alignments(2)
    assert k == band + max(edits)
    unused = cq == NONE
    assert unused.sum() == nq * mc - n_cand.sum()
    assert (dist[unused] == 0xFFFFFFFF).all() and (a_end[unused] == NO_END).all() and (n_cigar[unused] == 0).all()
    assert (dist[~unused] <= k + 1).all()
    checked = 0
    for i, slot in found:
        if abs(int(cp[slot]) - int(cb[slot]) - origin[i][1]) <= band:     # then the window holds the read's own alignment
            assert dist[slot] <= edits[i], (i, int(dist[slot]), edits[i])
            checked += 1
    assert checked * 10 >= 9 * nq
    # the candidates of a read are ranked, and distinct
    for i in range(nq):
        w = cw[i * mc:i * mc + int(n_cand[i])].astype(np.int64)
        assert (np.diff(w) <= 0).all() and (w > 0).all()


def test_a_more_repetitive_collection_has_skipped_seeds():
    c = chain_case(6)
    n_cand, n_groups, n_skipped, _, _, _, _, _, status = c["cands"]
    n_smems, _, _, _, start, end, _ = c["seeds"]
    print(f"{len(c['qs'])} reads: {int((n_skipped > 0).sum())} with skipped seeds, {int((n_groups == 0).sum())} without a group")
    assert not status.any() and (n_skipped > 0).sum() * 10 >= len(c["qs"])
    assert (n_skipped <= n_smems).all() and ((end - start) > CHAIN["max_occ"]).sum() == n_skipped.sum()
    assert ((n_skipped > 0) & (n_groups > 0)).any()                         # a read keeps the seeds that are not repeats


# ------------------------------------------------------------------------------------------------
# (c) the two calls are declared everywhere a binding looks for them

def _header_arg_counts(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(gdx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = len([x for x in args.split(",") if x.strip()])
    return out


def test_header_library_stub_and_rust_binding_have_both_calls():
    from genedex_amd import _lib

    counts = _header_arg_counts("gdx_experimental.h")
    assert counts.get("gdx_seed_candidates_many") == 19 and counts.get("gdx_seed_candidates_many_dev") == 20
    lib = ctypes.CDLL(_lib.LIB_PATH)
    rust = open(os.path.join(ROOT, "bindings", "rust", "gdx.rs")).read()
    for name in NAMES:
        assert hasattr(lib, name), name + " is not exported by libgdx.so"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == counts[name], name
        assert re.search(r"pub fn " + name + r"\s*\(", rust), name
    assert re.search(r"pub fn seed_candidates_many\b", rust)  # the safe wrapper of GpuFmIndex
    header = open(os.path.join(ROOT, "include", "gdx_experimental.h")).read()
    for name, text, value in (("GDX_CAND_NONE", "0xFFFFFFFFu", NONE), ("GDX_CAND_BAD_SEEDS", "1", BAD_SEEDS),
                              ("GDX_CAND_MAX_ANCHORS", "1024u", MAX_ANCHORS)):
        assert re.search(r"#define\s+" + name + r"\s+" + text + r"\s", header), name
        assert getattr(_lib, name) == value, name
        assert re.search(r"pub const " + name + r": u\d+ = ", rust), name


def test_the_candidate_tuple():
    import genedex_amd

    cand = genedex_amd.SeedCandidate(3, 0, 5, 6)
    assert (cand.begin, cand.text_id, cand.position, cand.weight) == (3, 0, 5, 6)
    assert genedex_amd.SeedCandidate._fields == ("begin", "text_id", "position", "weight")
