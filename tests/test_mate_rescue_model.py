"""The CPU model of gdx_mate_rescue_many[_dev]: the definition of include/gdx_experimental.h "mate rescue" on numpy arrays (the
attempts of a batch side by side, a table column per step), checked against a plain cell-by-cell programme, hand-worked cases with
the numbers written out, the generator of planted pairs of the device's end-to-end test, and the declarations a binding looks
for.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from genedex_amd import alphabet as alph
from test_edit_distance_model import INVALID, MAX_LEN, NO_END, TOO_LONG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gdx_mate_rescue_many", "gdx_mate_rescue_many_dev")
OUT_NAMES = ("resc_dist", "resc_end", "resc_mate", "resc_pair_dist", "resc_span", "win_query", "win_begin", "win_text_id",
             "win_position")
NONE = 0xFFFFFFFF            # GDX_PAIR_NONE, GDX_CAND_NONE and GDX_RESCUE_NONE
NOT_TRIED = 0xFFFFFFFD
MAX_SPREAD = 4096
MAX_MATE_SLOTS = 32
A = alph.ascii_dna_with_n()


def _codes(alphabet, seqs):
    dense = np.asarray(alphabet.io_to_dense_table, dtype=np.uint8)
    return [dense[np.frombuffer(bytes(s), dtype=np.uint8)].astype(np.int64) for s in seqs]


def attempts_of(n_proper, mate_slot, n_pairs):
    """-> bool[2 n_pairs]: attempt (p, o) exists when the pair has no proper combination and the OTHER mate has a winner"""
    n = int(n_pairs)
    placed = (np.asarray(mate_slot).astype(np.int64).reshape(n, 2) != NONE)
    return ((np.asarray(n_proper).astype(np.int64).reshape(n, 1) == 0) & placed[:, ::-1]).reshape(-1)


def _anchor_view(queries_len, end, mate_slot, win_query, win_begin, win_text_id, win_position, n_pairs, mate_slots, lo, hi):
    """per mate 2p + o the numbers its attempt would use, from its anchor 2p + 1 - o -> dict of int64[2 n_pairs]"""
    n, ms = int(n_pairs), int(mate_slots)
    swap = np.arange(2 * n) ^ 1
    i64 = lambda x: np.asarray(x).astype(np.int64).reshape(-1)[:2 * n]  # noqa: E731
    slot, wq, wb, wt, wp = (i64(x)[swap] for x in (mate_slot, win_query, win_begin, win_text_id, win_position))
    mate = np.arange(2 * n)
    strand_a = wq & 1
    rq = 4 * (mate >> 1) + 2 * (mate & 1) + (1 - strand_a)
    L = np.asarray(queries_len, dtype=np.int64)[np.minimum(rq, max(4 * n - 1, 0))] if n else np.zeros(0, np.int64)
    diag_a = wp - wb
    slot_ok = slot < ms
    right_a = np.asarray(end).astype(np.int64).reshape(-1)[np.where(slot_ok, swap * ms + slot, 0)] if n else np.zeros(0, np.int64)
    ylo = np.where(strand_a == 0, diag_a + lo, right_a - hi + L)
    yhi = np.where(strand_a == 0, diag_a + hi, right_a - lo + L)
    return dict(slot_ok=slot_ok, strand_a=strand_a, rq=rq, L=L, T=wt, diag_a=diag_a, right_a=right_a, ylo=ylo, yhi=yhi)


def rescue_model(texts, alphabet, queries, end, n_proper, mate_slot, mate_dist, win_query, win_begin, win_text_id, win_position,
                 n_pairs, mate_slots, max_edits, min_insert, max_insert, batch=512):
    """-> the nine arrays of OUT_NAMES (resc_dist, resc_end and the four winner arrays of 2 n_pairs entries, the three per pair of
    n_pairs), u32 values in int64.  queries: the 4 n_pairs queries.  The attempts run side by side: the read's rows of every
    attempt as one matrix, one table column per step (min(diagonal, left) and a running minimum down the column), D[L][y] kept
    per column, then the least admissible one."""
    n, ms, k, lo, hi = int(n_pairs), int(mate_slots), int(max_edits), int(min_insert), int(max_insert)
    assert 1 <= ms <= MAX_MATE_SLOTS and k <= MAX_LEN and lo <= hi <= (1 << 31) - 1 and hi - lo <= MAX_SPREAD and len(queries) == 4 * n
    tq, tt = _codes(alphabet, queries), _codes(alphabet, texts)
    v = _anchor_view([q.size for q in tq], end, mate_slot, win_query, win_begin, win_text_id, win_position, n, ms, lo, hi)
    tried = attempts_of(n_proper, mate_slot, n)
    resc_dist = np.where(tried, k + 1, NOT_TRIED).astype(np.int64)
    resc_end = np.full(2 * n, NO_END, dtype=np.int64)
    todo = []
    for m in np.flatnonzero(tried):
        if v["T"][m] >= len(texts) or not v["slot_ok"][m]:
            resc_dist[m] = INVALID
        elif v["L"][m] > MAX_LEN:
            resc_dist[m] = TOO_LONG
        else:
            size = tt[v["T"][m]].size
            x0 = min(max(v["ylo"][m] - v["L"][m] - k, 0), size)
            x1 = min(max(v["yhi"][m], 0), size)
            todo.append((m, int(x0), int(x1)))
    for at in range(0, len(todo), batch):
        part = todo[at:at + batch]
        r = len(part)
        ms_ = np.array([m for m, _, _ in part])
        lens, x0 = v["L"][ms_], np.array([a for _, a, _ in part])
        width = np.array([b - a for _, a, b in part])
        Q = np.zeros((r, max(int(lens.max()), 1)), dtype=np.int64)                # padded with 0, which matches nothing
        W = np.zeros((r, max(int(width.max()), 1)), dtype=np.int64)
        for i, (m, a, b) in enumerate(part):
            Q[i, :lens[i]] = tq[v["rq"][m]]
            W[i, :b - a] = tt[v["T"][m]][a:b]
        searchable = (Q >= 1) & (Q <= 4)
        idx = np.arange(Q.shape[1] + 1)
        rows = np.arange(r)
        col = np.broadcast_to(idx, (r, idx.size)).copy()                          # D[i][x0] = i
        last = np.zeros((r, int(width.max()) + 1), dtype=np.int64)
        last[:, 0] = lens
        tmp = np.zeros_like(col)
        for j in range(int(width.max())):                                         # (columns past an attempt's window are masked below)
            mismatch = 1 - (searchable & (Q == W[:, j:j + 1]))
            tmp[:, 1:] = np.minimum(col[:, :-1] + mismatch, col[:, 1:] + 1)
            tmp[:, 0] = 0                                                         # D[0][y] = 0
            col = np.minimum.accumulate(tmp - idx, axis=1) + idx
            last[:, j + 1] = col[rows, lens]
        y = x0[:, None] + np.arange(last.shape[1])[None, :]
        ok = (np.arange(last.shape[1])[None, :] <= width[:, None]) & (y >= v["ylo"][ms_][:, None]) & (y <= v["yhi"][ms_][:, None])
        last = np.where(ok, last, 1 << 30)
        best, best_j = last.min(axis=1), last.argmin(axis=1)                      # the first: the smallest y wins
        found = best <= k
        resc_dist[ms_] = np.where(found, best, k + 1)
        resc_end[ms_] = np.where(found, x0 + best_j, NO_END)
    return (resc_dist, resc_end) + merge(v, resc_dist, resc_end, mate_dist, win_query, win_begin, win_text_id, win_position, n, k)


def merge(v, resc_dist, resc_end, mate_dist, win_query, win_begin, win_text_id, win_position, n_pairs, k):
    """the merge per pair and the final winners -> (resc_mate, resc_pair_dist, resc_span, win_query, win_begin, win_text_id,
    win_position)"""
    n = int(n_pairs)
    swap = np.arange(2 * n) ^ 1
    i64 = lambda x: np.asarray(x).astype(np.int64).reshape(-1)[:2 * n].copy()  # noqa: E731
    md, wq, wb, wt, wp = (i64(x) for x in (mate_dist, win_query, win_begin, win_text_id, win_position))
    success = resc_dist <= k
    score = np.where(success, (md[swap] + resc_dist) & 0xFFFFFFFF, 1 << 40).reshape(n, 2)
    pick = np.where(score[:, 1] < score[:, 0], 1, 0)                              # the least (score, o)
    any_ = success.reshape(n, 2).any(axis=1)
    resc_mate = np.where(any_, pick, NONE)
    at = 2 * np.arange(n) + pick                                                  # the rescued mate, where there is one
    y, L = resc_end[at], v["L"][at]
    span = np.where(v["strand_a"][at] == 0, y - v["diag_a"][at], v["right_a"][at] - (y - L))
    r = at[any_]
    wq[r], wb[r], wt[r], wp[r] = v["rq"][r], np.maximum(0, L - y)[any_], v["T"][r], np.maximum(0, y - L)[any_]
    return (resc_mate, np.where(any_, score[np.arange(n), pick], 2 * k + 2), np.where(any_, span & 0xFFFFFFFF, 0), wq, wb, wt, wp)


def rescue_naive(texts, alphabet, queries, end, n_proper, mate_slot, mate_dist, win_query, win_begin, win_text_id, win_position,
                 n_pairs, mate_slots, max_edits, min_insert, max_insert):
    """the same results pair by pair and cell by cell, in plain integers"""
    ms, k, lo, hi = int(mate_slots), int(max_edits), int(min_insert), int(max_insert)
    tq, tt = _codes(alphabet, queries), _codes(alphabet, texts)
    per_mate, per_pair, winners = [], [], []
    for p in range(int(n_pairs)):
        found = {}
        for o in (0, 1):
            a = 2 * p + 1 - o
            if int(n_proper[p]) != 0 or int(mate_slot[a]) == NONE:
                per_mate.append((NOT_TRIED, NO_END))
                continue
            strand_a, T = int(win_query[a]) & 1, int(win_text_id[a])
            rq = 4 * p + 2 * o + (1 - strand_a)
            q = [int(c) for c in tq[rq]]
            L = len(q)
            if T >= len(texts) or int(mate_slot[a]) >= ms:
                per_mate.append((INVALID, NO_END))
                continue
            if L > MAX_LEN:
                per_mate.append((TOO_LONG, NO_END))
                continue
            t = [int(c) for c in tt[T]]
            diag_a = int(win_position[a]) - int(win_begin[a])
            right_a = int(end[a * ms + int(mate_slot[a])])
            if strand_a == 0:
                ylo, yhi = diag_a + lo, diag_a + hi
            else:
                ylo, yhi = right_a - hi + L, right_a - lo + L
            x0, x1 = min(max(ylo - L - k, 0), len(t)), min(max(yhi, 0), len(t))
            D = [[0] * (x1 - x0 + 1) for _ in range(L + 1)]
            for i in range(L + 1):
                D[i][0] = i
            for i in range(1, L + 1):
                for j in range(1, x1 - x0 + 1):
                    same = q[i - 1] == t[x0 + j - 1] and 1 <= q[i - 1] <= 4
                    D[i][j] = min(D[i - 1][j - 1] + (0 if same else 1), D[i - 1][j] + 1, D[i][j - 1] + 1)
            best = None
            for y in range(max(ylo, x0), min(yhi, x1) + 1):
                if best is None or D[L][y - x0] < best[0]:
                    best = (D[L][y - x0], y)
            if best is None or best[0] > k:
                per_mate.append((k + 1, NO_END))
                continue
            per_mate.append(best)
            span = best[1] - diag_a if strand_a == 0 else right_a - (best[1] - L)
            found[o] = ((int(mate_dist[a]) + best[0], o), span, (rq, max(0, L - best[1]), T, max(0, best[1] - L)))
        both = [(int(win_query[m]), int(win_begin[m]), int(win_text_id[m]), int(win_position[m])) for m in (2 * p, 2 * p + 1)]
        if found:
            (score, o), span, cand = min(found.values())
            per_pair.append((o, score, span))
            both[o] = cand
        else:
            per_pair.append((NONE, 2 * k + 2, 0))
        winners += both
    cols = lambda rows, width: tuple(np.array(c, dtype=np.int64).reshape(-1) for c in zip(*rows)) if rows \
        else tuple(np.zeros(0, np.int64) for _ in range(width))  # noqa: E731
    return cols(per_mate, 2) + cols(per_pair, 3) + cols(winners, 4)


def assert_same(got, want, what):
    assert len(got) == len(want) == len(OUT_NAMES)
    for g, w, name in zip(got, want, OUT_NAMES):
        g, w = np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64)
        assert g.shape == w.shape, f"{what}: {name}: shape {g.shape} != {w.shape}"
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what}: {name} differs in {bad.size} entries, first at {bad[0]}: {g[bad[0]]} != {w[bad[0]]}"


# ------------------------------------------------------------------------------------------------
# random inputs: what gdx_pair_hits_many could have left, and reads planted around the admissible ends

def random_text(rng, n, n_rate=0.0):
    t = bytearray(b"ACGT"[i] for i in rng.integers(0, 4, n))
    for i in np.flatnonzero(rng.random(n) < n_rate):
        t[i] = ord("N")
    return bytes(t)


def random_rescue_case(rng, texts, n_pairs, mate_slots, k, lo, hi, lengths, p_open=0.7, p_placed=0.7, p_planted=0.8, n_rate=0.02,
                       bad=True):
    """n_pairs pairs as gdx_pair_hits_many could have left them, and their 4 n_pairs queries.  A pair is open (n_proper == 0) with
    p_open; a mate has a winner with p_placed: a strand, a text, a diagonal in [-6, |T|) on begin 0 .. 9 (a negative diagonal
    has position < begin), a slot whose end is the diagonal + 30 .. 70, a distance 0 .. k.  The query a possible attempt would
    search has one of `lengths` symbols and is, with p_planted, a piece of the anchor's text that ends at an admissible y drawn
    from [ylo - 3, yhi + 3] (so ends at and beyond both bounds occur), with 0 .. k + 1 edits and its length restored on the left;
    otherwise random.  With `bad` one anchor in fifty names a text that is not there and one in fifty a slot >= mate_slots.
    -> (queries, end, n_proper, mate_slot, mate_dist, win_query, win_begin, win_text_id, win_position)"""
    n, ms = int(n_pairs), int(mate_slots)
    lengths = list(lengths)
    sizes = np.array([len(t) for t in texts])
    n_proper = np.where(rng.random(n) < p_open, 0, rng.integers(1, 4, n))
    placed = rng.random(2 * n) < p_placed
    strand, T = rng.integers(0, 2, 2 * n), rng.integers(0, len(texts), 2 * n)
    diag = rng.integers(-6, sizes[T])
    wb = np.where(diag < 0, -diag + rng.integers(0, 3, 2 * n), rng.integers(0, 10, 2 * n))
    slot = rng.integers(0, ms, 2 * n)
    end = rng.integers(0, 1 << 20, 2 * n * ms)
    end[np.arange(2 * n) * ms + slot] = np.maximum(diag + rng.integers(30, 71, 2 * n), 0)
    if bad:
        T = np.where(placed & (rng.random(2 * n) < 0.02), len(texts) + rng.integers(0, 3, 2 * n), T)
        slot = np.where(placed & (rng.random(2 * n) < 0.02), ms + rng.integers(0, 3, 2 * n), slot)
    mate = np.arange(2 * n)
    wq = np.where(placed, 4 * (mate >> 1) + 2 * (mate & 1) + strand, NONE)
    queries = [random_text(rng, lengths[int(rng.integers(0, len(lengths)))], n_rate) for _ in range(4 * n)]
    for a in np.flatnonzero(placed):                                              # the query an attempt from anchor a would search
        if rng.random() >= p_planted or T[a] >= len(texts) or slot[a] >= ms:
            continue
        rq = 4 * (a >> 1) + 2 * ((a & 1) ^ 1) + (1 - strand[a])
        L, t = len(queries[rq]), texts[T[a]]
        right_a = int(end[a * ms + slot[a]])
        ylo, yhi = (diag[a] + lo, diag[a] + hi) if strand[a] == 0 else (right_a - hi + L, right_a - lo + L)
        y = int(rng.integers(ylo - 3, yhi + 4))
        piece = bytearray(t[max(0, min(y - L, len(t))):max(0, min(y, len(t)))])
        for _ in range(int(rng.integers(0, k + 2))):
            if not piece:
                break
            i, kind = int(rng.integers(0, len(piece))), int(rng.integers(0, 3))
            if kind == 0:
                piece[i] = b"ACGT"[int(rng.integers(0, 4))]
            elif kind == 1:
                piece.insert(i, b"ACGT"[int(rng.integers(0, 4))])
            else:
                del piece[i]
        piece = (random_text(rng, L, 0) + bytes(piece))[-L:] if L else b""
        if n_rate == 0:
            piece = piece.replace(b"N", b"A")                                     # (a batch without N stays one: it packs)
        queries[rq] = piece
    zero = lambda x: np.where(placed, x, 0)  # noqa: E731
    return (queries, end, n_proper, np.where(placed, slot, NONE), np.where(placed, rng.integers(0, k + 1, 2 * n), k + 1), wq,
            zero(wb), zero(T), zero(diag + wb))


# ------------------------------------------------------------------------------------------------
# (a) the model against the cell-by-cell programme

@pytest.mark.parametrize("k", (0, 2, 5))
def test_model_equals_the_cell_by_cell_programme(k):
    rng = np.random.default_rng(22000 + k)
    texts = [random_text(rng, 90, 0.03), random_text(rng, 7, 0), random_text(rng, 140, 0.03)]
    seen = np.zeros(6, dtype=np.int64)
    for ms, lo, hi, lengths in ((1, 20, 50, (12,)), (3, 0, 0, (0, 1, 9)), (5, 35, 36, (17, 25)), (32, 10, 90, (1, 30, 300))):
        case = random_rescue_case(rng, texts, 120, ms, k, lo, hi, lengths)
        want = rescue_naive(texts, A, *case, 120, ms, k, lo, hi)
        assert_same(rescue_model(texts, A, *case, 120, ms, k, lo, hi, batch=37), want, f"ms = {ms}, insert [{lo}, {hi}]")
        d, mate = want[0], want[2]
        seen += [(d <= k).sum(), (d == k + 1).sum(), (d == NOT_TRIED).sum(), (d == INVALID).sum(), (d == TOO_LONG).sum(),
                 ((mate != NONE) & (d.reshape(-1, 2) <= k).all(axis=1)).sum()]
    # the inputs show something: found, not found, not tried, both markers, and pairs in which two attempts succeed
    assert (seen > 0).all(), seen


# ------------------------------------------------------------------------------------------------
# (b) hand-worked cases

#       0         1         2         3         4         5         6         7
#       01234567890123456789012345678901234567890123456789012345678901234567890123456789
TEXT = b"TTGACCATGCGTAAGCTTCAGGATCCGTACGATTGCAACGGTCTAGCATCGATTACGGCTAAGTCCGATGCATGGCTAAC"
READ = TEXT[40:50]            # "GTCTAGCATC": ends at y = 50
assert len(TEXT) == 80 and TEXT.count(READ) == 1


def one_pair(queries, anchors, k, lo, hi, texts=(TEXT,), n_proper=0, ms=2):
    """queries: the four of the pair; anchors: per mate None or (win_query, win_begin, text, position, mate_dist, right end), its
    slot being ms - 1 -> both implementations' record of the pair: (resc_dist, resc_end) of mate 0, of mate 1, (resc_mate,
    resc_pair_dist, resc_span), the winner (query, begin, text, position) of mate 0 and of mate 1"""
    end = np.full(2 * ms, 777777, dtype=np.int64)
    cols = []
    for s, a in enumerate(anchors):
        if a is None:
            cols.append((NONE, 4, NONE, 0, 0, 0))
        else:
            end[s * ms + ms - 1] = a[5]
            cols.append((ms - 1, a[4], a[0], a[1], a[2], a[3]))
    slot, md, wq, wb, wt, wp = (np.array(c, dtype=np.int64) for c in zip(*cols))
    args = (list(texts), A, list(queries), end, np.array([n_proper]), slot, md, wq, wb, wt, wp, 1, ms, k, lo, hi)
    got = rescue_model(*args)
    assert_same(rescue_naive(*args), got, "hand-worked")
    g = [[int(x) for x in col] for col in got]
    return ((g[0][0], g[1][0]), (g[0][1], g[1][1]), (g[2][0], g[3][0], g[4][0]),
            (g[5][0], g[6][0], g[7][0], g[8][0]), (g[5][1], g[6][1], g[7][1], g[8][1]))


NOT = (NOT_TRIED, NO_END)
RC = alph.reverse_complement
Q4 = lambda q: [b"AAAA", b"TTTT", q, RC(q)]  # noqa: E731  (mate 0's strands say nothing; query 2 = q, query 3 = its reverse complement)


def test_a_forward_anchor_rescues_the_reverse_mate():
    # mate 0 forward (query 0) on diagonal 5 (position 7, begin 2): the searched query is 4p + 2 + 1 = 3 and y its right end;
    # insert [40, 50] admits y in [45, 55]; READ ends at 50: distance 0, span 50 - 5 = 45; the candidate's diagonal is 50 - 10
    anchor = (0, 2, 0, 7, 1, 35)
    r = one_pair([b"AAAA", b"TTTT", RC(READ), READ], (anchor, None), 2, 40, 50)
    assert r == (NOT, (0, 50), (1, 1, 45), (0, 2, 0, 7), (3, 0, 0, 40))
    # one substitution in the read: distance 1, score 2
    q = bytearray(READ)
    q[4] = ord("T")
    assert one_pair([b"A", b"T", b"C", bytes(q)], (anchor, None), 2, 40, 50)[1:3] == ((1, 50), (1, 2, 45))
    # y at ylo and at yhi, and one beyond each: [45, 50] and [50, 55] admit y = 50, [51, 60] and [40, 49] do not admit it
    for lo, hi, dist in ((45, 50, 0), (40, 45, 0), (46, 55, None), (35, 44, None)):
        r = one_pair([b"A", b"T", b"C", READ], (anchor, None), 0, lo, hi)
        assert r[1] == ((0, 50) if dist == 0 else (1, NO_END)), (lo, hi, r)
        assert r[2] == ((1, 1, 45) if dist == 0 else (NONE, 2, 0))
    # with k = 3 and y = 50 just outside [51, 60]: an alignment that ends at 51 pays one edit for the text symbol it takes in
    assert one_pair([b"A", b"T", b"C", READ], (anchor, None), 3, 46, 55)[1] == (1, 51)
    assert one_pair([b"A", b"T", b"C", READ], (anchor, None), 3, 35, 44)[1] == (1, 49)       # and the last symbol inserted


def test_a_reverse_anchor_rescues_the_forward_mate():
    # mate 1 reverse (query 7 of pair 1 would be; here pair 0: query 3) with right end 78: the searched query is 4p + 0 + 0 = 0,
    # forward, its diagonal y - L; insert [30, 40] admits y - 10 in [38, 48]: y in [48, 58]; READ's diagonal is 40: span 38
    anchor = (3, 0, 0, 68, 2, 78)
    r = one_pair([READ, b"T", b"C", b"G"], (None, anchor), 2, 30, 40)
    assert r == ((0, 50), NOT, (0, 2, 38), (0, 0, 0, 40), (3, 0, 0, 68))
    # the bounds: span 38 exactly at both ends, and one beyond each
    for lo, hi, found in ((38, 38, True), (38, 44, True), (30, 38, True), (39, 44, False), (30, 37, False)):
        r = one_pair([READ, b"T", b"C", b"G"], (None, anchor), 0, lo, hi)
        assert r[0] == ((0, 50) if found else (1, NO_END)), (lo, hi, r)
    # the anchor's right end comes from `end`, not from its diagonal: another end, another window
    assert one_pair([READ, b"T", b"C", b"G"], (None, (3, 0, 0, 68, 2, 300)), 2, 30, 40)[0] == (3, NO_END)


def test_windows_clipped_at_both_ends_of_the_text():
    # forward anchor on diagonal 0, insert [0, 12]: ylo = 0, x0 = clamp(0 - 10 - 2) = 0; the read TEXT[0:10] ends at 10
    anchor = (0, 0, 0, 0, 0, 30)
    assert one_pair(Q4(RC(TEXT[:10])), (anchor, None), 2, 0, 12)[1] == (0, 10)
    # a read that hangs over the start by three symbols pays three insertions: ends at 7 with distance 3
    over = b"CCC" + TEXT[:7]
    assert one_pair(Q4(RC(over)), (anchor, None), 3, 0, 12)[1] == (3, 7)
    assert one_pair(Q4(RC(over)), (anchor, None), 2, 0, 12)[1] == (3, NO_END)
    # the end of the text: diagonal 40, insert [35, 60] admits y up to 100, the text ends at 80: TEXT[70:80] ends at 80
    anchor = (0, 0, 0, 40, 0, 70)
    assert one_pair(Q4(RC(TEXT[70:])), (anchor, None), 2, 35, 60)[1] == (0, 80)
    # a neighbouring text would continue the alignment but must not: the read runs three symbols into the next text
    texts = (TEXT, b"GGG" + TEXT[:20])
    assert one_pair(Q4(RC(TEXT[73:] + b"GGG")), (anchor, None), 3, 35, 60, texts=texts)[1] == (3, 80)
    assert one_pair(Q4(RC(TEXT[73:] + b"GGG")), (anchor, None), 2, 35, 60, texts=texts)[1] == (3, NO_END)
    # the window lies wholly behind the text, or wholly in front of it: the admissible range is empty
    assert one_pair(Q4(RC(READ)), ((0, 0, 0, 79, 0, 70), None), 2, 40, 50)[1] == (3, NO_END)
    assert one_pair([READ, b"T", b"C", b"G"], (None, (3, 0, 0, 0, 0, 5)), 2, 40, 50)[0] == (3, NO_END)   # yhi = 5 - 40 + 10 < 0


def test_the_empty_read_and_a_negative_anchor_diagonal():
    # L = 0: D[0][y] = 0 everywhere, the least admissible y wins: ylo = 5 + 40
    anchor = (0, 2, 0, 7, 1, 35)
    r = one_pair([b"A", b"T", b"C", b""], (anchor, None), 2, 40, 50)
    assert r == (NOT, (0, 45), (1, 1, 40), (0, 2, 0, 7), (3, 0, 0, 45))
    assert one_pair([b"A", b"T", b"C", b""], ((0, 0, 0, 70, 1, 35), None), 2, 40, 50)[1] == (3, NO_END)   # ylo = 110 > |T|
    # position 2 < begin 9: the diagonal is -7, kept in 64 bits; insert [50, 60] admits y in [43, 53]; span 50 - (-7) = 57
    r = one_pair(Q4(RC(READ)), ((0, 9, 0, 2, 0, 30), None), 2, 50, 60)
    assert r == (NOT, (0, 50), (1, 0, 57), (0, 9, 0, 2), (3, 0, 0, 40))
    # the candidate of a read longer than its end: begin = L - end, position 0, the diagonal end - L kept exactly
    long_read = b"ACGTACG" + TEXT[:5]                                             # 12 symbols, ends at 5 after 7 inserted ones
    r = one_pair(Q4(RC(long_read)), ((0, 0, 0, 0, 0, 30), None), 7, 0, 9)
    assert r[1] == (7, 5) and r[4] == (3, 7, 0, 0)


def test_two_attempts_and_the_tie_rule():
    # both mates placed, no proper combination (both forward): each is the other's anchor.  Mate 0 forward on diagonal 5 searches
    # query 3 (READ, distance 0); mate 1 forward on diagonal 10 searches query 1 (TEXT[55:65] with one substitution, distance 1)
    other = bytearray(TEXT[55:65])
    other[3] = ord("A") if other[3] != ord("A") else ord("C")
    queries = [b"A", bytes(other), b"C", READ]
    m0, m1 = (0, 2, 0, 7, 1, 35), (2, 0, 0, 10, 0, 40)
    r = one_pair(queries, (m0, m1), 2, 40, 60)
    # attempt o = 1 scores mate_dist[0] + 0 = 1, attempt o = 0 scores mate_dist[1] + 1 = 1: a tie, the smaller o wins
    assert r[0] == (1, 65) and r[1] == (0, 50) and r[2] == (0, 1, 55)
    assert r[3] == (1, 0, 0, 55) and r[4] == (2, 0, 0, 10)
    # one edit more on the anchor of attempt 0 and attempt 1 wins
    r = one_pair(queries, (m0, (2, 0, 0, 10, 1, 40)), 2, 40, 60)
    assert r[2] == (1, 1, 45) and r[3] == (0, 2, 0, 7) and r[4] == (3, 0, 0, 40)
    # a pair with a proper combination is not tried, and its winners pass through
    assert one_pair(queries, (m0, m1), 2, 40, 60, n_proper=1) == (NOT, NOT, (NONE, 6, 0), (0, 2, 0, 7), (2, 0, 0, 10))
    assert one_pair(queries, (None, None), 2, 40, 60) == (NOT, NOT, (NONE, 6, 0), (NONE, 0, 0, 0), (NONE, 0, 0, 0))


def test_an_n_on_either_side_never_matches():
    anchor = (0, 2, 0, 7, 1, 35)
    q = bytearray(READ)
    q[5] = ord("N")
    assert one_pair([b"A", b"T", b"C", bytes(q)], (anchor, None), 2, 40, 50)[1] == (1, 50)
    t = bytearray(TEXT)
    t[45] = ord("N")
    assert one_pair([b"A", b"T", b"C", READ], (anchor, None), 2, 40, 50, texts=(bytes(t),))[1] == (1, 50)
    assert one_pair([b"A", b"T", b"C", bytes(q)], (anchor, None), 2, 40, 50, texts=(bytes(t),))[1] == (1, 50)   # N against N


def test_the_markers():
    anchor = (0, 2, 0, 7, 1, 35)
    assert one_pair([b"A", b"T", b"C", b"ACGT" * 65], (anchor, None), 2, 40, 50)[1] == (TOO_LONG, NO_END)
    assert one_pair([b"A", b"T", b"C", READ], ((0, 2, 1, 7, 1, 35), None), 2, 40, 50)[1:3] == ((INVALID, NO_END), (NONE, 6, 0))
    r = one_pair([b"A", b"T", b"C", b"ACGT" * 64], (anchor, None), 256, 40, 50)        # 256 symbols, k = 256: all inserted
    assert r[1][0] <= 256 and r[2][0] == 1


# ------------------------------------------------------------------------------------------------
# (c) planted pairs for the end-to-end test

PLANTED = dict(text_len=3000, fragment=(200, 400), mate_len=60, subs=(7, 22, 37, 52), min_length=19, max_edits=5, min_insert=150,
               max_insert=450, max_smems=16, max_occ=8, band=8, max_candidates=2)


def planted_pairs(rng, text, n_pairs):
    """n_pairs fragments of the text; mate 0 = the first 60 symbols, mate 1 = the reverse complement of the last 60; in every
    second pair the two change places.  One mate of each pair (alternating with p // 2) carries substitutions at read positions
    7, 22, 37 and 52, so none of its exact stretches reaches 19 symbols -> (reads, mates interleaved; per pair the damaged mate;
    per read (the diagonal its forward form was taken from, strand))"""
    ln = PLANTED["mate_len"]
    reads, damaged, origin = [], [], []
    for p in range(n_pairs):
        size = int(rng.integers(PLANTED["fragment"][0], PLANTED["fragment"][1] + 1))
        start = int(rng.integers(0, len(text) - size + 1))
        first, last = bytearray(text[start:start + ln]), bytearray(text[start + size - ln:start + size])
        hurt = (p // 2) % 2                                                       # 0: the fragment's first mate, 1: its last
        for i in PLANTED["subs"]:
            piece = (first, last)[hurt]
            at = i if hurt == 0 else ln - 1 - i                                   # read positions: the last mate is reversed
            piece[at] = b"ACGT"[(b"ACGT".index(piece[at]) + 1 + int(rng.integers(0, 3))) % 4]
        mates = [(bytes(first), (start, 0)), (RC(bytes(last)), (start + size - ln, 1))]
        order = mates[::-1] if p % 2 else mates
        for read, where in order:
            reads.append(read), origin.append(where)
        damaged.append(hurt ^ (p % 2))
    return reads, damaged, origin


def test_the_model_rescues_every_planted_pair():
    rng = np.random.default_rng(22100)
    text = random_text(rng, PLANTED["text_len"])
    n, k, ln = 200, PLANTED["max_edits"], PLANTED["mate_len"]
    reads, damaged, origin = planted_pairs(rng, text, n)
    # the damaged mate has no exact stretch of min_length symbols
    for p in range(n):
        read, (diag, strand) = reads[2 * p + damaged[p]], origin[2 * p + damaged[p]]
        fwd = read if strand == 0 else RC(read)
        same = np.frombuffer(fwd, dtype=np.uint8) == np.frombuffer(text[diag:diag + ln], dtype=np.uint8)
        runs = np.diff(np.flatnonzero(np.concatenate([[True], ~same, [True]]))) - 1
        assert (~same).sum() == 4 and runs.max() < PLANTED["min_length"]
    got = rescue_model(*planted_args(text, reads, damaged, origin))
    diag, strand = (np.array([o[i] for o in origin]) for i in (0, 1))
    hurt = 2 * np.arange(n) + np.array(damaged)
    assert (got[2] == np.array(damaged)).all() and (got[0][hurt] == 4).all() and (got[3] == 4).all()
    assert (got[1][hurt] == diag[hurt] + ln).all()                                # the end at the origin, both anchor strands
    assert (got[5][hurt] == 2 * hurt + strand[hurt]).all() and (got[8][hurt] == diag[hurt]).all()
    assert set(strand[hurt ^ 1]) == {0, 1}
    few = 24                                                                      # the first pairs once more, cell by cell
    want = rescue_naive(*planted_args(text, reads[:2 * few], damaged[:few], origin[:2 * few]))
    assert_same(tuple(g[:few] if name in OUT_NAMES[2:5] else g[:2 * few] for g, name in zip(got, OUT_NAMES)), want, "cell by cell")


def planted_args(text, reads, damaged, origin):
    """what the pairing leaves of planted pairs -- the intact mate alone, placed exactly, in slot 1 of 4 -- as the arguments of
    rescue_model"""
    n, k, ln = len(damaged), PLANTED["max_edits"], PLANTED["mate_len"]
    qs = [q for r in reads for q in (r, RC(r))]
    mate = np.arange(2 * n)
    placed = np.repeat(np.array(damaged), 2) != (mate & 1)
    diag, strand = (np.array([o[i] for o in origin]) for i in (0, 1))
    end = np.zeros(2 * n * 4, dtype=np.int64)
    end[mate * 4 + 1] = diag + ln
    return ([text], A, qs, end, np.zeros(n), np.where(placed, 1, NONE), np.where(placed, 0, k + 1),
            np.where(placed, 2 * mate + strand, NONE), np.zeros(2 * n), np.zeros(2 * n), np.where(placed, diag, 0), n, 4, k,
            PLANTED["min_insert"], PLANTED["max_insert"])


# ------------------------------------------------------------------------------------------------
# (d) the two calls are declared everywhere a binding looks for them

def test_header_library_stub_and_rust_binding_have_both_calls():
    from genedex_amd import _lib
    from test_candidates_model import _header_arg_counts

    counts = _header_arg_counts("gdx_experimental.h")
    assert counts.get("gdx_mate_rescue_many") == 24 and counts.get("gdx_mate_rescue_many_dev") == 26
    assert "gdx_mate_rescue_many" not in _header_arg_counts("gdx.h")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    rust = open(os.path.join(ROOT, "bindings", "rust", "gdx.rs")).read()
    for name in NAMES:
        assert hasattr(lib, name), name + " is not exported by libgdx.so"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == counts[name], name
        assert re.search(r"pub fn " + name + r"\s*\(", rust), name
    assert re.search(r"pub fn mate_rescue_many\b", rust)  # the safe wrapper of GpuFmIndex
    header = open(os.path.join(ROOT, "include", "gdx_experimental.h")).read()
    for name, text, value in (("GDX_RESCUE_NONE", "0xFFFFFFFFu", NONE), ("GDX_RESCUE_NOT_TRIED", "0xFFFFFFFDu", NOT_TRIED),
                              ("GDX_RESCUE_MAX_SPREAD", "4096u", MAX_SPREAD)):
        assert re.search(r"#define\s+" + name + r"\s+" + text + r"\s", header), name
        assert getattr(_lib, name) == value, name
        assert re.search(r"pub const " + name + r": u\d+ = ", rust), name
    # the pairing's text points at the new call instead of listing the rescue as out of scope
    assert "gdx_mate_rescue_many below" in header
