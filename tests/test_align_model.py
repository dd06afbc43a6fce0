"""The CPU model of gdx_align_many (alignment traceback of verified seed hits), written straight from the definition in
include/gdx.h with a plain table on bytes and the alphabet's io_to_dense table -- no index, no bit vectors, nothing of the
library --, a replay checker that knows nothing of the table, the model's check against the edit-distance model and against
hand-worked cases, and the ABI bookkeeping of the two new calls (header, library, ctypes stub, Rust declarations).
tests/test_gpu_align.py holds the GPU against this model."""
import ctypes
import os
import re

import numpy as np

from genedex_amd import alphabet as alph
from test_edit_distance_model import INVALID, MAX_LEN, NO_END, T0, T1, TOO_LONG, _header_arg_counts, edit_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gdx_align_many", "gdx_align_many_dev")
INS, DEL, EQ, DIFF = 1, 2, 7, 8
OP_CHAR = {INS: "I", DEL: "D", EQ: "=", DIFF: "X"}
A = alph.ascii_dna_with_n()


def align_model(texts, alphabet, queries, cand_query, cand_begin, hits, max_edits, batch=64):
    """(dist, begin, end, n_cigar, cigar[m, 2 k + 1]), uint32 arrays; cigar is zero from n_cigar on.  Candidate c: q, T, the
    window T[x0, x1) and the markers as in edit_model.  The table D[i][y], 0 <= i <= L, x0 <= y <= x1: D[0][y] = 0, D[i][x0] = i,
    D[i][y] = min(D[i-1][y-1] + mismatch, D[i-1][y] + 1, D[i][y-1] + 1); dist = min_y D[L][y], end = the smallest such y.  When
    dist <= k the walk from (L, end) takes the first rule that applies: 1. y > x0 and a match: '=' to (i-1, y-1); 2. y > x0 and
    D[i-1][y-1] + 1 == D[i][y]: 'X' to (i-1, y-1); 3. D[i-1][y] + 1 == D[i][y]: 'I' to (i-1, y); 4. 'D' to (i, y-1), where
    y > x0 and D[i][y-1] + 1 == D[i][y] are asserted.  begin = the y at i == 0.  The whole table of a batch of candidates is kept
    (tab[r, y - x0, i]); columns follow from their left neighbour by min(diagonal, left) and a running minimum down the column."""
    dense = np.asarray(alphabet.io_to_dense_table, dtype=np.uint8)
    tq = [dense[np.frombuffer(bytes(q), dtype=np.uint8)].astype(np.int64) for q in queries]
    tt = [dense[np.frombuffer(bytes(t), dtype=np.uint8)].astype(np.int64) for t in texts]
    m, k = len(cand_query), int(max_edits)
    dist = np.zeros(m, dtype=np.uint32)
    begin = np.full(m, NO_END, dtype=np.uint32)
    end = np.full(m, NO_END, dtype=np.uint32)
    n_cigar = np.zeros(m, dtype=np.uint32)
    cigar = np.zeros((m, 2 * k + 1), dtype=np.uint32)
    todo = []
    for c, (qi, b, (text_id, position)) in enumerate(zip(cand_query, cand_begin, hits)):
        qi, b, text_id, position = int(qi), int(b), int(text_id), int(position)
        if qi >= len(queries) or text_id >= len(texts):
            dist[c] = INVALID
        elif tq[qi].size > MAX_LEN:
            dist[c] = TOO_LONG
        else:
            n, s, ln = tt[text_id].size, position - b, tq[qi].size
            todo.append((c, qi, text_id, min(max(s - k, 0), n), min(max(s + ln + k, 0), n)))
    for at in range(0, len(todo), batch):
        part = todo[at:at + batch]
        n = len(part)
        lens = np.array([tq[qi].size for _, qi, _, _, _ in part])
        x0 = np.array([a for _, _, _, a, _ in part])
        width = np.array([b - a for _, _, _, a, b in part])
        Q = np.zeros((n, max(int(lens.max()), 1)), dtype=np.int64)        # padded with 0, which matches nothing
        W = np.zeros((n, max(int(width.max()), 1)), dtype=np.int64)
        for r, (_, qi, text_id, a, b) in enumerate(part):
            Q[r, :lens[r]] = tq[qi]
            W[r, :b - a] = tt[text_id][a:b]
        searchable = (Q >= 1) & (Q <= 4)
        idx = np.arange(Q.shape[1] + 1)
        tab = np.zeros((n, int(width.max()) + 1, idx.size), dtype=np.int64)
        tab[:, 0, :] = idx
        tmp = np.zeros((n, idx.size), dtype=np.int64)
        for j in range(int(width.max())):                                 # (columns past a candidate's window are never read)
            mismatch = 1 - (searchable & (Q == W[:, j:j + 1]))
            tmp[:, 1:] = np.minimum(tab[:, j, :-1] + mismatch, tab[:, j, 1:] + 1)
            tab[:, j + 1, :] = np.minimum.accumulate(tmp - idx, axis=1) + idx
        rows = np.arange(n)
        last = tab[rows, :, lens].copy()                                  # D[L][y] of every column
        last[np.arange(last.shape[1])[None, :] > width[:, None]] = 1 << 30
        best = last.min(axis=1)
        best_j = last.argmin(axis=1)                                      # the first: the leftmost end wins
        # the walk, every candidate of the batch at its own cell
        walking = best <= k
        i, j = np.where(walking, lens, 0), best_j.copy()
        steps = []
        while (i > 0).any():
            on = i > 0
            i1, j1 = np.maximum(i - 1, 0), np.maximum(j - 1, 0)
            d = tab[rows, j, i]
            in_text = on & (j > 0)
            match = in_text & searchable[rows, i1] & (Q[rows, i1] == W[rows, j1])
            assert (tab[rows, j1, i1][match] == d[match]).all()
            rule2 = in_text & ~match & (tab[rows, j1, i1] + 1 == d)
            rule3 = on & ~match & ~rule2 & (tab[rows, j, i1] + 1 == d)
            rule4 = on & ~match & ~rule2 & ~rule3
            assert (j[rule4] > 0).all() and (tab[rows, j1, i][rule4] + 1 == d[rule4]).all()
            steps.append(np.where(match, EQ, np.where(rule2, DIFF, np.where(rule3, INS, np.where(rule4, DEL, 0)))))
            i = i - (match | rule2 | rule3)
            j = j - (match | rule2 | rule4)
        steps = np.array(steps).reshape(len(steps), n)
        for r, (c, _, _, _, _) in enumerate(part):
            if not walking[r]:
                dist[c] = k + 1
                continue
            dist[c], begin[c], end[c] = best[r], x0[r] + j[r], x0[r] + best_j[r]
            ops = steps[:, r][steps[:, r] != 0][::-1]                     # from the read's first symbol to its last
            if ops.size:
                cut = np.flatnonzero(np.diff(ops)) + 1
                starts = np.concatenate([[0], cut])
                run_len = np.diff(np.concatenate([starts, [ops.size]]))
                n_cigar[c] = starts.size
                cigar[c, :starts.size] = (run_len << 4) | ops[starts]
    return dist, begin, end, n_cigar, cigar


def runs_of(n_cigar, cigar_row):
    return [(int(w) >> 4, int(w) & 15) for w in cigar_row[:int(n_cigar)]]


def sam(runs):
    return "".join("%d%s" % (n, OP_CHAR[op]) for n, op in runs)


def replay(alphabet, q, t, begin, end, runs, dist):
    """the runs as an edit script of q against t[begin, end): they consume exactly both, '=' sits on matching pairs only and 'X'
    on pairs that do not match, the ops other than '=' number dist, adjacent runs differ, there are at most 2 dist + 1 of them
    and neither end is 'D'.  Knows nothing of the table."""
    dense = alphabet.io_to_dense_table
    assert 0 <= begin <= end <= len(t)
    i, y, cost = 0, begin, 0
    for n, op in runs:
        assert n >= 1 and op in OP_CHAR
        for _ in range(n):
            if op in (EQ, DIFF):
                assert i < len(q) and y < end
                a, b = dense[q[i]], dense[t[y]]
                assert (a == b and 1 <= a <= 4) == (op == EQ), (i, y, op)
                i, y = i + 1, y + 1
            elif op == INS:
                assert i < len(q)
                i += 1
            else:
                assert y < end
                y += 1
            cost += op != EQ
    assert i == len(q) and y == end, (i, y)
    assert cost == dist
    assert all(a[1] != b[1] for a, b in zip(runs, runs[1:]))
    assert len(runs) <= 2 * dist + 1
    assert not runs or (runs[0][1] != DEL and runs[-1][1] != DEL)
    return True


def replay_all(alphabet, texts, queries, cand_query, hits, result):
    """replay() on every alignment of a result -> how many there were; rows without one hold the markers"""
    dist, begin, end, n_cigar, cigar = result
    count = 0
    for c in range(len(cand_query)):
        if end[c] == NO_END:
            assert begin[c] == NO_END and n_cigar[c] == 0, c
            continue
        replay(alphabet, queries[int(cand_query[c])], texts[int(hits[c][0])], int(begin[c]), int(end[c]),
               runs_of(n_cigar[c], cigar[c]), int(dist[c]))
        count += 1
    return count


def table(alphabet, q, t):
    """the plain table of q against the whole of t (x0 = 0), one cell at a time: D[i][y]"""
    dense = alphabet.io_to_dense_table
    D = [[0] * (len(t) + 1) for _ in range(len(q) + 1)]
    for i in range(1, len(q) + 1):
        D[i][0] = i
        for y in range(1, len(t) + 1):
            a, b = dense[q[i - 1]], dense[t[y - 1]]
            D[i][y] = min(D[i - 1][y - 1] + (0 if (a == b and 1 <= a <= 4) else 1), D[i - 1][y] + 1, D[i][y - 1] + 1)
    return D


# ------------------------------------------------------------------------------------------------
# (a) the model against the edit-distance model, and the replay checker on all it returns

def test_dist_and_end_equal_the_edit_distance_model_and_every_alignment_replays():
    rng = np.random.default_rng(12100)                  # the generator of test_the_model_equals_a_plain_dynamic_programme
    symbols = b"ACGT" * 5 + b"N"
    texts = [bytes(symbols[i] for i in rng.integers(0, len(symbols), n)) for n in (90, 0, 1, 47)]
    qs, cq, cb, hits = [], [], [], []
    for i in range(400):
        text_id = int(rng.integers(0, len(texts)))
        t = texts[text_id]
        ln = int(rng.integers(0, 25))
        start = int(rng.integers(-8, len(t) + 8))
        q = bytearray()
        p = start
        while len(q) < ln:                              # the text from `start` on, with edits of all three kinds
            r = int(rng.integers(0, 12))
            if r == 1:                                  # a symbol the text does not have
                q.append(b"ACGT"[int(rng.integers(0, 4))])
                continue
            if r == 0:
                q.append(b"ACGTN#"[int(rng.integers(0, 6))])
            elif r != 2:                                # (2: the read skips a text symbol)
                q.append(t[p] if 0 <= p < len(t) else b"ACGT"[int(rng.integers(0, 4))])
            p += 1
        b = int(rng.integers(0, ln + 3))
        qs.append(bytes(q)), cq.append(i), cb.append(b), hits.append((text_id, max(start + b + int(rng.integers(-2, 3)), 0)))
    ops_seen, most_runs = set(), False
    for k in (0, 1, 2, 5, 40):
        got = align_model(texts, A, qs, cq, cb, hits, k)
        dist, end = edit_model(texts, A, qs, cq, cb, hits, k)
        assert np.array_equal(got[0], dist) and np.array_equal(got[2], end), k
        assert all(x.dtype == np.uint32 for x in got) and got[4].shape == (400, 2 * k + 1)
        assert replay_all(A, texts, qs, cq, hits, got) == int((end != NO_END).sum())
        assert (got[1][end != NO_END] <= end[end != NO_END]).all()
        for c in np.flatnonzero(end != NO_END):
            runs = runs_of(got[3][c], got[4][c])
            ops_seen.update(op for _, op in runs)
            most_runs |= got[0][c] > 0 and len(runs) == 2 * got[0][c] + 1
            assert not got[4][c, got[3][c]:].any()
    assert ops_seen == {INS, DEL, EQ, DIFF} and most_runs        # all four ops occur and the bound on the runs is reached


# ------------------------------------------------------------------------------------------------
# (b) cases worked by hand

def one(texts, q, begin, text_id, position, k):
    """-> (dist, begin, end, SAM string or None)"""
    got = align_model(texts, A, [q], [0], [begin], [(text_id, position)], k)
    dist, end = edit_model(texts, A, [q], [0], [begin], [(text_id, position)], k)
    assert (got[0][0], got[2][0]) == (dist[0], end[0])
    if got[2][0] == NO_END:
        assert got[1][0] == NO_END and got[3][0] == 0
        return int(got[0][0]), NO_END, NO_END, None
    runs = runs_of(got[3][0], got[4][0])
    replay(A, q, texts[text_id], int(got[1][0]), int(got[2][0]), runs, int(got[0][0]))
    return int(got[0][0]), int(got[1][0]), int(got[2][0]), sam(runs)


def test_identical_window_and_one_substitution():
    assert one([T0], T0[3:15], 0, 0, 3, 2) == (0, 3, 15, "12=")
    assert one([T0], T0[3:15], 5, 0, 8, 2) == (0, 3, 15, "12=")
    assert one([T0], b"ACGTTGCTAGG", 0, 0, 0, 2) == (1, 0, 11, "7=1X3=")
    assert one([T0], b"ACGTTGCTAGG", 0, 0, 0, 0) == (1, NO_END, NO_END, None)


def test_one_inserted_read_symbol_and_one_deleted_text_symbol():
    q = T0[2:7] + b"T" + T0[7:12]                                 # GTTGC T AAGGC: a T the text does not have
    assert one([T0], q, 0, 0, 2, 1) == (1, 2, 12, "5=1I5=")
    assert one([T0], q, 8, 0, 9, 1) == (1, 2, 12, "5=1I5=")       # ... named by a seed behind the insertion
    q = T0[2:7] + T0[8:14]                                        # GTTGC . AGGCTT: the read skips T0[7]
    assert one([T0], q, 0, 0, 2, 1) == (1, 2, 14, "5=1D6=")
    assert one([T0], q, 7, 0, 10, 1) == (1, 2, 14, "5=1D6=")


def test_overhang_is_a_run_of_insertions_at_that_end():
    assert one([T0], b"GG" + T0[:6], 2, 0, 0, 2) == (2, 0, 6, "2I6=")         # two read symbols in front of the text
    assert one([T0], T0[17:] + b"CA", 0, 0, 17, 2) == (2, 17, 22, "5=2I")     # two symbols past the end
    assert one([T0], T0[17:] + b"CA", 2, 0, 19, 1) == (2, NO_END, NO_END, None)


def test_n_against_n_is_a_substitution():
    t = b"ACGNNACGT"
    assert one([t], b"ACGNNACGT", 0, 0, 0, 3) == (2, 0, 9, "3=2X4=")
    assert one([t], b"ACGAAACGT", 0, 0, 0, 3) == (2, 0, 9, "3=2X4=")
    assert one([T0], b"AC#TT", 0, 0, 0, 2) == (1, 0, 5, "2=1X2=")


def test_the_leftmost_end_the_empty_read_and_the_empty_text():
    assert one([b"ACAC"], b"AC", 0, 0, 2, 2) == (0, 0, 2, "2=")               # both AC cost 0: the leftmost end
    assert one([b"ACAC"], b"AC", 0, 0, 2, 0) == (0, 2, 4, "2=")               # ... unless the window holds only the second
    assert one([T0], b"", 7, 0, 3, 2) == (0, 0, 0, "")                        # the empty read: begin == end == x0, no run
    assert one([T0], b"", 0, 0, 5, 2) == (0, 3, 3, "") and one([T0], b"", 0, 0, 5, 0) == (0, 5, 5, "")
    texts = [T0, T1, b"", b"G"]
    assert one(texts, b"ACG", 0, 2, 0, 5) == (3, 0, 0, "3I")                  # an empty text with k >= L
    assert one(texts, b"ACG", 0, 2, 0, 2) == (3, NO_END, NO_END, None)
    assert one([T0], T0[:10], 0, 0, 0xFFFFFFFF, 10) == (10, 22, 22, "10I")    # an empty window at the text's end


def test_rows_without_an_alignment_hold_the_markers():
    long_read = (T0 * 12)[:257]
    got = align_model([T0], A, [long_read, long_read[:256], b"T"], [0, 1, 3, 2, 2], [0] * 5,
                      [(0, 0), (0, 0), (0, 0), (1, 0), (0, 3)], 3)
    assert got[0].tolist() == [TOO_LONG, 4, INVALID, INVALID, 0]
    assert got[1].tolist() == [NO_END, NO_END, NO_END, NO_END, 3] and got[2].tolist() == [NO_END, NO_END, NO_END, NO_END, 4]
    assert got[3].tolist() == [0, 0, 0, 0, 1] and got[4][4, 0] == (1 << 4 | EQ) and got[4].shape == (5, 7)
    assert not got[4][:4].any()


def test_a_tie_that_only_the_rule_order_decides():
    """read AC against text GC: after the '=' of the two C the walk stands at (1, 1), where A / G does not match and both
    D[0][0] + 1 == D[1][1] (rule 2, 'X', begin 0) and D[0][1] + 1 == D[1][1] (rule 3, 'I', begin 1) hold: 'X' is taken"""
    q, t = b"AC", b"GC"
    D = table(A, q, t)
    assert D[2].index(min(D[2])) == 2 and D[2][2] == 1 and D[1][1] == D[2][2]      # ends at (2, 2); the '=' leads to (1, 1)
    assert D[0][0] + 1 == D[1][1] and D[0][1] + 1 == D[1][1]                         # both equalities hold there
    assert one([t], q, 0, 0, 0, 1) == (1, 0, 2, "1X1=")
    replay(A, q, t, 1, 2, [(1, INS), (1, EQ)], 1)                                    # (the other choice is an alignment too)


# ------------------------------------------------------------------------------------------------
# (c) the two calls are declared everywhere a binding looks for them

def test_header_library_stub_and_rust_binding_have_both_calls():
    from genedex_amd import _lib

    counts = _header_arg_counts()
    assert counts.get("gdx_align_many") == 14 and counts.get("gdx_align_many_dev") == 19
    lib = ctypes.CDLL(_lib.LIB_PATH)
    rust = open(os.path.join(ROOT, "bindings", "rust", "gdx.rs")).read()
    for name in NAMES:
        assert hasattr(lib, name), name + " is not exported by libgdx.so"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == counts[name], name
        assert re.search(r"pub fn " + name + r"\s*\(", rust), name
    assert re.search(r"pub fn align_many\b", rust)  # the safe wrapper of GpuFmIndex
    header = open(os.path.join(ROOT, "include", "gdx.h")).read()
    for name, value in (("GDX_CIGAR_INS", INS), ("GDX_CIGAR_DEL", DEL), ("GDX_CIGAR_EQ", EQ), ("GDX_CIGAR_DIFF", DIFF)):
        assert re.search(r"#define\s+" + name + r"\s+%du" % value, header), name
        assert getattr(_lib, name) == value, name
        assert re.search(r"pub const " + name + r": u32 = %d;" % value, rust), name


def test_the_alignment_tuple_and_its_sam_string():
    import genedex_amd

    al = genedex_amd.Alignment(1, 2, 12, "5=1I5=")
    assert (al.dist, al.begin, al.end, al.cigar) == (1, 2, 12, "5=1I5=") and genedex_amd.Alignment._fields == ("dist", "begin", "end", "cigar")
    words = np.array([5 << 4 | EQ, 1 << 4 | INS, 5 << 4 | EQ, 0x5A5A5A5A], dtype=np.uint32)
    assert genedex_amd.index.cigar_string(words[:3]) == "5=1I5=" and genedex_amd.index.cigar_string(words[:0]) == ""
