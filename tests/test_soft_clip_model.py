"""The model of gdx_soft_clip_many[_dev] (include/gdx_experimental.h "soft clipping"), written from the header's definition as a
brute force over all run intervals, and its own checks: a single-pass variant against the brute force on random rows, the hand
cases (shared with tests/test_gpu_soft_clip.py), the invariants of kept rows, and that header, library, stub and Rust binding
name both calls."""
import ctypes
import os
import re

import numpy as np

from test_edit_distance_model import INVALID, NO_END, TOO_LONG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gdx_soft_clip_many", "gdx_soft_clip_many_dev")
OUT_NAMES = ("score", "dist", "begin", "end", "clip_left", "clip_right", "n_cigar", "cigar", "status")
INS, DEL, SOFT, EQ, DIFF = 1, 2, 4, 7, 8
NO_SCORE = -0x80000000        # GDX_CLIP_NO_SCORE as the i32 it is stored as
BAD_CIGAR = 1
MAX_RUN_SUM = 65536
MAX_SCORE_PARAM = 1024
OPS = "MIDNSHP=X"
DEFAULT = (1, 4, 6, 1)        # the scoring of the hand cases


def run_value(op, ln, scoring):
    match, mismatch, gap_open, gap_extend = scoring
    return match * ln if op == EQ else -mismatch * ln if op == DIFF else -(gap_open + gap_extend * ln)


def best_interval(values):
    """step 3 as it is written: over all 0 <= i <= j < n the greatest sum, then the smallest i, then the greatest j -> (best, i, j)"""
    best = None
    for i in range(len(values)):
        s = 0
        for j in range(i, len(values)):
            s += values[j]
            key = (s, -i, j)
            if best is None or key > best:
                best = key
    return best[0], -best[1], best[2]


def best_interval_single_pass(values):
    """the same in one pass: for every j the least prefix sum at or before it (the earliest on ties) is its best i"""
    best, prefix, low, low_at = None, 0, 0, 0
    for j, v in enumerate(values):
        if prefix < low:
            low, low_at = prefix, j
        prefix += v
        key = (prefix - low, -low_at, j)
        if best is None or key > best:
            best = key
    return best[0], -best[1], best[2]


def clip_model(dist, begin, end, n_cigar, cigar, k, match, mismatch, gap_open, gap_extend, min_score=0, fill=0, single_pass=False):
    """-> the nine outputs in the order of OUT_NAMES.  cigar: m rows of 2k + 1 words; the words of an output row from out_n_cigar on
    hold `fill` (a number, or an array of the output's shape: what the caller's row held)"""
    scoring = (match, mismatch, gap_open, gap_extend)
    assert k <= 256 and all(1 <= x <= MAX_SCORE_PARAM for x in (match, mismatch, gap_extend)) and 0 <= gap_open <= MAX_SCORE_PARAM
    assert 0 <= min_score <= 1 << 30
    m, stride = len(dist), 2 * k + 1
    cigar = np.asarray(cigar, dtype=np.uint32).reshape(m, stride)
    score = np.zeros(m, dtype=np.int32)
    out = {name: np.zeros(m, dtype=np.uint32) for name in OUT_NAMES[1:7]}
    out_cigar = np.broadcast_to(np.asarray(fill, dtype=np.uint32), (m, stride)).copy()
    status = np.zeros(m, dtype=np.uint8)
    interval = best_interval_single_pass if single_pass else best_interval

    def none(c, d, s):
        out["begin"][c] = out["end"][c] = NO_END
        out["dist"][c], score[c] = d, s

    for c in range(m):
        b, e, n = int(begin[c]), int(end[c]), int(n_cigar[c])
        if e == NO_END:                                                           # 1.
            none(c, int(dist[c]), NO_SCORE)
            continue
        runs = [(int(w) & 15, int(w) >> 4) for w in cigar[c][:n]] if n <= stride else []
        if (n > stride or any(op not in (INS, DEL, EQ, DIFF) or ln < 1 for op, ln in runs) or sum(ln for _, ln in runs) > MAX_RUN_SUM
                or b > e or e - b != sum(ln for op, ln in runs if op in (EQ, DIFF, DEL))):   # 2.
            none(c, k + 1, NO_SCORE)
            status[c] = BAD_CIGAR
            continue
        best, i, j = interval([run_value(op, ln, scoring) for op, ln in runs]) if runs else (0, 0, -1)   # 3.
        if best < max(1, min_score):                                              # 4.
            none(c, k + 1, best)
            continue
        text = lambda part: sum(ln for op, ln in part if op in (EQ, DIFF, DEL))  # noqa: E731
        read = lambda part: sum(ln for op, ln in part if op in (EQ, DIFF, INS))  # noqa: E731
        left, right = read(runs[:i]), read(runs[j + 1:])                          # 5.
        score[c] = best
        out["begin"][c], out["end"][c] = b + text(runs[:i]), e - text(runs[j + 1:])
        out["clip_left"][c], out["clip_right"][c] = left, right
        out["dist"][c] = sum(ln for op, ln in runs[i:j + 1] if op != EQ)
        row = ([left << 4 | SOFT] if left else []) + [int(w) for w in cigar[c][i:j + 1]] + ([right << 4 | SOFT] if right else [])
        out["n_cigar"][c] = len(row)
        out_cigar[c, :len(row)] = row
    return (score,) + tuple(out[name] for name in OUT_NAMES[1:7]) + (out_cigar, status)


def words(text):
    """'2= 1X 20=' -> the CIGAR words"""
    return [(int(n) << 4) | OPS.index(op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def cigar_text(row, n):
    return " ".join("%d%s" % (int(w) >> 4, OPS[int(w) & 15]) for w in row[:n])


def row_arrays(rows, k):
    """rows: [(dist, begin, end, n_cigar or None, words)] -> the five input arrays; n_cigar None = the number of words"""
    cigar = np.zeros((len(rows), 2 * k + 1), dtype=np.uint32)
    for c, row in enumerate(rows):
        cigar[c, :len(row[4])] = row[4]
    col = lambda i: np.array([row[i] for row in rows], dtype=np.uint32)  # noqa: E731
    n = np.array([len(row[4]) if row[3] is None else row[3] for row in rows], dtype=np.uint32)
    return col(0), col(1), col(2), n, cigar


def valid_row(text, begin=1000):
    """a row as the traceback leaves it for the runs of `text`: (dist, begin, end, None, words)"""
    w = words(text)
    edits = sum(x >> 4 for x in w if x & 15 != EQ)
    return edits, begin, begin + sum(x >> 4 for x in w if x & 15 in (EQ, DIFF, DEL)), None, w


# name -> (runs, scoring, min_score, expected): expected = None for a row that is clipped away, otherwise (output runs, begin
# moved by, end moved by, dist, score); k = 3 (stride 7) throughout
HAND_KEPT = {
    "unchanged": ("10=", DEFAULT, 0, ("10=", 0, 0, 0, 10)),
    "left end": ("2= 1X 20=", DEFAULT, 0, ("3S 20=", 3, 0, 0, 20)),
    "right end": ("20= 1X 2=", DEFAULT, 0, ("20= 3S", 0, -3, 0, 20)),
    "kept whole": ("5= 1X 5=", DEFAULT, 0, ("5= 1X 5=", 0, 0, 1, 6)),
    "the tie is kept whole": ("4= 1X 4=", DEFAULT, 0, ("4= 1X 4=", 0, 0, 1, 4)),
    "insertion in front": ("3I 20=", DEFAULT, 0, ("3S 20=", 0, 0, 0, 20)),
    "deletion near the end": ("20= 2D 1=", DEFAULT, 0, ("20= 1S", 0, -3, 0, 20)),
    "deletion in front": ("2D 20=", DEFAULT, 0, ("20=", 2, 0, 0, 20)),
    "insertion kept": ("30= 2I 30=", DEFAULT, 0, ("30= 2I 30=", 0, 0, 2, 52)),
    "min_score at the best": ("10= 1X 3=", DEFAULT, 10, ("10= 4S", 0, -4, 0, 10)),
    "both sides": ("1= 1X 30= 2I 1=", DEFAULT, 0, ("2S 30= 3S", 2, -1, 0, 30)),
    "seven runs kept whole": ("9= 1X 9= 1I 9= 1D 9=", DEFAULT, 0, ("9= 1X 9= 1I 9= 1D 9=", 0, 0, 3, 18)),
    "seven runs, both sides": ("1= 1X 9= 1I 9= 1D 1=", DEFAULT, 0, ("2S 9= 1I 9= 1S", 2, -2, 1, 11)),
    "free gap opening": ("3= 1I 3=", (1, 1, 0, 1), 0, ("3= 1I 3=", 0, 0, 1, 5)),
    "the largest parameters": ("2= 1X 3=", (1024, 1024, 1024, 1024), 0, ("2= 1X 3=", 0, 0, 1, 4096)),
}
HAND_AWAY = {
    "mismatches only": ("3X", DEFAULT, 0, -12),
    "min_score one above the best": ("10= 1X 3=", DEFAULT, 11, 10),
    "a deletion only": ("2D", DEFAULT, 0, -8),
}


def hand_rows():
    """-> (names, rows for row_arrays, per row (scoring, min_score)): the kept and the clipped-away hand cases, then the empty read"""
    names = list(HAND_KEPT) + list(HAND_AWAY) + ["the empty read"]
    specs = list(HAND_KEPT.values()) + list(HAND_AWAY.values())
    rows = [valid_row(spec[0]) for spec in specs] + [(0, 500, 500, 0, [])]
    return names, rows, [(spec[1], spec[2]) for spec in specs] + [(DEFAULT, 0)]


def assert_hand_case(name, got, k=3, begin=1000):
    """got: the nine outputs of one row (scalars, the cigar row) for the hand case `name`"""
    score, dist, b, e, left, right, n, row, status = got
    assert status == 0, name
    if name in HAND_KEPT:
        runs, _, _, (want, db, de, want_dist, want_score) = HAND_KEPT[name]
        _, b0, e0, _, _ = valid_row(runs, begin)
        assert cigar_text(row, n) == want and (b, e, dist, score) == (b0 + db, e0 + de, want_dist, want_score), (name, cigar_text(row, n), got)
        s = [int(w) >> 4 if int(w) & 15 == SOFT else 0 for w in row[:n]]
        assert (left, right) == (s[0], s[-1] if n > 1 else 0), name
    else:
        want_score = 0 if name == "the empty read" else HAND_AWAY[name][3]
        assert (score, dist, b, e, left, right, n) == (want_score, k + 1, NO_END, NO_END, 0, 0, 0), (name, got)


# the rows that pass through (step 1) and the rows that fail the check (step 2), one rule each; k = 3
MARKER_ROWS = [(INVALID, NO_END, NO_END, 0, []), (TOO_LONG, NO_END, NO_END, 0, []), (4, NO_END, NO_END, 0, []),
               (4, 77, NO_END, 0xFFFFFFFF, words("3= 2S"))]                  # (only `end` decides; nothing else of the row is looked at)
BAD_ROWS = {
    "op 4": (0, 10, 20, None, words("5= 2S 5=")),
    "op 0": (0, 10, 15, None, words("5= 5M")),
    "a zero-length run": (0, 10, 20, None, words("5= 0X 5=")),
    "n_cigar 8": (0, 10, 20, 8, words("10=")),
    "a text sum that is not end - begin": (1, 10, 20, None, words("5= 1I 4=")),
    "begin > end": (0, 20, 10, None, words("10=")),
    "a run sum of 65537": (1, 10, 10 + 65536, None, words("65536= 1I")),
}


def random_rows(rng, m, k, bad_share=1 / 16):
    """m rows shaped like the traceback's -- adjacent ops differ, at most k symbols that are not '=' -- of which about one in
    sixteen is a marker row or a bad row -> the five input arrays"""
    stride = 2 * k + 1
    dist, begin, end, n_cigar = (np.zeros(m, dtype=np.uint32) for _ in range(4))
    cigar = np.zeros((m, stride), dtype=np.uint32)
    for c in range(m):
        # most rows carry a few edits, one in ten as many as k allows, one in thirty is full: 2k + 1 runs of one symbol
        shape = rng.random()
        budget = k if shape < 0.1 else int(rng.integers(0, min(k, 12) + 1))
        runs, last = [], 0
        short = rng.random() < 0.5                                                # short '=' runs make every end a close call
        if shape < 0.033:
            runs = [(EQ, 1) if i % 2 == 0 else (int(rng.choice([INS, DEL, DIFF])), 1) for i in range(stride)]
            budget = 0
        elif rng.random() < 0.7:
            runs.append((EQ, int(rng.integers(1, 6 if short else 60))))
            last = EQ
        while budget > 0:
            op = int(rng.choice([x for x in (INS, DEL, DIFF) if x != last]))
            ln = int(rng.integers(1, min(budget, 3) + 1))
            runs.append((op, ln))
            budget, last = budget - ln, op
            if rng.random() < 0.8:
                runs.append((EQ, int(rng.integers(1, 6 if short else 60))))
                last = EQ
        assert len(runs) <= stride
        b = int(rng.integers(0, 1 << 20))
        cigar[c, :len(runs)] = [(ln << 4) | op for op, ln in runs]
        cigar[c, len(runs):] = rng.integers(0, 1 << 32, stride - len(runs), dtype=np.uint64)   # what lies behind n_cigar is not looked at
        dist[c] = sum(ln for op, ln in runs if op != EQ)
        begin[c], end[c], n_cigar[c] = b, b + sum(ln for op, ln in runs if op != INS), len(runs)
        if rng.random() < bad_share:
            kind = int(rng.integers(0, 7))
            if kind == 0:
                dist[c], begin[c], end[c], n_cigar[c] = rng.choice([INVALID, TOO_LONG, k + 1]), NO_END, NO_END, rng.choice([0, 0xFFFFFFFF])
            elif kind == 1:
                n_cigar[c] = stride + 1 + int(rng.integers(0, 5))
            elif kind == 2 and runs:
                cigar[c, int(rng.integers(0, len(runs)))] = (3 << 4) | int(rng.choice([0, 3, 4, 5, 6, 9, 15]))
            elif kind == 3 and runs:
                cigar[c, int(rng.integers(0, len(runs)))] &= 15
            elif kind == 4:
                end[c] = int(end[c]) + (int(rng.choice([-1, 1])) if end[c] > 0 else 1)
            elif kind == 5 and runs:
                cigar[c, int(rng.integers(0, len(runs)))] += (MAX_RUN_SUM + 1) << 4
            elif kind == 6 and end[c] > begin[c]:
                begin[c], end[c] = end[c], begin[c]
    return dist, begin, end, n_cigar, cigar


def assert_invariants(inputs, outputs, k):
    """what holds for every kept row, whatever the scoring"""
    dist, begin, end, n_cigar, cigar = inputs
    score, out_dist, out_begin, out_end, left, right, out_n, out_cigar, status = outputs
    kept = out_end != NO_END
    assert ((score[kept] >= 1) & (status[kept] == 0)).all()
    for c in np.flatnonzero(kept):
        row = [(int(w) & 15, int(w) >> 4) for w in out_cigar[c][:int(out_n[c])]]
        inner = [r for r in row if r[0] != SOFT]
        assert inner[0][0] == EQ and inner[-1][0] == EQ, c
        assert out_n[c] <= n_cigar[c] and out_begin[c] <= out_end[c] and out_dist[c] <= dist[c], c
        read_in = sum(int(w) >> 4 for w in cigar[c][:int(n_cigar[c])] if int(w) & 15 in (EQ, DIFF, INS))
        assert int(left[c]) + sum(ln for op, ln in inner if op in (EQ, DIFF, INS)) + int(right[c]) == read_in, c
        assert [r for r in row if r[0] == SOFT] == ([(SOFT, int(left[c]))] if left[c] else []) + ([(SOFT, int(right[c]))] if right[c] else []), c
        assert int(out_end[c]) - int(out_begin[c]) == sum(ln for op, ln in inner if op in (EQ, DIFF, DEL)), c
    gone = ~kept
    assert ((out_n[gone] == 0) & (out_begin[gone] == NO_END) & (left[gone] == 0) & (right[gone] == 0)).all()


def assert_same(got, want, what):
    for name, g, w in zip(OUT_NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0]
            raise AssertionError((what, name, "first difference at", at.tolist(), g[tuple(at)], w[tuple(at)]))


SCORINGS = ((1, 4, 6, 1), (1, 1, 0, 1), (1024, 1024, 1024, 1024))


# ------------------------------------------------------------------------------------------------
# (a) the single-pass variant against the brute force, with the tie rule

def test_single_pass_equals_the_brute_force_on_random_rows():
    rng = np.random.default_rng(26100)
    n_rows = 0
    for values in ([5], [-3], [0, 0], [4, -4, 4], [4, -5, 4], [-1, 3, -3, 3, -1], [2, -2, 2, -2, 2]):
        assert best_interval(values) == best_interval_single_pass(values), values
    assert best_interval([4, -4, 4]) == (4, 0, 2) and best_interval([2, -2, 2, -2, 2]) == (2, 0, 4) and best_interval([-3, -1]) == (-1, 1, 1)
    while n_rows < 100_000:
        n = int(rng.integers(1, 9))
        for _ in range(500):                                                      # small values: ties in every second row
            values = [int(v) for v in rng.integers(-3, 4, n)]
            assert best_interval(values) == best_interval_single_pass(values), values
        n_rows += 500
    for k, scoring in zip((1, 8, 32), SCORINGS):
        rows = random_rows(rng, 1000, k)
        assert_same(clip_model(*rows, k, *scoring, single_pass=True), clip_model(*rows, k, *scoring), (k, scoring))


# ------------------------------------------------------------------------------------------------
# (b) the hand cases, the markers, the bad rows

def test_hand_cases():
    names, rows, knobs = hand_rows()
    for c, name in enumerate(names):
        scoring, min_score = knobs[c]
        got = clip_model(*row_arrays([rows[c]], 3), 3, *scoring, min_score, fill=0xA5A5A5A5)
        assert_hand_case(name, tuple(x[0] for x in got))
        assert (got[7][0][int(got[6][0]):] == 0xA5A5A5A5).all(), name             # the words from out_n_cigar on are the caller's


def test_markers_pass_through_and_bad_rows_are_flagged():
    k = 3
    got = clip_model(*row_arrays(MARKER_ROWS, k), k, *DEFAULT)
    assert got[0].tolist() == [NO_SCORE] * 4 and got[1].tolist() == [INVALID, TOO_LONG, 4, 4] and not got[8].any()
    assert (got[2] == NO_END).all() and (got[3] == NO_END).all() and not got[6].any() and not got[4].any() and not got[5].any()
    # k = 3 has no room for 65536 + 1 in seven runs' budget of edits, but the check does not ask: the rule stands on its own
    for name, row in BAD_ROWS.items():
        got = clip_model(*row_arrays([row], k), k, *DEFAULT)
        assert (got[8][0], got[0][0], got[1][0], got[2][0], got[3][0], got[6][0]) == (BAD_CIGAR, NO_SCORE, k + 1, NO_END, NO_END, 0), name
    fine = clip_model(*row_arrays([(0, 10, 10 + 65536, None, words("65536="))], k), k, *DEFAULT)   # the cap itself passes
    assert fine[8][0] == 0 and fine[0][0] == 65536
    top = clip_model(*row_arrays([(0, 0, 65536, None, words("65536="))], k), k, 1024, 1, 0, 1)     # the largest score
    assert top[0][0] == 65536 * 1024


def test_invariants_on_random_rows():
    rng = np.random.default_rng(26200)
    for k in (0, 1, 3, 8, 31):
        for scoring in SCORINGS:
            rows = random_rows(rng, 400, k)
            got = clip_model(*rows, k, *scoring, min_score=int(rng.integers(0, 30)))
            assert_invariants(rows, got, k)
            kept = got[3] != NO_END
            assert k == 0 or (kept.sum() > 100 and ((got[4] != 0) | (got[5] != 0)).sum() > 5), (k, scoring)
            assert (got[8] != 0).sum() >= 3 or k == 0


# ------------------------------------------------------------------------------------------------
# (c) the two calls are declared everywhere a binding looks for them

def test_header_library_stub_and_rust_binding_have_both_calls():
    from genedex_amd import _lib
    from test_candidates_model import _header_arg_counts

    counts = _header_arg_counts("gdx_experimental.h")
    assert counts.get("gdx_soft_clip_many") == 22 and counts.get("gdx_soft_clip_many_dev") == 23
    assert "gdx_soft_clip_many" not in _header_arg_counts("gdx.h")
    assert "gdx_debug_set_clip_grid" in _header_arg_counts("gdx_bench.h") and "gdx_debug_set_clip_grid" in _lib.SIGNATURES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    rust = open(os.path.join(ROOT, "bindings", "rust", "gdx.rs")).read()
    for name in NAMES:
        assert hasattr(lib, name), name + " is not exported by libgdx.so"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == counts[name], name
        assert re.search(r"pub fn " + name + r"\s*\(", rust), name
    header = open(os.path.join(ROOT, "include", "gdx_experimental.h")).read()
    for name, text, value in (("GDX_CIGAR_SOFT_CLIP", "4u", SOFT), ("GDX_CLIP_NO_SCORE", "0x80000000u", NO_SCORE),
                              ("GDX_CLIP_BAD_CIGAR", "1", BAD_CIGAR), ("GDX_CLIP_MAX_RUN_SUM", "65536u", MAX_RUN_SUM),
                              ("GDX_CLIP_MAX_SCORE_PARAM", "1024u", MAX_SCORE_PARAM)):
        assert re.search(r"#define\s+" + name + r"\s+" + text + r"\s", header), name
        assert getattr(_lib, name) == value, name
        assert re.search(r"pub const " + name + r": u\d+ = ", rust), name
    # the SAM records' text points at the new call instead of listing soft clipping as out of scope
    assert "gdx_soft_clip_many below" in header
    from genedex_amd.device import DeviceEngine
    from genedex_amd.index import FmIndex

    assert hasattr(FmIndex, "soft_clip_raw") and hasattr(DeviceEngine, "soft_clip")
