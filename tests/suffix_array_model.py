"""A plain model of the suffix sorter (build_sa.hip; wide.hip's wide_suffix_array for 64-bit storage) and of what it reports.

The sorter's result is THE suffix array of the dense text: sentinels are ordinary symbols 0, a text ends with one, and the end of
the string compares smallest.  It is unique, so any correct sorter gives it, and a linear-time check decides whether an array is
it -- no second sorter is needed for large texts.  What the 32-bit sorter reports (gdx_index_build_stats) follows from the text:
  initial order h0      1 + k0 symbols: the first symbol (the bucket) and a 64-bit key of the next k0 = min(32, 64 / sym_bits),
                        a symbol c stored as c + 1 in sym_bits = bits for the values 0 .. sigma ("beyond the end" is 0)
  pending after sort    the suffixes that share their first h0 symbols with another suffix (a position beyond the end counts as
                        a symbol below all others, so a suffix shorter than h0 shares its window with nobody)
  rounds                every round doubles the order, and a round runs while anything is pending: the smallest r >= 0 with
                        max LCP < h0 * 2^r
Written from build_sa.hip's header comment and DESIGN.md, not from the kernels.  Pure numpy; nothing of the library is imported."""
from __future__ import annotations

import numpy as np

BRUTE_LIMIT = 20_000   # brute_suffix_array copies every suffix
KASAI_LIMIT = 300_000  # max_lcp_kasai is a Python loop


def dense_concat(texts, alphabet) -> np.ndarray:
    """uint8[n]: the texts densely encoded and concatenated as the library does, one sentinel 0 after every text"""
    parts = []
    for t in texts:
        parts.append(alphabet.encode(t))
        parts.append(np.zeros(1, dtype=np.uint8))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def brute_suffix_array(dense) -> np.ndarray:
    """int64[n]: the suffixes sorted as byte strings (Python's bytes order: a proper prefix is smaller, so the end of the string
    compares smallest)"""
    b = np.asarray(dense, dtype=np.uint8).tobytes()
    if len(b) > BRUTE_LIMIT:
        raise ValueError(f"brute_suffix_array is for n <= {BRUTE_LIMIT}")
    return np.array(sorted(range(len(b)), key=lambda i: b[i:]), dtype=np.int64)


def first_bad_row(dense, sa):
    """None if `sa` is the suffix array of `dense`, else the first row that shows it is not: a row whose value is out of range or
    repeats an earlier row, or the upper row j + 1 of a neighbouring pair in the wrong order.  Linear time: suffix sa[j] is below
    suffix sa[j + 1] iff its first symbol is smaller, or the symbols are equal and the suffix after it, sa[j] + 1, stands in a
    lower row than sa[j + 1] + 1 (the empty suffix n in row -1)."""
    text = np.asarray(dense, dtype=np.uint8)
    n = text.size
    sa = np.asarray(sa)
    if sa.ndim != 1 or sa.size != n:
        return min(sa.size, n) if sa.ndim == 1 else 0
    if n == 0:
        return None
    sa = sa.astype(np.int64)
    out_of_range = (sa < 0) | (sa >= n)
    if out_of_range.any():
        return int(np.flatnonzero(out_of_range)[0])
    order = np.argsort(sa, kind="stable")
    repeats = sa[order][1:] == sa[order][:-1]
    if repeats.any():
        return int(order[1:][repeats].min())  # (stable sort: order[1:][k] is the later row of the two)
    rank = np.empty(n + 1, dtype=np.int64)
    rank[sa] = np.arange(n, dtype=np.int64)
    rank[n] = -1
    a, b = sa[:-1], sa[1:]
    bad = (text[a] > text[b]) | ((text[a] == text[b]) & (rank[a + 1] >= rank[b + 1]))
    if bad.any():
        return int(np.flatnonzero(bad)[0]) + 1
    return None


def check_suffix_array(dense, sa, raise_on_error=True):
    """The exact check of a suffix array in linear time.  Raises AssertionError naming the first offending row, or, with
    raise_on_error=False, returns that row (None for a correct array)."""
    row = first_bad_row(dense, sa)
    if row is not None and raise_on_error:
        sa = np.asarray(sa)
        lo, hi = max(row - 1, 0), min(row + 2, sa.size)
        raise AssertionError(f"not the suffix array: first offending row {row} of {sa.size} (rows {lo}..{hi - 1} hold "
                             f"{sa[lo:hi].tolist()})")
    return row


def bwt_from_sa(dense, sa) -> np.ndarray:
    """uint8[n]: text[sa - 1], the row with sa == 0 wrapping to the last symbol (fm_index.hip: bwt.rs:93-116)"""
    text = np.asarray(dense, dtype=np.uint8)
    sa = np.asarray(sa).astype(np.int64)
    return text[np.where(sa > 0, sa, text.size) - 1] if text.size else text.copy()


def _bits_for(values: int) -> int:
    """bits that hold 0 .. values - 1, at least 1"""
    b = 1
    while (1 << b) < values:
        b += 1
    return b


def initial_order(sigma: int) -> int:
    """h0 = 1 + k0 (sigma counts the sentinel): DNA = 5 dense symbols -> 3 bits -> k0 = 21 -> 22"""
    sym_bits = _bits_for(sigma + 1)  # a symbol is stored as symbol + 1, 0 = beyond the end
    return 1 + min(32, 64 // sym_bits)


def window_columns(dense, width: int) -> list:
    """the first `width` symbols of every suffix (symbol + 1, 0 beyond the end) packed into uint64 columns, most significant
    column first: two suffixes share their window iff all columns agree.  (33 symbols of a 2-symbol alphabet: two columns.)"""
    text = np.asarray(dense, dtype=np.uint8)
    n = text.size
    padded = np.zeros(n + width, dtype=np.uint64)
    padded[:n] = text.astype(np.uint64) + np.uint64(1)
    bits = _bits_for(int(text.max()) + 2) if n else 1  # the values 0 .. max symbol + 1
    per_col = 64 // bits
    cols = []
    for t0 in range(0, width, per_col):
        col = np.zeros(n, dtype=np.uint64)
        for t in range(t0, min(t0 + per_col, width)):
            col = (col << np.uint64(bits)) | padded[t:t + n]
        cols.append(col)
    return cols


def shared_window_count(dense, width: int) -> int:
    """the number of suffixes whose first `width` symbols are shared with at least one other suffix"""
    n = np.asarray(dense).size
    if n < 2:
        return 0
    cols = window_columns(dense, width)
    order = np.lexsort(cols[::-1])  # (lexsort: the last key is the primary one)
    same = np.ones(n - 1, dtype=bool)
    for c in cols:
        s = c[order]
        same &= s[1:] == s[:-1]
    member = np.zeros(n, dtype=bool)
    member[1:] |= same
    member[:-1] |= same
    return int(member.sum())


def pending_after_key_sort(dense, sigma: int) -> int:
    return shared_window_count(dense, initial_order(sigma))


def max_lcp_kasai(dense, sa) -> int:
    """the largest longest-common-prefix of two neighbouring rows (Kasai et al.); `sa` must be the checked suffix array"""
    n = len(dense)
    if n > KASAI_LIMIT:
        raise ValueError(f"max_lcp_kasai is for n <= {KASAI_LIMIT}")
    if n < 2:
        return 0
    text = np.asarray(dense, dtype=np.uint8).tobytes()
    sa = np.asarray(sa).astype(np.int64)
    rank = np.empty(n, dtype=np.int64)
    rank[sa] = np.arange(n, dtype=np.int64)
    sa_l, rank_l = sa.tolist(), rank.tolist()
    best = h = 0
    for i in range(n):
        r = rank_l[i]
        if r == 0:
            h = 0
            continue
        j = sa_l[r - 1]
        while i + h < n and j + h < n and text[i + h] == text[j + h]:
            h += 1
        if h > best:
            best = h
        if h:
            h -= 1
    return best


def max_lcp_capped(dense, sa, cap: int) -> int:
    """min(max LCP of neighbouring rows, cap), vectorised: one pass per symbol over the pairs that still agree.  For large texts
    whose ties are short (i.i.d. symbols)."""
    text = np.asarray(dense, dtype=np.uint8)
    n = text.size
    sa = np.asarray(sa).astype(np.int64)
    a, b = sa[:-1], sa[1:]
    depth = 0
    while a.size and depth < cap:
        inside = (a + depth < n) & (b + depth < n)
        a, b = a[inside], b[inside]
        agree = text[a + depth] == text[b + depth]
        a, b = a[agree], b[agree]
        if a.size:
            depth += 1
    return depth


def rounds_for_max_lcp(max_lcp: int, sigma: int) -> int:
    """the smallest r >= 0 with max_lcp < h0 * 2^r"""
    r, h = 0, initial_order(sigma)
    while max_lcp >= h:
        h *= 2
        r += 1
    return r


def doubling_rounds(dense, sa, sigma: int) -> int:
    return rounds_for_max_lcp(max_lcp_kasai(dense, sa), sigma)


# ---- texts with known ties (inputs of the tests, as sequences of 0/1 or bytes) ------------------------------------------------

def repeat_to(unit: bytes, length: int) -> bytes:
    """`unit` repeated and cut to `length` symbols"""
    return (unit * (length // len(unit) + 1))[:length]


def fibonacci_bits(length: int) -> np.ndarray:
    """the Fibonacci word S(k) = S(k-1) S(k-2), S(0) = 0, S(1) = 01, cut to `length`"""
    a, b = [0], [0, 1]
    while len(b) < length:
        a, b = b, b + a
    return np.array(b[:length], dtype=np.uint8)


def thue_morse_bits(length: int) -> np.ndarray:
    """t[i] = parity of the ones in the binary form of i"""
    i = np.arange(length, dtype=np.uint64)
    p = np.zeros(length, dtype=np.uint64)
    while i.any():
        p ^= i & np.uint64(1)
        i >>= np.uint64(1)
    return p.astype(np.uint8)


def de_bruijn_bits(order: int) -> np.ndarray:
    """a binary de Bruijn sequence B(2, order) written out as a string of 2^order + order - 1 symbols: every word of `order`
    symbols occurs exactly once (the standard construction from Lyndon words, Fredricksen-Maiorana)"""
    seq, a = [], [0] * (order + 1)

    def db(t, p):
        if t > order:
            if order % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 2):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return np.array(seq + seq[:order - 1], dtype=np.uint8)


def bits_to_text(bits, symbols: bytes) -> bytes:
    return np.frombuffer(symbols, dtype=np.uint8)[np.asarray(bits, dtype=np.int64)].tobytes()
