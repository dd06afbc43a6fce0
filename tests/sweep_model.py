"""The exhaustive sweep: one fixed small collection and a model of what every read taken from it must answer.

The collection holds every shape the per-position and per-row structures of an index can be wrong at alone -- a text of length
0, 1, k - 1, k, k + 32 and k + 33, N, repeats of two to five and of forty copies, tandem repeats -- and is just large enough for
rows on both sides of a superblock border.  The sweep asks for the read ENDING at every text position, at every length, so no
entry of any structure stays unvisited.

The model rests on the suffix array alone: the array comes from the oracle (sa_rate = 1), is proved with the linear-time check
of suffix_array_model, and everything else is derived from it and the dense text -- neighbouring-row LCPs (Kasai, cut at
sentinels), and for a length L the interval of the read at position p as the maximal run of rows around ISA[p] whose LCP is
>= L.  No rank structure, no LF step and no backward search is involved.  Reads that do not occur (one substituted symbol) are
counted by a dictionary over the texts' byte windows.  Pure numpy; of the library only the alphabet's encoding table is used."""
from __future__ import annotations

import numpy as np

from suffix_array_model import check_suffix_array, dense_concat

K = 12                 # the seed length the sweep builds with unless a variant names its own
RNG_SEED = 181018      # the collection is a function of this seed and of `bulk` alone
BULK = 40_000
HIT_CAP = 1 << 19      # total hits of a whole sweep at any locate length (a cap, not a measurement)
MIN_LOCATE_LENGTH = 8
NEAR_MISS_KINDS = ("last", "first", "before-seed")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _acgt(rng, n) -> bytes:
    return _ACGT[rng.integers(0, 4, n)].tobytes()


def sweep_texts(bulk: int = BULK, k: int = K, seed: int = RNG_SEED):
    """the ten texts of the sweep collection, in their fixed order (alphabet ascii_dna_with_n)"""
    rng = np.random.default_rng(seed)
    t_bulk = _acgt(rng, bulk)
    withn = np.frombuffer(_acgt(rng, 20_000), dtype=np.uint8).copy()
    withn[rng.random(20_000) < 0.01] = ord("N")
    short = _acgt(rng, k - 1)
    # rep: families of 2, 3, 4 and 5 copies of a unit of 200 and one of 40 copies of a unit of 100, every copy followed by a
    # spacer of its own, the blocks shuffled
    blocks = []
    for length, copies in ((200, 2), (200, 3), (200, 4), (200, 5), (100, 40)):
        unit = _acgt(rng, length)
        for _ in range(copies):
            blocks.append(unit + _acgt(rng, int(rng.integers(40, 81))))
    rep = _acgt(rng, 50) + b"".join(blocks[i] for i in rng.permutation(len(blocks)))
    exact = _acgt(rng, k)
    tandem = _acgt(rng, 40) + b"A" * 300 + _acgt(rng, 40) + b"ACGTTGCA" * 60 + _acgt(rng, 40)
    return [t_bulk, b"", withn.tobytes(), b"A", short, rep, exact, tandem, _acgt(rng, k + 32), _acgt(rng, k + 33)]


def sweep_lengths(k: int):
    """count / interval lengths of a sweep with seed length k"""
    return sorted({1, 2, 3, k - 1, k, k + 1, k + 31, k + 32, k + 33, k + 63, k + 64, k + 65, 150, 256})


def locate_lengths(k: int):
    return [ln for ln in sweep_lengths(k) if ln >= MIN_LOCATE_LENGTH]


def near_miss_lengths(k: int):
    return [k, k + 1, k + 32, k + 33, k + 64]


def kasai_lcp(dense, sa) -> np.ndarray:
    """int64[n]: lcp[r] = the symbols suffix sa[r - 1] and suffix sa[r] share before either reaches a sentinel (lcp[0] = 0);
    `sa` must be the checked suffix array.  (Kasai et al.; the cut keeps the invariant lcp(i + 1) >= lcp(i) - 1: the distance to
    the next sentinel falls by one per position too.)"""
    n = len(dense)
    text = np.asarray(dense, dtype=np.uint8).tobytes()
    sa = np.asarray(sa).astype(np.int64)
    rank = np.empty(n, dtype=np.int64)
    rank[sa] = np.arange(n, dtype=np.int64)
    sa_l, rank_l = sa.tolist(), rank.tolist()
    lcp = [0] * n
    h = 0
    for i in range(n):
        r = rank_l[i]
        if r == 0:
            h = 0
            continue
        j = sa_l[r - 1]
        while i + h < n and j + h < n and text[i + h] == text[j + h] and text[i + h] != 0:
            h += 1
        lcp[r] = h
        if h:
            h -= 1
    return np.array(lcp, dtype=np.int64)


class SweepModel:
    """texts + alphabet + THE suffix array of their dense concatenation -> every read of the sweep and its answers"""

    def __init__(self, texts, alphabet, sa):
        self.texts = [bytes(t) for t in texts]
        self.alphabet = alphabet
        self.dense = dense_concat(self.texts, alphabet)
        self.n = int(self.dense.size)
        self.sa = np.asarray(sa).astype(np.int64)
        check_suffix_array(self.dense, self.sa)
        self.isa = np.empty(self.n, dtype=np.int64)
        self.isa[self.sa] = np.arange(self.n, dtype=np.int64)
        self.lcp = kasai_lcp(self.dense, self.sa)
        self.text_len = np.array([len(t) for t in self.texts], dtype=np.int64)
        self.text_start = np.concatenate([[0], np.cumsum(self.text_len + 1)[:-1]]).astype(np.int64)
        # the IO symbols in the layout of the dense text (a 0 where a sentinel stands: no read covers one)
        self.io = np.zeros(self.n, dtype=np.uint8)
        for start, t in zip(self.text_start, self.texts):
            self.io[start:start + len(t)] = np.frombuffer(t, dtype=np.uint8)
        self._windows, self._rows, self._reads, self._hits, self._dicts = {}, {}, {}, {}, {}

    # ---- the reads ---------------------------------------------------------------------------------------------------------
    def windows(self, length: int):
        """(global start, text id, start in the text) of every window of `length` symbols that fits its text, in text order:
        read i of the sweep at this length is the read ending at text position pos[i] + length - 1"""
        if length not in self._windows:
            fits = np.maximum(self.text_len - length + 1, 0)
            tid = np.repeat(np.arange(len(self.texts), dtype=np.int64), fits)
            first = np.concatenate([[0], np.cumsum(fits)[:-1]]).astype(np.int64)
            pos = np.arange(int(fits.sum()), dtype=np.int64) - np.repeat(first, fits)
            self._windows[length] = (self.text_start[tid] + pos, tid, pos)
        return self._windows[length]

    def gathered(self, length: int) -> np.ndarray:
        """uint8[nq, length]: the symbols of every read (a fresh array)"""
        start = self.windows(length)[0]
        return self.io[start[:, None] + np.arange(length, dtype=np.int64)[None, :]]

    @staticmethod
    def as_batch(reads2d: np.ndarray):
        """(qbuf, qoff) of reads of one length: the rows back to back, qoff = arange * length (qbuf padded to whole words)"""
        nq, length = reads2d.shape
        qbuf = np.zeros((nq * length + 8 + 7) // 8 * 8, dtype=np.uint8)
        qbuf[: nq * length] = reads2d.reshape(-1)
        return qbuf, np.arange(nq + 1, dtype=np.uint64) * np.uint64(length)

    def reads(self, length: int):
        if length not in self._reads:
            self._reads[length] = self.as_batch(self.gathered(length))
        return self._reads[length]

    def clean(self, length: int) -> np.ndarray:
        """bool[nq]: the read holds none but the alphabet's searchable symbols (what the 2-bit form can express)"""
        start = self.windows(length)[0]
        bad = np.concatenate([[0], np.cumsum(self.dense > self.alphabet.num_searchable_dense_symbols())])
        return bad[start + length] == bad[start]

    def near_misses(self, length: int, kind: str, k: int) -> np.ndarray:
        """uint8[nq, length]: every read with one symbol replaced by the next of A C G T (N becomes A) -- the last symbol, the
        first, or the one right in front of the seed (index length - k - 1; needs length > k)"""
        at = {"last": length - 1, "first": 0, "before-seed": length - k - 1}[kind]
        if at < 0:
            raise ValueError("no symbol in front of the seed")
        reads = self.gathered(length)
        nxt = np.full(256, ord("A"), dtype=np.uint8)
        nxt[_ACGT] = np.roll(_ACGT, -1)
        reads[:, at] = nxt[reads[:, at]]
        return reads

    # ---- what they answer --------------------------------------------------------------------------------------------------
    def row_intervals(self, length: int):
        """(lo, hi)[row]: the maximal run of rows around `row` whose suffixes share their first `length` symbols"""
        if length not in self._rows:
            rows = np.arange(self.n, dtype=np.int64)
            border = self.lcp < length                      # row r opens a run (lcp[0] = 0: row 0 always does)
            lo = np.maximum.accumulate(np.where(border, rows, 0))
            nxt = np.minimum.accumulate(np.where(border, rows, self.n)[::-1])[::-1]  # the first border at or behind a row
            hi = np.concatenate([nxt[1:], [self.n]])
            self._rows[length] = (lo, hi)
        return self._rows[length]

    def intervals(self, length: int):
        """(lo, hi)[read]: the suffix-array interval of every read of the sweep at this length"""
        lo, hi = self.row_intervals(length)
        row = self.isa[self.windows(length)[0]]
        return lo[row], hi[row]

    def total_hits(self, length: int) -> int:
        lo, hi = self.intervals(length)
        return int((hi - lo).sum())

    def hits(self, length: int):
        """(offsets[nq + 1], text ids, positions): SA[lo:hi] of every read in row order, mapped to (text, position)"""
        if length not in self._hits:
            lo, hi = self.intervals(length)
            counts = hi - lo
            off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            if int(off[-1]) > HIT_CAP:
                raise ValueError(f"{int(off[-1])} hits at length {length}: beyond the sweep's cap of {HIT_CAP}")
            rows = np.repeat(lo, counts) + (np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1], counts))
            at = self.sa[rows]
            tid = np.searchsorted(self.text_start, at, side="right") - 1
            self._hits[length] = (off, tid, at - self.text_start[tid])
        return self._hits[length]

    def capped_hits(self, length: int, max_hits: int):
        """the same when reads with more than max_hits hits get no slots (the device calls' max_hits)"""
        off, tid, pos = self.hits(length)
        counts = np.diff(off)
        keep = counts <= max_hits
        sel = np.repeat(keep, counts)
        return np.concatenate([[0], np.cumsum(np.where(keep, counts, 0))]).astype(np.int64), tid[sel], pos[sel]

    def window_counts(self, reads2d: np.ndarray) -> np.ndarray:
        """int64[nq]: how often each row of reads2d occurs among the windows of its length -- a dictionary over the texts' byte
        windows, nothing of the suffix array"""
        nq, length = reads2d.shape
        if length not in self._dicts:
            table = {}
            for w in self._as_keys(self.gathered(length)):
                table[w] = table.get(w, 0) + 1
            self._dicts[length] = table
        table = self._dicts[length]
        return np.fromiter((table.get(w, 0) for w in self._as_keys(reads2d)), dtype=np.int64, count=nq)

    @staticmethod
    def _as_keys(reads2d: np.ndarray):
        rows = np.ascontiguousarray(reads2d)
        return rows.view(np.dtype((np.void, rows.shape[1]))).ravel().tolist()

    # ---- what the sweep covers ---------------------------------------------------------------------------------------------
    def kmer_codes(self, k: int):
        """(code, global start) of every k-mer of the searchable symbols that fits its text: code = the symbols as 2-bit digits"""
        start = self.windows(k)[0][self.clean(k)]
        code = np.zeros(start.size, dtype=np.int64)
        for j in range(k):
            code = code * 4 + (self.dense[start + j].astype(np.int64) - 1)
        return code, start

    def clean_symbols_in_front(self, cap: int = 32) -> np.ndarray:
        """int64[n]: the searchable symbols of its own text that stand directly in front of a position, at most `cap`"""
        ok = (self.dense >= 1) & (self.dense <= self.alphabet.num_searchable_dense_symbols())
        idx = np.arange(self.n, dtype=np.int64)
        last_bad = np.maximum.accumulate(np.where(ok, -1, idx))  # the last position <= i that is no searchable symbol
        run = np.concatenate([[0], (idx - last_bad)[:-1]])        # searchable symbols ending right in front of i
        return np.minimum(run, cap)

    def where(self, length: int, read: int) -> str:
        """names read `read` of the sweep at `length`, for failure messages"""
        _, tid, pos = self.windows(length)
        t, p = int(tid[read]), int(pos[read])
        return f"read {read}: text {t} (of {int(self.text_len[t])} symbols), symbols [{p}, {p + length}), ending at position {p + length - 1}"


def oracle_suffix_array(texts, alphabet) -> np.ndarray:
    """the full suffix array as the oracle builds it (sa_rate = 1); SweepModel proves it before it uses it"""
    from oracle.oracle import OracleIndex

    o = OracleIndex.build(texts, alphabet.io_to_dense_table, alphabet.num_dense_symbols(), alphabet.num_searchable_dense_symbols(),
                          sa_rate=1)
    return o.sa_samples


def build_sweep_model(bulk: int = BULK) -> SweepModel:
    from genedex_amd import alphabet as alph

    a = alph.ascii_dna_with_n()
    texts = sweep_texts(bulk)
    return SweepModel(texts, a, oracle_suffix_array(texts, a))
