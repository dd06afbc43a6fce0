"""A plain model of the seed table's repeat records (IndexView::seed_pairs / seed_quads) and of the search records they
decide, with crafted texts that put the record path's edges in on purpose.

The model is written from the definitions, not from the kernels: the rows of a k-mer are those of the suffix array whose
suffix starts with it, a k-mer on two rows gets a 32-byte record and one on three or four rows a 64-byte record when every
occurrence has 32 symbols A C G T of its own text in front of it, and a read of k + 1 .. k + 32 symbols whose last k
symbols are such a k-mer is decided by comparing the symbols in front of its seed with those in front of each row.  The
16-byte search record it must get (kernels.hpp):
  none                 {0, 0, 0xffffffff, 0}
  resolved of one      {0, 1, h, kRecResolved}
  resolved of two      {h2, h2 + 2, h1, kRecResolved}           (h1 on the lower row: hit slot 0)
  masked (3 or 4 rows) {first row, first row + alive, mask, symbols | kRecMasked}
with h = SA[row] - symbols in front of the seed, in the coordinates of the concatenated texts (one sentinel after each).
Pure Python / numpy; the suffix array is the oracle's."""
from __future__ import annotations

import numpy as np

K_REC_MASKED = 1 << 23
K_REC_RESOLVED = 1 << 22
CONTEXT = 32  # symbols in front of each occurrence a record holds
KINDS = ("none", "one", "two", "masked3", "masked4")


class RecordModel:
    """texts (bytes), k, and the oracle index of the texts (OracleIndex: its dense text and full suffix array)"""

    def __init__(self, texts, k, oracle):
        self.texts = [bytes(t) for t in texts]
        self.k = k
        self.io_to_dense = np.asarray(oracle.io_to_dense, dtype=np.uint8)
        dense = oracle.dense_text
        sa = oracle.full_sa
        n = dense.size
        assert sa.size == n
        self.dense, self.sa = dense, sa
        self.starts = np.zeros(len(self.texts), dtype=np.int64)
        at = 0
        for t, txt in enumerate(self.texts):
            self.starts[t] = at
            at += len(txt) + 1
        assert at == n
        acgt = (dense >= 1) & (dense <= 4)
        # run[p] = A C G T symbols from p on (a sentinel or another symbol ends a run)
        run = np.zeros(n + 1, dtype=np.int64)
        for p in range(n - 1, -1, -1):
            run[p] = run[p + 1] + 1 if acgt[p] else 0
        # back[p] = A C G T symbols right in front of p
        back = np.zeros(n + 1, dtype=np.int64)
        for p in range(1, n + 1):
            back[p] = back[p - 1] + 1 if acgt[p - 1] else 0
        self.whole = back[:n] >= CONTEXT
        raw = dense.tobytes()
        # the k-mers in suffix-array order: rows [lo, hi) of each distinct A C G T k-mer
        self.kmers = {}
        r = 0
        while r < n:
            p = int(sa[r])
            if run[p] < k:
                r += 1
                continue
            key = raw[p:p + k]
            hi = r + 1
            while hi < n and run[int(sa[hi])] >= k and raw[int(sa[hi]):int(sa[hi]) + k] == key:
                hi += 1
            pos = [int(x) for x in sa[r:hi]]
            rows = hi - r
            kind = None
            if rows in (2, 3, 4) and all(self.whole[x] for x in pos):
                kind = "pair" if rows == 2 else "quad"
            self.kmers[key] = (r, hi, kind, pos)
            r = hi
        self.pair_records = sum(1 for v in self.kmers.values() if v[2] == "pair")
        self.quad_records = sum(1 for v in self.kmers.values() if v[2] == "quad")

    def dense_of(self, q):
        return bytes(self.io_to_dense[np.frombuffer(bytes(q), dtype=np.uint8)].tolist()) if q else b""

    def read(self, q):
        """None when no record decides the read, else (kind, mask, record as 4 u32, hits as global positions in order)"""
        q = bytes(q)
        k = self.k
        n_v = len(q) - k
        if not 1 <= n_v <= CONTEXT:
            return None
        d = self.dense_of(q)
        if any(not 1 <= c <= 4 for c in d):
            return None
        ent = self.kmers.get(d[n_v:])
        if ent is None or ent[2] is None:
            return None
        lo, hi, _, pos = ent
        ctx = d[:n_v]
        raw = self.dense.tobytes()
        mask = 0
        for j, p in enumerate(pos):
            if raw[p - n_v:p] == ctx:
                mask |= 1 << j
        alive = [pos[j] - n_v for j in range(len(pos)) if mask >> j & 1]
        m = len(alive)
        if m == 0:
            return "none", mask, (0, 0, 0xFFFFFFFF, 0), []
        if m == 1:
            return "one", mask, (0, 1, alive[0], K_REC_RESOLVED), alive
        if m == 2:
            return "two", mask, (alive[1], alive[1] + 2, alive[0], K_REC_RESOLVED), alive
        return f"masked{m}", mask, (lo, lo + m, mask, n_v | K_REC_MASKED), alive

    def text_pos(self, g):
        t = int(np.searchsorted(self.starts, g, side="right")) - 1
        return t, int(g - self.starts[t])


def expand_record(model, rec):
    """the hits a search record stands for (the decoders' reading of it), as global positions in hit order"""
    x, y, z, w = (int(v) & 0xFFFFFFFF for v in rec)
    if w & K_REC_RESOLVED:
        if y - x == 1:
            return [z]
        assert y - x == 2
        return [z, x]
    if w & K_REC_MASKED:
        sym = w & 0x1FFFFF
        return [int(model.sa[x + j]) - sym for j in range(4) if z >> j & 1]
    assert y == x
    return []


# ---- crafted texts -----------------------------------------------------------------------------------------------------

LEAD = 64  # symbols of the read in front of a crafted batch (crafted_reads)
SEED_ZONE = 24  # symbols of a family's seed: the k-mer of any k <= 24 starts there


def _acgt(rng, n):
    return bytes(b"ACGT"[i] for i in rng.integers(0, 4, n))


def _flip(b):
    return b"ACGT"[(b"ACGT".index(b) + 1) % 4]


class Family:
    """copies of CONTEXT + SEED_ZONE symbols, copy i followed by "ACGT"[i] (the rows of the seed's k-mers are then the
    copies in order); `ctx` is the context the family's reads carry, copy i's own context is ctxs[i]"""

    def __init__(self, rng, copies, alive=None, far_mismatch=True):
        self.zone = _acgt(rng, SEED_ZONE)
        self.ctx = _acgt(rng, CONTEXT)
        alive = set(range(copies)) if alive is None else set(alive)
        self.alive = alive
        self.ctxs = []
        first_dead = True
        for i in range(copies):
            c = bytearray(self.ctx)
            if i not in alive:
                # one symbol off: the first dead copy at the symbol farthest from the seed (the low end of the compare mask)
                at = 0 if (first_dead and far_mismatch) else int(rng.integers(0, CONTEXT))
                first_dead = False
                c[at] = _flip(c[at])
            self.ctxs.append(bytes(c))
        self.copies = copies

    def copy(self, i, rng):
        return self.ctxs[i] + self.zone + b"ACGTACGT"[i:i + 1] + _acgt(rng, int(rng.integers(8, 40)))


def crafted_texts(seed=0):
    """A few small texts holding, on purpose: families of 2, 3, 4 and 5 copies; for 2, 3 and 4 copies every set of copies
    whose context is the family's (so every alive mask); copies whose seed stands 31, 32 or 33 symbols after a text start;
    N at either end of a context and right in front of it; a three- and a four-copy k-mer with one copy not whole.
    Returns (texts, families)."""
    rng = np.random.default_rng(seed)
    fams = []
    for copies in (2, 3, 4):
        for mask in range(1 << copies):
            for rep in range(2):
                fams.append(Family(rng, copies, [i for i in range(copies) if mask >> i & 1], far_mismatch=rep == 0))
    for copies in (2, 3, 4, 5, 5):
        fams.append(Family(rng, copies))
    segments = []  # (flank + copy) pieces placed anywhere
    for f in fams:
        for i in range(f.copies):
            segments.append(_acgt(rng, int(rng.integers(0, 30))) + f.copy(i, rng))
    # copies at a text start: the seed `o` symbols after it (31: not whole; 32 and 33: whole)
    starts = []
    for o in (31, 32, 33):
        for copies in (2, 3, 4):
            f = Family(rng, copies)
            fams.append(f)
            for i in range(copies):
                piece = f.copy(i, rng)
                if i == 0:
                    starts.append(_acgt(rng, o - CONTEXT) + piece if o > CONTEXT else piece[CONTEXT - o:])
                else:
                    segments.append(_acgt(rng, int(rng.integers(0, 30))) + piece)
    # N at the far end of a context, right in front of the seed (both: no record), one symbol before the context (a record)
    for where in (0, CONTEXT - 1, -1):
        for copies in (2, 3, 4):
            f = Family(rng, copies)
            fams.append(f)
            for i in range(copies):
                piece = bytearray(f.copy(i, rng))
                if i == copies - 1:
                    if where >= 0:
                        piece[where] = ord("N")
                    else:
                        piece = bytearray(b"N") + piece
                segments.append(_acgt(rng, int(rng.integers(1, 30))) + bytes(piece))
    order = rng.permutation(len(segments))
    texts = [b"", b"", b""]
    for j, s in enumerate(order):
        texts[j % 3] += segments[s]
    texts = [_acgt(rng, 40) + t + _acgt(rng, 40) for t in texts]
    for s in starts:  # texts that begin with a copy (and hold a little more)
        texts.append(s + _acgt(rng, int(rng.integers(60, 200))))
    texts.append(_acgt(rng, 5000))  # (filler: the default shape's k is 16 for 16 K < n <= 64 K)
    return texts, fams


def crafted_reads(texts, fams, k, seed=1, n_random=2000):
    """reads per edge -- seed lengths k, k + 1, k + 31, k + 32, k + 33 (and 2, 16) with the family's context, a mismatch at
    either end of the compared context, reads from each copy as it stands -- and n_random reads from anywhere on top"""
    rng = np.random.default_rng(seed)
    # (first a read of 64 symbols that no record decides: the seed kernels load the 56 symbols in front of a read's end, and
    # a read that ends closer to the buffer's start is searched by the verify kernel's own seed lookup, without the records)
    qs = [_acgt(rng, LEAD)]
    for f in fams:
        kmer = f.zone[:k]
        for n_v in (0, 1, 2, 16, 31, 32, 33):
            front = (_acgt(rng, 1) + f.ctx) if n_v > CONTEXT else f.ctx[CONTEXT - n_v:] if n_v else b""
            q = front + kmer
            qs.append(q)
            if 1 <= n_v <= CONTEXT:
                far = bytearray(q)
                far[0] = _flip(far[0])  # the compared symbol farthest from the seed
                near = bytearray(q)
                near[n_v - 1] = _flip(near[n_v - 1])  # ... and the one right in front of it
                qs += [bytes(far), bytes(near)]
        for c in f.ctxs:  # each copy's own context
            for n_v in (1, 31, 32):
                qs.append(c[CONTEXT - n_v:] + kmer)
        # seeds further into the zone: the context then ends in the zone
        for shift in (1, SEED_ZONE - k):
            if shift > 0:
                qs.append(f.ctx[shift:] + f.zone[:shift + k])
    for t in texts:  # a text's first symbols: seeds 31 .. 33 symbols after its start
        for n_v in (30, 31, 32, 33):
            if len(t) >= n_v + k:
                qs.append(t[:n_v + k])
    for _ in range(n_random):
        t = texts[int(rng.integers(0, len(texts)))]
        ln = int(rng.integers(k, k + 40))
        if len(t) < ln:
            continue
        at = int(rng.integers(0, len(t) - ln + 1))
        q = bytearray(t[at:at + ln])
        if rng.random() < 0.3:
            j = int(rng.integers(0, ln))
            if q[j] != ord("N"):
                q[j] = _flip(q[j])
        qs.append(bytes(q))
    return [q for q in qs if b"N" not in q]
