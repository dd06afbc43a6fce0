"""A plain model of the offsets scan and store pass that ends a count + locate step (locate.hip: scan2_tile_sums_kernel ->
scan2_sums_kernel -> scan2_tile_scan_kernel, then one of the locate kernels), for batches whose search results are MADE BY HAND.

The pass reads, per read, a 16-byte search record {start row, end row, hint row, hint symbols | status << 24} and optionally a
compact word (kernels.hpp): the text position of the read's only hit, COMPACT_NONE = no occurrence, COMPACT_SEE = "see the record".
A plain finished read -- no hint, no status -- leaves {start, end, 0xffffffff, 0}; its hits are the suffix-array rows start ..
end - 1 in that order.  Written from that contract, not from the kernels:
  slots of a read    1 / 0 for a compact position / COMPACT_NONE, else (end - start) mod 2^32 with the max_hits rule: a read of more
                     than max_hits rows gets no slots ("count only", what the device calls do) or max_hits of them ("take k", what
                     gdx_query_options_t.max_hits_per_query means to the host calls)
  offsets            numpy.cumsum of the slots in uint64, a zero in front
  totals             {offsets[nq], the slots of the reads that say "see the record" (all reads when there are no compact words)}
  hits               the rows' (text id, position) from a per-row table the oracle's locate_intervals filled, or the compact
                     position split at the oracle's sentinel positions.
Pure numpy."""
from __future__ import annotations

import numpy as np

COMPACT_NONE = -1  # 0xffffffff as the int32 the tensors hold
COMPACT_SEE = -2   # 0xfffffffe
NO_HINT = -1       # third word of a record without a hint row


def record_words(starts, ends) -> np.ndarray:
    """int32[nq, 4]: the records of plain finished reads with these row intervals"""
    s = np.asarray(starts, dtype=np.uint64).astype(np.uint32)
    e = np.asarray(ends, dtype=np.uint64).astype(np.uint32)
    rec = np.zeros((s.size, 4), dtype=np.uint32)
    rec[:, 0], rec[:, 1], rec[:, 2] = s, e, np.uint32(0xFFFFFFFF)
    return rec.view(np.int32)


def slot_counts(starts, ends, compact=None, max_hits: int = 0, take: bool = False) -> np.ndarray:
    """uint64[nq]: the hit slots every read gets"""
    s = np.asarray(starts, dtype=np.uint64).astype(np.uint32)
    e = np.asarray(ends, dtype=np.uint64).astype(np.uint32)
    c = (e - s).astype(np.uint64)  # (32-bit wrap-around, as the records' words)
    if max_hits:
        c = np.where(c > np.uint64(max_hits), np.uint64(max_hits if take else 0), c)
    if compact is not None:
        cw = np.asarray(compact, dtype=np.int32)
        c = np.where(cw == COMPACT_SEE, c, np.where(cw == COMPACT_NONE, np.uint64(0), np.uint64(1)))
    return c.astype(np.uint64)


def offsets_of(counts) -> np.ndarray:
    """uint64[nq + 1]"""
    c = np.asarray(counts, dtype=np.uint64)
    off = np.zeros(c.size + 1, dtype=np.uint64)
    np.cumsum(c, dtype=np.uint64, out=off[1:])
    return off


def open_slots(counts, compact=None) -> int:
    """totals[1]: the slots of the reads whose hits come from their records"""
    c = np.asarray(counts, dtype=np.uint64)
    if compact is None:
        return int(c.sum(dtype=np.uint64))
    return int(c[np.asarray(compact, dtype=np.int32) == COMPACT_SEE].sum(dtype=np.uint64))


def split_positions(positions, sentinels):
    """positions in the concatenated texts (one sentinel behind each text) -> (text ids, positions in the text); sentinels:
    the oracle's sentinel_indices, ascending"""
    pos = np.asarray(positions, dtype=np.int64)
    sen = np.asarray(sentinels, dtype=np.int64)
    tid = np.searchsorted(sen, pos, side="left")
    first = np.where(tid > 0, sen[np.maximum(tid, 1) - 1] + 1, 0)
    return tid.astype(np.int64), pos - first


def expected_hits(starts, ends, compact, counts, row_text, row_pos, sentinels) -> np.ndarray:
    """int64[total, 2] = (text id, position) of every hit slot.  row_text / row_pos: the hit of every suffix-array row (the
    oracle's locate_intervals over [0, n)); a read of fewer slots than rows (take k) gets its first rows"""
    c = np.asarray(counts, dtype=np.int64)
    s = np.asarray(starts, dtype=np.int64)
    off = np.zeros(c.size + 1, dtype=np.int64)
    np.cumsum(c, out=off[1:])
    total = int(off[-1])
    owner = np.repeat(np.arange(c.size), c)
    within = np.arange(total, dtype=np.int64) - off[owner]
    rows = s[owner] + within
    out = np.zeros((total, 2), dtype=np.int64)
    by_record = np.ones(total, dtype=bool)
    if compact is not None:
        cw = np.asarray(compact, dtype=np.int32)
        by_record = cw[owner] == COMPACT_SEE
        tid, p = split_positions(cw[owner][~by_record].view(np.uint32).astype(np.int64), sentinels)
        out[~by_record, 0], out[~by_record, 1] = tid, p
    r = rows[by_record]
    out[by_record, 0], out[by_record, 1] = np.asarray(row_text)[r], np.asarray(row_pos)[r]
    return out


def sparse_offsets(at, counts, queries) -> np.ndarray:
    """offsets[queries] of a batch that is empty but for the reads `at` (ascending, distinct), which have `counts` slots: what a
    cumsum over the whole batch would give, without making it"""
    at = np.asarray(at, dtype=np.int64)
    assert np.all(np.diff(at) > 0)
    before = np.zeros(at.size + 1, dtype=np.uint64)
    np.cumsum(np.asarray(counts, dtype=np.uint64), dtype=np.uint64, out=before[1:])
    return before[np.searchsorted(at, np.asarray(queries, dtype=np.int64), side="left")]  # reads in front of q: at < q
