"""The plain model of the offsets scan and store pass (offsets_scan_model.py) against a naive loop over the reads and the CPU
oracle: the GPU tests of the pass (test_gpu_offsets_scan.py) trust it, so it is checked here first, without a GPU."""
import numpy as np
import pytest

import offsets_scan_model as model
from genedex_amd import alphabet as alph
from oracle.oracle import OracleIndex


@pytest.fixture(scope="module")
def small():
    """a collection of five short texts with repeats: (oracle, n, hit of every row, sentinels)"""
    rng = np.random.default_rng(31)
    a = alph.ascii_dna_with_n()
    body = bytes(b"ACGT"[i] for i in rng.integers(0, 4, 900))
    texts = [body[:400], b"ACG" * 120 + body[100:180], b"", body[350:] + b"N" + body[:90], b"T" * 70]
    o = OracleIndex.build(texts, a.io_to_dense_table, a.num_dense_symbols(), a.num_searchable_dense_symbols(), sa_rate=4,
                          lookup_depth=0, width=32)
    n = o.n
    _, t, p = o.locate_intervals([0], [n])
    return o, n, t.astype(np.int64), p.astype(np.int64), o.sentinel_indices.astype(np.int64)


def naive(starts, ends, compact, max_hits, take, o, sentinels):
    """one read after the other, hits through the oracle's locate_interval: (offsets, totals, hits)"""
    off, hits, rest = [0], [], 0
    for q in range(len(starts)):
        cw = None if compact is None else int(compact[q])
        if cw is not None and cw != model.COMPACT_SEE:
            if cw != model.COMPACT_NONE:
                pos = cw & 0xFFFFFFFF
                tid = 0
                while int(sentinels[tid]) < pos:
                    tid += 1
                hits.append((tid, pos - (int(sentinels[tid - 1]) + 1 if tid else 0)))
            off.append(len(hits))
            continue
        n = (int(ends[q]) - int(starts[q])) & 0xFFFFFFFF
        if max_hits and n > max_hits:
            n = max_hits if take else 0
        t, p = o.locate_interval(int(starts[q]), int(starts[q]) + n)
        hits += list(zip(t.tolist(), p.tolist()))
        rest += n
        off.append(len(hits))
    return off, (len(hits), rest), hits


@pytest.mark.parametrize("seed", range(8))
def test_model_equals_a_naive_loop(small, seed):
    """40 random small batches per seed (320 in all): records only and records + compact words, no limit, "count only" and
    "take k" -- offsets, both totals and every hit equal the loop's."""
    o, n, row_t, row_p, sen = small
    sa = o.full_sa.astype(np.int64)
    rng = np.random.default_rng(500 + seed)
    for case in range(40):
        nq = int(rng.integers(0, 70))
        starts = rng.integers(0, n, nq)
        widths = rng.choice([0, 0, 1, 1, 2, 3, 4, 7, 30], nq)
        ends = np.minimum(starts + widths, n)
        compact = None
        if case % 2:
            kind = rng.integers(0, 3, nq)
            compact = np.where(kind == 0, model.COMPACT_SEE, np.where(kind == 1, model.COMPACT_NONE, 0)).astype(np.int32)
            single = kind == 2
            compact[single] = sa[rng.integers(0, n, int(single.sum()))].astype(np.uint32).view(np.int32)
        max_hits, take = [(0, False), (1, False), (2, True), (3, False), (1, True), (30, True)][case % 6]
        counts = model.slot_counts(starts, ends, compact, max_hits, take)
        off = model.offsets_of(counts)
        hits = model.expected_hits(starts, ends, compact, counts, row_t, row_p, sen)
        want_off, want_totals, want_hits = naive(starts, ends, compact, max_hits, take, o, sen)
        assert off.dtype == np.uint64 and off.tolist() == want_off, (seed, case)
        assert (int(off[-1]), model.open_slots(counts, compact)) == want_totals, (seed, case)
        assert [tuple(h) for h in hits.tolist()] == want_hits, (seed, case)


def test_records_and_wrap_around():
    """the record words of a plain finished read, and counts in 32-bit arithmetic as the records hold them"""
    rec = model.record_words([5, 0xFFFFFFFE], [9, 0xFFFFFFFF])
    assert rec.dtype == np.int32 and rec.tolist() == [[5, 9, -1, 0], [-2, -1, -1, 0]]
    assert model.slot_counts([7, 10], [7, 2]).tolist() == [0, 2 ** 32 - 8]
    assert model.slot_counts([0, 0, 0], [2, 3, 4], max_hits=3).tolist() == [2, 3, 0]
    assert model.slot_counts([0, 0, 0], [2, 3, 4], max_hits=3, take=True).tolist() == [2, 3, 3]
    # a compact word wins over the record, whatever the limit
    cw = np.array([model.COMPACT_NONE, 17, model.COMPACT_SEE], dtype=np.int32)
    assert model.slot_counts([0, 0, 0], [9, 9, 9], cw, max_hits=3).tolist() == [0, 1, 0]
    assert model.open_slots([0, 1, 5], cw) == 5 and model.open_slots([0, 1, 5]) == 6


def test_split_positions_at_text_borders(small):
    """first and last symbol of every text and the sentinels themselves (an empty text: only its sentinel)"""
    o, n, row_t, row_p, sen = small
    sa = o.full_sa.astype(np.int64)
    tid, p = model.split_positions(sa, sen)
    assert tid.tolist() == row_t.tolist() and p.tolist() == row_p.tolist()
    tid, p = model.split_positions(sen, sen)
    assert tid.tolist() == list(range(sen.size))
    assert p.tolist() == [int(sen[0])] + (np.diff(sen) - 1).tolist()


@pytest.mark.parametrize("seed", range(3))
def test_sparse_offsets_equal_the_dense_cumsum(seed):
    rng = np.random.default_rng(900 + seed)
    nq = 5000
    at = np.sort(rng.choice(nq, 60, replace=False))
    counts = rng.integers(1, 6, at.size)
    dense = np.zeros(nq, dtype=np.uint64)
    dense[at] = counts.astype(np.uint64)
    want = model.offsets_of(dense)
    q = np.arange(nq + 1)
    assert model.sparse_offsets(at, counts, q).tolist() == want.tolist()
