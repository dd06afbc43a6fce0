"""The exhaustive sweep's collection and model (sweep_model.py), on the CPU: the conditions the collection must meet for the sweep
to visit every kind of entry, and the model itself -- against naive search for every (position, length) of a small collection,
and against the oracle's FM search for every position of the sweep collection, bit for bit and in hit order."""
import numpy as np
import pytest

from genedex_amd import alphabet as alph
from helpers import naive_search
from oracle.oracle import OracleIndex
from sweep_model import (HIT_CAP, K, NEAR_MISS_KINDS, SweepModel, build_sweep_model, kasai_lcp, locate_lengths, near_miss_lengths,
                         oracle_suffix_array, sweep_lengths, sweep_texts)

A = alph.ascii_dna_with_n()


@pytest.fixture(scope="module")
def model():
    return build_sweep_model()


def small_collection():
    rng = np.random.default_rng(5)
    acgt = lambda n: bytes(b"ACGT"[i] for i in rng.integers(0, 4, n))  # noqa: E731
    unit = acgt(23)
    return [acgt(90) + unit + acgt(7) + unit, b"", b"ACGTNNACGTNACG" + unit[:15], b"A", b"N", b"A" * 40 + b"C" + b"AC" * 21, acgt(60)]


# ---- the collection ------------------------------------------------------------------------------------------------------

def test_the_collection_is_fixed_and_has_its_ten_texts(model):
    texts = model.texts
    assert texts == sweep_texts()  # a function of the seed alone
    assert len(texts) == 10
    assert [len(texts[i]) for i in (0, 1, 2, 3, 4, 6, 8, 9)] == [40_000, 0, 20_000, 1, K - 1, K, K + 32, K + 33]
    assert texts[3] == b"A" and b"N" in texts[2] and b"A" * 300 in texts[7] and b"ACGTTGCA" * 60 in texts[7]
    assert all(b"N" not in t for i, t in enumerate(texts) if i != 2)
    assert model.n == sum(len(t) + 1 for t in texts)


def test_rows_on_both_sides_of_a_superblock_border_are_swept(model):
    assert model.n > 65_536 + 4_096


def test_every_kind_of_partial_seed_entry_occurs(model):
    """for every v in 0 .. 32: at least 100 positions start an N-free k-mer with exactly v symbols A C G T of their own text in
    front (32: or more)"""
    _, start = model.kmer_codes(K)
    per_v = np.bincount(model.clean_symbols_in_front(32)[start], minlength=33)
    assert per_v.size == 33 and int(per_v.min()) >= 100, per_v.tolist()


def test_kmers_of_every_row_count_occur(model):
    """k-mers on exactly 1, 2, 3, 4 and >= 5 rows; of those on 2, 3 and 4 rows some have 32 clean symbols in front of every copy"""
    code, start = model.kmer_codes(K)
    _, inverse, counts = np.unique(code, return_inverse=True, return_counts=True)
    assert all(int((counts == m).sum()) > 0 for m in (1, 2, 3, 4)) and int((counts >= 5).sum()) > 0
    full_context = model.clean_symbols_in_front(32)[start] == 32
    lacking = np.bincount(inverse, weights=~full_context, minlength=counts.size)
    for m in (2, 3, 4):
        assert int(((counts == m) & (lacking == 0)).sum()) > 0, m
    # and the model's intervals say the same of them
    lo, hi = model.intervals(K)
    assert np.array_equal((hi - lo)[model.clean(K)], counts[inverse])


def test_total_hits_stay_below_the_cap_at_every_locate_length(model):
    totals = {ln: model.total_hits(ln) for ln in locate_lengths(K)}
    assert all(t <= HIT_CAP for t in totals.values()), totals
    # (hits only fall with the length: every length a variant with another k sweeps is covered by the shortest)
    assert model.total_hits(8) <= HIT_CAP and list(totals.values()) == sorted(totals.values(), reverse=True)


def test_the_sweep_leaves_no_row_and_no_kmer_out(model):
    """at length 1 the reads' rows are all rows but the sentinels'; at length k the reads' seeds are all N-free k-mers"""
    rows = np.sort(model.isa[model.windows(1)[0]])
    assert np.array_equal(rows, np.flatnonzero(model.dense[model.sa] != 0))
    assert rows.size == model.n - len(model.texts)
    for k in (9, 10, K, 16):
        code, _ = model.kmer_codes(k)
        reads = model.gathered(k)[model.clean(k)]
        seeds = np.zeros(reads.shape[0], dtype=np.int64)
        for j in range(k):
            seeds = seeds * 4 + (A.io_to_dense_table[reads[:, j]].astype(np.int64) - 1)
        assert np.array_equal(np.unique(seeds), np.unique(code))


# ---- the model against naive search ----------------------------------------------------------------------------------------

def test_model_equals_naive_search_for_every_position_and_length():
    texts = small_collection()
    m = SweepModel(texts, A, oracle_suffix_array(texts, A))
    assert 200 < m.n < 500
    checked = 0
    for length in range(1, max(len(t) for t in texts) + 1):
        _, tid, pos = m.windows(length)
        assert tid.size == sum(max(len(t) - length + 1, 0) for t in texts)
        lo, hi = m.intervals(length)
        off, ht, hp = m.hits(length)
        reads = m.gathered(length)
        counts = m.window_counts(reads)
        for i in range(tid.size):
            q = texts[int(tid[i])][int(pos[i]):int(pos[i]) + length]
            assert reads[i].tobytes() == q
            want = naive_search(texts, q)
            got = list(zip(ht[off[i]:off[i + 1]].tolist(), hp[off[i]:off[i + 1]].tolist()))
            assert len(got) == len(want) == int(hi[i] - lo[i]) == int(counts[i]) and set(got) == want, (length, i, q)
            checked += 1
    assert checked > 5000


def test_near_misses_are_counted_like_naive_search():
    texts = small_collection()
    m = SweepModel(texts, A, oracle_suffix_array(texts, A))
    k = 5
    for length in (k, k + 1, 9, 14):
        original = m.gathered(length)
        for kind in NEAR_MISS_KINDS:
            if kind == "before-seed" and length == k:
                with pytest.raises(ValueError):
                    m.near_misses(length, kind, k)
                continue
            reads = m.near_misses(length, kind, k)
            at = {"last": length - 1, "first": 0, "before-seed": length - k - 1}[kind]
            changed = reads != original
            assert changed[:, at].all() and int(changed.sum()) == reads.shape[0]
            assert set(reads[:, at].tolist()) <= set(b"ACGT")
            counts = m.window_counts(reads)
            for i in range(reads.shape[0]):
                assert int(counts[i]) == len(naive_search(texts, reads[i].tobytes())), (length, kind, i)


def test_lcp_is_cut_at_sentinels():
    texts = [b"ACGT", b"ACGT", b"ACG"]
    m = SweepModel(texts, A, oracle_suffix_array(texts, A))
    assert int(m.lcp.max()) == 4  # the two ACGT: not 5 through the equal sentinels
    assert kasai_lcp(m.dense, m.sa).tolist() == m.lcp.tolist()
    lo, hi = m.intervals(3)
    assert (hi - lo).tolist() == [3, 2, 3, 2, 3]  # ACG, CGT | ACG, CGT | ACG


# ---- the model against the oracle's FM search --------------------------------------------------------------------------------

@pytest.mark.parametrize("length", [8, K + 33, 256])
def test_model_equals_oracle_for_every_position(model, length):
    """intervals, hit offsets and hits in the oracle's order, for the read ending at every position of the sweep collection"""
    c = OracleIndex.build(model.texts, A.io_to_dense_table, 6, 4, sa_rate=4, lookup_depth=0, width=32)
    assert c.n == model.n
    qbuf, qoff = model.reads(length)
    assert qoff.size - 1 == int(np.maximum(model.text_len - length + 1, 0).sum())
    cs, ce = c.cursors_for_many(qbuf, qoff, n_threads=4)
    lo, hi = model.intervals(length)
    assert np.array_equal(cs.astype(np.int64), lo) and np.array_equal(ce.astype(np.int64), hi)
    co, ct, cp = c.locate_intervals(cs, ce, n_threads=4)
    off, tid, pos = model.hits(length)
    assert np.array_equal(co.astype(np.int64), off)
    assert np.array_equal(ct.astype(np.int64), tid) and np.array_equal(cp.astype(np.int64), pos)
    # near misses: the oracle's counts are the dictionary's
    if length in near_miss_lengths(K):
        for kind in NEAR_MISS_KINDS:
            reads = model.near_misses(length, kind, K)
            ms, me = c.cursors_for_many(*model.as_batch(reads), n_threads=4)
            assert np.array_equal((me - ms).astype(np.int64), model.window_counts(reads)), kind


def test_sweep_lengths():
    assert sweep_lengths(K) == [1, 2, 3, 11, 12, 13, 43, 44, 45, 75, 76, 77, 150, 256]
    assert locate_lengths(K) == sweep_lengths(K)[3:] and locate_lengths(9)[0] == 8
    assert near_miss_lengths(K) == [12, 13, 44, 45, 76]
