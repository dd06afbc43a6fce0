"""The plain model of the suffix sorter (suffix_array_model.py) against brute force, the CPU oracle and values worked out by
hand: the GPU tests of the sorter (test_gpu_suffix_sort.py) trust it, so it is checked here first, without a GPU."""
import numpy as np
import pytest

import suffix_array_model as model
from genedex_amd import alphabet as alph
from oracle.oracle import OracleIndex

DNA = alph.ascii_dna()                       # sigma 5: h0 = 22
AC = alph.Alphabet.from_io_symbols(b"AC")    # sigma 3: h0 = 33


def small_texts():
    """a few hundred (dense text, name): random over 1 .. 4 symbols, periodic, degenerate, many sentinels"""
    rng = np.random.default_rng(2718)
    out = []
    for k in range(160):
        sigma = 2 + k % 4
        n = int(rng.integers(0, 120))
        out.append((rng.integers(0, sigma, n).astype(np.uint8), f"random{k}"))
    for k in range(80):
        unit = rng.integers(1, 3 + k % 3, int(rng.integers(1, 9))).astype(np.uint8)
        body = np.tile(unit, 40)[: int(rng.integers(1, 150))]
        out.append((np.concatenate([body, np.zeros(1, dtype=np.uint8)]), f"periodic{k}"))
    for k in range(40):
        out.append((np.concatenate([np.full(k, 1, dtype=np.uint8), np.zeros(1 + k % 3, dtype=np.uint8)]), f"run{k}"))
    out += [(np.zeros(0, dtype=np.uint8), "empty"), (np.zeros(1, dtype=np.uint8), "one sentinel"),
            (np.zeros(57, dtype=np.uint8), "sentinels only"), (np.arange(200, dtype=np.uint8)[::-1].copy(), "descending"),
            (np.concatenate([model.fibonacci_bits(233) + 1, [0]]).astype(np.uint8), "fibonacci"),
            (np.concatenate([model.thue_morse_bits(256) + 1, [0]]).astype(np.uint8), "thue-morse")]
    return out


SMALL = small_texts()


def naive_max_lcp(b: bytes) -> int:
    best = 0
    for i in range(len(b)):
        for j in range(i + 1, len(b)):
            h = 0
            while j + h < len(b) and b[i + h] == b[j + h]:
                h += 1
            best = max(best, h)
    return best


def test_checker_accepts_the_brute_force_array():
    assert len(SMALL) > 250
    for dense, name in SMALL:
        sa = model.brute_suffix_array(dense)
        assert model.check_suffix_array(dense, sa) is None, name
        assert model.check_suffix_array(dense, sa.astype(np.uint32)) is None, name  # (the library's export is u32)
        want = naive_max_lcp(dense.tobytes()) if dense.size <= 160 else None
        got = model.max_lcp_kasai(dense, sa)
        assert want is None or got == want, name
        for cap in (0, 1, 7, 1000):
            assert model.max_lcp_capped(dense, sa, cap) == min(got, cap), (name, cap)


def tie_rows(dense, sa):
    """rows j whose suffix starts with the symbol of row j + 1's (one first-symbol tie group)"""
    if sa.size < 2:
        return np.zeros(0, dtype=np.int64)
    return np.flatnonzero(dense[sa[:-1]] == dense[sa[1:]])


def test_checker_rejects_swapped_neighbours_of_a_tie_group():
    hit = 0
    for dense, name in SMALL:
        sa = model.brute_suffix_array(dense)
        rows = tie_rows(dense, sa)
        for j in rows[:: max(1, rows.size // 6)].tolist():
            bad = sa.copy()
            bad[j], bad[j + 1] = sa[j + 1], sa[j]
            row = model.check_suffix_array(dense, bad, raise_on_error=False)
            assert row is not None, (name, j)  # (it may lie before j: the rows of the suffixes one symbol longer see the swap too)
            with pytest.raises(AssertionError, match=f"first offending row {row} "):
                model.check_suffix_array(dense, bad)
            hit += 1
    assert hit > 500


def test_checker_rejects_a_duplicated_value():
    rng = np.random.default_rng(5)
    hit = 0
    for dense, name in SMALL:
        if dense.size < 2:
            continue
        sa = model.brute_suffix_array(dense)
        for _ in range(3):
            src, dst = (int(x) for x in rng.choice(dense.size, 2, replace=False))
            bad = sa.copy()
            bad[dst] = sa[src]
            assert model.check_suffix_array(dense, bad, raise_on_error=False) == max(src, dst), (name, src, dst)
            hit += 1
    assert hit > 500
    assert model.check_suffix_array(np.array([1, 1, 0], dtype=np.uint8), [2, 1, 3], raise_on_error=False) == 2  # out of range
    assert model.check_suffix_array(np.array([1, 1, 0], dtype=np.uint8), [2, 1], raise_on_error=False) == 2     # too short


def test_checker_rejects_a_moved_row():
    rng = np.random.default_rng(6)
    hit = 0
    for dense, name in SMALL:
        if dense.size < 3:
            continue
        sa = model.brute_suffix_array(dense)
        for _ in range(3):
            src, dst = (int(x) for x in rng.choice(dense.size, 2, replace=False))
            bad = np.insert(np.delete(sa, src), dst, sa[src])
            assert bad.size == sa.size and sorted(bad.tolist()) == sorted(sa.tolist())
            row = model.check_suffix_array(dense, bad, raise_on_error=False)
            assert row is not None, (name, src, dst)
            hit += 1
    assert hit > 500


@pytest.mark.parametrize("seed", range(6))
def test_checker_and_bwt_against_the_oracle(seed):
    rng = np.random.default_rng(40 + seed)
    a = [DNA, alph.ascii_dna_with_n(), AC, alph.u8_until(254), alph.ascii_amino_acid(), DNA][seed]
    symbols = [b"ACGT", b"ACGTN", b"AC", bytes(range(255)), b"ACDEFGHIKLMNPQRSTVWY", b"AC"][seed]
    texts = [bytes(symbols[i] for i in rng.integers(0, len(symbols), int(rng.integers(0, 3000)))) for _ in range(4)]
    texts += [b"", model.repeat_to(texts[0][:7], 500)]
    o = OracleIndex.build(texts, a.io_to_dense_table, a.num_dense_symbols(), a.num_searchable_dense_symbols(), sa_rate=1,
                          lookup_depth=0, width=32)
    dense = model.dense_concat(texts, a)
    assert dense.tolist() == o.dense_text.tolist()
    sa = o.sa_samples  # rate 1: every row
    assert sa.size == dense.size and model.check_suffix_array(dense, sa) is None
    assert sa.tolist() == model.brute_suffix_array(dense).tolist()
    assert model.bwt_from_sa(dense, sa).tolist() == o.bwt.tolist()


def test_initial_order_by_alphabet_size():
    # symbols + sentinel = sigma; a symbol is stored as symbol + 1 in the bits that hold 0 .. sigma
    assert [model.initial_order(s) for s in (2, 3, 4, 5, 6, 7, 8, 15, 16, 21, 31, 32, 127, 128, 255, 256)] == \
        [33, 33, 22, 22, 22, 22, 17, 17, 13, 13, 13, 11, 10, 9, 9, 8]


@pytest.mark.parametrize("a,h0", [(DNA, 22), (AC, 33)])
def test_a_run_of_one_symbol_by_hand(a, h0):
    """A^m $: suffix i is A^(m-i) $, the LCP of suffixes i < j is m - j, so max LCP = m - 1.  The windows of h0 symbols of the
    m + 1 - h0 longest suffixes are all A^h0, every other window holds the sentinel at a place of its own: m + 1 - h0 pending
    where that is at least two suffixes (one suffix alone shares its window with nobody), else none."""
    sigma = a.num_dense_symbols()
    assert model.initial_order(sigma) == h0
    for m in [0, 1, 10, h0 - 1, h0, h0 + 1, h0 + 2, 2 * h0 - 1, 2 * h0, 2 * h0 + 1, 4 * h0, h0 * 2 ** 7 - 1, h0 * 2 ** 7,
              h0 * 2 ** 7 + 1]:
        dense = model.dense_concat([b"A" * m], a)
        sa = model.brute_suffix_array(dense)
        assert sa.tolist() == list(range(m, -1, -1))
        shared = m + 1 - h0
        assert model.pending_after_key_sort(dense, sigma) == (shared if shared >= 2 else 0), m
        assert model.max_lcp_kasai(dense, sa) == max(m - 1, 0)
        rounds = model.doubling_rounds(dense, sa, sigma)
        if m <= h0:
            assert rounds == 0, m
        else:
            assert h0 * 2 ** (rounds - 1) <= m - 1 < h0 * 2 ** rounds, m
    assert model.pending_after_key_sort(model.dense_concat([b"A" * 10], a), sigma) == 0
    assert [model.doubling_rounds(d, model.brute_suffix_array(d), sigma)
            for d in (model.dense_concat([b"A" * m], a) for m in (h0, h0 + 1, 2 * h0, 2 * h0 + 1, h0 * 2 ** 7, h0 * 2 ** 7 + 1))] \
        == [0, 1, 1, 2, 7, 8]


def test_a_unit_of_five_repeated_to_sixty_by_hand():
    """u^12 $ with a primitive unit u of 5 symbols: suffixes i < j with j - i a multiple of 5 agree up to the end of the text,
    LCP = 60 - j, so max LCP = 55; two suffixes out of step agree on fewer than 2 * 5 symbols.  A window of h0 > 10 symbols is
    shared by the suffixes that start at 0 .. 60 - h0 (each has a partner one period away) and by nobody else."""
    rng = np.random.default_rng(12)
    for _ in range(20):
        unit = bytes(b"AC"[i] for i in rng.integers(0, 2, 5))
        if unit in (b"AAAAA", b"CCCCC"):
            continue  # not primitive
        text = unit * 12
        for a, h0, rounds in ((DNA, 22, 2), (AC, 33, 1)):  # 22 * 2 <= 55 < 22 * 4;  33 <= 55 < 33 * 2
            sigma = a.num_dense_symbols()
            dense = model.dense_concat([text], a)
            sa = model.brute_suffix_array(dense)
            assert model.max_lcp_kasai(dense, sa) == 55
            assert model.pending_after_key_sort(dense, sigma) == 60 - h0 + 1
            assert model.doubling_rounds(dense, sa, sigma) == rounds


def test_shared_windows_against_a_dictionary():
    for dense, name in SMALL[::3]:
        b = bytes(dense + 1)
        for width in (1, 2, 9, 33):
            seen = {}
            for i in range(len(b)):
                w = b[i:i + width].ljust(width, b"\0")
                seen[w] = seen.get(w, 0) + 1
            want = sum(c for c in seen.values() if c > 1)
            assert model.shared_window_count(dense, width) == want, (name, width)


def test_structured_words():
    fib = model.fibonacci_bits(10946)
    assert fib[:13].tolist() == [0, 1, 0, 0, 1, 0, 1, 0, 0, 1, 0, 0, 1] and int(fib.sum()) == 4181
    tm = model.thue_morse_bits(8192)
    assert tm[:16].tolist() == [0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0]
    db = model.de_bruijn_bits(13)
    assert db.size == 8192 + 12
    s = bytes(db)
    assert len({s[i:i + 13] for i in range(8192)}) == 8192                 # every 13-mer once
    twelve = [s[i:i + 12] for i in range(8193)]
    assert len(set(twelve)) == 4096 and all(twelve.count(w) <= 3 for w in set(twelve[:50]))
    assert model.bits_to_text([0, 1, 1], b"AC") == b"ACC"
