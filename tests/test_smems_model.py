"""The CPU model of gdx_smems_many (super-maximal exact matches of a read, found by a walk that alternates between the index
of the texts and the index of the reversed texts), the check of that model against brute-force substring search, and the
ABI bookkeeping of the two new calls (header, ctypes stub, Rust declarations).  tests/test_gpu_smems.py holds the GPU
against this model."""
import os
import re

import numpy as np
import pytest

from genedex_amd import alphabet as alph
from helpers import random_texts
from test_suffix_segments_model import occurrences, reads_with_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gdx_smems_many", "gdx_smems_many_dev")


def model_one(F, R, q, max_smems, min_length):
    """One query, exactly as the walk in include/gdx.h reads, on OracleIndex.extend_front (Cursor::extend_query_front).
    F indexes the texts, R the same texts each reversed.
    Returns (n_smems, remaining, [(begin, length, start, end), ...], status)."""
    m = len(q)
    p = m - 1
    smems = []
    while p >= 0 and len(smems) < max_smems:
        lo, hi, e = 0, R.n, p  # forward pass on R: the longest e with q[p:e] occurring
        while e < m:
            s2, e2, st = R.extend_front(lo, hi, q[e])
            if st:  # a symbol outside the alphabet that the walk reaches, also as the symbol that blocks
                return 0, m, [], 1
            if s2 == e2:
                break
            lo, hi, e = s2, e2, e + 1
        if e == p:  # q[p] occurs nowhere: no SMEM covers p
            p -= 1
            continue
        lo, hi, s = 0, F.n, e  # backward pass on F: the longest match that ends at e
        while s > 0:
            s2, e2, st = F.extend_front(lo, hi, q[s - 1])
            if st:
                return 0, m, [], 1
            if s2 == e2:
                break
            lo, hi, s = s2, e2, s - 1
        assert s <= p
        if e - s >= min_length:
            smems.append((s, e - s, lo, hi))
        p = s - 1
    return len(smems), (p + 1 if p >= 0 else 0), smems, 0


def model_arrays(F, R, queries, max_smems, min_length):
    """The six output arrays (+ status) of the call for a list of queries."""
    nq = len(queries)
    n_smems = np.zeros(nq, dtype=np.uint32)
    remaining = np.zeros(nq, dtype=np.uint32)
    begin = np.zeros(nq * max_smems, dtype=np.uint32)
    length = np.zeros(nq * max_smems, dtype=np.uint32)
    start = np.zeros(nq * max_smems, dtype=np.uint64)
    end = np.zeros(nq * max_smems, dtype=np.uint64)
    status = np.zeros(nq, dtype=np.uint8)
    for i, q in enumerate(queries):
        n_smems[i], remaining[i], smems, status[i] = model_one(F, R, bytes(q), max_smems, min_length)
        for j, (b, ln, s, e) in enumerate(smems):
            k = i * max_smems + j
            begin[k], length[k], start[k], end[k] = b, ln, s, e
    return n_smems, remaining, begin, length, start, end, status


def oracle_pair(texts, a, sa_rate=4):
    """(F, R): the oracle's index of the texts and of the texts each reversed"""
    from oracle.oracle import OracleIndex

    def build(ts):
        return OracleIndex.build(ts, a.io_to_dense_table, a.num_dense_symbols(), a.num_searchable_dense_symbols(),
                                 sa_rate=sa_rate, lookup_depth=0, width=32)

    return build(texts), build([bytes(t)[::-1] for t in texts])


def brute_force_smems(texts, q):
    """Every (b, e), b < e, whose substring q[b:e] is in some text, reduced to those not contained in another; by descending
    end.  (For one e the b are tried downwards and the search stops at the first substring that is in no text: a longer
    one that ends at the same e contains it and is in no text either.)"""
    matches = set()
    for e in range(1, len(q) + 1):
        b = e - 1
        while b >= 0 and any(q[b:e] in t for t in texts):
            matches.add((b, e))
            b -= 1
    by_end = {}
    for b, e in matches:  # the longest match of every end: the only one of that end that no other of that end contains
        by_end[e] = min(b, by_end.get(e, b))
    longest = [(b, e) for e, b in by_end.items()]
    smems = [(b, e) for b, e in longest if not any((b2, e2) != (b, e) and b2 <= b and e <= e2 for b2, e2 in longest)]
    return sorted(smems, key=lambda be: -be[1])


# ------------------------------------------------------------------------------------------------
# (a) the yardstick itself: the model against brute force

SEEDS = range(6)
_CASES = {}


def _case(seed):
    if seed not in _CASES:
        rng = np.random.default_rng(8000 + seed)
        with_n = seed % 2 == 1
        a = alph.ascii_dna_with_n() if with_n else alph.ascii_dna()
        symbols = b"ACGTN" if with_n else b"ACGT"
        texts = random_texts(rng, len_max=[300, 1500, 40][seed % 3], symbols=symbols)
        qs = reads_with_errors(rng, texts, 60, 30, 120, symbols=symbols) + [b"", b"A", bytes(texts[0])]
        _CASES[seed] = (texts, oracle_pair(texts, a), qs)
    return _CASES[seed]


@pytest.mark.parametrize("seed", SEEDS)
def test_model_equals_brute_force(seed):
    texts, (F, R), qs = _case(seed)
    for q in qs:
        want_all = brute_force_smems(texts, q)
        for max_smems in (1, 2, 64):
            for min_length in (1, 8):
                n_smems, remaining, smems, status = model_one(F, R, q, max_smems, min_length)
                assert status == 0 and n_smems == len(smems) <= max_smems
                want = [(b, e) for b, e in want_all if e - b >= min_length][:max_smems]
                assert [(b, b + ln) for b, ln, _, _ in smems] == want, (q, max_smems, min_length)  # the set and the order
                for b, ln, s, en in smems:
                    assert en - s == occurrences(texts, q[b:b + ln]) > 0
                if n_smems < max_smems:
                    assert remaining == 0
                else:  # the walk stopped right after its last record: everything left of that SMEM's begin is unseen
                    assert remaining == smems[-1][0]
                if max_smems == 1 and remaining > 0:  # a cut read
                    assert remaining == smems[0][0]


def test_the_inputs_hold_cut_reads_and_reads_with_more_than_two_smems():
    """what test_model_equals_brute_force asserts about cuts and order needs reads that have them"""
    n_reads = n_many = n_cut = 0
    for seed in SEEDS:
        _, (F, R), qs = _case(seed)
        for q in qs:
            n_reads += 1
            n_many += model_one(F, R, q, 64, 1)[0] > 2
            n_cut += model_one(F, R, q, 1, 1)[1] > 0
    print(f"{n_reads} reads, {n_many} with more than two SMEMs, {n_cut} cut at max_smems = 1")
    assert n_many * 5 >= n_reads and n_cut * 5 >= n_reads, (n_reads, n_many, n_cut)


def test_model_reports_a_symbol_outside_the_alphabet_only_when_reached():
    a = alph.ascii_dna()
    F, R = oracle_pair([b"ACGTACGGT"], a)
    # the backward pass from the read's end runs "T", "GT", "GGT" and then meets the X
    assert model_one(F, R, b"AXGGT", 4, 1) == (0, 5, [], 1)
    assert model_one(F, R, b"AXGGT", 1, 1) == (0, 5, [], 1)
    # "XTTGGT": "TGGT" does not occur, so the first SMEM is "GGT" = [3, 6) and one SMEM never looks at the X ...
    n_smems, remaining, smems, status = model_one(F, R, b"XTTGGT", 1, 1)
    assert (n_smems, remaining, status) == (1, 3, 0) and smems[0][:2] == (3, 3)
    # ... nor does min_length keep the walk from reaching it
    assert model_one(F, R, b"XTTGGT", 8, 1) == (0, 6, [], 1)
    assert model_one(F, R, b"XTTGGT", 8, 3) == (0, 6, [], 1)
    assert model_one(F, R, b"", 3, 1) == (0, 0, [], 0)
    # the forward pass meets it too: T occurs in no text here, so the walk steps over it and starts a pass at the X
    F2, R2 = oracle_pair([b"ACGACGG"], a)
    assert model_one(F2, R2, b"AXT", 4, 1) == (0, 3, [], 1)
    assert model_one(F2, R2, b"ACGTT", 4, 1)[::3] == (1, 0) and model_one(F2, R2, b"ACGTT", 4, 1)[2][0][:2] == (0, 3)
    # a valid symbol that blocks the forward pass is no error: [1, 2) = "A" is found, the X then stops the backward pass
    assert model_one(F2, R2, b"XAT", 1, 1) == (0, 3, [], 1)
    assert model_one(F2, R2, b"TAT", 4, 1)[:2] == (1, 0)


# ------------------------------------------------------------------------------------------------
# (b) the two calls are declared everywhere a binding looks for them

def _header_arg_counts():
    src = open(os.path.join(ROOT, "include", "gdx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(gdx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = len([x for x in args.split(",") if x.strip()])
    return out


def test_header_declares_both_calls():
    counts = _header_arg_counts()
    assert counts.get("gdx_smems_many") == 14
    assert counts.get("gdx_smems_many_dev") == 15


def test_ctypes_stub_has_both_calls_with_the_header_argument_counts():
    from genedex_amd import _lib

    counts = _header_arg_counts()
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name]) == counts[name], name


def test_rust_binding_declares_both_calls():
    src = open(os.path.join(ROOT, "bindings", "rust", "gdx.rs")).read()
    for name in NAMES:
        assert re.search(r"pub fn " + name + r"\s*\(", src), name
    assert re.search(r"pub fn smems_many\b", src)  # the safe wrapper of GpuFmIndex


def test_reversed_texts_helper():
    import genedex_amd

    assert genedex_amd.reversed_texts([b"ACGT", b"", bytearray(b"GA")]) == [b"TGCA", b"", b"AG"]
