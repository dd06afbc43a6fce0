"""The CPU model of gdx_suffix_segments_many (greedy backward factorisation of a read into its longest matching
suffix segments), the check of that model against plain substring search, and the ABI bookkeeping of the two new
calls (header, ctypes stub, Rust declarations).  tests/test_gpu_suffix_segments.py holds the GPU against this model."""
import os
import re

import numpy as np
import pytest

from genedex_amd import alphabet as alph
from helpers import random_texts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gdx_suffix_segments_many", "gdx_suffix_segments_many_dev")


def model_one(ix, q, max_segments):
    """One query, exactly as the definition reads, on OracleIndex.extend_front (Cursor::extend_query_front).
    Returns (n_segments, remaining, [(length, start, end), ...], status)."""
    m = len(q)
    e = m
    segments = []
    while e > 0 and len(segments) < max_segments:
        lo, hi, length = 0, ix.n, 0
        while e - length > 0:
            s2, e2, st = ix.extend_front(lo, hi, q[e - length - 1])
            if st:  # a symbol outside the alphabet that the walk reaches
                return 0, m, [], 1
            if s2 == e2:
                break
            lo, hi, length = s2, e2, length + 1
        if length > 0:
            segments.append((length, lo, hi))
            e -= length
        else:
            segments.append((0, 0, 0))
            e -= 1
    return len(segments), e, segments, 0


def model_arrays(ix, queries, max_segments):
    """The five output arrays (+ status) of the call for a list of queries."""
    nq = len(queries)
    n_seg = np.zeros(nq, dtype=np.uint32)
    remaining = np.zeros(nq, dtype=np.uint32)
    length = np.zeros(nq * max_segments, dtype=np.uint32)
    start = np.zeros(nq * max_segments, dtype=np.uint64)
    end = np.zeros(nq * max_segments, dtype=np.uint64)
    status = np.zeros(nq, dtype=np.uint8)
    for i, q in enumerate(queries):
        n_seg[i], remaining[i], segments, status[i] = model_one(ix, bytes(q), max_segments)
        for j, (ln, s, e) in enumerate(segments):
            length[i * max_segments + j], start[i * max_segments + j], end[i * max_segments + j] = ln, s, e
    return n_seg, remaining, length, start, end, status


def reads_with_errors(rng, texts, n_sampled, n_random, max_len, symbols=b"ACGT", max_subst=3):
    """reads sampled from the texts with 0..max_subst substitutions, plus purely random ones, lengths 0..max_len"""
    qs = []
    nonempty = [t for t in texts if len(t) > 0]
    for _ in range(n_sampled):
        if not nonempty:
            break
        t = nonempty[int(rng.integers(0, len(nonempty)))]
        ln = int(rng.integers(0, min(max_len, len(t)) + 1))
        p = int(rng.integers(0, len(t) - ln + 1))
        q = bytearray(t[p:p + ln])
        for _ in range(int(rng.integers(0, max_subst + 1))):
            if ln:
                q[int(rng.integers(0, ln))] = symbols[int(rng.integers(0, len(symbols)))]
        qs.append(bytes(q))
    for _ in range(n_random):
        ln = int(rng.integers(0, max_len + 1))
        qs.append(bytes(symbols[i] for i in rng.integers(0, len(symbols), ln)))
    order = rng.permutation(len(qs))
    return [qs[i] for i in order]


def occurrences(texts, sub):
    n = 0
    for t in texts:
        p = t.find(sub)
        while p >= 0:
            n += 1
            p = t.find(sub, p + 1)
    return n


# ------------------------------------------------------------------------------------------------
# (a) the yardstick itself: the model against plain substring search

@pytest.mark.parametrize("seed", range(6))
def test_model_equals_plain_substring_search(seed):
    from oracle.oracle import OracleIndex

    rng = np.random.default_rng(7000 + seed)
    with_n = seed % 2 == 1
    a = alph.ascii_dna_with_n() if with_n else alph.ascii_dna()
    symbols = b"ACGTN" if with_n else b"ACGT"
    texts = random_texts(rng, len_max=[300, 1500, 40][seed % 3], symbols=symbols)
    ix = OracleIndex.build(texts, a.io_to_dense_table, a.num_dense_symbols(), a.num_searchable_dense_symbols(),
                           sa_rate=4, lookup_depth=0, width=32)
    qs = reads_with_errors(rng, texts, 60, 30, 120, symbols=symbols) + [b"", b"A", bytes(texts[0])]
    seen_cut = seen_many = False
    for max_segments in (1, 2, 8):
        for q in qs:
            n_seg, remaining, segments, status = model_one(ix, q, max_segments)
            assert status == 0 and n_seg == len(segments) <= max_segments
            e = len(q)
            for ln, s, en in segments:
                # the longest suffix of q[:e] that is a substring of some text
                want = 0
                while want < e and any(q[e - want - 1:e] in t for t in texts):
                    want += 1
                assert ln == want, (q, e)
                if ln:
                    assert en - s == occurrences(texts, q[e - ln:e]) > 0
                else:
                    assert (s, en) == (0, 0)
                e -= max(ln, 1)
            assert remaining == e
            assert remaining == 0 or n_seg == max_segments
            seen_cut |= remaining > 0
            seen_many |= n_seg > 2
    assert seen_cut and seen_many


def test_model_reports_a_symbol_outside_the_alphabet_only_when_reached():
    from oracle.oracle import OracleIndex

    a = alph.ascii_dna()
    ix = OracleIndex.build([b"ACGTACGGT"], a.io_to_dense_table, a.num_dense_symbols(), a.num_searchable_dense_symbols(),
                           sa_rate=4, lookup_depth=0, width=32)
    assert model_one(ix, b"AXGGT", 4) == (0, 5, [], 1)
    # with one segment the walk stops at the X's right neighbour only if that one blocks; here "GGT" extends to the X
    assert model_one(ix, b"AXGGT", 1) == (0, 5, [], 1)
    # "XTTGGT": "TGGT" does not occur, so the first segment is "GGT" and one segment never looks at the X
    n_seg, remaining, segments, status = model_one(ix, b"XTTGGT", 1)
    assert (n_seg, remaining, status) == (1, 3, 0) and segments[0][0] == 3
    assert model_one(ix, b"XTTGGT", 8) == (0, 6, [], 1)
    assert model_one(ix, b"", 3) == (0, 0, [], 0)


# ------------------------------------------------------------------------------------------------
# (b) the two calls are declared everywhere a binding looks for them

def _header_arg_counts():
    src = open(os.path.join(ROOT, "include", "gdx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(gdx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = len([x for x in args.split(",") if x.strip()])
    return src, out


def test_header_declares_both_calls_and_the_flag():
    src, counts = _header_arg_counts()
    assert counts.get("gdx_suffix_segments_many") == 12
    assert counts.get("gdx_suffix_segments_many_dev") == 13
    assert re.search(r"#define\s+GDX_SEGMENTS_LF_ONLY\s+1u", src)


def test_ctypes_stub_has_both_calls_with_the_header_argument_counts():
    from genedex_amd import _lib

    _, counts = _header_arg_counts()
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name]) == counts[name], name
    assert _lib.GDX_SEGMENTS_LF_ONLY == 1


def test_rust_binding_declares_both_calls():
    src = open(os.path.join(ROOT, "bindings", "rust", "gdx.rs")).read()
    for name in NAMES:
        assert re.search(r"pub fn " + name + r"\s*\(", src), name
    assert re.search(r"pub fn suffix_segments_many\b", src)  # the safe wrapper of GpuFmIndex
