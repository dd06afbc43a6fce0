"""The CPU model of gdx_hamming_many (Hamming verification of located seeds against the text), written straight from the
definition in include/gdx.h on bytes and the alphabet's io_to_dense table alone -- no index, no oracle --, its check against
hand-worked cases, and the ABI bookkeeping of the two new calls (header, library, ctypes stub, Rust declarations).
tests/test_gpu_hamming.py holds the GPU against this model."""
import ctypes
import os
import re

import numpy as np

from genedex_amd import alphabet as alph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gdx_hamming_many", "gdx_hamming_many_dev")
INVALID = 0xFFFFFFFF


def hamming_model(texts, alphabet, queries, cand_query, cand_begin, hits, max_mismatches):
    """out[c] = min(dist, max_mismatches + 1) where dist counts the symbols j of q = queries[cand_query[c]] that do NOT match:
    j matches when 0 <= s + j < |T|, dense(q[j]) is one of 1..4 and dense(T[s + j]) == dense(q[j]), with T = texts[text_id]
    and s = position - cand_begin[c].  INVALID for cand_query[c] >= len(queries) or text_id >= len(texts)."""
    dense = np.asarray(alphabet.io_to_dense_table, dtype=np.uint8)
    tq = [dense[np.frombuffer(bytes(q), dtype=np.uint8)].astype(np.int64) for q in queries]
    tt = [dense[np.frombuffer(bytes(t), dtype=np.uint8)].astype(np.int64) for t in texts]
    out = np.zeros(len(cand_query), dtype=np.uint32)
    for c, (qi, b, (text_id, position)) in enumerate(zip(cand_query, cand_begin, hits)):
        qi, b, text_id, position = int(qi), int(b), int(text_id), int(position)
        if qi >= len(queries) or text_id >= len(texts):
            out[c] = INVALID
            continue
        q, t = tq[qi], tt[text_id]
        at = position - b + np.arange(q.size, dtype=np.int64)           # s + j
        inside = (at >= 0) & (at < t.size)
        tsym = np.zeros(q.size, dtype=np.int64)
        tsym[inside] = t[at[inside]]
        match = inside & (q >= 1) & (q <= 4) & (tsym == q)
        out[c] = min(int(q.size - match.sum()), int(max_mismatches) + 1)
    return out


# ------------------------------------------------------------------------------------------------
# (a) the model against cases worked by hand

A = alph.ascii_dna_with_n()
#            0         1         2
#            0123456789012345678901
T0 = b"ACGTTGCAAGGCTTAACCGGAT"
T1 = b"ATCCGGAA"          # what would continue T0[18:] + ... : see test_a_neighbouring_text
BIG = 1 << 31


def one(texts, q, begin, text_id, position, k=BIG, a=A):
    return int(hamming_model(texts, a, [q], [0], [begin], [(text_id, position)], k)[0])


def test_identical_window_and_one_substitution():
    assert one([T0], T0[3:15], 0, 0, 3) == 0
    assert one([T0], T0[3:15], 5, 0, 8) == 0                      # the same diagonal named by a seed that begins at symbol 5
    assert one([T0], T0, 0, 0, 0) == 0
    assert one([T0], b"ACGTTGCTAGG", 0, 0, 0) == 1                # A -> T at symbol 7
    assert one([T0], b"ACGTTGCTAGG", 8, 0, 8) == 1
    assert one([T0], b"ACGTTGCTAGG", 0, 0, 1) == 9                # off the diagonal: only T0[5], T0[9] agree by chance
    assert sum(x == y for x, y in zip(b"ACGTTGCTAGG", T0[1:12])) == 2


def test_n_on_either_side_never_matches():
    t = b"ACGNNACGT"
    assert one([t], b"ACGNNACGT", 0, 0, 0) == 2                   # N against N: two mismatches
    assert one([t], b"ACGAAACGT", 0, 0, 0) == 2                   # N in the text only
    assert one([T0], b"ACNTT", 0, 0, 0) == 1                      # N in the read only
    assert one([T0], b"AC#TT", 0, 0, 0) == 1                      # a byte outside the alphabet: one mismatch, nothing raised
    assert one([T0], b"NNNN", 0, 0, 4) == 4


def test_lower_case_matches_under_a_case_insensitive_alphabet():
    assert one([T0.lower()], T0[2:12], 0, 0, 2) == 0
    assert one([T0], T0[2:12].lower(), 0, 0, 2) == 0
    sensitive = alph.Alphabet.from_io_symbols(b"ACGT")
    assert one([T0], T0[2:12].lower(), 0, 0, 2, a=sensitive) == 10


def test_windows_that_hang_over_the_text():
    q = T0[:10]
    assert one([T0], q, 3, 0, 0) == 9                             # position < cand_begin: s = -3; TTGCAAG on ACGTTGC: one G agrees
    assert one([T0], b"GGG" + T0[:7], 3, 0, 0) == 3               # ... and q[3:] equal to T0[:7]: exactly the three in front
    assert one([T0], q, 0, 0, 0) == 0
    assert one([T0], T0[15:] + b"AC", 0, 0, 15) == 2              # two symbols past the end
    assert one([T0], T0[15:] + b"AC", 2, 0, 17) == 2
    assert one([T0], q, 0, 0, len(T0)) == 10                      # starts at the end: nothing inside
    assert one([T0], q, 0, 0, 0xFFFFFFFF) == 10                   # any u32 is a position
    assert one([T0], q, 0xFFFFFFFF, 0, 0) == 10                   # cand_begin may exceed the length
    assert one([T0], q, 12, 0, 12) == 0                           # ... and only the difference counts


def test_a_neighbouring_text_that_would_continue_the_match_still_mismatches():
    texts = [T0, T1, b"", b"G"]
    q = T0[16:] + T1[:4]                                          # T0's end, then T1's start: contiguous in the concatenation
    assert one(texts, q, 0, 0, 16) == 4                           # over T0's end: T1's symbols do not count
    assert one(texts, q, 6, 1, 0) == 6                            # the same read on T1's diagonal: the part in front of T1
    assert one(texts, b"G", 0, 3, 0) == 0 and one(texts, b"GG", 0, 3, 0) == 1 and one(texts, b"GG", 1, 3, 0) == 1
    assert one(texts, b"ACG", 0, 2, 0) == 3                       # an empty text matches nothing


def test_the_cap_the_empty_read_and_candidates_out_of_range():
    q = b"TTTTTTTTTT"
    assert one([T0], q, 0, 0, 0) == 8
    assert [one([T0], q, 0, 0, 0, k) for k in (0, 1, 7, 8, 9, BIG)] == [1, 2, 8, 8, 8, 8]
    assert one([T0], T0[:5], 0, 0, 0, 0) == 0
    assert one([T0], b"", 0, 0, 0) == 0 and one([T0], b"", 7, 0, 3, 0) == 0
    got = hamming_model([T0, T1], A, [b"ACG", b"T"], [0, 2, 1, 1], [0, 0, 0, 0], [(0, 0), (0, 0), (2, 0), (1, 1)], 3)
    assert got.dtype == np.uint32 and got.tolist() == [0, INVALID, INVALID, 0]


# ------------------------------------------------------------------------------------------------
# (b) the two calls are declared everywhere a binding looks for them

def _header_arg_counts():
    src = open(os.path.join(ROOT, "include", "gdx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(gdx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = len([x for x in args.split(",") if x.strip()])
    return out


def test_header_library_stub_and_rust_binding_have_both_calls():
    from genedex_amd import _lib

    counts = _header_arg_counts()
    assert counts.get("gdx_hamming_many") == 10 and counts.get("gdx_hamming_many_dev") == 12
    lib = ctypes.CDLL(_lib.LIB_PATH)
    rust = open(os.path.join(ROOT, "bindings", "rust", "gdx.rs")).read()
    for name in NAMES:
        assert hasattr(lib, name), name + " is not exported by libgdx.so"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == counts[name], name
        assert re.search(r"pub fn " + name + r"\s*\(", rust), name
    assert re.search(r"pub fn hamming_many\b", rust)  # the safe wrapper of GpuFmIndex
    header = open(os.path.join(ROOT, "include", "gdx.h")).read()
    assert re.search(r"#define\s+GDX_HAMMING_INVALID\s+0xFFFFFFFFu", header) and _lib.GDX_HAMMING_INVALID == INVALID
