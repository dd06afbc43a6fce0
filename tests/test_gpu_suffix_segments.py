"""gdx_suffix_segments_many[_dev] on the GPU against the CPU model of tests/test_suffix_segments_model.py (the definition
written on OracleIndex.extend_front), bit for bit, on every index shape and kernel variant, with the text route
(flags 0) and without it (GDX_SEGMENTS_LF_ONLY)."""
import numpy as np
import pytest

import test_gpu_parity as parity
from genedex_amd import alphabet as alph
from helpers import naive_search, random_texts
from oracle.oracle import pack_queries
from test_gpu_parity import _VARIANTS, cpu_index, gpu_index
from test_suffix_segments_model import model_arrays, reads_with_errors

pytestmark = pytest.mark.gpu

ARRAYS = ("n_segments", "remaining", "length", "start", "end", "status")


@pytest.fixture(params=list(_VARIANTS))  # the default shape first
def variant(request):
    query, build = _VARIANTS[request.param]
    parity._QUERY_OPTIONS.clear()
    parity._QUERY_OPTIONS.update(query)
    parity._BUILD_OPTIONS.clear()
    parity._BUILD_OPTIONS.update(build)
    yield request.param
    parity._QUERY_OPTIONS.clear()
    parity._BUILD_OPTIONS.clear()


def check_against(g, want, qs, max_segments, strict=False):
    """both routes of the GPU call equal the model's six arrays; returns the arrays of the default route"""
    qbuf, qoff = pack_queries(qs)
    first = None
    for lf_only in (False, True):
        got = g.suffix_segments_raw(qbuf, qoff, max_segments, lf_only=lf_only, strict=strict)
        for name, a, b in zip(ARRAYS, got, want):
            assert a.shape == b.shape, (name, lf_only)
            bad = np.flatnonzero(a != b)
            if bad.size:
                k = int(bad[0])
                q = qs[k // max_segments if a.size != len(qs) or name in ("length", "start", "end") else k]
                raise AssertionError((name, "lf_only" if lf_only else "default route", max_segments, k, int(a[k]), int(b[k]), q))
        first = first or got
    return first


# ------------------------------------------------------------------------------------------------
# 1. random collections, reads with substitutions, every variant, both routes

_RANDOM_CASES = {}


def _random_case(seed):
    if seed not in _RANDOM_CASES:
        rng = np.random.default_rng(9100 + seed)
        a = alph.ascii_dna_with_n()
        symbols = b"ACGTN" if seed % 2 else b"ACGT"
        texts = random_texts(rng, len_max=[6000, 1500, 20000][seed % 3], symbols=symbols)
        qs = reads_with_errors(rng, texts, 220, 80, 200, symbols=symbols)
        c = cpu_index(texts, a)
        _RANDOM_CASES[seed] = (a, texts, qs, {ms: model_arrays(c, qs, ms) for ms in (1, 2, 8)})
    return _RANDOM_CASES[seed]


@pytest.mark.parametrize("seed", range(3))
def test_random_reads_equal_the_model(seed, variant):
    a, texts, qs, want = _random_case(seed)
    g = gpu_index(texts, a)
    if variant == "default":
        from genedex_amd.device import DeviceEngine

        aux = DeviceEngine(g).aux_info()  # the text route needs all three, and this is the shape that has them
        assert aux["text_units"] and aux["full_suffix_array"] and aux["inverse_suffix_array"] and aux["pair_lines"]
    for ms in (1, 2, 8):
        n_seg, remaining, length, _, _, status = check_against(g, want[ms], qs, ms)
        assert not status.any()
        for i, q in enumerate(qs):  # the segments tile q[remaining, m) from the right
            covered = sum(max(int(x), 1) for x in length[i * ms:i * ms + int(n_seg[i])])
            assert covered + int(remaining[i]) == len(q)
    assert (want[8][0] > 1).sum() > 50 and (want[1][1] > 0).sum() > 50


# ------------------------------------------------------------------------------------------------
# 2. every stock alphabet: symbols that occur nowhere, symbols outside the alphabet

_ALPHABETS = {
    # name: (constructor, symbols texts are drawn from, a valid symbol that occurs in no text)
    "ascii_dna": (alph.ascii_dna, b"ACGacg", b"T"),
    "ascii_dna_with_n": (alph.ascii_dna_with_n, b"ACGTacgt", b"N"),
    "ascii_dna_iupac": (alph.ascii_dna_iupac, b"ACGTNRYKMSWBDHacgtnry", b"V"),
    "ascii_dna_iupac_as_dna_with_n": (alph.ascii_dna_iupac_as_dna_with_n, b"ACGacg", b"T"),
    "ascii_amino_acid": (alph.ascii_amino_acid, b"ACDEFGHIKLMNPQRSTVWacdef", b"Y"),
    "ascii_amino_acid_iupac": (alph.ascii_amino_acid_iupac, b"ACDEFGHIKLMNPQRSTVWYBZacd", b"X"),
    "u8_until": (lambda: alph.u8_until(200), bytes(range(200)), bytes([200])),
    "ascii_printable": (alph.ascii_printable, bytes(range(0x20, 0x7e)), bytes([0x7e])),
}


@pytest.mark.parametrize("name", list(_ALPHABETS))
def test_every_stock_alphabet(name):
    from genedex_amd import GdxError, _lib

    make, text_symbols, absent = _ALPHABETS[name]
    a = make()
    table = np.asarray(a.io_to_dense_table)
    assert table[absent[0]] != 0
    outside = bytes([int(np.flatnonzero(table == 0)[-1])])
    rng = np.random.default_rng(sum(name.encode()))
    texts = [bytes(text_symbols[i] for i in rng.integers(0, len(text_symbols), int(rng.integers(0, 3000)))) for _ in range(4)]
    g, c = gpu_index(texts, a, sa_rate=3), cpu_index(texts, a, sa_rate=3)
    valid = reads_with_errors(rng, texts, 150, 50, 40, symbols=text_symbols + absent)
    valid += [absent, absent * 3, texts[0][:10] + absent + texts[0][10:20]]
    for ms in (1, 3, 8):
        want = model_arrays(c, valid, ms)
        assert not want[5].any() and (want[2][:: ms][want[0] > 0] == 0).any()  # zero-length segments are among them
        check_against(g, want, valid, ms, strict=True)
    broken = []
    for q in valid[:120]:
        if len(q) > 2:
            k = int(rng.integers(0, len(q)))
            q = q[:k] + outside + q[k + 1:]
        broken.append(q)
    for ms in (1, 8):
        want = model_arrays(c, broken, ms)
        bad = want[5] != 0
        assert bad.sum() > 20 and (~bad).sum() > 5
        got = check_against(g, want, broken, ms)
        for i in np.flatnonzero(bad):  # status, n_segments 0, remaining m, every slot zero
            assert got[0][i] == 0 and got[1][i] == len(broken[i]) and got[5][i] == _lib.GDX_Q_INVALID_SYMBOL
            assert not got[2][i * ms:(i + 1) * ms].any() and not got[3][i * ms:(i + 1) * ms].any() \
                and not got[4][i * ms:(i + 1) * ms].any()
        with pytest.raises(GdxError) as err:
            g.suffix_segments_raw(*pack_queries(broken), ms)  # strict
        assert err.value.status == _lib.GDX_ERR_QUERY_STATUS


# ------------------------------------------------------------------------------------------------
# 3. edge cases by hand

def test_edge_cases_by_hand():
    from genedex_amd.device import DeviceEngine

    rng = np.random.default_rng(9300)
    a = alph.ascii_dna_with_n()
    body = bytes(b"ACGT"[i] for i in rng.integers(0, 4, 700))
    texts = [b"ACGTTGCA", b"GGATCCAT", body]
    c = cpu_index(texts, a)
    depth = 6
    g = gpu_index(texts, a, top_table_depth=depth)
    assert DeviceEngine(g).aux_info()["top_table_depth"] == depth

    def occurs(s):
        return any(s in t for t in texts)

    # empty batch
    out = g.suffix_segments_raw(np.zeros(8, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 3)
    assert [x.size for x in out] == [0] * 6
    # a read that runs across a text border: the first segment ends at the border
    across = texts[0][-4:] + texts[1][:4]
    assert not occurs(b"A" + texts[1][:4])
    # the blocking symbol is the read's first symbol
    k = 100
    wrong = bytes([b"ACGT"[(b"ACGT".index(body[k - 1]) + 1) % 4]])
    blocked_first = wrong + body[k:k + 40]
    assert occurs(blocked_first[1:]) and not occurs(blocked_first)
    # a segment exactly `depth` long, and a frozen top entry (a 6-mer that does not occur)
    exact = frozen = None
    for i in range(1, len(body) - depth):
        for x in b"ACGT":
            cand = bytes([x]) + body[i:i + depth]
            if exact is None and not occurs(cand):
                exact = cand
    for v in range(4 ** depth):
        cand = bytes(b"ACGT"[(v >> (2 * j)) & 3] for j in range(depth))
        if not occurs(cand):
            frozen = body[300:330] + cand
            break
    assert exact is not None and frozen is not None
    qs = [b"", texts[0], body, across, blocked_first, exact, frozen, body[10:10 + depth], body[20:20 + depth - 1], b"ACG", b"T",
          b"N", b"NNNN", body[50:90] + b"N" + body[91:130]]
    for ms in (1, 2, 8):
        want = model_arrays(c, qs, ms)
        n_seg, remaining, length, start, end, status = check_against(g, want, qs, ms, strict=True)
        assert n_seg[0] == 0 and remaining[0] == 0                                  # the empty query
        assert n_seg[1] == 1 and length[1 * ms] == len(texts[0])                    # a whole text
        assert n_seg[2] == 1 and length[2 * ms] == len(body) and end[2 * ms] - start[2 * ms] == 1
        assert length[3 * ms] == 4                                                  # ends at the border
        assert length[4 * ms] == 40 and remaining[4] == (1 if ms == 1 else 0)       # max_segments cuts the walk
        if ms > 1:
            assert n_seg[4] == 2 and length[4 * ms + 1] == 1
        assert length[5 * ms] == depth                                              # exactly the top table's depth
        assert 0 < length[6 * ms] < depth                                           # the frozen entry: redone step by step
        assert length[7 * ms] == depth and length[8 * ms] == depth - 1              # reads as long as / shorter than the table
    # a top table deeper than every read
    deep = gpu_index(texts, a, top_table_depth=9)
    assert DeviceEngine(deep).aux_info()["top_table_depth"] == 9
    short = [q for q in qs if len(q) < 9] + [body[5:13], body[7:12] + b"N"]
    for ms in (1, 4):
        check_against(deep, model_arrays(c, short, ms), short, ms, strict=True)


# ------------------------------------------------------------------------------------------------
# 4. repeats: intervals wider than one row for a segment's whole length

_REPEAT_CASE = []


def _repeat_case():
    if not _REPEAT_CASE:
        rng = np.random.default_rng(9400)
        a = alph.ascii_dna_with_n()
        unit = bytes(b"ACGT"[i] for i in rng.integers(0, 4, 997))
        t1 = bytearray(unit * 40)
        for pos in rng.integers(0, len(t1), 60):
            t1[pos] = b"ACGT"[int(rng.integers(0, 4))]
        block = bytes(b"ACGT"[i] for i in rng.integers(0, 4, 300))
        spacers = [bytes(b"ACGT"[i] for i in rng.integers(0, 4, 500)) for _ in range(4)]
        texts = [bytes(t1), unit * 3, b"A" * 3000, spacers[0] + block + spacers[1] + block + spacers[2] + block + spacers[3]]
        qs = reads_with_errors(rng, texts, 260, 20, 300)
        qs += [b"A" * 50, b"A" * 2999, b"A" * 3001, b"C" + b"A" * 100, block[20:280], block[:150] + b"G" + block[151:]]
        c = cpu_index(texts, a, sa_rate=8)
        _REPEAT_CASE.append((a, texts, qs, {ms: model_arrays(c, qs, ms) for ms in (1, 8)}))
    return _REPEAT_CASE[0]


def test_repeats_and_a_long_tandem_repeat(variant):
    a, texts, qs, want = _repeat_case()
    g = gpu_index(texts, a, sa_rate=8)
    for ms in (1, 8):
        n_seg, _, length, start, end, _ = check_against(g, want[ms], qs, ms, strict=True)
    wide = (length >= 30) & (end - start > 1)  # long segments that never narrowed to one row
    assert wide.sum() > 100


# ------------------------------------------------------------------------------------------------
# 5. consistency with the calls that exist

def test_consistent_with_cursors_locate_and_the_device_call():
    import torch

    from genedex_amd.device import DeviceEngine, DeviceQueries

    rng = np.random.default_rng(9500)
    a = alph.ascii_dna()
    texts = random_texts(rng, len_max=3000)
    while sum(len(t) for t in texts) < 500:
        texts = random_texts(rng, len_max=3000)
    g = gpu_index(texts, a)
    qs = reads_with_errors(rng, texts, 150, 30, 120)
    # a read that occurs has one segment, and its interval is the one cursors_for_many_queries gives
    whole = [q for q in qs if len(q) > 0 and naive_search(texts, q)]
    assert len(whole) > 20
    cursors = g.cursors_for_many_queries(whole)
    for q, segs, cur in zip(whole, g.suffix_segments_many(whole, 4), cursors):
        assert len(segs) == 1 and segs[0].query_end == len(q) and segs[0].length == len(q)
        assert segs[0].cursor.interval() == cur.interval()
    # every segment's cursor locates exactly the occurrences of its substring
    for q, segs in list(zip(qs, g.suffix_segments_many(qs, 128)))[:60]:  # (128 >= every read's length: nothing is cut)
        e = len(q)
        for s in segs:
            assert s.query_end == e
            if s.length:
                sub = q[e - s.length:e]
                assert {tuple(h) for h in s.cursor.locate()} == naive_search(texts, sub)
                assert s.cursor.count() == len(naive_search(texts, sub))
            else:
                assert s.cursor.count() == 0 and not naive_search(texts, q[e - 1:e])
            e -= max(s.length, 1)
        assert e == 0
    length, cur = g.longest_suffix_match(whole[0])
    assert length == len(whole[0]) and cur.count() == len(naive_search(texts, whole[0]))
    assert g.longest_suffix_match(b"")[0] == 0
    # the device-pointer call writes what the host call returns
    qbuf, qoff = pack_queries(qs)
    eng = DeviceEngine(g)
    dq = DeviceQueries.from_host(qbuf, qoff)
    for ms in (1, 8):
        for lf_only in (False, True):
            host = g.suffix_segments_raw(qbuf, qoff, ms, lf_only=lf_only)
            out = eng.alloc_segments(dq.nq, ms)
            for t in out.values():
                t.fill_(0x55)
            eng.suffix_segments(dq, ms, out, lf_only=lf_only)
            torch.cuda.synchronize()
            for name, h in zip(ARRAYS, host):
                d = out[name].cpu().numpy()
                d = d.view(np.uint32) if d.dtype == np.int32 else d
                assert d.astype(np.uint64).tolist() == h.astype(np.uint64).tolist(), (name, ms, lf_only)


# ------------------------------------------------------------------------------------------------
# 6. what the call refuses

def test_invalid_arguments_and_the_64_bit_engine():
    from genedex_amd import FmIndexConfig, GdxError, _lib

    a = alph.ascii_dna_with_n()
    texts = [b"ACGTACGTTGCA", b"GGA"]
    g = gpu_index(texts, a)
    qbuf, qoff = pack_queries([b"ACGT", b"TTT"])
    with pytest.raises(GdxError) as err:
        g.suffix_segments_raw(qbuf, qoff, 0)
    assert err.value.status == _lib.GDX_ERR_INVALID_ARGUMENT
    lib = _lib.load()
    outs = [np.zeros(8, dtype=t) for t in (np.uint32, np.uint32, np.uint32, np.uint64, np.uint64, np.uint8)]
    ptrs = [o.ctypes.data_as(p) for o, p in zip(outs, (_lib.u32p, _lib.u32p, _lib.u32p, _lib.u64p, _lib.u64p, _lib.u8p))]
    for flags in (2, 0x80000000, 3):
        st = lib.gdx_suffix_segments_many(g._h, qbuf.ctypes.data_as(_lib.u8p), qoff.ctypes.data_as(_lib.u64p), 2, 2, flags, *ptrs)
        assert st == _lib.GDX_ERR_INVALID_ARGUMENT, flags
    assert lib.gdx_suffix_segments_many(g._h, qbuf.ctypes.data_as(_lib.u8p), qoff.ctypes.data_as(_lib.u64p), 2, 2, 1, *ptrs) == 0
    assert outs[0][:2].tolist() == [1, 2]  # "ACGT" occurs; "TTT" is "TT" (of "GTTG") and "T"
    lib.gdx_debug_force_wide(1)
    try:
        w = FmIndexConfig("i64").suffix_array_sampling_rate(4).construct_index(texts, a)
    finally:
        lib.gdx_debug_force_wide(0)
    assert w.info.index_width == 64
    with pytest.raises(GdxError) as err:
        w.suffix_segments_raw(qbuf, qoff, 2)
    assert err.value.status == _lib.GDX_ERR_UNSUPPORTED
