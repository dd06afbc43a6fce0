"""gdx_smems_many[_dev] on the GPU against the CPU model of tests/test_smems_model.py (the walk of include/gdx.h written on
OracleIndex.extend_front), bit for bit, on every index shape and kernel variant."""
import numpy as np
import pytest

import test_gpu_parity as parity
from genedex_amd import alphabet as alph
from genedex_amd import reversed_texts
from helpers import naive_search, random_texts
from oracle.oracle import pack_queries
from test_gpu_parity import _VARIANTS, gpu_index
from test_gpu_suffix_segments import _ALPHABETS, _repeat_case
from test_smems_model import model_arrays, oracle_pair
from test_suffix_segments_model import reads_with_errors

pytestmark = pytest.mark.gpu

ARRAYS = ("n_smems", "remaining", "begin", "length", "start", "end", "status")


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


def gpu_pair(texts, a, companion_options=None, **kw):
    """(the index of the texts, the index of the reversed texts), built alike unless companion_options says otherwise"""
    rkw = dict(kw)
    rkw.update(companion_options or {})
    return gpu_index(texts, a, **kw), gpu_index(reversed_texts(texts), a, **rkw)


def check_against(g, r, want, qs, max_smems, min_length, strict=False):
    """the GPU call equals the model's seven arrays; returns them"""
    qbuf, qoff = pack_queries(qs)
    got = g.smems_raw(r, qbuf, qoff, max_smems, min_length, strict=strict)
    for name, a, b in zip(ARRAYS, got, want):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        bad = np.flatnonzero(a != b)
        if bad.size:
            k = int(bad[0])
            q = qs[k // max_smems if name in ("begin", "length", "start", "end") else k]
            raise AssertionError((name, max_smems, min_length, k, int(a[k]), int(b[k]), q))
    return got


# ------------------------------------------------------------------------------------------------
# 1. random collections, reads with substitutions, every variant

_RANDOM_CASES = {}
_KNOBS = [(ms, ml) for ms in (1, 2, 16) for ml in (1, 12)]


def _random_case(seed):
    if seed not in _RANDOM_CASES:
        rng = np.random.default_rng(9600 + seed)
        a = alph.ascii_dna_with_n()
        symbols = b"ACGTN" if seed % 2 else b"ACGT"
        texts = random_texts(rng, len_max=[6000, 1500, 20000][seed % 3], symbols=symbols)
        qs = reads_with_errors(rng, texts, 220, 80, 200, symbols=symbols)
        F, R = oracle_pair(texts, a)
        _RANDOM_CASES[seed] = (a, texts, qs, {k: model_arrays(F, R, qs, *k) for k in _KNOBS})
    return _RANDOM_CASES[seed]


def _check_random(seed, g, r):
    a, texts, qs, want = _random_case(seed)
    for ms, ml in _KNOBS:
        n_smems, remaining, begin, length, _, _, status = check_against(g, r, want[ms, ml], qs, ms, ml)
        assert not status.any()
        for i in range(len(qs)):  # by descending end, none inside another, all at least min_length long
            b = begin[i * ms:i * ms + int(n_smems[i])].astype(np.int64)
            e = b + length[i * ms:i * ms + int(n_smems[i])]
            assert (np.diff(e) < 0).all() and (np.diff(b) < 0).all() and (e - b >= ml).all() and (e <= len(qs[i])).all()
    assert (want[16, 1][0] > 2).sum() * 5 >= len(qs) and (want[1, 1][1] > 0).sum() * 5 >= len(qs)


@pytest.mark.parametrize("seed", range(3))
def test_random_reads_equal_the_model(seed, variant):
    a, texts, _, _ = _random_case(seed)
    g, r = gpu_pair(texts, a)
    if variant == "default":
        from genedex_amd.device import DeviceEngine

        assert DeviceEngine(g).aux_info()["pair_lines"] and DeviceEngine(r).aux_info()["pair_lines"]
    _check_random(seed, g, r)


def test_random_reads_with_pair_lines_on_one_side_only():
    """the mixed dispatch: the pair-line instance needs pair lines in BOTH indexes, otherwise both passes run on rank lines"""
    from genedex_amd.device import DeviceEngine

    a, texts, _, _ = _random_case(0)
    g, r = gpu_pair(texts, a, companion_options=dict(pair_lines=False))
    assert DeviceEngine(g).aux_info()["pair_lines"] and not DeviceEngine(r).aux_info()["pair_lines"]
    _check_random(0, g, r)
    g2, r2 = gpu_index(texts, a, pair_lines=False), gpu_index(reversed_texts(texts), a)  # and the other way round
    assert not DeviceEngine(g2).aux_info()["pair_lines"] and DeviceEngine(r2).aux_info()["pair_lines"]
    _check_random(0, g2, r2)


def test_the_recommended_companion_shape():
    """the companion as include/gdx.h recommends it: occurrence table, pair lines and top table only"""
    a, texts, _, _ = _random_case(2)
    g, r = gpu_pair(texts, a, companion_options=dict(seed_symbols=0, text_units=False, full_suffix_array=False,
                                                     inverse_suffix_array=False, jump_entry_bytes=0))
    _check_random(2, g, r)


# ------------------------------------------------------------------------------------------------
# 2. every stock alphabet: symbols that occur nowhere, symbols outside the alphabet

@pytest.mark.parametrize("name", list(_ALPHABETS))
def test_every_stock_alphabet(name):
    from genedex_amd import GdxError, _lib

    make, text_symbols, absent = _ALPHABETS[name]
    a = make()
    table = np.asarray(a.io_to_dense_table)
    assert table[absent[0]] != 0
    outside = bytes([int(np.flatnonzero(table == 0)[-1])])
    rng = np.random.default_rng(sum(name.encode()) + 1)
    texts = [bytes(text_symbols[i] for i in rng.integers(0, len(text_symbols), int(rng.integers(0, 3000)))) for _ in range(4)]
    g, r = gpu_pair(texts, a, sa_rate=3)
    F, R = oracle_pair(texts, a, sa_rate=3)
    valid = reads_with_errors(rng, texts, 150, 50, 40, symbols=text_symbols + absent)
    valid += [absent, absent * 3, texts[0][:10] + absent + texts[0][10:20]]
    for ms, ml in ((1, 1), (3, 2), (16, 1)):
        want = model_arrays(F, R, valid, ms, ml)
        assert not want[6].any()
        assert want[0][-3] == 0 and want[0][-2] == 0 and want[1][-2] == 0  # the absent symbol alone: no SMEM, walked through
        check_against(g, r, want, valid, ms, ml, strict=True)
    broken = []
    for q in valid[:120]:
        if len(q) > 2:
            k = int(rng.integers(0, len(q)))
            q = q[:k] + outside + q[k + 1:]
        broken.append(q)
    for ms, ml in ((1, 1), (16, 1)):
        want = model_arrays(F, R, broken, ms, ml)
        bad = want[6] != 0
        # one SMEM often ends right of the poked symbol; sixteen take the walk through the whole read, and only the reads
        # too short to be poked stay valid
        assert bad.sum() > 20 and (~bad).sum() > (5 if ms == 1 else 0)
        got = check_against(g, r, want, broken, ms, ml)
        for i in np.flatnonzero(bad):  # status, n_smems 0, remaining m, every slot zero
            assert got[0][i] == 0 and got[1][i] == len(broken[i]) and got[6][i] == _lib.GDX_Q_INVALID_SYMBOL
            assert not any(x[i * ms:(i + 1) * ms].any() for x in got[2:6])
        with pytest.raises(GdxError) as err:
            g.smems_raw(r, *pack_queries(broken), ms, ml)  # strict
        assert err.value.status == _lib.GDX_ERR_QUERY_STATUS


# ------------------------------------------------------------------------------------------------
# 3. edge cases by hand

DEPTH = 6


def edge_case():
    """(alphabet, texts, named reads) of test_edge_cases_by_hand; what the names promise is asserted on the MODEL's results
    there, so it can be checked without a GPU"""
    rng = np.random.default_rng(9700)
    a = alph.ascii_dna_with_n()

    def rand(n):
        return bytes(b"ACGT"[i] for i in rng.integers(0, 4, n))

    body, left, right, tail = rand(700), rand(40), rand(40), rand(20)
    texts = [left, right, body, body[200:215] + tail]

    def occurs(s):
        return any(s in t for t in texts)

    def other(c):
        return bytes([b"ACGT"[(b"ACGT".index(c) + 1) % 4]])

    k = 100
    qs = {"empty": b"", "whole text": left, "whole long text": body,
          "across a border": left[-20:] + right[:20],
          "first symbol wrong": other(body[k - 1]) + body[k:k + 40],
          "last symbol wrong": body[k:k + 40] + other(body[k + 40]),
          "shorter than the table": body[20:20 + DEPTH - 1], "as long as the table": body[10:10 + DEPTH], "three": b"ACG", "one": b"T",
          "N": b"N", "NNNN": b"NNNN", "N in the middle": body[50:90] + b"N" + body[91:130],
          # body[185:215] and body[200:215] + tail are both in a text, their union is not: two SMEMs that share 15 symbols
          "two overlapping": body[185:215] + tail}
    for i in range(1, len(body) - DEPTH):
        for x in b"ACGT":
            back = bytes([x]) + body[i:i + DEPTH]     # the backward pass from the end takes DEPTH symbols and is blocked
            fwd = body[i:i + DEPTH] + bytes([x])      # [1, DEPTH + 1) is an SMEM, then the forward pass from 0 takes DEPTH
            if "backward pass of the table's depth" not in qs and not occurs(back):
                qs["backward pass of the table's depth"] = back
            if "forward pass of the table's depth" not in qs and not occurs(fwd) and occurs(fwd[1:]):
                qs["forward pass of the table's depth"] = fwd
    for v in range(4 ** DEPTH):
        cand = bytes(b"ACGT"[(v >> (2 * j)) & 3] for j in range(DEPTH))
        if not occurs(cand):  # a D-mer of no text: its entry is frozen in the top table of F, reversed in that of R
            qs["frozen entry on F"] = body[300:330] + cand
            qs["frozen entry on R"] = cand + body[300:330]
            break
    return a, texts, qs


def check_edge_model(texts, qs, want, ms):
    """what the names of edge_case() promise, on the model's arrays for max_smems = ms >= 4 and min_length = 1"""
    names = list(qs)
    n_smems, remaining, begin, length = want[:4]

    def smems(name):
        i = names.index(name)
        return [(int(begin[i * ms + j]), int(begin[i * ms + j] + length[i * ms + j])) for j in range(int(n_smems[i]))]

    assert not want[6].any() and not remaining.any()
    assert smems("empty") == [] and smems("whole text") == [(0, 40)] and smems("whole long text") == [(0, 700)]
    assert (20, 40) in smems("across a border") and (0, 20) in smems("across a border")  # they begin / end at the border
    assert smems("first symbol wrong")[0] == (1, 41) and smems("first symbol wrong")[-1][0] == 0
    assert smems("last symbol wrong")[-1] == (0, 40) and smems("last symbol wrong")[0][1] == 41
    assert smems("backward pass of the table's depth")[0] == (1, DEPTH + 1)
    assert smems("forward pass of the table's depth") == [(1, DEPTH + 1), (0, DEPTH)]
    assert 0 < smems("frozen entry on F")[0][1] - smems("frozen entry on F")[0][0] < DEPTH  # a backward pass from the end
    assert smems("frozen entry on R")[0][1] == DEPTH + 30 and smems("frozen entry on R")[0][0] <= DEPTH
    # forward passes start at the read's last symbol and in front of every SMEM: some start on a D-mer of no text
    frozen_r = 0
    for name, q in qs.items():
        for p in [len(q) - 1] + [b - 1 for b, _ in smems(name)]:
            frozen_r += 0 <= p <= len(q) - DEPTH and not any(q[p:p + DEPTH] in t for t in texts)
    assert frozen_r >= 5
    assert smems("shorter than the table") == [(0, DEPTH - 1)] and smems("as long as the table") == [(0, DEPTH)]
    assert smems("N") == [] and smems("NNNN") == []
    assert smems("N in the middle") == [(41, 80), (0, 40)]
    assert smems("two overlapping") == [(15, 50), (0, 30)]


def test_edge_cases_by_hand():
    from genedex_amd.device import DeviceEngine

    a, texts, named = edge_case()
    qs = list(named.values())
    F, R = oracle_pair(texts, a)
    g, r = gpu_pair(texts, a, top_table_depth=DEPTH)
    assert DeviceEngine(g).aux_info()["top_table_depth"] == DEPTH and DeviceEngine(r).aux_info()["top_table_depth"] == DEPTH
    # empty batch
    out = g.smems_raw(r, np.zeros(8, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 3)
    assert [x.size for x in out] == [0] * 7
    for ms, ml in ((1, 1), (2, 1), (16, 1), (16, 7)):
        want = model_arrays(F, R, qs, ms, ml)
        if (ms, ml) == (16, 1):
            check_edge_model(texts, named, want, ms)
        check_against(g, r, want, qs, ms, ml, strict=True)
    # a top table deeper than most of these reads, on either side and on both
    deep_g, deep_r = gpu_pair(texts, a, top_table_depth=9)
    assert DeviceEngine(deep_g).aux_info()["top_table_depth"] == 9 and DeviceEngine(deep_r).aux_info()["top_table_depth"] == 9
    body = texts[2]
    more = qs + [body[5:13], body[7:12] + b"N", body[5:14], body[5:15]]
    for ms, ml in ((1, 1), (4, 1)):
        want = model_arrays(F, R, more, ms, ml)
        check_against(deep_g, deep_r, want, more, ms, ml, strict=True)
        check_against(g, deep_r, want, more, ms, ml, strict=True)
        check_against(deep_g, r, want, more, ms, ml, strict=True)


# ------------------------------------------------------------------------------------------------
# 4. repeats: SMEMs whose intervals stay wider than one row

_REPEAT_WANT = {}


def repeat_want():
    if not _REPEAT_WANT:
        a, texts, qs, _ = _repeat_case()
        F, R = oracle_pair(texts, a, sa_rate=8)
        _REPEAT_WANT.update({k: model_arrays(F, R, qs, *k) for k in ((1, 1), (16, 1), (16, 12))})
    return _REPEAT_WANT


def test_repeats_and_a_long_tandem_repeat(variant):
    a, texts, qs, _ = _repeat_case()
    g, r = gpu_pair(texts, a, sa_rate=8)
    for (ms, ml), want in repeat_want().items():
        _, _, _, length, start, end, _ = check_against(g, r, want, qs, ms, ml, strict=True)
    wide = (length >= 30) & (end - start > 1)  # long SMEMs that never narrowed to one row
    assert wide.sum() > 100


# ------------------------------------------------------------------------------------------------
# 5. consistency with the calls that exist

def test_consistent_with_cursors_locate_segments_and_the_device_call():
    import torch

    from genedex_amd.device import DeviceEngine, DeviceQueries

    rng = np.random.default_rng(9800)
    a = alph.ascii_dna()
    texts = random_texts(rng, len_max=3000)
    while sum(len(t) for t in texts) < 500:
        texts = random_texts(rng, len_max=3000)
    g, r = gpu_pair(texts, a)
    qs = reads_with_errors(rng, texts, 150, 30, 120)
    # a read that occurs has exactly one SMEM, [0, m), with the interval cursors_for_many_queries gives
    whole = [q for q in qs if len(q) > 0 and naive_search(texts, q)]
    assert len(whole) > 20
    for q, smems, cur in zip(whole, g.smems_many(whole, r, 4), g.cursors_for_many_queries(whole)):
        assert len(smems) == 1 and (smems[0].query_begin, smems[0].query_end) == (0, len(q))
        assert smems[0].cursor.interval() == cur.interval()
    # every SMEM's cursor locates exactly the occurrences of its substring
    all_smems = g.smems_many(qs, r, 128)  # (128 >= every read's length: nothing is cut)
    n_located = 0
    for q, smems in list(zip(qs, all_smems))[:60]:
        for s in smems:
            sub = q[s.query_begin:s.query_end]
            assert {tuple(h) for h in s.cursor.locate()} == naive_search(texts, sub)
            assert s.cursor.count() == len(naive_search(texts, sub)) > 0
            n_located += 1
    assert n_located > 100
    # a read's first suffix segment ends where its first SMEM ends, and is no longer than it
    n_compared = 0
    for q, smems, segs in zip(qs, all_smems, g.suffix_segments_many(qs, 1)):
        if smems:
            assert segs[0].query_end == smems[0].query_end and segs[0].length <= smems[0].query_end - smems[0].query_begin
            n_compared += 1
    assert n_compared > 100
    # the device-pointer call writes what the host call returns
    qbuf, qoff = pack_queries(qs)
    eng, reng = DeviceEngine(g), DeviceEngine(r)
    dq = DeviceQueries.from_host(qbuf, qoff)
    for ms, ml, companion in ((1, 1, reng), (16, 1, r), (16, 12, reng)):
        host = g.smems_raw(r, qbuf, qoff, ms, ml)
        out = eng.alloc_smems(dq.nq, ms)
        for t in out.values():
            t.fill_(0x55)
        eng.smems(dq, companion, ms, ml, out)
        torch.cuda.synchronize()
        for name, h in zip(ARRAYS, host):
            d = out[name].cpu().numpy()
            d = d.view(np.uint32) if d.dtype == np.int32 else d
            assert d.astype(np.uint64).tolist() == h.astype(np.uint64).tolist(), (name, ms, ml)


# ------------------------------------------------------------------------------------------------
# 6. what the call refuses

def test_invalid_arguments_companions_that_cannot_be_and_the_64_bit_engine():
    from genedex_amd import FmIndexConfig, GdxError, _lib

    a = alph.ascii_dna_with_n()
    texts = [b"ACGTACGTTGCA", b"GGA"]
    g, r = gpu_pair(texts, a)
    qbuf, qoff = pack_queries([b"ACGT", b"TTT"])

    def refused(f, rev, max_smems=2, min_length=1):
        with pytest.raises(GdxError) as err:
            f.smems_raw(rev, qbuf, qoff, max_smems, min_length)
        return err.value.status

    n_smems, remaining, begin, length = g.smems_raw(r, qbuf, qoff, 2)[:4]
    assert n_smems.tolist() == [1, 2] and remaining.tolist() == [0, 0]  # "ACGT" occurs; "TTT" is "TT" (of "GTTG") twice
    assert begin.tolist() == [0, 0, 1, 0] and length.tolist() == [4, 0, 2, 2]
    assert refused(g, r, max_smems=0) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert refused(g, r, min_length=0) == _lib.GDX_ERR_INVALID_ARGUMENT
    # companions that cannot be: other symbol counts, another number of texts, another length, another alphabet
    assert refused(g, gpu_index([b"ACGTACGTTGCC", b"GGA"], a)) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert refused(g, gpu_index([b"ACGTACGTTGCAGGA"], a)) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert refused(g, gpu_index([b"ACGTACGTTGCAA", b"GGA"], a)) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert refused(g, gpu_index(reversed_texts(texts), alph.ascii_dna())) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert refused(g, gpu_index(reversed_texts(texts), alph.ascii_dna_iupac_as_dna_with_n())) == _lib.GDX_ERR_INVALID_ARGUMENT
    # a companion of the same symbol counts that was built from other texts (here: the texts, not reversed) is not
    # detected; the call still ends, with results that mean nothing
    out = g.smems_raw(g, qbuf, qoff, 2)
    assert (out[0] <= 2).all() and not out[6].any()
    # the device call refuses the same
    import torch

    from genedex_amd.device import DeviceEngine, DeviceQueries

    eng = DeviceEngine(g)
    dq = DeviceQueries.from_host(qbuf, qoff)
    outs = eng.alloc_smems(dq.nq, 2)
    for args in ((r, 0, 1), (r, 2, 0), (gpu_index([b"ACGTACGTTGCC", b"GGA"], a), 2, 1)):
        with pytest.raises(GdxError) as err:
            eng.smems(dq, *args, outs)
        assert err.value.status == _lib.GDX_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    lib = _lib.load()
    lib.gdx_debug_force_wide(1)
    try:
        w = FmIndexConfig("i64").suffix_array_sampling_rate(4).construct_index(texts, a)
        wr = FmIndexConfig("i64").suffix_array_sampling_rate(4).construct_index(reversed_texts(texts), a)
    finally:
        lib.gdx_debug_force_wide(0)
    assert w.info.index_width == 64 and wr.info.index_width == 64
    assert refused(w, r) == _lib.GDX_ERR_UNSUPPORTED
    assert refused(g, wr) == _lib.GDX_ERR_UNSUPPORTED
    assert refused(w, wr) == _lib.GDX_ERR_UNSUPPORTED
