"""gdx_edit_distance_many[_dev] on the GPU against the CPU model of tests/test_edit_distance_model.py (the definition of
include/gdx.h on bytes and the alphabet table).  Outputs are integers: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_parity as parity
from genedex_amd import GdxError, _lib, reversed_texts
from genedex_amd import alphabet as alph
from oracle.oracle import pack_queries
from test_edit_distance_model import INVALID, NO_END, TOO_LONG, edit_model
from test_gpu_hamming import expand_candidates
from test_gpu_parity import _VARIANTS, gpu_index
from test_hamming_model import hamming_model
from test_smems_model import model_arrays, oracle_pair
from test_strands_model import host_batches, join

pytestmark = pytest.mark.gpu

BIG = 1 << 31
GARBAGE = 0x5A5A5A5A


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


def status_of(fn):
    with pytest.raises(GdxError) as e:
        fn()
    return e.value.status


def host_call(g, qs, cq, cb, hits, k, want_end=True):
    qbuf, qoff = pack_queries(qs)
    hits = np.asarray(hits, dtype=np.uint64).reshape(-1, 2)
    return g.edit_distance_raw(qbuf, qoff, cq, cb, hits[:, 0], hits[:, 1], k, want_end=want_end)


def assert_equal(got, want, what):
    for g, w, name in zip(got, want, ("dist", "end")):
        assert g.dtype == np.uint32 and g.shape == w.shape, (what, name)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, name, int(bad.size), int(bad[0]), int(g[bad[0]]), int(w[bad[0]]))


def device_call(eng, dq, cq, cb, hits, k, want_end=True):
    """gdx_edit_distance_many_dev on host-made candidates -> (dist, end) u32[m]; the outputs start as garbage: every entry must
    be written.  want_end=False passes NULL for d_out_end and returns (dist, None)."""
    import torch

    def dev(x, shape=None):
        x = np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)
        return torch.from_numpy(x.reshape(shape) if shape else x).cuda()

    m = len(cq)
    dist = torch.full((max(m, 1),), GARBAGE, dtype=torch.int32, device="cuda")
    end = torch.full((max(m, 1),), GARBAGE, dtype=torch.int32, device="cuda") if want_end else None
    eng.edit_distance(dq, dev(cq), dev(cb), dev(np.asarray(hits, dtype=np.uint64).reshape(-1, 2), (-1, 2)), k, dist, end,
                      want_end=want_end)
    torch.cuda.synchronize()
    return dist.cpu().numpy().view(np.uint32)[:m], (end.cpu().numpy().view(np.uint32)[:m] if want_end else None)


def planted_read(rng, t, start, ln, n_edits, symbols=b"ACGT"):
    """a read of ln symbols that follows t from `start` on with n_edits edits at distinct offsets in [5, ln - 5), each a
    substitution, an inserted symbol or a skipped text symbol -> (read, where[j] = the text position of read symbol j or -1
    for an edited one); needs start + ln + n_edits <= len(t)"""
    at = set(int(x) for x in rng.choice(np.arange(5, ln - 5), size=n_edits, replace=False)) if n_edits else set()
    q, where, p = bytearray(), [], start
    for j in range(ln):
        if j in at:
            kind = int(rng.integers(0, 3))
            if kind == 0:                               # substitution: another symbol
                q.append(symbols[(symbols.index(t[p]) + 1 + int(rng.integers(0, len(symbols) - 1))) % len(symbols)])
                where.append(-1)
                p += 1
                continue
            if kind == 1:                               # a symbol the text does not have
                q.append(symbols[int(rng.integers(0, len(symbols)))])
                where.append(-1)
                continue
            p += 1                                      # the read skips a text symbol, then goes on unedited
        q.append(t[p])
        where.append(p)
        p += 1
    return bytes(q), where


# ------------------------------------------------------------------------------------------------
# 1. random reads with indels, every variant

_RANDOM_CASES = {}
_LIMITS = (0, 3, 8, 256)


def _random_case(seed):
    """(alphabet, texts, reads, candidates, planted edits per candidate (-1: a random place), {limit: model})"""
    if seed in _RANDOM_CASES:
        return _RANDOM_CASES[seed]
    rng = np.random.default_rng(12000 + seed)
    a = alph.ascii_dna_with_n()
    clean = [bytes(b"ACGT"[i] for i in rng.integers(0, 4, n)) for n in (3000, 1700, 600)]
    qs, cq, cb, hits, planted = [], [], [], [], []
    for i in range(300):
        t = clean[i % 3]
        ln = int(rng.integers(40, 201))
        start = int(rng.integers(0, len(t) - ln - 4))
        q, where = planted_read(rng, t, start, ln, i % 5)
        qs.append(q)
        unedited = [j for j in range(ln) if where[j] >= 0]
        for j in rng.choice(unedited, size=2, replace=False):     # the true diagonal, named through two unedited symbols
            cq.append(i), cb.append(int(j)), hits.append((i % 3, where[int(j)])), planted.append(i % 5)
        text_id = int(rng.integers(0, 3))                         # anywhere, out of the text included
        cq.append(i), cb.append(int(rng.integers(0, ln + 6))), planted.append(-1)
        hits.append((text_id, int(rng.integers(0, len(clean[text_id]) + 60))))
    texts = list(clean)
    if seed % 2:                                                  # N in one text, one symbol in 120: about one per read there
        t = bytearray(texts[1])
        for p in np.flatnonzero(rng.integers(0, 120, len(t)) == 0):
            t[int(p)] = ord("N")
        texts[1] = bytes(t)
    want = {k: edit_model(texts, a, qs, cq, cb, hits, k) for k in _LIMITS}
    ham = hamming_model(texts, a, qs, cq, cb, hits, BIG)
    _RANDOM_CASES[seed] = (a, texts, qs, (cq, cb, hits), np.array(planted), want, ham)
    return _RANDOM_CASES[seed]


@pytest.mark.parametrize("seed", range(2))
def test_random_reads_with_indels_equal_the_model(seed, variant):
    from genedex_amd.device import DeviceEngine

    a, texts, qs, (cq, cb, hits), planted, want, ham = _random_case(seed)
    # the preconditions, on the models alone, at limit 3
    dist3, end3 = want[3]
    m = len(cq)
    assert m == 900
    assert (dist3 <= 3).sum() * 5 >= 2 * m and (dist3 < np.minimum(ham, 4)).sum() * 5 >= m
    assert (dist3 == 4).sum() * 4 >= m and (dist3 == 0).sum() > 0
    if seed == 0:                                                 # (seed 1: an N under a read is one more edit)
        for k in _LIMITS:                                         # a true candidate costs at most what was planted
            assert (want[k][0][planted >= 0] <= planted[planted >= 0]).all(), k
    g = gpu_index(texts, a)
    if not DeviceEngine(g).aux_info()["text_units"]:
        assert status_of(lambda: host_call(g, qs, cq, cb, hits, 3)) == _lib.GDX_ERR_UNSUPPORTED
        return
    for k in _LIMITS:
        assert_equal(host_call(g, qs, cq, cb, hits, k), want[k], (seed, variant, k))


# ------------------------------------------------------------------------------------------------
# 7. (of the issue's list) cross-check with gdx_hamming_many on the GPU, on the candidates of test 1

@pytest.mark.parametrize("seed", range(2))
def test_against_the_hamming_call_on_the_gpu(seed):
    a, texts, qs, (cq, cb, hits), _, _, _ = _random_case(seed)
    g = gpu_index(texts, a)
    qbuf, qoff = pack_queries(qs)
    h = np.asarray(hits, dtype=np.uint64)
    full = g.hamming_raw(qbuf, qoff, cq, cb, h[:, 0], h[:, 1], BIG)
    dist0, _ = host_call(g, qs, cq, cb, hits, 0)
    assert np.array_equal(dist0, np.minimum(full, 1))
    for k in (3, 8, 256):
        dist, end = host_call(g, qs, cq, cb, hits, k)
        assert (dist <= np.minimum(full, k + 1)).all(), k
        assert ((dist <= k) == (end != NO_END)).all(), k


# ------------------------------------------------------------------------------------------------
# 2. word borders and window phases: every block count and last-block bit, every phase of the window's first unit, both ends
#    of a text

_SWEEP = {}
_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
_SWEEP_LIMITS = (0, 1, 5, 33)


def _sweep_case():
    if _SWEEP:
        return _SWEEP
    rng = np.random.default_rng(12050)
    a = alph.ascii_dna_with_n()

    def rand(n, symbols=b"ACGT"):
        return bytes(symbols[i] for i in rng.integers(0, len(symbols), n))

    # text 0 sits behind the pad units; text 1 directly behind text 0; an empty text and a text of one symbol; the last text
    texts = [rand(401), rand(397, b"ACGTACGTACGTN"), b"", b"G", rand(333)]
    qs, cq, cb, hits = [], [], [], []
    for text_id in (0, 1, 4):
        t = texts[text_id]
        # the neighbours as they lie in the concatenation, one symbol where the sentinel is: a read cut from `around` goes on
        # matching over the text's ends unless the text's own bounds clip it
        before = (texts[text_id - 1] if text_id == 1 else rand(64))[-64:]
        behind = (texts[text_id + 1] if text_id == 0 else rand(64))[:64]
        around, base = before + b"A" + t + b"C" + behind, len(before) + 1
        for ln in _LENGTHS:
            starts = list(range(40, 72)) + [-40, -1, 0] + [len(t) + e - ln for e in (-1, 0, 1, 40)]
            for n, s in enumerate(starts):
                lo, hi = max(base + s, 0), max(base + s + ln, 0)
                q = bytearray(around[lo:hi].rjust(ln, b"T")[:ln].ljust(ln, b"T"))
                if n % 4 == 1 and ln > 8:                         # one inserted symbol, the tail moves on by one
                    at = int(rng.integers(2, ln - 2))
                    q = q[:at] + b"ACGT"[int(rng.integers(0, 4)):][:1] + q[at:ln - 1]
                elif n % 4 == 3 and ln > 8:                       # one skipped symbol, the tail comes from one further on
                    at = int(rng.integers(2, ln - 2))
                    q = q[:at] + q[at + 1:] + around[hi:hi + 1].ljust(1, b"T")
                for _ in range(int(rng.integers(0, 3))):
                    q[int(rng.integers(0, ln))] = b"ACGTN"[int(rng.integers(0, 5))]
                assert len(q) == ln
                b = int(rng.integers(max(-s, 0), max(-s, 0) + ln + 1))   # (may exceed the read's length)
                qs.append(bytes(q)), cq.append(len(qs) - 1), cb.append(b), hits.append((text_id, s + b))
    for text_id in (2, 3):  # the empty text and the text of one symbol, between their neighbours
        for q, b, p in ((b"G", 0, 0), (b"GG", 1, 0), (b"GG", 0, 0), (texts[1][-3:] + b"AG", 4, 0), (b"", 0, 0), (b"G" + texts[4][:40], 0, 0)):
            qs.append(q), cq.append(len(qs) - 1), cb.append(b), hits.append((text_id, p))
    qs.append(rand(257)), cq.append(len(qs) - 1), cb.append(0), hits.append((0, 20))      # one read over the limit
    _SWEEP.update(a=a, texts=texts, qs=qs, cand=(cq, cb, hits),
                  want={k: edit_model(texts, a, qs, cq, cb, hits, k) for k in _SWEEP_LIMITS})
    return _SWEEP


def test_word_borders_and_window_phases():
    c = _sweep_case()
    texts, qs, (cq, cb, hits) = c["texts"], c["qs"], c["cand"]
    lens = np.array([len(qs[i]) for i in cq])
    for k in _SWEEP_LIMITS:                             # the window's first column takes every phase of a text unit
        phases = set()
        for (t, p), b, ln in zip(hits, cb, lens):
            x0, x1 = min(max(p - b - k, 0), len(texts[t])), min(max(p - b + ln + k, 0), len(texts[t]))
            if x0 < x1:
                phases.add((sum(len(x) + 1 for x in texts[:t]) + x0) % 32)
        assert phases == set(range(32)), k
    # the inputs do what they are for: exact windows, reads one indel away, reads that hang over an end, and the long read
    dist5, end5 = c["want"][5]
    ham = hamming_model(texts, c["a"], qs, cq, cb, hits, BIG)
    assert (dist5 == 0).sum() > 100 and ((dist5 > 0) & (dist5 <= 5)).sum() > 500 and (dist5 == 6).sum() > 30
    assert ((dist5 <= 2) & (ham > 8)).sum() > 150 and dist5[-1] == TOO_LONG and end5[-1] == NO_END
    g = gpu_index(texts, c["a"])
    for k in _SWEEP_LIMITS:
        assert_equal(host_call(g, qs, cq, cb, hits, k), c["want"][k], k)


# ------------------------------------------------------------------------------------------------
# 3. all four query layouts

_LAYOUT_CASES = {}


def _layouts_case(ulen):
    """300 reads of ulen symbols with planted edits or over an end of their text, one candidate each in shuffled order
    -> (alphabet, texts, reads, (cand_query, cand_begin, hits)); shared with test_gpu_align.py"""
    if ulen in _LAYOUT_CASES:
        return _LAYOUT_CASES[ulen]
    rng = np.random.default_rng(12060 + ulen)
    a = alph.ascii_dna()
    texts = [bytes(b"ACGT"[i] for i in rng.integers(0, 4, n)) for n in (2100, 900)]
    qs, cq, cb, hits = [], [], [], []
    for i in range(300):
        text_id = i % 2
        t = texts[text_id]
        if i % 10 == 9:                                 # over an end of the text
            start = int(rng.integers(-20, 0)) if i % 20 == 9 else len(t) - ulen + int(rng.integers(1, 20))
            window = t[max(start, 0):max(start + ulen, 0)]
            q, b = (window.rjust(ulen, b"A") if start < 0 else window.ljust(ulen, b"A")), int(rng.integers(20, ulen + 1))
            position = start + b
        else:
            start = int(rng.integers(0, len(t) - ulen - 4))
            q, where = planted_read(rng, t, start, ulen, i % 5)
            b = int(rng.choice([j for j in range(ulen) if where[j] >= 0]))
            position = where[b]
        qs.append(q), cq.append(i), cb.append(b), hits.append((text_id, position))
    order = rng.permutation(300)                        # candidates need not come in query order
    cq, cb, hits = [cq[i] for i in order], [cb[i] for i in order], [hits[i] for i in order]
    _LAYOUT_CASES[ulen] = (a, texts, qs, (cq, cb, hits))
    return _LAYOUT_CASES[ulen]


# 1, 2, 3 and 4 blocks (edit_kernel<1 and 2, true, 1..4>, <1 and 2, false, 4>); the last block's top bit is 49, 5, 21 and 63
@pytest.mark.parametrize("ulen", (50, 70, 150, 256))
def test_all_four_layouts_give_the_same_arrays(ulen):
    from genedex_amd.device import DeviceEngine, DeviceQueries

    a, texts, qs, (cq, cb, hits) = _layouts_case(ulen)
    wants = {k: edit_model(texts, a, qs, cq, cb, hits, k) for k in (0, 2, 3, 9)}
    for k in (2, 9):                                    # the input condition, on the models alone
        want, ham = wants[k], hamming_model(texts, a, qs, cq, cb, hits, k)
        assert (want[0] <= 2).sum() > 60 and (want[0] > 2).sum() > 60 and (want[0] < ham).sum() > 60
    g = gpu_index(texts, a)
    eng = DeviceEngine(g)
    assert eng.aux_info()["default_shape"]
    plain = DeviceQueries.from_host(*join(qs))
    forms = {"plain": plain, "uniform": plain.as_uniform(ulen), "packed": plain.as_packed(g),
             "packed + uniform": plain.as_uniform(ulen).as_packed(g)}
    assert forms["packed + uniform"].packed and forms["packed + uniform"].uniform_len == ulen
    for k, want in wants.items():
        for name, dq in forms.items():
            assert_equal(device_call(eng, dq, cq, cb, hits, k), want, (name, k))
            dist, end = device_call(eng, dq, cq, cb, hits, k, want_end=False)      # d_out_end = NULL
            assert end is None
            assert_equal((dist,), want[:1], (name, k, "no end"))
        assert_equal(host_call(g, qs, cq, cb, hits, k), want, ("host", k))
        dist, end = host_call(g, qs, cq, cb, hits, k, want_end=False)
        assert end is None
        assert_equal((dist,), want[:1], ("host", k, "no end"))


@pytest.mark.parametrize("ulen", (0, 50, 70, 150, 256))   # 0: lengths 1 .. 256 behind offsets; else 1, 2, 3 and 4 blocks
def test_alphabet_whose_symbols_share_their_low_three_bits(ulen):
    """A, I, Q and Y agree in their low three bits, so the index has no v_perm tables and plain reads are translated through
    the alphabet table in LDS (edit_kernel<0, false, 4> and <0, true, 1..4>), which no stock DNA alphabet reaches"""
    from genedex_amd.device import DeviceEngine, DeviceQueries

    rng = np.random.default_rng(12065 + ulen)
    a = alph.Alphabet.from_io_symbols(b"AIQY")
    assert a.num_searchable_dense_symbols() == 4 and len({s & 7 for s in b"AIQY"}) == 1
    texts = [bytes(b"AIQY"[i] for i in rng.integers(0, 4, n)) for n in (700, 450)]
    wrong = b"AIQYAIQYaiBN\x00\xff"                     # another symbol of the alphabet, or a byte outside it
    qs, cq, cb, hits = [], [], [], []
    for i in range(300):
        text_id = i % 2
        t = texts[text_id]
        ln = ulen or int(rng.integers(1, 257))
        if i % 3 == 0 or ln < 20:                       # anywhere around the text, with substitutions
            start = int(rng.integers(-20, len(t) - ln + 20))
            window = t[max(start, 0):max(start + ln, 0)]
            q = bytearray(window.rjust(ln, b"A") if start < 0 else window.ljust(ln, b"A"))
            b = max(-start, 0) + int(rng.integers(0, ln + 1))      # (may exceed the read's length)
            position = start + b
        else:
            start = int(rng.integers(0, len(t) - ln - 4))
            q, where = planted_read(rng, t, start, ln, i % 4, symbols=b"AIQY")
            q = bytearray(q)
            b = int(rng.choice([j for j in range(ln) if where[j] >= 0]))
            position = where[b]
        for _ in range(i % 2):
            q[int(rng.integers(0, ln))] = wrong[int(rng.integers(0, len(wrong)))]
        qs.append(bytes(q)), cq.append(i), cb.append(b), hits.append((text_id, position))
    wants = {k: edit_model(texts, a, qs, cq, cb, hits, k) for k in (0, 2, 3, 7)}
    for want in (wants[2], wants[7]):                   # the input condition, on the model alone
        assert (want[0] == 0).sum() > 20 and ((want[0] > 0) & (want[0] <= 2)).sum() > 60 and (want[0] > 2).sum() > 30
    g = gpu_index(texts, a)
    eng = DeviceEngine(g)
    assert eng.aux_info()["text_units"]
    dq = DeviceQueries.from_host(*join(qs))
    if ulen:
        dq = dq.as_uniform(ulen)
    for k, want in wants.items():
        assert_equal(device_call(eng, dq, cq, cb, hits, k), want, ("device", k))
        assert_equal(host_call(g, qs, cq, cb, hits, k), want, ("host", k))


# ------------------------------------------------------------------------------------------------
# 5. downstream of the both-strand expand

def test_candidates_on_the_rows_of_a_both_strand_batch():
    from genedex_amd.device import DeviceEngine, DeviceQueries

    rng = np.random.default_rng(12070)
    a = alph.ascii_dna_with_n()
    texts = [bytes(b"ACGT"[i] for i in rng.integers(0, 4, n)) for n in (1500, 800)]
    qs, origin = [], []
    for i in range(200):
        text_id, ln = i % 2, 50
        start = int(rng.integers(0, len(texts[text_id]) - ln - 4))
        q, where = planted_read(rng, texts[text_id], start, ln, i % 3)
        q = bytearray(q)
        if i % 5 == 0:
            q[int(rng.integers(0, ln))] = ord("N")
        qs.append(bytes(q) if i % 4 < 2 else alph.reverse_complement(bytes(q)))   # half of them come from the reverse strand
        origin.append((text_id, start))
    _, both = host_batches(qs)                      # row 2i the read as given, row 2i + 1 its reverse complement
    cq, cb, hits = [], [], []
    for row in range(2 * len(qs)):
        b = int(rng.integers(0, 6))                 # (in front of every edit: on the diagonal of the read's start)
        cq.append(row), cb.append(b), hits.append((origin[row // 2][0], origin[row // 2][1] + b))
    want = edit_model(texts, a, both, cq, cb, hits, 3)
    assert (want[0] <= 3).sum() == len(qs) and (want[0] == 4).sum() == len(qs)    # each read fits on exactly one strand
    g = gpu_index(texts, a)
    eng = DeviceEngine(g)
    plain = DeviceQueries.from_host(*join(qs))
    assert_equal(device_call(eng, plain.with_strands(g, "both"), cq, cb, hits, 3), want, "plain")
    assert_equal(device_call(eng, plain.as_uniform(50).with_strands(g, "both"), cq, cb, hits, 3), want, "uniform")
    clean = [q.replace(b"N", b"A") for q in qs]
    _, both_clean = host_batches(clean)
    want = edit_model(texts, a, both_clean, cq, cb, hits, 3)
    dq = DeviceQueries.from_host(*join(clean)).as_uniform(50).as_packed(g).with_strands(g, "both")
    assert dq.packed and dq.nq == 2 * len(qs)
    assert_equal(device_call(eng, dq, cq, cb, hits, 3), want, "packed + uniform")


# ------------------------------------------------------------------------------------------------
# 6. end to end: SMEMs -> cursor locate -> candidates -> edit distance

def test_smems_locate_edit_distance_end_to_end():
    rng = np.random.default_rng(12080)
    a = alph.ascii_dna()
    texts = [bytes(b"ACGT"[i] for i in rng.integers(0, 4, n)) for n in (3000, 1700, 600)]
    qs, planted = [], []
    for i in range(150):
        t = texts[i % 3]
        ln = int(rng.integers(60, 140))
        start = int(rng.integers(0, len(t) - ln - 4))
        q, where = planted_read(rng, t, start, ln, 1 + i % 3)
        qs.append(q)
        planted.append(1 + i % 3)
    ms, ml, k = 16, 12, 3
    # the input condition, on the models and the oracle alone
    F, R = oracle_pair(texts, a)
    n_smems, remaining, begin, length, start_, end_, status = model_arrays(F, R, qs, ms, ml)
    assert not status.any() and not remaining.any()
    off, t_ids, pos = F.locate_intervals(start_, end_)
    cq, cb = expand_candidates(n_smems, begin, off, ms)
    hits = np.stack([t_ids, pos], axis=1)
    want = edit_model(texts, a, qs, cq, cb, hits, k)
    ham = hamming_model(texts, a, qs, cq, cb, hits, k)
    best = np.full(len(qs), k + 1)
    np.minimum.at(best, cq, want[0])
    best_ham = np.full(len(qs), k + 1)
    np.minimum.at(best_ham, cq, ham)
    assert cq.size >= len(qs) and (best <= np.array(planted)).all()           # every read is found within what was planted
    assert (best < best_ham).sum() * 3 >= len(qs)                             # ... where the Hamming call gives many up
    # the same chain on the GPU
    g, r = gpu_index(texts, a), gpu_index(reversed_texts(texts), a)
    qbuf, qoff = pack_queries(qs)
    g_n, _, g_begin, _, g_start, g_end, _ = g.smems_raw(r, qbuf, qoff, ms, ml)
    g_off, g_t, g_p = g.locate_intervals_raw(g_start, g_end)
    g_cq, g_cb = expand_candidates(g_n, g_begin, g_off, ms)
    assert np.array_equal(g_cq, cq) and np.array_equal(g_cb, cb) and np.array_equal(g_t, t_ids) and np.array_equal(g_p, pos)
    assert_equal(g.edit_distance_raw(qbuf, qoff, g_cq, g_cb, g_t, g_p, k), want, "raw")
    many = g.edit_distance_many(qs, g_cq, g_cb, list(zip(g_t.tolist(), g_p.tolist())), k)
    assert_equal(many, want, "edit_distance_many")


# ------------------------------------------------------------------------------------------------
# 8. the contract

def test_contract():
    import torch

    from genedex_amd import FmIndexConfig
    from genedex_amd.device import DeviceEngine, DeviceQueries

    a = alph.ascii_dna_with_n()
    texts = [b"ACGTACGTTGCA", b"GGA", b""]
    g = gpu_index(texts, a)
    eng = DeviceEngine(g)
    long_read = (b"ACGTTGCA" * 33)[:257]
    qs = [b"ACGTACGT", b"GG#", b"", long_read, long_read[:256]]
    qbuf, qoff = pack_queries(qs)
    none = np.zeros(0, dtype=np.uint32)
    # m == 0 and nq == 0
    assert all(x.size == 0 for x in g.edit_distance_raw(qbuf, qoff, none, none, none, none, 3))
    assert all(x.size == 0 for x in g.edit_distance_raw(np.zeros(8, dtype=np.uint8), np.zeros(1, dtype=np.uint64), none, none, none, none, 3))
    # (nq == 0 is GDX_OK in both forms: candidates of an empty batch are all out of range)
    dist, end = g.edit_distance_raw(np.zeros(8, dtype=np.uint8), np.zeros(1, dtype=np.uint64), [0, 1], [0, 0], [0, 1], [0, 0], 3)
    assert dist.tolist() == [INVALID, INVALID] and end.tolist() == [NO_END, NO_END]
    dq = DeviceQueries.from_host(qbuf, qoff)
    assert all(x.size == 0 for x in device_call(eng, dq, [], [], [], 3))
    empty = DeviceQueries.from_host(np.zeros(8, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    assert all(x.size == 0 for x in device_call(eng, empty, [], [], [], 3))
    dist, end = device_call(eng, empty, [0, 1], [0, 0], [(0, 0), (1, 0)], 3)
    assert dist.tolist() == [INVALID, INVALID] and end.tolist() == [NO_END, NO_END]
    # the definition's corners: a byte outside the alphabet is one edit and raises nothing; overhang; the empty read; the empty
    # text; a read over the limit among the others (the call stays GDX_OK); 256 symbols are within it
    cq = [0, 1, 1, 0, 2, 2, 0, 3, 4, 0]
    cb = [0, 0, 1, 4, 0, 5, 0, 0, 0, 0]
    hits = [(0, 0), (1, 0), (1, 1), (0, 8), (0, 7), (1, 0), (2, 0), (0, 0), (0, 0), (0, 4)]
    want = edit_model(texts, a, qs, cq, cb, hits, 3)
    # (candidates 3 and 9: the window begins at symbol 1, so CGTACGT = T[1, 8) with the read's first A inserted beats the diagonal)
    assert want[0].tolist() == [0, 1, 1, 1, 0, 0, 4, TOO_LONG, 4, 1]
    assert want[1].tolist() == [8, 2, 2, 8, 4, 0, NO_END, NO_END, NO_END, 8]
    assert_equal(host_call(g, qs, cq, cb, hits, 3), want, "host")
    assert_equal(device_call(eng, dq, cq, cb, hits, 3), want, "device")
    for k in (0, 8):
        want_k = edit_model(texts, a, qs, cq, cb, hits, k)
        assert_equal(host_call(g, qs, cq, cb, hits, k), want_k, ("host", k))
        assert_equal(device_call(eng, dq, cq, cb, hits, k), want_k, ("device", k))
    # a uniform batch over the limit: every candidate is too long
    uni = DeviceQueries.from_host(*join([long_read, long_read])).as_uniform(257)
    dist, end = device_call(eng, uni, [0, 1, 2], [0, 0, 0], [(0, 0), (1, 0), (0, 0)], 3)
    assert dist.tolist() == [TOO_LONG, TOO_LONG, INVALID] and end.tolist() == [NO_END] * 3
    # a query or a text id out of range: the device form writes GDX_EDIT_INVALID, the host form refuses, also a position >= 2^32
    cq2, hits2 = [0, 5, 1, 0xFFFFFFFF], [(0, 0), (0, 0), (3, 0), (0xFFFFFFFF, 0)]
    dist, end = device_call(eng, dq, cq2, [0, 0, 0, 0], hits2, 3)
    assert dist.tolist() == [0, INVALID, INVALID, INVALID] and end.tolist() == [8, NO_END, NO_END, NO_END]
    assert status_of(lambda: host_call(g, qs, [0, 5], [0, 0], [(0, 0), (0, 0)], 3)) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert status_of(lambda: host_call(g, qs, [0, 1], [0, 0], [(0, 0), (3, 0)], 3)) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert status_of(lambda: host_call(g, qs, [0, 1], [0, 0], [(0, 0), (1, 1 << 32)], 3)) == _lib.GDX_ERR_INVALID_ARGUMENT
    # max_edits: 256 is the largest, in both forms
    want = edit_model(texts, a, qs, cq, cb, hits, 256)
    assert_equal(host_call(g, qs, cq, cb, hits, 256), want, "256")
    assert_equal(device_call(eng, dq, cq, cb, hits, 256), want, "256, device")
    assert status_of(lambda: host_call(g, qs, cq, cb, hits, 257)) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert status_of(lambda: device_call(eng, dq, cq, cb, hits, 257)) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert status_of(lambda: device_call(eng, dq, cq, cb, hits, 0xFFFFFFFF)) == _lib.GDX_ERR_INVALID_ARGUMENT
    # ... and a refused call writes nothing
    lib = _lib.load()
    z = torch.full((8,), 7, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = lib.gdx_edit_distance_many_dev(g._h, p(dq.qbuf), p(dq.qoff), dq.nq, None, p(z), p(z), p(z), 1, 257, p(z), p(z[4:]), None)
    assert st == _lib.GDX_ERR_INVALID_ARGUMENT
    # an unknown layout
    lay = _lib.QueryLayout()
    lib.gdx_query_layout_init(C.byref(lay))
    lay.packed = 2
    st = lib.gdx_edit_distance_many_dev(g._h, p(dq.qbuf), p(dq.qoff), dq.nq, C.byref(lay), p(z), p(z), p(z), 1, 3, p(z), p(z[4:]), None)
    assert st == _lib.GDX_ERR_INVALID_ARGUMENT
    # an index without text units, the packed form on an index that takes no packed queries, the 64-bit engine
    bare = gpu_index(texts, a, text_units=False, seed_symbols=0, full_suffix_array=False, inverse_suffix_array=False)
    assert not DeviceEngine(bare).aux_info()["text_units"]
    assert status_of(lambda: host_call(bare, qs, cq, cb, hits, 3)) == _lib.GDX_ERR_UNSUPPORTED
    assert status_of(lambda: device_call(DeviceEngine(bare), dq, cq, cb, hits, 3)) == _lib.GDX_ERR_UNSUPPORTED
    three = gpu_index([b"ACGACGGACA"], alph.Alphabet.from_io_symbols(b"ACG"), text_units=True)   # dense symbol 4 does not exist
    assert DeviceEngine(three).aux_info()["text_units"]
    dist, end = device_call(DeviceEngine(three), DeviceQueries.from_host(*pack_queries([b"GACGT"])), [0], [0], [(0, 2)], 9)
    assert (dist.tolist(), end.tolist()) == ([1], [6])
    packed = DeviceQueries(dq.qbuf, dq.qoff, dq.nq, dq.total_bytes, True, 0)
    assert status_of(lambda: device_call(DeviceEngine(three), packed, [0], [0], [(0, 0)], 3)) == _lib.GDX_ERR_UNSUPPORTED
    lib.gdx_debug_force_wide(1)
    try:
        w = FmIndexConfig("i64").suffix_array_sampling_rate(4).construct_index(texts, a)
    finally:
        lib.gdx_debug_force_wide(0)
    assert w.info.index_width == 64
    assert status_of(lambda: host_call(w, qs, cq, cb, hits, 3)) == _lib.GDX_ERR_UNSUPPORTED
    st = lib.gdx_edit_distance_many_dev(w._h, p(dq.qbuf), p(dq.qoff), dq.nq, None, p(z), p(z), p(z), 1, 3, p(z), p(z[4:]), None)
    assert st == _lib.GDX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert z.cpu().tolist() == [7] * 8              # (nothing was written by any of the refused calls)
