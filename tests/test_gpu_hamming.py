"""gdx_hamming_many[_dev] on the GPU against the CPU model of tests/test_hamming_model.py (the definition of include/gdx.h on
bytes and the alphabet table).  Outputs are integers: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_parity as parity
from genedex_amd import GdxError, _lib, reversed_texts
from genedex_amd import alphabet as alph
from helpers import random_texts
from oracle.oracle import pack_queries
from test_gpu_parity import _VARIANTS, gpu_index
from test_hamming_model import INVALID, hamming_model
from test_smems_model import model_arrays, oracle_pair
from test_strands_model import host_batches, join
from test_suffix_segments_model import reads_with_errors

pytestmark = pytest.mark.gpu

BIG = 1 << 31


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


def host_call(g, qs, cq, cb, hits, k):
    qbuf, qoff = pack_queries(qs)
    hits = np.asarray(hits, dtype=np.uint64).reshape(-1, 2)
    return g.hamming_raw(qbuf, qoff, cq, cb, hits[:, 0], hits[:, 1], k)


def assert_equal(got, want, what):
    assert got.dtype == np.uint32 and got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, int(bad.size), int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


def device_call(eng, dq, cq, cb, hits, k):
    """gdx_hamming_many_dev on host-made candidates -> u32[m]; the output starts as garbage: every entry must be written"""
    import torch

    def dev(x, shape=None):
        x = np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)
        return torch.from_numpy(x.reshape(shape) if shape else x).cuda()

    m = len(cq)
    out = torch.full((max(m, 1),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    eng.hamming(dq, dev(cq), dev(cb), dev(np.asarray(hits, dtype=np.uint64).reshape(-1, 2), (-1, 2)), k, out)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)[:m]


# ------------------------------------------------------------------------------------------------
# 1. random collections, every variant

_RANDOM_CASES = {}
_LIMITS = (0, 1, 3, BIG)


def find_origin(texts, a, q):
    """(text_id, start) of the diagonal q was sampled from (at most a dozen mismatches on it), found through an exact quarter
    of q; or None"""
    if len(q) < 24:
        return None
    step = len(q) // 4
    for k in range(4):
        piece = q[k * step:(k + 1) * step]
        for text_id, t in enumerate(texts):
            p = t.find(piece)
            if p >= k * step and hamming_model(texts, a, [q], [0], [0], [(text_id, p - k * step)], BIG)[0] <= 12:
                return text_id, p - k * step
    return None


def _random_case(seed):
    """(alphabet, texts, reads, candidates, {limit: model}); the generator's seeds are chosen so that the precondition below holds"""
    if seed in _RANDOM_CASES:
        return _RANDOM_CASES[seed]
    rng = np.random.default_rng(9900 + seed)
    a = alph.ascii_dna_with_n()
    symbols = b"ACGT" * 6 + b"N" if seed % 2 else b"ACGT"   # (one symbol in 25 an N: uniform ACGTN leaves no read near its origin)
    texts = random_texts(rng, len_max=[5000, 2500][seed % 2], symbols=symbols)
    while sum(len(t) for t in texts) < 1500:
        texts = random_texts(rng, len_max=5000, symbols=symbols)
    qs = reads_with_errors(rng, texts, 160, 40, [200, 80][seed % 2], symbols=symbols)
    cq, cb, hits = [], [], []
    for i, q in enumerate(qs):
        origin = find_origin(texts, a, q)
        if origin is not None:
            text_id, start = origin
            for _ in range(2):                        # the true origin, named by two seeds
                b = int(rng.integers(0, len(q) + 1))
                cq.append(i), cb.append(b), hits.append((text_id, start + b))
            for d in ((i % 3) + 1, -((i % 3) + 1)):   # ... and shifted by -3 .. +3
                b = int(rng.integers(3, len(q) + 1))
                if start + b + d >= 0:
                    cq.append(i), cb.append(b), hits.append((text_id, start + b + d))
        text_id = int(rng.integers(0, len(texts)))    # anywhere, out of the text included
        cq.append(i), cb.append(int(rng.integers(0, len(q) + 6))), hits.append((text_id, int(rng.integers(0, len(texts[text_id]) + 60))))
    want = {k: hamming_model(texts, a, qs, cq, cb, hits, k) for k in _LIMITS}
    _RANDOM_CASES[seed] = (a, texts, qs, (cq, cb, hits), want)
    return _RANDOM_CASES[seed]


@pytest.mark.parametrize("seed", range(2))
def test_random_collections_equal_the_model(seed, variant):
    from genedex_amd.device import DeviceEngine

    a, texts, qs, (cq, cb, hits), want = _random_case(seed)
    # the precondition, on the model alone: not everything saturates, not everything is a perfect match
    full = want[BIG]
    assert len(cq) > 500 and (full <= 3).sum() * 5 >= len(cq) and (want[3] == 4).sum() * 5 >= len(cq)
    assert (full == 0).sum() > 0 and ((full > 0) & (full <= 3)).sum() > 50
    g = gpu_index(texts, a)
    if not DeviceEngine(g).aux_info()["text_units"]:
        assert status_of(lambda: host_call(g, qs, cq, cb, hits, 3)) == _lib.GDX_ERR_UNSUPPORTED
        return
    for k in _LIMITS:
        assert_equal(host_call(g, qs, cq, cb, hits, k), want[k], (seed, variant, k))


# ------------------------------------------------------------------------------------------------
# 2. alignment sweep: every phase of the window in its units, every chunk count, both ends of a text

_SWEEP = {}
_LENGTHS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300)


def _sweep_case():
    if _SWEEP:
        return _SWEEP
    rng = np.random.default_rng(9950)
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
            starts = list(range(10, 42)) + [-40, -1, 0] + [len(t) + e - ln for e in (-1, 0, 1, 40)]
            for s in starts:
                lo, hi = max(base + s, 0), max(base + s + ln, 0)
                q = bytearray(around[lo:hi].rjust(ln, b"T")[:ln].ljust(ln, b"T"))
                for _ in range(int(rng.integers(0, 3))):
                    q[int(rng.integers(0, ln))] = b"ACGTN"[int(rng.integers(0, 5))]
                b = int(rng.integers(max(-s, 0), max(-s, 0) + ln + 1))   # (may exceed the read's length)
                qs.append(bytes(q)), cq.append(len(qs) - 1), cb.append(b), hits.append((text_id, s + b))
    phases = {(sum(len(x) + 1 for x in texts[:t]) + p - b) % 32 for (t, p), b in zip(hits, cb)}
    assert phases == set(range(32))
    for text_id in (2, 3):  # the empty text and the text of one symbol, between their neighbours
        for q, b, p in ((b"G", 0, 0), (b"GG", 1, 0), (b"GG", 0, 0), (texts[1][-3:] + b"AG", 4, 0), (b"", 0, 0), (b"G" + texts[4][:40], 0, 0)):
            qs.append(q), cq.append(len(qs) - 1), cb.append(b), hits.append((text_id, p))
    _SWEEP.update(a=a, texts=texts, qs=qs, cand=(cq, cb, hits),
                  want={k: hamming_model(texts, a, qs, cq, cb, hits, k) for k in (1, BIG)})
    return _SWEEP


def test_alignment_sweep():
    c = _sweep_case()
    full = c["want"][BIG]
    lens = np.array([len(c["qs"][i]) for i in c["cand"][0]])
    # the inputs do what they are for: reads that hang over an end count the overhang, and most windows inside agree
    assert (full == 0).sum() > 100 and ((full > 0) & (full < 3)).sum() > 300 and (full >= np.minimum(lens, 40)).sum() > 30
    g = gpu_index(c["texts"], c["a"])
    for k in (1, BIG):
        assert_equal(host_call(g, c["qs"], *c["cand"], k), c["want"][k], k)


# ------------------------------------------------------------------------------------------------
# 3. all four query layouts

@pytest.mark.parametrize("ulen", (50, 137))
def test_all_four_layouts_give_the_same_array(ulen):
    from genedex_amd.device import DeviceEngine, DeviceQueries

    rng = np.random.default_rng(9960 + ulen)
    a = alph.ascii_dna()
    texts = [bytes(b"ACGT"[i] for i in rng.integers(0, 4, n)) for n in (2100, 900)]
    qs, cq, cb, hits = [], [], [], []
    for i in range(300):
        text_id = i % 2
        start = int(rng.integers(-20, len(texts[text_id]) - ulen + 20))
        window = texts[text_id][max(start, 0):max(start + ulen, 0)]
        q = bytearray(window.rjust(ulen, b"A") if start < 0 else window.ljust(ulen, b"A"))
        for _ in range(i % 5):
            q[int(rng.integers(0, ulen))] = b"ACGT"[int(rng.integers(0, 4))]
        b = int(rng.integers(max(-start, 0), ulen + 1))
        qs.append(bytes(q)), cq.append(i), cb.append(b), hits.append((text_id, start + b))
    order = rng.permutation(300)                      # candidates need not come in query order
    cq, cb, hits = [cq[i] for i in order], [cb[i] for i in order], [hits[i] for i in order]
    g = gpu_index(texts, a)
    eng = DeviceEngine(g)
    assert eng.aux_info()["default_shape"]
    plain = DeviceQueries.from_host(*join(qs))
    forms = {"plain": plain, "uniform": plain.as_uniform(ulen), "packed": plain.as_packed(g),
             "packed + uniform": plain.as_uniform(ulen).as_packed(g)}
    assert forms["packed + uniform"].packed and forms["packed + uniform"].uniform_len == ulen
    for k in (2, BIG):
        want = hamming_model(texts, a, qs, cq, cb, hits, k)
        assert (want <= 2).sum() > 60 and (want > 2).sum() > 60
        for name, dq in forms.items():
            assert_equal(device_call(eng, dq, cq, cb, hits, k), want, (name, k))
        assert_equal(host_call(g, qs, cq, cb, hits, k), want, ("host", k))


@pytest.mark.parametrize("ulen", (0, 70))   # 0: lengths 1 .. 200 behind offsets
def test_alphabet_whose_symbols_share_their_low_three_bits(ulen):
    """A, I, Q and Y agree in their low three bits, so the index has no v_perm tables and plain reads are translated through
    the alphabet table in LDS (hamming_kernel<0, .>), which no stock DNA alphabet reaches"""
    from genedex_amd.device import DeviceEngine, DeviceQueries

    rng = np.random.default_rng(9965 + ulen)
    a = alph.Alphabet.from_io_symbols(b"AIQY")
    assert a.num_searchable_dense_symbols() == 4 and len({s & 7 for s in b"AIQY"}) == 1
    texts = [bytes(b"AIQY"[i] for i in rng.integers(0, 4, n)) for n in (700, 450)]
    wrong = b"AIQYAIQYaiBN\x00\xff"                     # another symbol of the alphabet, or a byte outside it
    qs, cq, cb, hits = [], [], [], []
    for i in range(300):
        text_id = i % 2
        ln = ulen or int(rng.integers(1, 201))
        start = int(rng.integers(-20, len(texts[text_id]) - ln + 20))
        window = texts[text_id][max(start, 0):max(start + ln, 0)]
        q = bytearray(window.rjust(ln, b"A") if start < 0 else window.ljust(ln, b"A"))
        for _ in range(i % 5):
            q[int(rng.integers(0, ln))] = wrong[int(rng.integers(0, len(wrong)))]
        b = max(-start, 0) + int(rng.integers(0, ln + 1))      # (may exceed the read's length)
        qs.append(bytes(q)), cq.append(i), cb.append(b), hits.append((text_id, start + b))
    g = gpu_index(texts, a)
    eng = DeviceEngine(g)
    assert eng.aux_info()["text_units"]
    dq = DeviceQueries.from_host(*join(qs))
    if ulen:
        dq = dq.as_uniform(ulen)
    for k in (2, BIG):
        want = hamming_model(texts, a, qs, cq, cb, hits, k)
        assert (want == 0).sum() > 20 and ((want > 0) & (want <= 2)).sum() > 60 and (want > 2).sum() > 60
        assert_equal(device_call(eng, dq, cq, cb, hits, k), want, ("device", k))
        assert_equal(host_call(g, qs, cq, cb, hits, k), want, ("host", k))


# ------------------------------------------------------------------------------------------------
# 4. downstream of the both-strand expand

def test_candidates_on_the_rows_of_a_both_strand_batch():
    from genedex_amd.device import DeviceEngine, DeviceQueries

    rng = np.random.default_rng(9970)
    a = alph.ascii_dna_with_n()
    texts = [bytes(b"ACGT"[i] for i in rng.integers(0, 4, n)) for n in (1500, 800)]
    qs, origin = [], []
    for i in range(200):
        text_id, ln = i % 2, 50
        start = int(rng.integers(0, len(texts[text_id]) - ln))
        q = bytearray(texts[text_id][start:start + ln])
        if i % 3 == 0:
            q[int(rng.integers(0, ln))] = ord("N")
        qs.append(bytes(q) if i % 4 < 2 else alph.reverse_complement(bytes(q)))   # half of them come from the reverse strand
        origin.append((text_id, start))
    _, both = host_batches(qs)                      # row 2i the read as given, row 2i + 1 its reverse complement
    cq, cb, hits = [], [], []
    for row in range(2 * len(qs)):
        b = int(rng.integers(0, 51))
        cq.append(row), cb.append(b), hits.append((origin[row // 2][0], origin[row // 2][1] + b))
    g = gpu_index(texts, a)
    eng = DeviceEngine(g)
    want = hamming_model(texts, a, both, cq, cb, hits, 3)
    assert (want <= 1).sum() == len(qs) and (want == 4).sum() > len(qs) * 4 // 5    # each read fits on exactly one strand
    plain = DeviceQueries.from_host(*join(qs))
    assert_equal(device_call(eng, plain.with_strands(g, "both"), cq, cb, hits, 3), want, "plain")
    assert_equal(device_call(eng, plain.as_uniform(50).with_strands(g, "both"), cq, cb, hits, 3), want, "uniform")
    clean = [q.replace(b"N", b"A") for q in qs]
    _, both_clean = host_batches(clean)
    want = hamming_model(texts, a, both_clean, cq, cb, hits, 3)
    dq = DeviceQueries.from_host(*join(clean)).as_uniform(50).as_packed(g).with_strands(g, "both")
    assert dq.packed and dq.nq == 2 * len(qs)
    assert_equal(device_call(eng, dq, cq, cb, hits, 3), want, "packed + uniform")


# ------------------------------------------------------------------------------------------------
# 5. end to end: SMEMs -> cursor locate -> candidates -> hamming

def expand_candidates(n_smems, begin, hit_offsets, max_smems):
    """per located hit the query of its cursor and where the cursor's seed begins in it"""
    per_slot = np.diff(hit_offsets.astype(np.int64))
    slots = np.arange(per_slot.size)
    used = (slots % max_smems) < n_smems[slots // max_smems]
    assert not per_slot[~used].any()
    return np.repeat(slots // max_smems, per_slot).astype(np.uint32), np.repeat(begin, per_slot).astype(np.uint32)


def test_smems_locate_hamming_end_to_end():
    rng = np.random.default_rng(9980)
    a = alph.ascii_dna()
    texts = [bytes(b"ACGT"[i] for i in rng.integers(0, 4, n)) for n in (3000, 1700, 600)]
    qs, planted = [], []
    for i in range(150):
        t = texts[i % 3]
        ln = int(rng.integers(60, 140))
        start = int(rng.integers(0, len(t) - ln))
        q = bytearray(t[start:start + ln])
        for k in rng.choice(ln, size=1 + i % 3, replace=False):
            q[int(k)] = b"ACGT"[int(rng.integers(0, 4))]
        qs.append(bytes(q))
        planted.append(sum(x != y for x, y in zip(q, t[start:start + ln])))   # the substitutions that changed the symbol
    ms, ml, k = 16, 12, 3
    # the input condition, on the model and the oracle alone
    F, R = oracle_pair(texts, a)
    n_smems, remaining, begin, length, start_, end_, status = model_arrays(F, R, qs, ms, ml)
    assert not status.any() and not remaining.any()
    off, t_ids, pos = F.locate_intervals(start_, end_)
    cq, cb = expand_candidates(n_smems, begin, off, ms)
    hits = np.stack([t_ids, pos], axis=1)
    want = hamming_model(texts, a, qs, cq, cb, hits, k)
    best = np.full(len(qs), k + 1)
    np.minimum.at(best, cq, want)
    assert cq.size >= len(qs) and (best == np.array(planted)).sum() * 5 >= len(qs) and min(planted) == 0 and max(planted) == 3
    # the same chain on the GPU
    g, r = gpu_index(texts, a), gpu_index(reversed_texts(texts), a)
    qbuf, qoff = pack_queries(qs)
    g_n, _, g_begin, _, g_start, g_end, _ = g.smems_raw(r, qbuf, qoff, ms, ml)
    g_off, g_t, g_p = g.locate_intervals_raw(g_start, g_end)
    g_cq, g_cb = expand_candidates(g_n, g_begin, g_off, ms)
    assert np.array_equal(g_cq, cq) and np.array_equal(g_cb, cb) and np.array_equal(g_t, t_ids) and np.array_equal(g_p, pos)
    assert_equal(g.hamming_raw(qbuf, qoff, g_cq, g_cb, g_t, g_p, k), want, "raw")
    many = g.hamming_many(qs, g_cq, g_cb, list(zip(g_t.tolist(), g_p.tolist())), k)
    assert_equal(many, want, "hamming_many")


# ------------------------------------------------------------------------------------------------
# 6. the contract

def test_contract():
    import torch

    from genedex_amd import FmIndexConfig
    from genedex_amd.device import DeviceEngine, DeviceQueries

    a = alph.ascii_dna_with_n()
    texts = [b"ACGTACGTTGCA", b"GGA"]
    g = gpu_index(texts, a)
    eng = DeviceEngine(g)
    qs = [b"ACGTACGT", b"GG#"]
    qbuf, qoff = pack_queries(qs)
    none = np.zeros(0, dtype=np.uint32)
    # m == 0 and nq == 0
    assert g.hamming_raw(qbuf, qoff, none, none, none, none, 3).size == 0
    assert g.hamming_raw(np.zeros(8, dtype=np.uint8), np.zeros(1, dtype=np.uint64), none, none, none, none, 3).size == 0
    # (nq == 0 is GDX_OK in both forms: candidates of an empty batch are all out of range and get GDX_HAMMING_INVALID)
    got = g.hamming_raw(np.zeros(8, dtype=np.uint8), np.zeros(1, dtype=np.uint64), [0, 1], [0, 0], [0, 1], [0, 0], 3)
    assert got.tolist() == [INVALID, INVALID]
    dq = DeviceQueries.from_host(qbuf, qoff)
    assert device_call(eng, dq, [], [], [], 3).size == 0
    empty = DeviceQueries.from_host(np.zeros(8, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    assert device_call(eng, empty, [], [], [], 3).size == 0
    assert device_call(eng, empty, [0, 1], [0, 0], [(0, 0), (1, 0)], 3).tolist() == [INVALID, INVALID]
    # a byte outside the alphabet counts as one mismatch and raises nothing
    cq, cb, hits = [0, 1, 1, 0], [0, 0, 1, 4], [(0, 0), (1, 0), (1, 1), (0, 8)]
    want = hamming_model(texts, a, qs, cq, cb, hits, 3)
    assert want.tolist() == [0, 1, 1, 4]
    assert_equal(host_call(g, qs, cq, cb, hits, 3), want, "host")
    assert_equal(device_call(eng, dq, cq, cb, hits, 3), want, "device")
    # a query or a text id out of range: the device form writes GDX_HAMMING_INVALID, the host form refuses
    cq2, hits2 = [0, 2, 1, 0xFFFFFFFF], [(0, 0), (0, 0), (2, 0), (0xFFFFFFFF, 0)]
    assert device_call(eng, dq, cq2, [0, 0, 0, 0], hits2, 3).tolist() == [0, INVALID, INVALID, INVALID]
    assert status_of(lambda: host_call(g, qs, [0, 2], [0, 0], [(0, 0), (0, 0)], 3)) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert status_of(lambda: host_call(g, qs, [0, 1], [0, 0], [(0, 0), (2, 0)], 3)) == _lib.GDX_ERR_INVALID_ARGUMENT
    # max_mismatches: 2^31 is the largest
    assert_equal(host_call(g, qs, cq, cb, hits, BIG), hamming_model(texts, a, qs, cq, cb, hits, BIG), "2^31")
    assert status_of(lambda: host_call(g, qs, cq, cb, hits, BIG + 1)) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert status_of(lambda: device_call(eng, dq, cq, cb, hits, 0xFFFFFFFF)) == _lib.GDX_ERR_INVALID_ARGUMENT
    # an unknown layout
    lay = _lib.QueryLayout()
    _lib.load().gdx_query_layout_init(C.byref(lay))
    lay.packed = 2
    z = torch.zeros(8, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = _lib.load().gdx_hamming_many_dev(g._h, p(dq.qbuf), p(dq.qoff), dq.nq, C.byref(lay), p(z), p(z), p(z), 1, 3, p(z), None)
    assert st == _lib.GDX_ERR_INVALID_ARGUMENT
    # an index without text units, the packed form on an index that takes no packed queries, the 64-bit engine
    bare = gpu_index(texts, a, text_units=False, seed_symbols=0, full_suffix_array=False, inverse_suffix_array=False)
    assert not DeviceEngine(bare).aux_info()["text_units"]
    assert status_of(lambda: host_call(bare, qs, cq, cb, hits, 3)) == _lib.GDX_ERR_UNSUPPORTED
    assert status_of(lambda: device_call(DeviceEngine(bare), dq, cq, cb, hits, 3)) == _lib.GDX_ERR_UNSUPPORTED
    three = gpu_index([b"ACGACGGACA"], alph.Alphabet.from_io_symbols(b"ACG"), text_units=True)   # dense symbol 4 does not exist
    assert DeviceEngine(three).aux_info()["text_units"]
    assert device_call(DeviceEngine(three), DeviceQueries.from_host(*pack_queries([b"GACGT"])), [0], [0], [(0, 2)], 9).tolist() == [1]
    packed = DeviceQueries(dq.qbuf, dq.qoff, dq.nq, dq.total_bytes, True, 0)
    assert status_of(lambda: device_call(DeviceEngine(three), packed, [0], [0], [(0, 0)], 3)) == _lib.GDX_ERR_UNSUPPORTED
    lib = _lib.load()
    lib.gdx_debug_force_wide(1)
    try:
        w = FmIndexConfig("i64").suffix_array_sampling_rate(4).construct_index(texts, a)
    finally:
        lib.gdx_debug_force_wide(0)
    assert w.info.index_width == 64
    assert status_of(lambda: host_call(w, qs, cq, cb, hits, 3)) == _lib.GDX_ERR_UNSUPPORTED
    st = lib.gdx_hamming_many_dev(w._h, p(dq.qbuf), p(dq.qoff), dq.nq, None, p(z), p(z), p(z), 1, 3, p(z), None)
    assert st == _lib.GDX_ERR_UNSUPPORTED
    assert z.cpu().tolist() == [0] * 8              # (and nothing was written)
