"""gdx_align_many[_dev] on the GPU against the CPU model of tests/test_align_model.py (the definition of include/gdx.h with a
plain table) and against gdx_edit_distance_many on the GPU.  Outputs are integers: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from genedex_amd import GdxError, _lib, reversed_texts
from genedex_amd import alphabet as alph
from oracle.oracle import pack_queries
from test_align_model import DEL, INS, align_model, replay_all, runs_of, sam
from test_edit_distance_model import INVALID, NO_END, TOO_LONG
from test_gpu_edit_distance import _LIMITS, _layouts_case, _random_case, planted_read, status_of, variant  # noqa: F401  (variant: a fixture)
from test_gpu_hamming import expand_candidates
from test_gpu_parity import gpu_index
from test_smems_model import model_arrays, oracle_pair
from test_strands_model import host_batches, join

pytestmark = pytest.mark.gpu

GARBAGE = 0x5A5A5A5A
NAMES = ("dist", "begin", "end", "n_cigar", "cigar")


def host_call(g, qs, cq, cb, hits, k):
    qbuf, qoff = pack_queries(qs)
    hits = np.asarray(hits, dtype=np.uint64).reshape(-1, 2)
    return g.align_raw(qbuf, qoff, cq, cb, hits[:, 0], hits[:, 1], k)


def device_call(eng, dq, cq, cb, hits, k, workspace_bytes=None, raw=False):
    """gdx_align_many_dev on host-made candidates -> (dist, begin, end, n_cigar, cigar[m, 2 k + 1]) as uint32 arrays.  The
    outputs start as GARBAGE (raw=False: the cigar words from n_cigar on are then checked to be GARBAGE still and come back as
    zero, like the model's).  workspace_bytes: the size of the workspace handed over, None for the best size."""
    import torch

    def dev(x, shape=None):
        x = np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)
        return torch.from_numpy(x.reshape(shape) if shape else x).cuda()

    m = len(cq)
    out = {name: torch.full((max(m, 1),), GARBAGE, dtype=torch.int32, device="cuda") for name in NAMES[:4]}
    out["cigar"] = torch.full((max(m, 1), 2 * min(k, 256) + 1), GARBAGE, dtype=torch.int32, device="cuda")
    ws = None if workspace_bytes is None else torch.empty(workspace_bytes, dtype=torch.uint8, device="cuda")
    got = eng.align(dq, dev(cq), dev(cb), dev(np.asarray(hits, dtype=np.uint64).reshape(-1, 2), (-1, 2)), k, out=out, workspace=ws)
    torch.cuda.synchronize()
    assert all(got[name] is out[name] for name in NAMES)
    res = [out[name].cpu().numpy().view(np.uint32)[:m] for name in NAMES]
    if raw:
        return tuple(res)
    beyond = np.arange(res[4].shape[1])[None, :] >= res[3][:, None]
    assert (res[4][beyond] == GARBAGE).all(), "a cigar word from n_cigar on was written"
    res[4] = np.where(beyond, 0, res[4]).astype(np.uint32)
    return tuple(res)


def assert_equal(got, want, what):
    """all five outputs; cigar rows are compared below n_cigar (both sides hold zero behind it)"""
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == np.uint32 and g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, len(bad), bad[0].tolist(), int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


# ------------------------------------------------------------------------------------------------
# 1. random reads with indels, every variant

_MODELS = {}


def _random_model(seed, k):
    if (seed, k) not in _MODELS:
        a, texts, qs, (cq, cb, hits), _, _, _ = _random_case(seed)
        _MODELS[seed, k] = align_model(texts, a, qs, cq, cb, hits, k)
    return _MODELS[seed, k]


@pytest.mark.parametrize("seed", range(2))
def test_random_reads_with_indels_equal_the_model(seed, variant):  # noqa: F811
    from genedex_amd.device import DeviceEngine

    a, texts, qs, (cq, cb, hits), _, edit_want, _ = _random_case(seed)
    m = len(cq)
    assert m == 900
    want3 = _random_model(seed, 3)                                 # the preconditions, on the model alone, at limit 3
    aligned = np.flatnonzero(want3[2] != NO_END)
    with_indel = sum(any(op in (INS, DEL) for _, op in runs_of(want3[3][c], want3[4][c])) for c in aligned)
    assert aligned.size * 5 >= 2 * m and with_indel * 10 >= aligned.size
    for k in _LIMITS:                                              # the model agrees with the edit-distance model, and replays
        want = _random_model(seed, k)
        assert np.array_equal(want[0], edit_want[k][0]) and np.array_equal(want[2], edit_want[k][1])
        assert replay_all(a, texts, qs, cq, hits, want) == int((want[2] != NO_END).sum())
    g = gpu_index(texts, a)
    if not DeviceEngine(g).aux_info()["text_units"]:
        assert status_of(lambda: host_call(g, qs, cq, cb, hits, 3)) == _lib.GDX_ERR_UNSUPPORTED
        return
    for k in _LIMITS:
        assert_equal(host_call(g, qs, cq, cb, hits, k), _random_model(seed, k), (seed, variant, k))


# ------------------------------------------------------------------------------------------------
# 2. dist and end are those of gdx_edit_distance_many on the GPU, marker rows included

def test_dist_and_end_equal_the_edit_distance_call_on_the_gpu():
    import torch

    from genedex_amd.device import DeviceEngine, DeviceQueries

    a, texts, qs, (cq, cb, hits), _, _, _ = _random_case(1)
    qs = list(qs) + [(texts[0] * 2)[:257], (texts[0] * 2)[7:263]]            # a read over the limit and one of 256 symbols
    cq = list(cq) + [len(qs) - 2, len(qs) - 1, len(qs), 0, 0xFFFFFFFF]        # ... and rows out of range
    cb = list(cb) + [0, 0, 0, 0, 0]
    hits = list(hits) + [(0, 0), (0, 7), (0, 0), (len(texts), 0), (0, 0)]
    g = gpu_index(texts, a)
    eng = DeviceEngine(g)
    dq = DeviceQueries.from_host(*join(qs))
    dev = lambda x, shape=None: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32).reshape(shape or -1)).cuda()  # noqa: E731
    d_cq, d_cb, d_hits = dev(cq), dev(cb), dev(np.asarray(hits, dtype=np.uint64), (-1, 2))
    for k in _LIMITS:
        got = device_call(eng, dq, cq, cb, hits, k)
        dist, end = eng.edit_distance(dq, d_cq, d_cb, d_hits, k)
        torch.cuda.synchronize()
        dist, end = dist.cpu().numpy().view(np.uint32), end.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[0], dist) and np.array_equal(got[2], end), k
        assert got[0][-5:].tolist() == [TOO_LONG, 0, INVALID, INVALID, INVALID] and (got[2][-5:] == NO_END).tolist() == [True, False, True, True, True]
        assert ((got[2] == NO_END) == (got[1] == NO_END)).all() and (got[3][got[2] == NO_END] == 0).all()
        assert (got[1][got[2] != NO_END] <= got[2][got[2] != NO_END]).all()


# ------------------------------------------------------------------------------------------------
# 3. word borders and unit phases: every block count and last-block bit, one edit of each kind at the block seam (read rows
#    62..65) and at the unit seam (a text position that is a multiple of 32, give or take one), every phase of the window's
#    first unit, windows clipped at both ends of a text, a text directly behind another

_SWEEP = {}
_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
_SWEEP_LIMITS = (0, 1, 5, 33)


def _sweep_case(symbols):
    """reads sorted by length; per length 3 texts x 36 window starts, the edit kind cycling none / inserted / skipped /
    substituted -> dict(a, texts, qs, cand, by_len={ln: slice}, want={k: model}, kinds)"""
    if symbols in _SWEEP:
        return _SWEEP[symbols]
    rng = np.random.default_rng(13050 + len(_SWEEP))
    a = alph.ascii_dna() if symbols == b"ACGT" else alph.Alphabet.from_io_symbols(symbols)

    def rand(n):
        return bytes(symbols[i] for i in rng.integers(0, 4, n))

    # text 0 sits behind the pad units; text 1 directly behind text 0; an empty text and a text of one symbol; the last text
    texts = [rand(401), rand(397), b"", symbols[2:3], rand(333)]
    base = {0: 0, 1: 402, 4: 402 + 398 + 1 + 2}                    # where a text begins in the concatenation (sentinels counted)
    qs, cq, cb, hits, kinds, by_len, seams = [], [], [], [], [], {}, set()
    for ln in _LENGTHS:
        first = len(qs)
        for text_id in (0, 1, 4):
            t = texts[text_id]
            noise = rand(1200)                                     # what a read holds where it hangs over an end of its text
            src = lambda p: t[p] if 0 <= p < len(t) else noise[p + 400]  # noqa: E731
            starts = list(range(40, 72)) + [-3, 0, len(t) - ln, len(t) - ln + 2]
            for n, start in enumerate(starts):
                kind = n % 4 if ln > 8 else 0
                if (n // 4) % 2 == 0:                              # the block seam, where the length allows
                    rows = [r for r in (62, 63, 64, 65) if 1 <= r < ln - 2]
                    row = rows[(n // 8) % len(rows)] if rows else ln // 2
                else:                                              # the unit seam: the edited symbol's text position
                    rows = [r for r in range(2, max(ln - 2, 3)) if (base[text_id] + start + r) % 32 in (31, 0, 1)]
                    row = rows[(n // 8) % len(rows)] if rows else ln // 2
                    if rows and kind:
                        seams.add((base[text_id] + start + row) % 32)
                if kind == 0:
                    q = bytes(src(start + j) for j in range(ln))
                elif kind == 1:                                    # an inserted symbol, the tail moves on by one
                    q = bytes(src(start + j) for j in range(row)) + rand(1) + bytes(src(start + j) for j in range(row, ln - 1))
                elif kind == 2:                                    # a skipped text symbol, the tail comes from one further on
                    q = bytes(src(start + j) for j in range(row)) + bytes(src(start + j + 1) for j in range(row, ln))
                else:                                              # another symbol
                    other = symbols[(symbols.index(src(start + row)) + 1 + int(rng.integers(0, 3))) % 4]
                    q = bytes(src(start + j) for j in range(row)) + bytes([other]) + bytes(src(start + j) for j in range(row + 1, ln))
                assert len(q) == ln
                b = max(-start, 0) + n % 3                         # (may exceed a short read's length)
                qs.append(q), cq.append(len(qs) - 1), cb.append(b), hits.append((text_id, start + b)), kinds.append(kind)
        by_len[ln] = slice(first, len(qs))
    assert seams == {31, 0, 1}
    _SWEEP[symbols] = dict(a=a, texts=texts, qs=qs, cand=(cq, cb, hits), by_len=by_len, kinds=np.array(kinds),
                           want={k: align_model(texts, a, qs, cq, cb, hits, k) for k in _SWEEP_LIMITS})
    return _SWEEP[symbols]


def _check_sweep_inputs(c):
    texts, qs, (cq, cb, hits) = c["texts"], c["qs"], c["cand"]
    lens = np.array([len(qs[i]) for i in cq])
    for k in _SWEEP_LIMITS:                             # the window's first column takes every phase of a text unit
        phases = set()
        for (t, p), b, ln in zip(hits, cb, lens):
            x0, x1 = min(max(p - b - k, 0), len(texts[t])), min(max(p - b + ln + k, 0), len(texts[t]))
            if x0 < x1:
                phases.add((sum(len(x) + 1 for x in texts[:t]) + x0) % 32)
        assert phases == set(range(32)), k
    # the inputs do what they are for: at limit 5 nearly every read aligns, the planted indel is found as one, reads hang over
    # both ends (a run of insertions first or last), and at limit 0 only the exact windows are left
    dist, begin, end, n_cigar, cigar = c["want"][5]
    assert replay_all(c["a"], texts, qs, cq, hits, c["want"][5]) >= len(cq) - 10
    strings = [sam(runs_of(n_cigar[i], cigar[i])) for i in range(len(cq))]
    for kind, letter in ((1, "I"), (2, "D"), (3, "X")):
        of_kind = np.flatnonzero(c["kinds"] == kind)
        assert sum(letter in strings[i] for i in of_kind) * 10 >= 9 * of_kind.size, kind
    assert sum(s[1:2] == "I" for s in strings) >= 24 and sum(s.endswith("I") for s in strings) >= 24   # of 36 reads each
    assert (c["want"][0][2] != NO_END).sum() > 100 and (c["want"][0][0] == 1).sum() > 500


def _slice_of(want, part):
    return tuple(x[part] for x in want)


def test_word_borders_and_unit_phases_in_both_layouts():
    from genedex_amd.device import DeviceEngine, DeviceQueries

    c = _sweep_case(b"ACGT")
    _check_sweep_inputs(c)
    texts, qs, (cq, cb, hits) = c["texts"], c["qs"], c["cand"]
    g = gpu_index(texts, c["a"])
    eng = DeviceEngine(g)
    assert eng.aux_info()["default_shape"]
    plain = DeviceQueries.from_host(*join(qs))
    for k in _SWEEP_LIMITS:                             # plain + offsets: align_kernel<1, false, 4>
        assert_equal(device_call(eng, plain, cq, cb, hits, k), c["want"][k], ("plain", k))
    for ln, part in c["by_len"].items():                # packed + uniform: align_kernel<2, true, 1..4>
        dq = DeviceQueries.from_host(*join(qs[part])).as_uniform(ln).as_packed(g)
        assert dq.packed and dq.uniform_len == ln
        local = [i - part.start for i in cq[part]]
        for k in _SWEEP_LIMITS:
            assert_equal(device_call(eng, dq, local, cb[part], hits[part], k), _slice_of(c["want"][k], part), ("packed + uniform", ln, k))
    # the two forms the sweep leaves out, on the reads of test_gpu_edit_distance's layouts test: plain + uniform of 1, 2, 3 and
    # 4 blocks (align_kernel<1, true, 1..4>) and packed + offsets (align_kernel<2, false, 4>)
    for ulen in (50, 70, 150, 256):
        a, texts, qs, (cq, cb, hits) = _layouts_case(ulen)
        g = gpu_index(texts, a)
        eng = DeviceEngine(g)
        plain = DeviceQueries.from_host(*join(qs))
        for k in (0, 3):
            want = align_model(texts, a, qs, cq, cb, hits, k)
            assert (want[2] != NO_END).sum() > 30 and (want[2] == NO_END).sum() > 30   # the input condition
            assert_equal(device_call(eng, plain.as_uniform(ulen), cq, cb, hits, k), want, ("uniform", ulen, k))
            assert_equal(device_call(eng, plain.as_packed(g), cq, cb, hits, k), want, ("packed", ulen, k))


def test_word_borders_and_unit_phases_with_the_alphabet_table_in_lds():
    """A, I, Q and Y agree in their low three bits, so the index has no v_perm tables and plain reads are translated through
    the alphabet table in LDS (align_kernel<0, ., .>)"""
    from genedex_amd.device import DeviceEngine, DeviceQueries

    c = _sweep_case(b"AIQY")
    _check_sweep_inputs(c)
    texts, qs, (cq, cb, hits) = c["texts"], c["qs"], c["cand"]
    g = gpu_index(texts, c["a"])
    eng = DeviceEngine(g)
    assert eng.aux_info()["text_units"]
    plain = DeviceQueries.from_host(*join(qs))
    for k in _SWEEP_LIMITS:                             # offsets: align_kernel<0, false, 4>
        assert_equal(device_call(eng, plain, cq, cb, hits, k), c["want"][k], ("plain", k))
    for ln, part in c["by_len"].items():                # uniform: align_kernel<0, true, 1..4>
        dq = DeviceQueries.from_host(*join(qs[part])).as_uniform(ln)
        local = [i - part.start for i in cq[part]]
        for k in (1, 33):
            assert_equal(device_call(eng, dq, local, cb[part], hits[part], k), _slice_of(c["want"][k], part), ("uniform", ln, k))


# ------------------------------------------------------------------------------------------------
# 4. slot reuse and workspace sizes

def test_slot_reuse_and_workspace_sizes():
    import torch

    from genedex_amd.device import DeviceEngine, DeviceQueries

    rng = np.random.default_rng(13060)
    a = alph.ascii_dna_with_n()
    texts = [bytes(b"ACGT"[i] for i in rng.integers(0, 4, n)) for n in (5000, 2500)]
    qs, cq, cb, hits, long_one = [], [], [], [], []
    m, k = 2000, 6
    for c in range(m):
        is_long = (c // 256 + c) % 2 == 0                           # so that c, c + 256 and c + 768 differ in kind
        ln = int(rng.integers(200, 257)) if is_long else int(rng.integers(1, 41))
        t = texts[c % 2]
        start = int(rng.integers(0, len(t) - ln - 8))
        q, where = planted_read(rng, t, start, ln, (c % 4) if ln > 14 else 0)
        b = int(rng.choice([j for j in range(ln) if where[j] >= 0]))
        qs.append(q), cq.append(c), cb.append(b), hits.append((c % 2, where[b])), long_one.append(is_long)
    long_one = np.array(long_one)
    for stride in (256, 768):                                       # every lane of a grid of 1 and of 3 blocks takes both kinds
        for lane in range(stride):
            assert 0 < long_one[lane::stride].sum() < long_one[lane::stride].size
    want = align_model(texts, a, qs, cq, cb, hits, k)
    assert (want[2] != NO_END).sum() * 10 >= 9 * m and (want[3] > 1).sum() * 3 >= m
    g = gpu_index(texts, a)
    eng = DeviceEngine(g)
    dq = DeviceQueries.from_host(*join(qs))
    least, best = eng.align_workspace_bytes(dq, m, k)
    assert least % (16 * 256) == 0 and best == 8 * least            # 2000 candidates: 8 blocks of 256 lanes
    results = [device_call(eng, dq, cq, cb, hits, k, workspace_bytes=size) for size in (least, 3 * least, best)]
    for got, size in zip(results, (least, 3 * least, best)):
        assert_equal(got, want, size)
    # the sizes are pure functions of m, the limit and the layout, and stop growing with m
    sizes = {m_: eng.align_workspace_bytes(dq, m_, k) for m_ in (1, 10 ** 6, 10 ** 8)}
    assert sizes[1] == (least, least) and sizes[10 ** 6] == sizes[10 ** 8] and sizes[10 ** 6][0] == least
    assert least < sizes[10 ** 6][1] <= 4 << 30
    uni = DeviceQueries(dq.qbuf, dq.qoff, dq.nq, dq.total_bytes, False, 150)   # (only its layout counts for the sizes)
    u_least, u_best = eng.align_workspace_bytes(uni, 10 ** 8, 8)
    assert u_least == 16 * 256 * ((150 + 16) * 3 + 5) and u_best == 1024 * u_least
    worst = eng.align_workspace_bytes(dq, 10 ** 8, 256)
    assert worst[0] == 16 * 256 * (768 * 4 + 129) and worst[1] <= 4 << 30 and worst[1] % worst[0] == 0
    # a workspace too small by one element, or not aligned: refused, nothing written
    lib = _lib.load()
    z = torch.full((4096,), GARBAGE, dtype=torch.int32, device="cuda")
    ws = torch.empty(least + 16, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    args = (g._h, p(dq.qbuf), p(dq.qoff), dq.nq, None, p(z), p(z), p(z), 1, k, p(z), p(z[8:]), p(z[16:]), p(z[24:]), p(z[32:]))
    assert ws.data_ptr() % 16 == 0
    assert lib.gdx_align_many_dev(*args, p(ws), least - 16, None, None) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert lib.gdx_align_many_dev(*args, C.c_void_p(ws.data_ptr() + 8), least, None, None) == _lib.GDX_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert (z.cpu().numpy().view(np.uint32) == GARBAGE).all()
    # the size query launches nothing and looks at no device pointer: every other pointer is null
    out = (C.c_uint64 * 2)(7, 7)
    assert lib.gdx_align_many_dev(g._h, None, None, dq.nq, None, None, None, None, m, k, None, None, None, None, None, None, 0, out,
                                  None) == _lib.GDX_OK
    assert (out[0], out[1]) == (least, best)
    assert lib.gdx_align_many_dev(g._h, None, None, dq.nq, None, None, None, None, m, k, None, None, None, None, None, None, 0, None,
                                  None) == _lib.GDX_OK


# ------------------------------------------------------------------------------------------------
# 5. every output is written, nothing else is

@pytest.mark.parametrize("k", (0, 3))
def test_every_output_is_written_and_nothing_else(k):
    from genedex_amd.device import DeviceEngine, DeviceQueries

    rng = np.random.default_rng(13070 + k)
    a = alph.ascii_dna_with_n()
    texts = [bytes(b"ACGT"[i] for i in rng.integers(0, 4, 1500))]
    qs, cq, cb, hits = [], [], [], []
    for c in range(300):                                            # 300: one full block of lanes and a part of one
        ln = int(rng.integers(20, 120))
        start = int(rng.integers(0, 1300))
        q, where = planted_read(rng, texts[0], start, ln, c % 3)
        qs.append(q), cq.append(c), cb.append(0), hits.append((0, start if c % 7 else start + 400))
    g = gpu_index(texts, a)
    eng = DeviceEngine(g)
    dq = DeviceQueries.from_host(*join(qs))
    for m in (0, 1, 300):
        want = align_model(texts, a, qs, cq[:m], cb[:m], hits[:m], k)
        got = device_call(eng, dq, cq[:m], cb[:m], hits[:m], k, raw=True)
        assert got[4].shape == (m, 2 * k + 1)                       # (stride 1 at limit 0)
        for name, x in zip(NAMES[:4], got):
            assert not (x == GARBAGE).any(), (m, name)
        below = np.arange(2 * k + 1)[None, :] < got[3][:, None]
        assert (got[4][~below] == GARBAGE).all() and not (got[4][below] == GARBAGE).any(), m
        assert_equal(got[:4] + (np.where(below, got[4], 0).astype(np.uint32),), want, (m, k))
        if m == 300:
            assert (want[3] > 0).sum() > 60 and (want[3] == 0).sum() > 30 and (k == 0 or (want[3] > 2).any())
        host = host_call(g, qs, cq[:m], cb[:m], hits[:m], k)
        assert_equal(host, want, ("host", m, k))


# ------------------------------------------------------------------------------------------------
# 6. end to end: SMEMs -> cursor locate -> candidates -> alignments

def test_smems_locate_align_end_to_end():
    rng = np.random.default_rng(13080)
    a = alph.ascii_dna()
    texts = [bytes(b"ACGT"[i] for i in rng.integers(0, 4, n)) for n in (3000, 1700, 600)]
    qs, origin = [], []
    for i in range(150):
        t = texts[i % 3]
        ln = int(rng.integers(60, 140))
        start = int(rng.integers(0, len(t) - ln - 4))
        q, where = planted_read(rng, t, start, ln, 1 + i % 3)
        qs.append(q)
        origin.append((i % 3, start))
    ms, ml, k = 16, 12, 3
    # the input condition, on the models and the oracle alone
    F, R = oracle_pair(texts, a)
    n_smems, remaining, begin, length, start_, end_, status = model_arrays(F, R, qs, ms, ml)
    assert not status.any() and not remaining.any()
    off, t_ids, pos = F.locate_intervals(start_, end_)
    cq, cb = expand_candidates(n_smems, begin, off, ms)
    hits = np.stack([t_ids, pos], axis=1)
    want = align_model(texts, a, qs, cq, cb, hits, k)

    def origins_found(result):
        found = set()
        for c in np.flatnonzero(result[2] != NO_END):
            if (int(hits[c][0]), int(result[1][c])) == origin[int(cq[c])]:
                found.add(int(cq[c]))
        return found

    assert origins_found(want) == set(range(len(qs)))                           # every read's true origin is among the begins
    assert sum("I" in sam(runs_of(n, row)) or "D" in sam(runs_of(n, row)) for n, row in zip(want[3], want[4])) >= 30
    # the same chain on the GPU
    g, r = gpu_index(texts, a), gpu_index(reversed_texts(texts), a)
    qbuf, qoff = pack_queries(qs)
    g_n, _, g_begin, _, g_start, g_end, _ = g.smems_raw(r, qbuf, qoff, ms, ml)
    g_off, g_t, g_p = g.locate_intervals_raw(g_start, g_end)
    g_cq, g_cb = expand_candidates(g_n, g_begin, g_off, ms)
    assert np.array_equal(g_cq, cq) and np.array_equal(g_cb, cb) and np.array_equal(g_t, t_ids) and np.array_equal(g_p, pos)
    got = g.align_raw(qbuf, qoff, g_cq, g_cb, g_t, g_p, k)
    assert replay_all(a, texts, qs, g_cq, hits, got) == int((got[2] != NO_END).sum()) > 0   # against the host copy of the texts
    assert origins_found(got) == set(range(len(qs)))
    assert_equal(got, want, "raw")
    many = g.align_many(qs, g_cq, g_cb, list(zip(g_t.tolist(), g_p.tolist())), k)
    assert len(many) == len(cq)
    for c, al in enumerate(many):
        if want[2][c] == NO_END:
            assert al == (int(want[0][c]), None, None, None)
        else:
            assert al == (int(want[0][c]), int(want[1][c]), int(want[2][c]), sam(runs_of(want[3][c], want[4][c])))


# ------------------------------------------------------------------------------------------------
# 7. the contract

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
    assert all(x.shape[0] == 0 for x in g.align_raw(qbuf, qoff, none, none, none, none, 3))
    got = g.align_raw(np.zeros(8, dtype=np.uint8), np.zeros(1, dtype=np.uint64), [0, 1], [0, 0], [0, 1], [0, 0], 3)
    assert got[0].tolist() == [INVALID] * 2 and got[1].tolist() == [NO_END] * 2 and got[2].tolist() == [NO_END] * 2
    assert got[3].tolist() == [0, 0] and not got[4].any()
    dq = DeviceQueries.from_host(qbuf, qoff)
    empty = DeviceQueries.from_host(np.zeros(8, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    assert all(x.shape[0] == 0 for x in device_call(eng, dq, [], [], [], 3))
    got = device_call(eng, empty, [0, 1], [0, 0], [(0, 0), (1, 0)], 3)
    assert got[0].tolist() == [INVALID] * 2 and got[1].tolist() == [NO_END] * 2 and got[2].tolist() == [NO_END] * 2 and got[3].tolist() == [0, 0]
    # the definition's corners, in both forms (the candidates of the edit-distance contract test)
    cq = [0, 1, 1, 0, 2, 2, 0, 3, 4, 0]
    cb = [0, 0, 1, 4, 0, 5, 0, 0, 0, 0]
    hits = [(0, 0), (1, 0), (1, 1), (0, 8), (0, 7), (1, 0), (2, 0), (0, 0), (0, 0), (0, 4)]
    for k in (0, 3, 8, 256):
        want = align_model(texts, a, qs, cq, cb, hits, k)
        if k == 3:
            assert want[0].tolist() == [0, 1, 1, 1, 0, 0, 4, TOO_LONG, 4, 1]
            assert want[1].tolist() == [0, 0, 0, 1, 4, 0, NO_END, NO_END, NO_END, 1]
            assert want[2].tolist() == [8, 2, 2, 8, 4, 0, NO_END, NO_END, NO_END, 8]
            assert [sam(runs_of(n, row)) for n, row in zip(want[3], want[4])] == ["8=", "2=1I", "2=1I", "1I7=", "", "", "", "", "", "1I7="]
        assert_equal(host_call(g, qs, cq, cb, hits, k), want, ("host", k))
        assert_equal(device_call(eng, dq, cq, cb, hits, k), want, ("device", k))
    # a query or a text id out of range: the device form writes the markers, the host form refuses, also a position >= 2^32
    cq2, hits2 = [0, 5, 1, 0xFFFFFFFF], [(0, 0), (0, 0), (3, 0), (0xFFFFFFFF, 0)]
    got = device_call(eng, dq, cq2, [0, 0, 0, 0], hits2, 3)
    assert got[0].tolist() == [0, INVALID, INVALID, INVALID] and got[2].tolist() == [8, NO_END, NO_END, NO_END]
    assert got[1].tolist() == [0, NO_END, NO_END, NO_END] and got[3].tolist() == [1, 0, 0, 0]
    assert status_of(lambda: host_call(g, qs, [0, 5], [0, 0], [(0, 0), (0, 0)], 3)) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert status_of(lambda: host_call(g, qs, [0, 1], [0, 0], [(0, 0), (3, 0)], 3)) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert status_of(lambda: host_call(g, qs, [0, 1], [0, 0], [(0, 0), (1, 1 << 32)], 3)) == _lib.GDX_ERR_INVALID_ARGUMENT
    # max_edits: 256 is the largest, in both forms
    assert status_of(lambda: host_call(g, qs, cq, cb, hits, 257)) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert status_of(lambda: device_call(eng, dq, cq, cb, hits, 257)) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert status_of(lambda: eng.align_workspace_bytes(dq, 10, 257)) == _lib.GDX_ERR_INVALID_ARGUMENT
    # a null output, in both forms; a refused call writes nothing
    lib = _lib.load()
    z = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    least, best = eng.align_workspace_bytes(dq, 1, 3)
    ws = torch.empty(best, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    outs = [p(z), p(z[8:]), p(z[16:]), p(z[24:]), p(z[32:])]
    head = (g._h, p(dq.qbuf), p(dq.qoff), dq.nq, None, p(z), p(z), p(z), 1)
    for missing in range(5):
        o = list(outs)
        o[missing] = None
        assert lib.gdx_align_many_dev(*head, 3, *o, p(ws), best, None, None) == _lib.GDX_ERR_INVALID_ARGUMENT, missing
    h_out = [np.full(8, 7, dtype=np.uint32) for _ in range(5)]
    hit = (_lib.HitStruct * 1)()
    u32 = lambda x: x.ctypes.data_as(_lib.u32p)  # noqa: E731
    h_head = (g._h, qbuf.ctypes.data_as(_lib.u8p), qoff.ctypes.data_as(_lib.u64p), len(qs), u32(np.zeros(1, dtype=np.uint32)),
              u32(np.zeros(1, dtype=np.uint32)), hit, 1, 3)
    for missing in range(5):
        o = [u32(x) for x in h_out]
        o[missing] = None
        assert lib.gdx_align_many(*h_head, *o) == _lib.GDX_ERR_INVALID_ARGUMENT, missing
    assert all((x == 7).all() for x in h_out)
    assert lib.gdx_align_many_dev(*head, 257, *outs, p(ws), best, None, None) == _lib.GDX_ERR_INVALID_ARGUMENT
    # an unknown layout
    lay = _lib.QueryLayout()
    lib.gdx_query_layout_init(C.byref(lay))
    lay.packed = 2
    assert lib.gdx_align_many_dev(g._h, p(dq.qbuf), p(dq.qoff), dq.nq, C.byref(lay), p(z), p(z), p(z), 1, 3, *outs, p(ws), best, None,
                                  None) == _lib.GDX_ERR_INVALID_ARGUMENT
    # an index without text units, the packed form on an index that takes no packed queries, the 64-bit engine
    bare = gpu_index(texts, a, text_units=False, seed_symbols=0, full_suffix_array=False, inverse_suffix_array=False)
    assert not DeviceEngine(bare).aux_info()["text_units"]
    assert status_of(lambda: host_call(bare, qs, cq, cb, hits, 3)) == _lib.GDX_ERR_UNSUPPORTED
    assert status_of(lambda: device_call(DeviceEngine(bare), dq, cq, cb, hits, 3)) == _lib.GDX_ERR_UNSUPPORTED
    three = gpu_index([b"ACGACGGACA"], alph.Alphabet.from_io_symbols(b"ACG"), text_units=True)   # dense symbol 4 does not exist
    got = device_call(DeviceEngine(three), DeviceQueries.from_host(*pack_queries([b"GACGT"])), [0], [0], [(0, 2)], 9)
    assert (got[0].tolist(), got[1].tolist(), got[2].tolist(), sam(runs_of(got[3][0], got[4][0]))) == ([1], [2], [6], "4=1I")
    packed = DeviceQueries(dq.qbuf, dq.qoff, dq.nq, dq.total_bytes, True, 0)
    assert status_of(lambda: device_call(DeviceEngine(three), packed, [0], [0], [(0, 0)], 3)) == _lib.GDX_ERR_UNSUPPORTED
    lib.gdx_debug_force_wide(1)
    try:
        w = FmIndexConfig("i64").suffix_array_sampling_rate(4).construct_index(texts, a)
    finally:
        lib.gdx_debug_force_wide(0)
    assert w.info.index_width == 64
    assert status_of(lambda: host_call(w, qs, cq, cb, hits, 3)) == _lib.GDX_ERR_UNSUPPORTED
    assert lib.gdx_align_many_dev(w._h, p(dq.qbuf), p(dq.qoff), dq.nq, None, p(z), p(z), p(z), 1, 3, *outs, p(ws), best, None,
                                  None) == _lib.GDX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert z.cpu().tolist() == [7] * 64             # (nothing was written by any of the refused calls)


def test_candidates_on_the_rows_of_a_both_strand_batch():
    """rows made by with_strands go straight in: row 2 i the read as given, row 2 i + 1 its reverse complement"""
    from genedex_amd.device import DeviceEngine, DeviceQueries

    rng = np.random.default_rng(13090)
    a = alph.ascii_dna_with_n()
    texts = [bytes(b"ACGT"[i] for i in rng.integers(0, 4, n)) for n in (1500, 800)]
    qs, origin = [], []
    for i in range(200):
        text_id, ln = i % 2, 50
        start = int(rng.integers(0, len(texts[text_id]) - ln - 4))
        q, where = planted_read(rng, texts[text_id], start, ln, i % 3)
        qs.append(bytes(q) if i % 4 < 2 else alph.reverse_complement(bytes(q)))   # half of them come from the reverse strand
        origin.append((text_id, start))
    _, both = host_batches(qs)
    cq, cb, hits = [], [], []
    for row in range(2 * len(qs)):
        b = int(rng.integers(0, 6))                 # (in front of every edit: on the diagonal of the read's start)
        cq.append(row), cb.append(b), hits.append((origin[row // 2][0], origin[row // 2][1] + b))
    want = align_model(texts, a, both, cq, cb, hits, 3)
    assert (want[2] != NO_END).sum() == len(qs)                                   # each read fits on exactly one strand
    assert replay_all(a, texts, both, cq, hits, want) == len(qs)
    g = gpu_index(texts, a)
    eng = DeviceEngine(g)
    plain = DeviceQueries.from_host(*join(qs))
    assert_equal(device_call(eng, plain.with_strands(g, "both"), cq, cb, hits, 3), want, "plain")
    assert_equal(device_call(eng, plain.as_uniform(50).with_strands(g, "both"), cq, cb, hits, 3), want, "uniform")
    dq = plain.as_uniform(50).as_packed(g).with_strands(g, "both")
    assert dq.packed and dq.nq == 2 * len(qs)
    assert_equal(device_call(eng, dq, cq, cb, hits, 3), want, "packed + uniform")
