"""Both strands on the device: gdx_strands_expand_dev against the numpy model of tests/test_strands_model.py (bit for bit over
the whole output buffer), the calls downstream on the expanded batch against the same calls on a host-made batch and
against the oracle, the two host calls and the Python layer."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_parity as parity
from genedex_amd import GdxError, _lib, reversed_texts
from genedex_amd import alphabet as alph
from test_gpu_parity import _VARIANTS, cpu_index, gpu_index
from test_strands_model import BOTH, REVERSE, expand_model, host_batches, join, out_bytes, pack_codes, packed_bytes, random_reads

pytestmark = pytest.mark.gpu

_CACHE = {}


def small_index(name="ascii_dna_with_n"):
    """one small index per alphabet for the expand tests (the call only looks at the handle's alphabet and table layout)"""
    if name not in _CACHE:
        rng = np.random.default_rng(5)
        symbols = b"ACDEFGHIKL" if name == "ascii_amino_acid" else b"ACGT"
        _CACHE[name] = gpu_index([bytes(symbols[k] for k in rng.integers(0, len(symbols), 3000))], getattr(alph, name)())
    return _CACHE[name]


def expand(ix, buf, off, nq, mode, packed=False, ulen=0, complement=None, layout=True):
    """gdx_strands_expand_dev on a host-made input -> (the whole output buffer, the output offsets or None), as numpy"""
    import torch

    lib = _lib.load()
    total = nq * ulen if ulen else (int(off[nq]) if nq else 0)
    d_in = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.uint64).view(np.int64)).cuda() if off is not None else None
    d_out = torch.full((out_bytes(total, packed, mode),), 0xAB, dtype=torch.uint8, device="cuda")  # every byte must be written
    writes_off = mode == BOTH and not ulen
    d_out_off = torch.full((2 * nq + 1,), -1, dtype=torch.int64, device="cuda") if writes_off else None
    lay = _lib.QueryLayout()
    lib.gdx_query_layout_init(C.byref(lay))
    lay.packed, lay.uniform_len = int(packed), int(ulen)
    comp = None if complement is None else np.ascontiguousarray(complement, dtype=np.uint8).ctypes.data_as(_lib.u8p)
    st = lib.gdx_strands_expand_dev(ix._h, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_off.data_ptr()) if d_off is not None and not ulen else None,
                                    nq, C.byref(lay) if (layout or packed or ulen) else None, total, comp, mode, C.c_void_p(d_out.data_ptr()),
                                    C.c_void_p(d_out_off.data_ptr()) if writes_off else None,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(st)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), (d_out_off.cpu().numpy().view(np.uint64) if writes_off else None)


def packed_input(buf, total, dense):
    return pack_codes(dense[buf[:total]] - 1, packed_bytes(total))


def check_expand(ix, qs, ulen=0, plain_only=False, complement=None, view_from=0):
    """both modes, plain and packed, against the model"""
    buf, off = join(qs)
    nq = len(qs) - view_from
    off = off[view_from:]
    total = int(off[-1])
    dense = ix.alphabet().io_to_dense_table
    for packed in ((False,) if plain_only else (False, True)):
        src = packed_input(buf, total, dense) if packed else buf
        for mode in (REVERSE, BOTH):
            want, want_off = expand_model(src, off, nq, mode, packed=packed, uniform_len=ulen, complement=complement)
            got, got_off = expand(ix, src, off, nq, mode, packed=packed, ulen=ulen, complement=complement)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (packed, mode, ulen, nq, int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
            assert (got_off is None) == (want_off is None)
            if want_off is not None:
                assert np.array_equal(got_off, want_off), (packed, mode, nq)


# ------------------------------------------------------------------------------------------------
# 1. the expand against the model

@pytest.mark.parametrize("ulen", (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 49, 50, 51, 64, 65))
def test_uniform_batches(ulen):
    ix = small_index()
    rng = np.random.default_rng(ulen)
    for nq in (1, 2, 33, 257):
        qs = random_reads(rng, nq, ulen, ulen)
        check_expand(ix, qs, ulen=ulen)   # as a uniform batch
        check_expand(ix, qs)              # the same reads with offsets


@pytest.mark.parametrize("seed", range(3))
def test_mixed_lengths(seed):
    ix = small_index()
    rng = np.random.default_rng(100 + seed)
    qs = random_reads(rng, 300, 0, 70)
    qs[10:40] = random_reads(rng, 30, 0, 3)      # runs of reads shorter than 4 symbols, empty ones among them
    qs[50:60] = [b""] * 10
    qs[-1] = random_reads(rng, 1, 13 + seed, 13 + seed)[0]  # the batch ends inside a word
    assert any(len(q) == 0 for q in qs) and sum(map(len, qs)) % 8 != 0
    check_expand(ix, qs)
    check_expand(ix, [b"", b""] + qs[:5] + [b""])


def test_no_queries_a_view_and_one_long_query():
    ix = small_index()
    rng = np.random.default_rng(3)
    for packed in (False, True):
        for mode in (REVERSE, BOTH):
            got, got_off = expand(ix, np.zeros(16, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 0, mode, packed=packed)
            assert got.size == out_bytes(0, packed, mode) and not got.any()
            assert got_off is None or got_off.tolist() == [0]
            got, _ = expand(ix, np.zeros(16, dtype=np.uint8), None, 0, mode, packed=packed, ulen=50)
            assert not got.any()
    qs = random_reads(rng, 40, 0, 45)
    for first in (3, 17):
        assert sum(map(len, qs[:first])) > 0
        check_expand(ix, qs, view_from=first)    # qoff[0] > 0
    check_expand(ix, random_reads(rng, 1, 5000, 5000))
    check_expand(ix, random_reads(rng, 1, 5000, 5000), ulen=5000)


def test_plain_batches_with_every_kind_of_byte_and_a_custom_table():
    ix = small_index()
    rng = np.random.default_rng(4)
    qs = random_reads(rng, 120, 0, 40, b"ACGTNacgtnRYKMBVDHSWrykmbvdhsw") + [bytes(rng.integers(0, 256, 37, dtype=np.uint8)) for _ in range(20)]
    check_expand(ix, qs, plain_only=True)
    check_expand(ix, [q[:9].ljust(9, b"#") for q in qs], ulen=9, plain_only=True)
    # a table that is not the stock one: A <-> C and G <-> T (keeps validity; not what packed batches could use)
    swap = np.arange(256, dtype=np.uint8)
    for a, b in (b"AC", b"CA", b"GT", b"TG", b"ac", b"ca", b"gt", b"tg"):
        swap[a] = b
    check_expand(ix, qs, plain_only=True, complement=swap)
    buf, off = join([b"AACG"])
    got, _ = expand(ix, buf, off, 1, REVERSE, complement=swap)
    assert bytes(got[:4]) == b"TACC"
    got, _ = expand(ix, buf, off, 1, REVERSE)
    assert bytes(got[:4]) == b"CGTT"
    got, _ = expand(ix, buf, off, 1, REVERSE, layout=False)   # layout == NULL: the plain form
    assert bytes(got[:4]) == b"CGTT"


def test_argument_errors():
    ix = small_index()
    buf, off = join([b"ACGT", b"GGA"])

    def status_of(fn):
        with pytest.raises(GdxError) as e:
            fn()
        return e.value.status

    for mode in (0, 3):
        assert status_of(lambda: expand(ix, buf, off, 2, mode)) == _lib.GDX_ERR_INVALID_ARGUMENT
    amino = small_index("ascii_amino_acid")
    assert status_of(lambda: expand(amino, buf, off, 2, BOTH)) == _lib.GDX_ERR_INVALID_ARGUMENT   # V is valid, B is not
    assert status_of(lambda: expand(amino, buf, off, 2, BOTH, packed=True)) == _lib.GDX_ERR_UNSUPPORTED  # takes no packed queries
    swap = np.arange(256, dtype=np.uint8)
    for a, b in (b"AC", b"CA", b"GT", b"TG", b"ac", b"ca", b"gt", b"tg"):
        swap[a] = b
    packed = packed_input(buf, 7, ix.alphabet().io_to_dense_table)
    assert status_of(lambda: expand(ix, packed, off, 2, BOTH, packed=True, complement=swap)) == _lib.GDX_ERR_INVALID_ARGUMENT
    expand(ix, buf, off, 2, BOTH, complement=swap)   # fine in the plain form
    drop = alph.dna_complement_table()
    drop[ord("A")] = ord("#")                        # a valid byte whose complement is not
    assert status_of(lambda: expand(ix, buf, off, 2, REVERSE, complement=drop)) == _lib.GDX_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------
# 2. end to end: the calls downstream on the expanded batch

@pytest.fixture(params=["default", "pair", "quad", "ref-flat64"])  # default shape, no seed table, rank lines only, a reference layout
def variant(request):
    query, build = _VARIANTS[request.param]
    parity._QUERY_OPTIONS.clear()
    parity._QUERY_OPTIONS.update(query)
    parity._BUILD_OPTIONS.clear()
    parity._BUILD_OPTIONS.update(build)
    yield request.param
    parity._QUERY_OPTIONS.clear()
    parity._BUILD_OPTIONS.clear()


_READS = {}


def reads_of_both_strands(name):
    """(texts, 400 reads, the indices of the reads sampled from the reverse complement, those with an invalid byte)"""
    if name in _READS:
        return _READS[name]
    rng = np.random.default_rng(11)
    dense = getattr(alph, name)().io_to_dense_table

    def text(n):
        codes = rng.integers(0, 4, n)
        if name == "ascii_dna_with_n":
            codes[rng.random(n) < 0.01] = 4
        return bytes(b"ACGTN"[k] for k in codes)

    texts = [text(n) for n in (1800, 1200, 700)]
    qs, from_reverse = [], []
    for i in range(400):
        t = texts[int(rng.integers(0, len(texts)))]
        ln = int(rng.integers(12, 60))
        p = int(rng.integers(0, len(t) - ln))
        q = bytearray(t[p:p + ln] if i % 2 == 0 else alph.reverse_complement(t[p:p + ln]))
        changed = False
        if i % 40 == 6 or i % 40 == 7:        # one substituted base
            k = int(rng.integers(0, ln))
            q[k] = b"ACGT"[(b"ACGT".find(bytes([q[k]])) + 1) % 4]
            changed = True
        if i % 50 in (8, 9):
            q[int(rng.integers(0, ln))] = ord("N")
            changed = True
        if i % 50 in (10, 11):
            q[int(rng.integers(0, ln))] = ord("#")
            changed = True
        if i == 399:                          # an invalid byte that the walk reaches on both strands: two symbols from the read's start
            q = bytearray(texts[0][100:130])
            q[2] = ord("#")
            changed = True
        if i % 2 and not changed:
            from_reverse.append(i)
        qs.append(bytes(q))
    invalid = [i for i, q in enumerate(qs) if (dense[np.frombuffer(q, dtype=np.uint8)] == 0).any()]
    _READS[name] = texts, qs, from_reverse, invalid
    return _READS[name]


def one_call_step(eng, dq):
    """counts, status, hit offsets, hits of gdx_locate_many_step_compact_layout_dev on a device batch"""
    import torch

    nq = dq.nq
    rec, cw = eng.alloc_records(nq), eng.alloc_compact(nq)
    off = torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda")
    cap = 64 * nq + 4096
    hits = torch.full((cap, 2), -1, dtype=torch.int32, device="cuda")
    totals = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    sws = torch.empty(max(eng.totals_workspace_bytes(nq), 16), dtype=torch.uint8, device="cuda")
    ws = torch.empty(max(eng.locate_workspace_bytes(cap), 16), dtype=torch.uint8, device="cuda")
    eng.locate_step(dq, rec, cw, sws, totals, off, hits, ws)
    counts = torch.empty(nq, dtype=torch.int32, device="cuda")
    status = torch.empty(nq, dtype=torch.uint8, device="cuda")
    eng.unpack_records(rec, nq, counts, status, compact=cw)
    torch.cuda.synchronize()
    tot = int(totals[0].item())
    assert tot <= cap
    h = hits[:tot].cpu().numpy().astype(np.uint32)
    return counts.cpu().numpy().astype(np.uint32), status.cpu().numpy(), off.cpu().numpy().astype(np.uint64), h[:, 0], h[:, 1]


@pytest.mark.parametrize("name", ("ascii_dna", "ascii_dna_with_n"))
def test_search_and_locate_on_the_expanded_batch(name, variant):
    import torch

    from genedex_amd.device import DeviceEngine, DeviceQueries

    a = getattr(alph, name)()
    texts, qs, from_reverse, invalid = reads_of_both_strands(name)
    g, cpu = gpu_index(texts, a), cpu_index(texts, a)
    eng = DeviceEngine(g)
    rc, both = host_batches(qs)
    qbuf, qoff = join(qs)
    hbuf, hoff = join(both)
    # the existing calls on the host-made interleaved batch, and the oracle
    ws, we, wst = g.cursors_raw(hbuf, hoff, strict=False)
    wcnt, wst2 = g.count_raw(hbuf, hoff, strict=False)
    woff, wt, wp, _ = g.locate_raw(hbuf, hoff, strict=False)
    os_, oe, ost = cpu.cursors_single(hbuf, hoff)
    assert np.array_equal(ws, os_) and np.array_equal(we, oe) and np.array_equal(wst, ost)
    ooff, ot, op = cpu.locate_intervals(os_, oe)
    assert np.array_equal(woff, ooff) and np.array_equal(wt, ot) and np.array_equal(wp, op)
    # the expanded batch
    dq = DeviceQueries.from_host(qbuf, qoff).with_strands(g, "both")
    assert dq.nq == 2 * len(qs)
    out = eng.alloc_outputs(dq.nq)
    eng.search(dq, out)
    counts = torch.empty(dq.nq, dtype=torch.int32, device="cuda")
    cstatus = torch.empty(dq.nq, dtype=torch.uint8, device="cuda")
    eng.count(dq, counts, cstatus)
    torch.cuda.synchronize()
    assert np.array_equal(out["start"].cpu().numpy().astype(np.uint32), os_) and np.array_equal(out["end"].cpu().numpy().astype(np.uint32), oe)
    assert np.array_equal(out["status"].cpu().numpy(), ost)
    assert np.array_equal(counts.cpu().numpy().astype(np.uint32), wcnt) and np.array_equal(cstatus.cpu().numpy(), wst2)
    scnt, sst, soff, st_, sp = one_call_step(eng, dq)
    assert np.array_equal(scnt, wcnt) and np.array_equal(sst, wst2)
    assert np.array_equal(soff, ooff) and np.array_equal(st_, ot) and np.array_equal(sp, op)
    # a read sampled from the reverse strand is found there
    assert len(from_reverse) > 150
    for i in from_reverse:
        assert scnt[2 * i + 1] >= 1, i
    # an invalid byte: the status of each row is the oracle's for that row (the walk reaches it, or stops before it, on
    # either strand), and a read whose rows both report it exists
    assert 399 in invalid and sst[2 * 399] == _lib.GDX_Q_INVALID_SYMBOL and sst[2 * 399 + 1] == _lib.GDX_Q_INVALID_SYMBOL
    clean = np.ones(len(qs), dtype=bool)
    clean[invalid] = False
    assert not sst.reshape(-1, 2)[clean].any()
    # the reverse batch alone
    dr = DeviceQueries.from_host(qbuf, qoff).with_strands(g, "reverse")
    out = eng.alloc_outputs(dr.nq)
    eng.search(dr, out)
    torch.cuda.synchronize()
    assert np.array_equal(out["start"].cpu().numpy().astype(np.uint32), os_[1::2]) and np.array_equal(out["end"].cpu().numpy().astype(np.uint32), oe[1::2])


def test_the_packed_uniform_form_end_to_end():
    from genedex_amd.device import DeviceEngine, DeviceQueries

    a = alph.ascii_dna()
    texts, _, _, _ = reads_of_both_strands("ascii_dna")
    rng = np.random.default_rng(21)
    qs = []
    for i in range(300):
        t = texts[i % 3]
        p = int(rng.integers(0, len(t) - 50))
        qs.append(t[p:p + 50] if i % 2 == 0 else alph.reverse_complement(t[p:p + 50]))
    g, cpu = gpu_index(texts, a), cpu_index(texts, a)
    eng = DeviceEngine(g)
    _, both = host_batches(qs)
    hbuf, hoff = join(both)
    os_, oe, _ = cpu.cursors_single(hbuf, hoff)
    ooff, ot, op = cpu.locate_intervals(os_, oe)
    dq = DeviceQueries.from_host(*join(qs)).as_uniform(50).as_packed(g).with_strands(g, "both")
    assert dq.packed and dq.uniform_len == 50 and dq.nq == 600
    scnt, sst, soff, st_, sp = one_call_step(eng, dq)
    assert not sst.any() and np.array_equal(scnt, (oe - os_).astype(np.uint32))
    assert np.array_equal(soff, ooff) and np.array_equal(st_, ot) and np.array_equal(sp, op)
    assert (scnt.reshape(-1, 2)[np.arange(300) % 2 == 0, 0] >= 1).all() and (scnt.reshape(-1, 2)[np.arange(300) % 2 == 1, 1] >= 1).all()


def test_suffix_segments_and_smems_on_the_expanded_batch():
    import torch

    from genedex_amd.device import DeviceEngine, DeviceQueries

    a = alph.ascii_dna_with_n()
    texts, qs, _, _ = reads_of_both_strands("ascii_dna_with_n")
    g, r = gpu_index(texts, a), gpu_index(reversed_texts(texts), a)
    eng = DeviceEngine(g)
    _, both = host_batches(qs)
    host = DeviceQueries.from_host(*join(both))
    dev = DeviceQueries.from_host(*join(qs)).with_strands(g, "both")
    assert torch.equal(dev.qoff, host.qoff)
    a_out, b_out = eng.alloc_segments(host.nq, 4), eng.alloc_segments(host.nq, 4)
    eng.suffix_segments(host, 4, a_out)
    eng.suffix_segments(dev, 4, b_out)
    torch.cuda.synchronize()
    for k in a_out:
        assert torch.equal(a_out[k], b_out[k]), k
    assert int(a_out["n_segments"].sum().item()) > host.nq // 2
    a_out, b_out = eng.alloc_smems(host.nq, 4), eng.alloc_smems(host.nq, 4)
    eng.smems(host, r, 4, 8, a_out)
    eng.smems(dev, r, 4, 8, b_out)
    torch.cuda.synchronize()
    for k in a_out:
        assert torch.equal(a_out[k], b_out[k]), k
    assert int(a_out["n_smems"].sum().item()) > host.nq // 2


# ------------------------------------------------------------------------------------------------
# 3. the host calls and the Python layer

def test_the_host_calls_equal_the_plain_calls_on_the_interleaved_batch():
    a = alph.ascii_dna_with_n()
    texts, qs, _, invalid = reads_of_both_strands("ascii_dna_with_n")
    g = gpu_index(texts, a)
    qs = qs + [b"A", b"", b"ACGT" * 3]
    _, both = host_batches(qs)
    qbuf, qoff = join(qs)
    hbuf, hoff = join(both)
    wcnt, wst = g.count_raw(hbuf, hoff, strict=False)
    assert wst.any()
    with pytest.raises(GdxError) as e:                      # GDX_ERR_QUERY_STATUS, the other rows valid
        g.count_strands_raw(qbuf, qoff)
    assert e.value.status == _lib.GDX_ERR_QUERY_STATUS
    cnt, st = g.count_strands_raw(qbuf, qoff, strict=False)
    assert np.array_equal(cnt, wcnt) and np.array_equal(st, wst)
    woff, wt, wp, _ = g.locate_raw(hbuf, hoff, strict=False)
    off, t, p, st = g.locate_strands_raw(qbuf, qoff, strict=False)
    assert np.array_equal(off, woff) and np.array_equal(t, wt) and np.array_equal(p, wp) and np.array_equal(st, wst)
    g.set_query_options(max_hits_per_query=1)
    try:
        woff, wt, wp, _ = g.locate_raw(hbuf, hoff, strict=False)
        off, t, p, _ = g.locate_strands_raw(qbuf, qoff, strict=False)
        assert int(np.diff(woff).max()) == 1 and int(wcnt.max()) > 1
        assert np.array_equal(off, woff) and np.array_equal(t, wt) and np.array_equal(p, wp)
    finally:
        g.set_query_options(max_hits_per_query=0)
    # nq == 0
    cnt, st = g.count_strands_raw(np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    assert cnt.size == 0 and st.size == 0
    off, t, p, st = g.locate_strands_raw(np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    assert off.tolist() == [0] and t.size == 0
    # a table the index cannot take
    bad = alph.dna_complement_table()
    bad[ord("A")] = ord("#")
    with pytest.raises(GdxError) as e:
        g.count_strands_raw(qbuf, qoff, complement=bad)
    assert e.value.status == _lib.GDX_ERR_INVALID_ARGUMENT


def test_the_python_layer():
    a = alph.ascii_dna()
    texts = [b"ACGTTGCAAGGCTTAACCGGATAT", b"GGGGACGTTGCAAAAA"]
    g = gpu_index(texts, a)
    qs = [b"ACGTTGCA", b"TGCAACGT", b"CCCC", b"TTTTT", b"ATAT"]
    _, both = host_batches(qs)
    counts = g.count_many_strands(qs)
    assert counts.shape == (5, 2) and np.array_equal(counts.reshape(-1), g.count_many(both))
    assert counts[0, 0] == 2 and counts[3].tolist() == [0, 1]
    pairs = g.locate_many_strands(qs)
    flat = g.locate_many(both)
    assert [list(p[0]) for p in pairs] == flat[0::2] and [list(p[1]) for p in pairs] == flat[1::2]
    assert {tuple(h) for h in pairs[3][1]} == {(1, 11)}       # TTTTT maps to the reverse strand at AAAAA
