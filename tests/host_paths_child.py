"""The index, the batches and the checks of tests/test_gpu_host_paths.py, and -- run as a program -- one pass of them in a
process of its own: libgdx.so reads GDX_HOST_RESULTS and GDX_HOST_WIDE_HITS once per process, so every combination of the two
needs a fresh one.  Prints PASS when every host-pointer call gave the oracle's result."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (an empty read matches every row: the two of the batch sit in the cluster's chunk as well)
CLUSTER = [b"", b"A", b"C", b"G", b"T", b"AC", b"CA", b"GT", b"TG", b"AA", b"CC", b"GG", b"TT", b""]
CLUSTER_AT = 2500   # (main batch; inside one chunk of 97 and of 4 * 97 reads, with and without the run of N reads before it)
N_RUN_AT, N_RUN = 1000, 200
LONG_READ = 7000    # symbols: longer than the byte limit of a chunk in the second chunking, packed or not
UNIFORM_LEN = 40


def _dna(rng, n, p_n):
    return bytes(b"ACGTN"[i] for i in rng.choice(5, n, p=[(1 - p_n) / 4] * 4 + [p_n]))


def _sampled(rng, texts, n, lo, hi, with_n=False):
    """n reads of lo..hi symbols cut from the texts: without an N, or (with_n) each across one"""
    out = []
    while len(out) < n:
        t = texts[int(rng.integers(0, len(texts)))]
        length = int(rng.integers(lo, hi + 1))
        pos = int(rng.integers(0, len(t) - length))
        q = t[pos:pos + length]
        if (b"N" in q) == with_n:
            out.append(q)
    return out


def _want(c, qs):
    from oracle.oracle import pack_queries

    qbuf, qoff = pack_queries(qs)
    cs, ce = c.cursors_for_many(qbuf, qoff)
    co, ct, cp = c.locate_intervals(cs, ce)
    return SimpleNamespace(start=cs, end=ce, off=co, text=ct, pos=cp)


def _form(case, name, qs, packed, uniform):
    from genedex_amd import _lib
    from oracle.oracle import pack_queries

    qbuf, qoff = pack_queries(qs)
    nq = len(qs)
    key = (tuple(qs[:3]), nq)
    if key not in case.wants:
        case.wants[key] = _want(case.c, qs)
    buf = qbuf
    if packed:
        buf = np.zeros(int(case.lib.gdx_packed_bytes(int(qoff[-1]))), dtype=np.uint8)
        n_exc = C.c_uint64(0)
        _lib.check(case.lib.gdx_pack_queries(case.g._h, qbuf.ctypes.data_as(_lib.u8p), qoff.ctypes.data_as(_lib.u64p), nq,
                                             buf.ctypes.data_as(_lib.u8p), None, 0, C.byref(n_exc)))
        assert n_exc.value == 0
    return SimpleNamespace(name=name, qs=qs, qbuf=qbuf, qoff=qoff, buf=buf, off=None if uniform else qoff, nq=nq, packed=packed,
                           ul=UNIFORM_LEN if uniform else 0, want=case.wants[key])


def build_case():
    """One small index (3 texts, 20 000 symbols, DNA with N, default build), its oracle, and the batch in four forms"""
    from genedex_amd import FmIndexConfig, _lib
    from genedex_amd import alphabet as alph
    from oracle.oracle import OracleIndex

    rng = np.random.default_rng(2107)
    a = alph.ascii_dna_with_n()
    t2 = _dna(rng, 7500, 0.0)       # no N: the long read lies here, and a stretch the other two texts repeat
    rep = t2[2000:2400]
    texts = [_dna(rng, 6100, 0.01) + rep, _dna(rng, 5200, 0.01) + rep + _dna(rng, 400, 0.01), t2]
    g = FmIndexConfig("u32").suffix_array_sampling_rate(4).construct_index(texts, a)
    c = OracleIndex.build(texts, a.io_to_dense_table, 6, 4, sa_rate=4, lookup_depth=0, width=32)
    case = SimpleNamespace(g=g, c=c, lib=_lib.load(), texts=texts, wants={})

    def rnd(n, lo, hi):
        return [bytes(b"ACGT"[i] for i in rng.integers(0, 4, int(k))) for k in rng.integers(lo, hi + 1, n)]

    # ragged: one hit, three hits (the repeat), none; then at fixed places the run of reads with an N, the
    # cluster of empty, one- and two-symbol reads (tens of thousands of hits in one chunk) and the long read
    body = _sampled(rng, texts, 2400, 18, 70) + _sampled(rng, [rep], 500, 18, 70) + rnd(640, 18, 70)
    body = [body[i] for i in rng.permutation(len(body))]
    clean = body[:CLUSTER_AT - N_RUN] + CLUSTER + body[CLUSTER_AT - N_RUN:3000] + [t2[100:100 + LONG_READ]] + body[3000:]
    main = clean[:N_RUN_AT] + _sampled(rng, texts[:2], N_RUN, 18, 70, with_n=True) + clean[N_RUN_AT:]
    assert main[CLUSTER_AT:CLUSTER_AT + len(CLUSTER)] == CLUSTER and len(main) > 9 * 4 * 97
    # uniform: reads of 40 symbols, the same kinds
    ubody = _sampled(rng, texts, 2900, UNIFORM_LEN, UNIFORM_LEN) + _sampled(rng, [rep], 400, UNIFORM_LEN, UNIFORM_LEN) \
        + rnd(300, UNIFORM_LEN, UNIFORM_LEN)
    uclean = [ubody[i] for i in rng.permutation(len(ubody))]
    umain = uclean[:N_RUN_AT] + _sampled(rng, texts[:2], 150, UNIFORM_LEN, UNIFORM_LEN, with_n=True) + uclean[N_RUN_AT:]
    case.forms = {
        "ascii": _form(case, "ascii", main, False, False),
        "packed": _form(case, "packed", clean, True, False),
        "uniform": _form(case, "uniform", umain, False, True),
        "packed-uniform": _form(case, "packed-uniform", uclean, True, True),
    }
    w = case.forms["ascii"].want
    counts = np.diff(w.off.astype(np.int64))
    assert (counts == 0).sum() > 500 and (counts == 1).sum() > 1500 and (counts == 3).sum() > 300
    chunk = slice(CLUSTER_AT // 388 * 388, CLUSTER_AT // 388 * 388 + 388)
    assert counts[chunk].sum() > 388 * 5 // 4 + 4096 + 388  # only this chunk's hits exceed what its buffers were sized for
    assert max(counts[k:k + 388].sum() for k in range(0, len(main), 388) if k != chunk.start) < 4096
    return case


def _same_hits(got, want, what):
    off, t, p = got
    assert off.tolist() == want.off.tolist(), what + ": hit offsets"
    assert t.tolist() == want.text.tolist() and p.tolist() == want.pos.tolist(), what + ": hits"


def check_form(case, f, flagged=True, wide=True, narrow=True):
    """Every host-pointer call that takes the form, against the oracle"""
    import torch

    from genedex_amd import _lib

    g, w, lay = case.g, f.want, dict(packed=f.packed, uniform_len=f.ul)
    if flagged:
        s, e, st = g.cursors_layout_raw(f.buf, f.off, f.nq, **lay)
        assert s.tolist() == w.start.tolist() and e.tolist() == w.end.tolist() and not st.any(), f.name + ": intervals"
        cnt, st = g.count_layout_raw(f.buf, f.off, f.nq, **lay)
        assert cnt.tolist() == (w.end - w.start).tolist() and not st.any(), f.name + ": counts"
    if wide:
        off, t, p, st = g.locate_layout_raw(f.buf, f.off, f.nq, **lay)
        _same_hits((off, t, p), w, f.name + ": gdx_locate_many_alloc_layout")
        assert not st.any()
    if wide and not f.packed and f.ul == 0:
        off, t, p, st = g.locate_raw(f.qbuf, f.qoff)  # the sizing call, then the fill
        _same_hits((off, t, p), w, f.name + ": gdx_locate_many")
        off, t, p, st = g.locate_alloc_raw(f.qbuf, f.qoff)
        _same_hits((off, t, p), w, f.name + ": gdx_locate_many_alloc")
        # a hit buffer that is too small: GDX_ERR_CAPACITY, the total and the offsets are right all the same
        total_want = int(w.off[-1])
        offs = np.zeros(f.nq + 1, dtype=np.uint64)
        small = np.zeros((total_want // 2, 2), dtype=np.uint64)
        total = C.c_uint64(0)
        rc = case.lib.gdx_locate_many(g._h, f.qbuf.ctypes.data_as(_lib.u8p), f.qoff.ctypes.data_as(_lib.u64p), f.nq,
                                      offs.ctypes.data_as(_lib.u64p), small.ctypes.data_as(C.POINTER(_lib.HitStruct)),
                                      small.shape[0], C.byref(total), None)
        assert rc == _lib.GDX_ERR_CAPACITY and total.value == total_want and offs.tolist() == w.off.tolist(), f.name + ": small buffer"
    if narrow:
        off, t, p, st = g.locate_layout32_raw(f.buf, f.off, f.nq, **lay)
        assert off.dtype == np.uint32 and t.dtype == np.uint32 and not st.any()
        _same_hits((off, t, p), w, f.name + ": gdx_locate_many_alloc_layout32")
        pinned = torch.from_numpy(f.buf.copy()).pin_memory()
        off, t, p, st = g.locate_layout32_raw(None, f.off, f.nq, qbuf_ptr=pinned.data_ptr(), **lay)
        _same_hits((off, t, p), w, f.name + ": gdx_locate_many_alloc_layout32, pinned input")
        assert not st.any()


def check_statuses(case):
    """One read with a byte outside the alphabet in the middle chunk: the strict form of every call fails, the other returns that
    read's status alone and everything else as before"""
    from genedex_amd import GdxError, _lib
    from oracle.oracle import pack_queries

    g, f = case.g, case.forms["ascii"]
    at = f.nq // 2
    good = case.texts[2][300:340]
    bad = list(f.qs)
    bad[at] = good[:-3] + b"#" + good[-2:]  # (two symbols matched when the search meets it: GDX_Q_INVALID_SYMBOL)
    bbuf, boff = pack_queries(bad)
    counts = np.diff(f.want.off.astype(np.int64))
    keep = np.arange(f.nq) != at
    first = f.want.off[:-1].astype(np.int64)
    rows = np.concatenate([np.arange(first[i], first[i] + counts[i]) for i in np.flatnonzero(keep)])
    counts[at] = 0
    want_off = np.concatenate([[0], np.cumsum(counts)])

    def one_status(st, what):
        assert np.flatnonzero(st).tolist() == [at] and st[at] == _lib.GDX_Q_INVALID_SYMBOL, what

    for call in (g.cursors_raw, g.count_raw, g.locate_raw, g.locate_alloc_raw,
                 lambda b, o, **kw: g.locate_layout32_raw(b, o, f.nq, **kw)):
        try:
            call(bbuf, boff)
        except GdxError:
            pass
        else:
            raise AssertionError("a strict call returned with a bad read in the batch")
    s, e, st = g.cursors_raw(bbuf, boff, strict=False)
    one_status(st, "intervals")
    assert s[keep].tolist() == f.want.start[keep].tolist() and e[keep].tolist() == f.want.end[keep].tolist()
    cnt, st = g.count_raw(bbuf, boff, strict=False)
    one_status(st, "counts")
    assert cnt.tolist() == counts.tolist()
    for what, res in (("gdx_locate_many", g.locate_raw(bbuf, boff, strict=False)),
                      ("gdx_locate_many_alloc", g.locate_alloc_raw(bbuf, boff, strict=False)),
                      ("gdx_locate_many_alloc_layout32", g.locate_layout32_raw(bbuf, boff, f.nq, strict=False))):
        off, t, p, st = res
        one_status(st, what)
        assert off.tolist() == want_off.tolist(), what
        assert t.tolist() == f.want.text[rows].tolist() and p.tolist() == f.want.pos[rows].tolist(), what


def main():
    case = build_case()
    case.lib.gdx_debug_set_host_chunking(97, 0)
    try:
        for f in case.forms.values():
            check_form(case, f)
        check_statuses(case)
    finally:
        case.lib.gdx_debug_set_host_chunking(0, 0)
    print("PASS")


if __name__ == "__main__":
    main()
