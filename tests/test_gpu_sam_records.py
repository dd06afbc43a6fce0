"""gdx_sam_records_many[_dev] (sam_records.hip) against the model of tests/test_sam_records_model.py, byte for byte, every output
prefilled with a garbage pattern: real alignments of the device's traceback, crafted inputs (ten-digit positions, 513 runs, names
of every length, records larger than a tile), batch sizes across workgroups with several tile and grid shapes, capacities cut at
several points, every refusal, the host form, and map_reads / map_pairs end to end through DeviceEngine.sam_records."""
import ctypes as C

import numpy as np
import pytest

from genedex_amd import _lib, reversed_texts
from genedex_amd import alphabet as alph
from test_edit_distance_model import NO_END
from test_gpu_parity import gpu_index
from test_mate_rescue_model import PLANTED, RC, planted_pairs, random_text
from test_sam_records_model import (A, MAX_RUN_SUM, NONE, PAIRED, SINGLE, random_alignments, rebuild_segment, record_bound, sam_model,
                                    words)
from test_strands_model import join

pytestmark = pytest.mark.gpu

FILL = 0xA5
_CASE = {}
TEXT_NAMES = [b"chr1", b"a_longer_name_of_a_text", b""]


def texts_and_engine():
    """three texts of a few hundred symbols with N and the engine on their index, made once"""
    from genedex_amd.device import DeviceEngine

    if "eng" not in _CASE:
        rng = np.random.default_rng(23100)
        _CASE["texts"] = [random_text(rng, 700, 0.02), random_text(rng, 90, 0.0), random_text(rng, 400, 0.05)]
        _CASE["g"] = gpu_index(_CASE["texts"], A)
        _CASE["eng"] = DeviceEngine(_CASE["g"])
    return _CASE["texts"], _CASE["g"], _CASE["eng"]


def dev_u32(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(np.uint32)).view(np.int32)).cuda()


def name_table(names):
    import torch

    off = np.zeros(len(names) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in names], out=off[1:])
    buf = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8).copy()
    return torch.from_numpy(buf).cuda(), torch.from_numpy(off).cuda()


def batch(queries, uniform=0):
    from genedex_amd.device import DeviceQueries

    dq = DeviceQueries.from_host(*join(queries))
    return dq.as_uniform(uniform) if uniform else dq


class Case:
    """the inputs of one call on the host: what the model takes"""

    def __init__(self, queries, strands, mode, k, wq, tid, dist, begin, end, n_cigar, cigar, mapq, proper=None, names=None,
                 text_names=None, dense_to_io=None, uniform=0):
        self.queries, self.strands, self.mode, self.k, self.uniform = queries, strands, mode, k, uniform
        self.cols = [np.asarray(x).astype(np.uint32) for x in (wq, tid, dist, begin, end, n_cigar)]
        self.cigar, self.mapq = np.asarray(cigar).astype(np.uint32).reshape(len(wq), 2 * k + 1), np.asarray(mapq).astype(np.uint32)
        self.proper, self.names, self.text_names, self.dense_to_io = proper, names, text_names, dense_to_io
        self.n = len(wq)

    def model(self, texts):
        wq, tid, dist, begin, end, n_cigar = self.cols
        return sam_model(texts, A, self.queries, self.strands, self.mode, self.k, wq, tid, dist, begin, end, n_cigar, self.cigar, self.mapq,
                         proper=self.proper, names=self.names, text_names=self.text_names, dense_to_io=self.dense_to_io)


def device_call(eng, case, capacity=None, sizing=False, tile=None, grid=None, status=True, slack=64, shift=0):
    """gdx_sam_records_many_dev on the case, out / rec_off / status FILL beforehand -> (out incl. `slack` bytes beyond the
    capacity, rec_off, status) as numpy arrays.  capacity None: the total of a sizing call made first.  shift: the address of
    `out` modulo 16"""
    import torch

    wq, tid, dist, begin, end, n_cigar = case.cols
    n = case.n
    dq = batch(case.queries, case.uniform)
    hits = dev_u32(np.stack([tid, np.full(n, 0x5A5A5A5A, dtype=np.uint32)], axis=1)) if n else dev_u32(np.zeros((1, 2)))
    names = name_table(case.names) if case.names is not None else (None, None)
    tnames = name_table(case.text_names) if case.text_names is not None else (None, None)
    rec_off = torch.full((n + 1,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
    st = torch.full((max(n, 1),), FILL, dtype=torch.uint8, device="cuda") if status else None
    args = [dq, n, case.strands, case.mode, case.k, dev_u32(wq), hits, dev_u32(dist), dev_u32(begin), dev_u32(end), dev_u32(n_cigar),
            dev_u32(case.cigar), dev_u32(case.mapq), rec_off]
    kw = dict(proper=dev_u32(case.proper) if case.proper is not None else None, names=names[0], name_off=names[1], text_names=tnames[0],
              text_name_off=tnames[1], dense_to_io=case.dense_to_io, status=st)
    lib = _lib.load()
    lib.gdx_debug_set_sam_tiling(tile or 0, grid or 0)
    try:
        if capacity is None or sizing:
            eng.sam_records_dev(*args, None, **kw)
            torch.cuda.synchronize()
            if sizing:
                return None, rec_off.cpu().numpy().astype(np.uint64), st.cpu().numpy()[:n] if status else None
            capacity = int(rec_off[n].item())
            rec_off.fill_(-0x5A5A5A5A5A5A5A5B)
        whole = torch.full((capacity + slack + 32,), FILL, dtype=torch.uint8, device="cuda")
        lead = (shift - whole.data_ptr()) % 16
        out = whole[lead:lead + capacity + slack]
        eng.sam_records_dev(*args, out, out_capacity=capacity, **kw)
        torch.cuda.synchronize()
    finally:
        lib.gdx_debug_set_sam_tiling(0, 0)
    assert (whole[:lead] == FILL).all() and (whole[lead + capacity + slack:] == FILL).all()     # nothing in front of out, nothing far behind
    return out.cpu().numpy(), rec_off.cpu().numpy().astype(np.uint64), st.cpu().numpy()[:n] if status else None


def expected(recs, capacity, slack=64):
    """the offsets, and the output buffer of `capacity + slack` bytes: the records that fit whole, FILL everywhere else"""
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    if capacity is None:
        capacity = int(off[-1])
    out = np.full(capacity + slack, FILL, dtype=np.uint8)
    fit = int(np.searchsorted(off, capacity, side="right")) - 1
    body = b"".join(recs[:fit])
    out[:len(body)] = np.frombuffer(body, dtype=np.uint8)
    return out, off


def assert_call(texts, eng, case, what, **kw):
    recs, status = case.model(texts)
    out, off, st = device_call(eng, case, **kw)
    want_out, want_off = expected(recs, kw.get("capacity"))
    assert np.array_equal(off, want_off), (what, "rec_off")
    if not np.array_equal(out, want_out):
        at = int(np.flatnonzero(out != want_out)[0])
        r = int(np.searchsorted(want_off, at, side="right")) - 1
        raise AssertionError((what, "first differing byte", at, "record", r, bytes(out[int(want_off[r]):int(want_off[min(r + 1, case.n)])]),
                              recs[min(r, case.n - 1)]))
    if st is not None:
        assert np.array_equal(st, np.array(status, dtype=np.uint8)), (what, "status")
    return recs


# ------------------------------------------------------------------------------------------------
# 1. real alignments: host-made candidates at planted loci -> the device's traceback -> the records

def aligned_case(strands, uniform):
    """~300 reads (lengths 0..256 with planted edits, or 100 symbols each), aligned on the device once per shape"""
    import torch

    key = ("aligned", strands, uniform)
    if key not in _CASE:
        texts, g, eng = texts_and_engine()
        rng = np.random.default_rng(23200 + strands)
        k, n = 6, 300
        lengths = (100,) if uniform else (0, 1, 5, 30, 63, 64, 65, 128, 150, 255, 256)
        reads, _, _, hits = random_alignments(rng, texts, n, k, lengths)
        if uniform:   # (an edit changes the length: cut or fill to the uniform one)
            reads = [(q + b"ACGT" * 25)[:100] for q in reads]
        strand = rng.integers(0, strands, n)
        queries, cq = [], []
        for r, q in enumerate(reads):  # the aligned form is the planted one: on strand 1 the read as given is its reverse complement
            queries += [q] if strands == 1 else ([q, RC(q)] if strand[r] == 0 else [RC(q), q])
            cq.append(r * strands + int(strand[r]))
        dq = batch(queries, uniform)
        res = eng.align(dq, dev_u32(cq), dev_u32(np.zeros(n)), dev_u32(hits), k)
        torch.cuda.synchronize()
        u32 = lambda name: res[name].cpu().numpy().view(np.uint32)[:n]  # noqa: E731
        end = u32("end")
        mapq = rng.choice([0, 1, 37, 60, 254, 255, 256, 0xFFFFFFFF], n)
        _CASE[key] = (queries, np.where(end != NO_END, np.array(cq), NONE), hits[:, 0], u32("dist"), u32("begin"), end, u32("n_cigar"),
                      res["cigar"].cpu().numpy().view(np.uint32).reshape(n, 2 * k + 1), mapq, k)
        assert (end != NO_END).sum() > 100
    return _CASE[key]


@pytest.mark.parametrize("uniform", (0, 100))
@pytest.mark.parametrize("with_names", (False, True))
@pytest.mark.parametrize("strands", (1, 2))
@pytest.mark.parametrize("mode", (SINGLE, PAIRED))
def test_real_alignments_through_the_device_chain(mode, strands, with_names, uniform):
    texts, g, eng = texts_and_engine()
    queries, wq, tid, dist, begin, end, n_cigar, cigar, mapq, k = aligned_case(strands, uniform)
    n = len(wq)
    rng = np.random.default_rng(23300)
    names = [bytes(rng.integers(33, 127, int(rng.integers(0, 30))).astype(np.uint8)) for _ in range(n)] if with_names else None
    case = Case(queries, strands, mode, k, wq, tid, dist, begin, end, n_cigar, cigar, mapq,
                proper=rng.integers(0, 2, n // 2) if mode == PAIRED else None, names=names, text_names=TEXT_NAMES if with_names else None,
                uniform=uniform)
    recs = assert_call(texts, eng, case, (mode, strands, with_names, uniform))
    # every record within the bound a caller sizes `out` with, and every mapped one rebuilds its piece of the text
    longest, bound_lib = max(len(q) for q in queries), _lib.load().gdx_sam_record_bound
    for r, line in enumerate(recs):
        name_len, tname_len = (max(len(x) for x in names), max(len(x) for x in TEXT_NAMES)) if with_names else (0, 0)
        assert bound_lib(longest, name_len, tname_len, k) == record_bound(longest, name_len, tname_len, k) >= len(line)
        if end[r] != NO_END:
            name, b, segment = rebuild_segment(line)
            t = TEXT_NAMES.index(name) if with_names else int(name)
            assert (t, b) == (tid[r], begin[r]) and segment == texts[t][b:int(end[r])], (r, line)


# ------------------------------------------------------------------------------------------------
# 2. inputs that need no alignment

def synthetic_case(rng, texts, n, strands, mode, k, names=False, max_len=80):
    """n reads as a chain could have left them, and as it could not: unmapped ones, winners of another read, texts that do not
    exist, too many runs, CIGARs that walk beyond their text, runs of length 0, every op code"""
    stride = 2 * k + 1
    queries, rows = [], []
    cigar = np.zeros((n, stride), dtype=np.uint32)
    for r in range(n):
        q = bytes(b"ACGTN"[i] for i in rng.integers(0, 5, int(rng.integers(0, max_len + 1))))
        queries += [q] if strands == 1 else [q, RC(q)]
        kind = rng.random()
        t = int(rng.integers(0, len(texts)))
        b = int(rng.integers(0, len(texts[t]) + 1))
        nc = int(rng.integers(0, min(stride, 7) + 1))
        cigar[r, :nc] = (rng.integers(0, 10, nc) << 4) | rng.choice([7, 7, 7, 8, 8, 1, 2, 2, 0, 3, 4, 5, 6, 9, 15], nc)
        row = [r * strands + int(rng.integers(0, strands)), t, int(rng.integers(0, k + 1)), b, b + int(rng.integers(0, 100)), nc]
        if kind < 0.2:
            row = [NONE, 0, k + 1, NO_END, NO_END, 0]
        elif kind < 0.23:
            row[0] = (row[0] + strands) % (n * strands)                  # another read's query
        elif kind < 0.26:
            row[1] = len(texts) + int(rng.integers(0, 3))
        elif kind < 0.29:
            row[5] = stride + 1 + int(rng.integers(0, 3))
        elif kind < 0.32:
            row[4] = NO_END                                              # a winner the traceback found nothing for
        rows.append(row)
    col = lambda i: [row[i] for row in rows]  # noqa: E731
    return Case(queries, strands, mode, k, col(0), col(1), col(2), col(3), col(4), col(5), cigar, rng.choice([0, 7, 60, 255, 1000], n),
                proper=rng.integers(0, 2, n // 2) if mode == PAIRED else None,
                names=[b"r%d" % r * int(rng.integers(0, 4)) for r in range(n)] if names else None, text_names=TEXT_NAMES if names else None)


def test_positions_near_2_32_and_513_runs():
    texts, g, eng = texts_and_engine()
    k = 256
    cigar = np.zeros((4, 2 * k + 1), dtype=np.uint32)
    cigar[0, 0], cigar[1, 0] = words([(10, "=")])[0], words([(10, "=")])[0]
    cigar[2] = words([(1, "="), (1, "X")] * k + [(1, "=")])                                     # 257 '=' and 256 'X': 513 runs
    cigar[3] = words([(2, "D"), (1, "I")] * k + [(MAX_RUN_SUM - 3 * k, "=")])                   # the run sum at its cap
    wq, tid = [0, 1, 2, 3], [0, 0, 2, 1]
    begin, end = [0xFFFFFF00, 0xFFFFFFF0, 100, 0], [0xFFFFFF0A, 0xFFFFFFFE, 613, 90]
    reads = [b"ACGTACGTAC", b"ACGTACGTAC", b"ACGT" * 128 + b"A", b"A" * 256]
    for mode in (SINGLE, PAIRED):
        case = Case(reads, 1, mode, k, wq, tid, [0, 0, 256, 256], begin, end, [1, 1, 513, 513], cigar, [60] * 4, proper=[1, 0])
        recs = assert_call(texts, eng, case, ("crafted", mode))
        f = [r.split(b"\t") for r in recs]
        assert f[0][3] == b"4294967041" and f[1][3] == b"4294967281" and f[2][5].count(b"X") == 256 and len(f[3][5]) > 1000
        if mode == PAIRED:
            assert (f[0][7], f[0][8], f[1][7], f[1][8]) == (b"4294967281", b"254", b"4294967041", b"-254")
    cigar[3, 2 * k] += 1 << 4                                                                    # one more: no record can be that long
    case = Case(reads, 1, SINGLE, k, wq, tid, [0, 0, 256, 256], begin, end, [1, 1, 513, 513], cigar, [60] * 4)
    recs = assert_call(texts, eng, case, "run sum beyond its cap")
    assert recs[3].split(b"\t")[1] == b"4"


def test_names_of_every_length_and_records_larger_than_a_tile():
    """names of 0..40 bytes and `out` at every address modulo 16 put record starts at every offset modulo 16; names and a read
    longer than a tile (4 KiB at the most) take the path of a record that is not staged, in the middle and at the end of the
    batch, mapped and unmapped"""
    texts, g, eng = texts_and_engine()
    rng = np.random.default_rng(23400)
    case = synthetic_case(rng, texts, 46, 1, SINGLE, 3)
    case.names = [bytes(rng.integers(33, 127, r).astype(np.uint8)) for r in range(41)] + [b"n" * 13000, b"x", b"y" * 30000, b"z", b"w" * 12289]
    case.queries[43] = bytes(b"ACGT"[i] for i in rng.integers(0, 4, 40000))
    case.text_names = [b"chr1", b"t" * 300, b""]
    recs = assert_call(texts, eng, case, "long records")
    assert max(len(r) for r in recs) > 40000
    for shift in range(1, 16):                                                     # every record start at every address modulo 16
        assert_call(texts, eng, case, ("long records", shift), shift=shift)
    case.mode, case.proper = PAIRED, [1] * 23
    assert_call(texts, eng, case, "long records, paired")
    assert_call(texts, eng, case, "long records, small tiles", tile=64, grid=5)


@pytest.mark.parametrize("n", (1, 2, 255, 256, 257, 1025))
def test_batch_sizes_tiles_and_grids(n):
    texts, g, eng = texts_and_engine()
    rng = np.random.default_rng(23500 + n)
    for mode, strands in ((SINGLE, 1), (PAIRED, 2)) if n % 2 == 0 else ((SINGLE, 2),):
        case = synthetic_case(rng, texts, n, strands, mode, 4, names=n % 2 == 1)
        for tile, grid in ((None, None), (64, 1), (256, 3), (4096, 4096), (12288, 2)):
            assert_call(texts, eng, case, (n, mode, tile, grid), tile=tile, grid=grid)


def test_sizing_call_and_capacities():
    texts, g, eng = texts_and_engine()
    rng = np.random.default_rng(23600)
    case = synthetic_case(rng, texts, 300, 2, PAIRED, 4, names=True)
    recs, status = case.model(texts)
    _, want_off = expected(recs, None)
    _, off, st = device_call(eng, case, sizing=True)
    assert np.array_equal(off, want_off) and np.array_equal(st, np.array(status, dtype=np.uint8))
    total = int(want_off[-1])
    for capacity in (0, 1, int(want_off[1]) - 1, int(want_off[1]), int(want_off[1]) + 1, int(want_off[150]) + 7, int(want_off[299]),
                     total - 1, total, total + 50):
        for tile, grid in ((None, None), (128, 7)):
            assert_call(texts, eng, case, ("capacity", capacity, tile), capacity=capacity, tile=tile, grid=grid)
    assert_call(texts, eng, case, "without status", status=False)


# ------------------------------------------------------------------------------------------------
# 3. the refusals and the host form

def test_refused_calls_write_nothing():
    import torch

    from genedex_amd import FmIndexConfig
    from genedex_amd.device import DeviceEngine

    texts, g, eng = texts_and_engine()
    lib = _lib.load()
    z = torch.full((4096,), 7, dtype=torch.int32, device="cuda")
    dq = batch([b"ACGT"] * 8)
    ws_bytes = int(lib.gdx_sam_workspace_bytes(4))
    assert ws_bytes > 0 and lib.gdx_sam_workspace_bytes(10_000_000) >= 10_000_000

    def dev(h=g._h, **kw):
        a = _lib.SamInputs()
        a.qbuf, a.qoff, a.nq, a.layout = dq.qbuf.data_ptr(), dq.qoff.data_ptr(), 4, None
        a.n_reads, a.strands, a.mode, a.max_edits = 4, 1, SINGLE, 3
        for i, name in enumerate(("win_query", "win_hits", "dist", "begin", "end", "n_cigar", "cigar", "mapq")):
            setattr(a, name, z[64 * i:].data_ptr())
        a.workspace, a.workspace_bytes = z[1024:].data_ptr(), ws_bytes
        a.rec_off, a.out, a.out_capacity, a.status = z[2048:].data_ptr(), z[2304:].data_ptr(), 4096, z[3584:].data_ptr()
        for name, value in kw.items():
            setattr(a, name, value)
        return lib.gdx_sam_records_many_dev(h, C.byref(a), None)

    bad_layout, packed = _lib.QueryLayout(), _lib.QueryLayout()
    for lay in (bad_layout, packed):
        lib.gdx_query_layout_init(C.byref(lay))
    bad_layout.packed, packed.packed = 2, 1
    invalid = [dict(strands=0), dict(strands=3), dict(nq=5), dict(nq=8), dict(strands=2, nq=4), dict(mode=2), dict(mode=PAIRED, n_reads=3, nq=3),
               dict(max_edits=257), dict(layout=C.pointer(bad_layout)), dict(workspace_bytes=ws_bytes - 1), dict(workspace=None),
               dict(names=z.data_ptr()), dict(text_name_off=z.data_ptr())]
    invalid += [{name: None} for name in ("qbuf", "qoff", "win_query", "win_hits", "dist", "begin", "end", "n_cigar", "cigar", "mapq", "rec_off")]
    for kw in invalid:
        assert dev(**kw) == _lib.GDX_ERR_INVALID_ARGUMENT, kw
    assert lib.gdx_sam_records_many_dev(g._h, None, None) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert dev(layout=C.pointer(packed)) == _lib.GDX_ERR_UNSUPPORTED
    bare = gpu_index(texts, A, text_units=False, seed_symbols=0, full_suffix_array=False, inverse_suffix_array=False)
    assert not DeviceEngine(bare).aux_info()["text_units"]
    assert dev(h=bare._h) == _lib.GDX_ERR_UNSUPPORTED
    lib.gdx_debug_force_wide(1)
    try:
        w = FmIndexConfig("i64").suffix_array_sampling_rate(4).construct_index([b"ACGTACGTTGCA"], A)
    finally:
        lib.gdx_debug_force_wide(0)
    assert w.info.index_width == 64 and dev(h=w._h) == _lib.GDX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (z.cpu().numpy() == 7).all()                                            # nothing was written by any refused call
    # the same arguments, accepted: four records of reads without a usable winner (win_query 7 is no read's), all flagged
    assert dev() == _lib.GDX_OK
    torch.cuda.synchronize()
    off = z[2048:2058].cpu().numpy().view(np.uint64)
    assert off[0] == 0 and off[4] == 4 * len(b"0\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\n")
    assert bytes(z[2304:2304 + 7].cpu().numpy().view(np.uint8)[:25]) == b"0\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\n"
    assert (z[3584:3585].cpu().numpy().view(np.uint8) == 1).all()
    # n_reads == 0 looks at nothing but rec_off
    z.fill_(7)
    assert dev(n_reads=0, nq=0, qbuf=None, qoff=None, win_query=None, cigar=None, out=None, status=None) == _lib.GDX_OK
    torch.cuda.synchronize()
    zz = z.cpu().numpy()
    assert (zz[2048:2050] == 0).all() and (np.delete(zz, [2048, 2049]) == 7).all()

    # the host form: the same causes; its outputs stay as they were
    qbuf, qoff = join([b"ACGT"] * 4)
    cols = [np.full(4 * 7, 7, dtype=np.uint32) for _ in range(7)]
    hits = (_lib.HitStruct * 4)()
    rec_off, out, status = np.full(5, 7, dtype=np.uint64), np.full(256, 7, dtype=np.uint8), np.full(4, 7, dtype=np.uint8)

    def host(h=g._h, hit=(0, 0), **kw):
        hits[0] = hit
        a = _lib.SamInputs()
        a.qbuf, a.qoff, a.nq, a.layout = qbuf.ctypes.data, qoff.ctypes.data, 4, None
        a.n_reads, a.strands, a.mode, a.max_edits = 4, 1, SINGLE, 3
        for x, name in zip(cols, ("win_query", "dist", "begin", "end", "n_cigar", "cigar", "mapq")):
            setattr(a, name, x.ctypes.data)
        a.win_hits = C.addressof(hits)
        a.rec_off, a.out, a.out_capacity, a.status = rec_off.ctypes.data, out.ctypes.data, 256, status.ctypes.data
        for name, value in kw.items():
            setattr(a, name, value)
        return lib.gdx_sam_records_many(h, C.byref(a))

    for kw in (dict(strands=3), dict(nq=5), dict(mode=7), dict(mode=PAIRED, n_reads=3, nq=3), dict(max_edits=257), dict(layout=C.pointer(bad_layout)),
               dict(hit=(1 << 32, 0)), dict(hit=(0, 1 << 32)), dict(rec_off=None), dict(qoff=None), dict(win_query=None), dict(cigar=None)):
        assert host(**kw) == _lib.GDX_ERR_INVALID_ARGUMENT, kw
    assert host(h=bare._h) == _lib.GDX_ERR_UNSUPPORTED and host(h=w._h) == _lib.GDX_ERR_UNSUPPORTED
    assert host(layout=C.pointer(packed)) == _lib.GDX_ERR_UNSUPPORTED
    assert (rec_off == 7).all() and (out == 7).all() and (status == 7).all()
    assert host() == _lib.GDX_OK and rec_off[0] == 0 and (status == 1).all() and bytes(out[:int(rec_off[1])]) == b"0\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\n"


def test_host_form_equals_the_device_form():
    texts, g, eng = texts_and_engine()
    rng = np.random.default_rng(23700)
    for n, strands, mode, k, names in ((301, 1, SINGLE, 3, True), (64, 2, PAIRED, 256, False), (1, 2, SINGLE, 0, True)):
        case = synthetic_case(rng, texts, n, strands, mode, k, names=names)
        recs, status = case.model(texts)
        want_out, want_off = expected(recs, None, slack=0)
        wq, tid, dist, begin, end, n_cigar = case.cols
        nm = name_off = tn = tn_off = None
        if names:
            (nm, name_off), (tn, tn_off) = ((np.frombuffer(b"".join(x), dtype=np.uint8), np.cumsum([0] + [len(y) for y in x]).astype(np.uint64))
                                            for x in (case.names, case.text_names))
        call = lambda **kw: g.sam_records_raw(*join(case.queries), wq, tid, dist, begin, end, n_cigar, case.cigar, case.mapq,  # noqa: E731
                                              strands=strands, mode=mode, max_edits=k, proper=case.proper, names=nm, name_off=name_off,
                                              text_names=tn, text_name_off=tn_off, **kw)
        out, off, st = call()
        assert np.array_equal(off, want_off) and np.array_equal(out, want_out) and np.array_equal(st, np.array(status, dtype=np.uint8))
        dev_out, dev_off, dev_st = device_call(eng, case, slack=0)
        assert np.array_equal(dev_out, out) and np.array_equal(dev_off, off) and np.array_equal(dev_st, st)
        cut = int(want_off[n // 2]) + 3                                            # a capacity inside a record: the whole ones before it
        out, off, _ = call(out_capacity=cut)
        want_cut, _ = expected(recs, cut, slack=0)
        assert np.array_equal(off, want_off) and np.array_equal(out, want_cut)
    out, off, st = g.sam_records_raw(np.zeros(8, dtype=np.uint8), np.zeros(1, dtype=np.uint64), *[np.zeros(0, dtype=np.uint32)] * 6,
                                     np.zeros((0, 7), dtype=np.uint32), np.zeros(0, dtype=np.uint32), max_edits=3)
    assert out.size == 0 and off.tolist() == [0] and st.size == 0


# ------------------------------------------------------------------------------------------------
# 4. end to end: map_pairs(rescue=True) and map_reads on planted reads through DeviceEngine.sam_records

def parse(out, rec_off):
    data = out.cpu().numpy().tobytes()
    off = rec_off.cpu().numpy()
    assert off[0] == 0 and off[-1] == len(data)
    lines = [data[int(off[r]):int(off[r + 1])] for r in range(len(off) - 1)]
    assert all(line.endswith(b"\n") and line.count(b"\n") == 1 and line.count(b"\t") in (10, 12) for line in lines)
    return lines


def test_planted_reads_end_to_end(tmp_path):
    import torch

    from genedex_amd import sam
    from genedex_amd.device import DeviceEngine, DeviceQueries
    from test_candidates_model import A as DNA

    rng = np.random.default_rng(23800)
    text = random_text(rng, PLANTED["text_len"])
    n, k = 100, PLANTED["max_edits"]
    reads, damaged, origin = planted_pairs(rng, text, n)
    g, r = gpu_index([text], DNA), gpu_index(reversed_texts([text]), DNA)
    eng = DeviceEngine(g)
    dq = DeviceQueries.from_host(*join(reads))
    sq = dq.with_strands(g, "both")
    knobs = dict(max_smems=PLANTED["max_smems"], min_length=PLANTED["min_length"], max_occ=PLANTED["max_occ"], band=PLANTED["band"],
                 max_candidates=PLANTED["max_candidates"], max_edits=k)
    pairs = eng.map_pairs(dq, r, rescue=True, min_insert=PLANTED["min_insert"], max_insert=PLANTED["max_insert"], **knobs)
    names = [b"pair%d" % (i // 2) for i in range(2 * n)]
    out, rec_off, status = eng.sam_records(sq, pairs, mode="paired", names=names, text_names=[b"chrT"])
    torch.cuda.synchronize()
    lines = parse(out, rec_off)
    u32 = lambda t: t.cpu().numpy().view(np.uint32).astype(np.int64)  # noqa: E731
    begin, end, proper = u32(pairs["begin"]), u32(pairs["end"]), (u32(pairs["n_proper"]) != 0) | (u32(pairs["resc_mate"]) != NONE)
    assert len(lines) == 2 * n and not status.cpu().numpy().any() and proper.all()          # (every planted pair is proper or rescued)
    for i, line in enumerate(lines):
        f = line.split(b"\t")
        assert f[0] == names[i] and end[i] != NO_END
        name, b, segment = rebuild_segment(line)
        assert name == b"chrT" and b == begin[i] and segment == text[b:int(end[i])], (i, line)
        flags = (int(f[1]), int(lines[i ^ 1].split(b"\t")[1]))
        assert flags in ((99, 147), (147, 99), (83, 163), (163, 83)), (i, flags)
        assert f[6] == b"=" and int(f[7]) == begin[i ^ 1] + 1 and int(f[8]) == -int(lines[i ^ 1].split(b"\t")[8]) != 0
    # the same reads single-end, numbers for names, through a file; and a caller-given capacity from the bound, without the sizing call
    single = eng.map_reads(dq, r, **knobs)
    out, rec_off, status = eng.sam_records(sq, single, mode="single")
    bound = eng.sam_record_bound(PLANTED["mate_len"], 0, 0, k)
    out2, rec_off2, _ = eng.sam_records(sq, single, mode="single", sizing=2 * n * bound)
    torch.cuda.synchronize()
    lines = parse(out, rec_off)
    total = int(rec_off[-1].item())
    assert torch.equal(rec_off, rec_off2) and torch.equal(out, out2[:total]) and max(len(x) for x in lines) <= bound
    begin, end, strand = u32(single["begin"]), u32(single["end"]), u32(single["strand"])
    mapped = 0
    for i, line in enumerate(lines):
        f = line.split(b"\t")
        assert f[0] == b"%d" % i
        if end[i] == NO_END:
            assert f[1] == b"4" and f[9] == reads[i]
            continue
        mapped += 1
        name, b, segment = rebuild_segment(line)
        assert name == b"0" and b == begin[i] and segment == text[b:int(end[i])] and int(f[1]) == 16 * strand[i], (i, line)
        assert f[9] == (reads[i] if strand[i] == 0 else RC(reads[i]))
    assert mapped >= n                                                                        # (the undamaged mate of every pair at least)
    path = tmp_path / "reads.sam"
    written = sam.write(str(path), out[:total], None, [len(text)])
    assert path.read_bytes() == sam.header(None, [len(text)]) + b"".join(lines) and written == path.stat().st_size
