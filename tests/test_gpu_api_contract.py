"""Contract of the C ABI (include/gdx.h) beyond the happy path: status codes where the reference panics, the
two-phase locate protocol, device-resident entry points, concurrent use of one handle."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from genedex_amd import alphabet as alph
from helpers import naive_occurrence_columns, random_texts
from oracle.oracle import OracleIndex, pack_queries

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    from genedex_amd import FmIndexConfig, _lib

    rng = np.random.default_rng(2024)
    a = alph.ascii_dna_with_n()
    texts = [bytes(b"ACGTN"[i] for i in rng.choice(5, 20000, p=[.2475, .2475, .2475, .2475, .01])) for _ in range(3)]
    g = FmIndexConfig("u32").lookup_table_depth(3).construct_index(texts, a)
    c = OracleIndex.build(texts, a.io_to_dense_table, 6, 4, sa_rate=4, lookup_depth=3, width=32)
    return _lib, _lib.load(), g, c, texts, rng


def test_invalid_arguments_are_reported_not_crashed(setup):
    _lib, lib, g, c, texts, rng = setup
    u8p, u64p = _lib.u8p, _lib.u64p
    qbuf, qoff = pack_queries([b"ACGT", b"GG"])
    out = np.zeros(2, dtype=np.uint64)
    # null handle / null outputs / decreasing offsets
    assert lib.gdx_count_many(None, qbuf.ctypes.data_as(u8p), qoff.ctypes.data_as(u64p), 2, out.ctypes.data_as(u64p), None) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert lib.gdx_count_many(g._h, qbuf.ctypes.data_as(u8p), qoff.ctypes.data_as(u64p), 2, None, None) == _lib.GDX_ERR_INVALID_ARGUMENT
    bad = np.array([0, 4, 2], dtype=np.uint64)
    assert lib.gdx_count_many(g._h, qbuf.ctypes.data_as(u8p), bad.ctypes.data_as(u64p), 2, out.ctypes.data_as(u64p), None) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert b"non-decreasing" in lib.gdx_last_error()
    # construction: sigma / rate / width / depth / device
    tab = alph.ascii_dna().io_to_dense_table
    h = C.c_void_p()
    tbuf, toff = pack_queries([b"ACGT"])

    def build(sigma=5, k=4, rate=4, depth=0, width=32, device=0):
        return lib.gdx_index_build(tbuf.ctypes.data_as(u8p), toff.ctypes.data_as(u64p), 1, tab.ctypes.data_as(u8p), sigma, k,
                                   rate, depth, width, device, C.byref(h))

    assert build(sigma=1) == _lib.GDX_ERR_INVALID_ARGUMENT      # condensed.rs:64
    assert build(rate=0) == _lib.GDX_ERR_INVALID_ARGUMENT       # config.rs:28
    assert build(width=16) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert build(depth=40) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert build(device=99) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert build(k=5) == _lib.GDX_ERR_INVALID_ARGUMENT          # alphabet.rs:183-186
    assert build() == _lib.GDX_OK
    lib.gdx_index_free(h)
    # zero queries is fine
    empty = np.zeros(1, dtype=np.uint64)
    assert lib.gdx_count_many(g._h, None, empty.ctypes.data_as(u64p), 0, None, None) == _lib.GDX_OK


def test_two_phase_locate_protocol(setup):
    _lib, lib, g, c, texts, rng = setup
    u8p, u64p = _lib.u8p, _lib.u64p
    qs = [texts[0][100:130], b"A", texts[1][5:60], b"ACGTACGTACGTACGTACGTAAAA"]
    qbuf, qoff = pack_queries(qs)
    off = np.zeros(len(qs) + 1, dtype=np.uint64)
    total = C.c_uint64(0)
    rc = lib.gdx_locate_many(g._h, qbuf.ctypes.data_as(u8p), qoff.ctypes.data_as(u64p), len(qs), off.ctypes.data_as(u64p),
                             None, 0, C.byref(total), None)
    assert rc == _lib.GDX_ERR_CAPACITY and total.value == off[-1] > 0
    hits = np.zeros((total.value, 2), dtype=np.uint64)
    rc = lib.gdx_locate_many(g._h, qbuf.ctypes.data_as(u8p), qoff.ctypes.data_as(u64p), len(qs), off.ctypes.data_as(u64p),
                             hits.ctypes.data_as(C.POINTER(_lib.HitStruct)), total.value - 1, C.byref(total), None)
    assert rc == _lib.GDX_ERR_CAPACITY
    rc = lib.gdx_locate_many(g._h, qbuf.ctypes.data_as(u8p), qoff.ctypes.data_as(u64p), len(qs), off.ctypes.data_as(u64p),
                             hits.ctypes.data_as(C.POINTER(_lib.HitStruct)), total.value, C.byref(total), None)
    assert rc == _lib.GDX_OK
    co, ct, cp = c.locate_many(qs)
    assert off.tolist() == co.tolist() and hits[:, 0].tolist() == ct.tolist() and hits[:, 1].tolist() == cp.tolist()


def test_one_handle_from_many_threads(setup):
    """FmIndex is Send + Sync in the reference; handles are immutable here."""
    _lib, lib, g, c, texts, rng = setup
    qs = [texts[int(rng.integers(0, 3))][s:s + 40] for s in rng.integers(0, 19000, 4000)]
    qs = [q for q in qs if b"N" not in q[-3:]]
    want = c.count_many(qs).tolist()
    errors = []

    def worker():
        try:
            for _ in range(3):
                got = g.count_many(qs).tolist()
                if got != want:
                    errors.append("mismatch")
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=worker) for _ in range(4)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors[:3]


@pytest.mark.parametrize("hint", [False, True])
def test_device_resident_entry_points(setup, hint):
    """hint=True: the search hands locate the sampled rows it passed through (gdx_*_hint_dev); same results."""
    torch = pytest.importorskip("torch")
    from genedex_amd.device import DeviceEngine, DeviceQueries

    _lib, lib, g, c, texts, rng = setup
    qs = [texts[int(rng.integers(0, 3))][s:s + int(rng.integers(1, 90))] for s in rng.integers(0, 19000, 5000)]
    qs = [q for q in qs if b"N" not in q[-3:]] + [b"", b"T" * 300]
    qbuf, qoff = pack_queries(qs)
    dq = DeviceQueries.from_host(qbuf, qoff)
    eng = DeviceEngine(g)
    out = eng.alloc_outputs(dq.nq, hint=hint)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # a non-default stream: the ABI must enqueue on the stream it is given
        eng.search(dq, out)
        eng.hit_offsets(out, dq.nq)
        stream.synchronize()
        total = int(out["hit_offsets"][dq.nq].item())
        hits = torch.empty((total, 2), dtype=torch.int32, device="cuda")
        ws = torch.empty(eng.locate_workspace_bytes(total), dtype=torch.uint8, device="cuda")
        eng.locate(out, dq.nq, total, hits, ws)
        counts = torch.empty(dq.nq, dtype=torch.int32, device="cuda")
        status = torch.empty(dq.nq, dtype=torch.uint8, device="cuda")
        eng.count(dq, counts, status)
        stream.synchronize()
    cs, ce = c.cursors_for_many(qbuf, qoff)
    assert (out["start"].cpu().numpy().astype(np.uint32) == cs.astype(np.uint32)).all()
    assert (out["end"].cpu().numpy().astype(np.uint32) == ce.astype(np.uint32)).all()
    assert (counts.cpu().numpy().astype(np.uint32) == (ce - cs).astype(np.uint32)).all()
    co, ct, cp = c.locate_intervals(cs, ce)
    h = hits.cpu().numpy().astype(np.uint32)
    assert np.array_equal(out["hit_offsets"].cpu().numpy().astype(np.uint64), co)
    assert np.array_equal(h[:, 0], ct.astype(np.uint32)) and np.array_equal(h[:, 1], cp.astype(np.uint32))
    # unaligned device query buffer is rejected (gdx.h: 8-byte alignment)
    rc = lib.gdx_count_many_dev(g._h, C.c_void_p(dq.qbuf.data_ptr() + 1), C.c_void_p(dq.qoff.data_ptr()), 1,
                                C.c_void_p(counts.data_ptr()), None, None)
    assert rc == _lib.GDX_ERR_INVALID_ARGUMENT


def test_device_entries_refuse_bad_arguments_in_order(setup):
    """What the _dev entries refuse, with which status and which gdx_last_error text, and which of two faults is reported
    (the order in which an entry looks at its arguments is part of the contract), read off capi.hip.  No case depends on a
    launch: every pointer that is not null lies inside one live zero-filled allocation, a misaligned one too, counts are zero
    or tiny wherever the refusal does not hang on them, and where it does (a batch without offsets, 2^32 - 1 cursors) the call
    could do nothing if it went on -- no candidates, an empty active list."""
    torch = pytest.importorskip("torch")
    from genedex_amd import FmIndexConfig

    _lib, lib, g, c, texts, rng = setup
    buf = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    A = (buf.data_ptr() + 255) // 256 * 256
    h = g._h
    INV, UNS, OK = _lib.GDX_ERR_INVALID_ARGUMENT, _lib.GDX_ERR_UNSUPPORTED, _lib.GDX_OK

    def layout(struct_size=None, packed=0, uniform_len=0):
        class Longer(C.Structure):  # room for a struct_size beyond what the library knows
            _fields_ = [("l", _lib.QueryLayout), ("more", C.c_uint64)]

        lo = Longer()
        lib.gdx_query_layout_init(C.byref(lo.l))
        assert lo.l.struct_size == C.sizeof(_lib.QueryLayout) == 16
        if struct_size is not None:
            lo.l.struct_size = struct_size
        lo.l.packed, lo.l.uniform_len = packed, uniform_len
        return C.cast(C.pointer(lo), C.POINTER(_lib.QueryLayout))

    need = (C.c_uint64 * 2)()  # align: the workspace one candidate needs
    assert lib.gdx_align_many_dev(h, None, None, 0, None, None, None, None, 1, 1, None, None, None, None, None, None, 0, need, None) == OK
    assert need[0] > 1
    QBUF8 = "d_qbuf must be 8-byte aligned"
    REC = "d_records must be a non-null 16-byte aligned device pointer"
    NARROW = "32-bit hit offsets need fewer than 2^32 hits"
    WIDTH = "offsets_width must be 32 or 64"
    LSIZE = "gdx_query_layout_t.struct_size"
    COUNTERS = "active lists need their counters"
    STEP = "gdx_locate_many_step_compact_layout_dev"

    def step(layout_=None, rec=A, scan=A, totals=A, off=A, width=64, hits=None, capacity=0, ws=None, qbuf=A, nq=0):
        return (STEP, (h, qbuf, A, nq, layout_, 0, rec, None, scan, totals, off, width, hits, capacity, ws, None, None))

    def ham(layout_, qbuf=A, qoff=A, nq=0):  # m = 0: the layout is looked at, then the entry returns
        return ("gdx_hamming_many_dev", (h, qbuf, qoff, nq, layout_, None, None, None, 0, 1, None, None))

    cases = [
        # the plain query side: 8-byte d_qbuf, then the entry's own outputs
        ("gdx_count_many_dev", (h, A + 1, A, 0, A, None, None), INV, QBUF8),
        ("gdx_cursors_for_many_queries_dev", (h, A + 4, A, 0, A, A, None, None), INV, QBUF8),
        ("gdx_cursors_for_many_queries_hint_dev", (h, A, A, 0, A, A, None, None, None), INV,
         "d_hint must be a non-null 8-byte aligned device pointer"),
        ("gdx_cursors_for_many_queries_hint_dev", (h, A, A, 0, A, A, None, A + 4, None), INV,
         "d_hint must be a non-null 8-byte aligned device pointer"),
        ("gdx_cursors_for_many_queries_hint_dev", (h, A + 1, A, 0, A, A, None, None, None), INV, QBUF8),  # two faults
        ("gdx_locate_many_search_dev", (h, A, A, 0, None, None), INV, REC),
        ("gdx_locate_many_search_dev", (h, A, A, 0, A + 8, None), INV, REC),
        ("gdx_locate_many_search_dev", (h, A + 2, A, 0, None, None), INV, QBUF8),  # two faults
        ("gdx_locate_many_search_compact_dev", (h, A, A, 1, A, None, None), INV, "d_compact is null"),
        ("gdx_locate_many_search_compact_dev", (h, A, A, 1, A + 8, None, None), INV, REC),  # two faults
        ("gdx_locate_many_search_compact_dev", (h, A, A, 0, A, None, None), OK, ""),  # (no queries: no compact array needed)
        # packed: 2-byte d_packed
        ("gdx_count_many_packed_dev", (h, A + 1, A, 0, A, None, None), INV, "d_packed must be 2-byte aligned"),
        ("gdx_cursors_for_many_queries_packed_dev", (h, A + 1, A, 0, A, A, None, None), INV, "d_packed must be 2-byte aligned"),
        ("gdx_locate_many_search_packed_dev", (h, A + 2, A, 0, None, None), INV, REC),
        ("gdx_locate_many_search_packed_dev", (h, A + 1, A, 0, None, None), INV, "d_packed must be 2-byte aligned"),  # two faults
        # the record side
        ("gdx_locate_many_offsets_capped_dev", (h, None, 0, 0, A, None), INV, REC),
        ("gdx_locate_many_hits_dev", (h, A + 8, 0, A, 0, A, A, None), INV, REC),
        ("gdx_locate_many_hits_compact_dev", (h, None, A, 0, A, 0, A, A, None), INV, REC),
        ("gdx_locate_many_unpack_dev", (h, None, 0, None, None, None), INV, REC),
        ("gdx_locate_many_unpack_dev", (h, A, 0, None, None, None), OK, ""),
        ("gdx_locate_many_unpack_compact_dev", (h, A + 4, A, 0, A, A, None), INV, REC),
        ("gdx_locate_many_totals_compact_dev", (h, A, A, 0, 0, None, A, None), INV, "gdx_locate_many_totals_compact_dev: null argument"),
        ("gdx_locate_many_totals_compact_dev", (h, A, A, 0, 0, A, None, None), INV, "gdx_locate_many_totals_compact_dev: null argument"),
        ("gdx_locate_many_totals_compact_dev", (h, None, A, 0, 0, None, A, None), INV, REC),  # two faults
        ("gdx_locate_many_offsets_hits_compact_dev", (h, A, None, 0, 0, None, A, 0, 0, A, A, None), INV,
         "gdx_locate_many_offsets_hits_compact_dev: null argument"),
        ("gdx_locate_many_offsets_hits_compact_dev", (h, A, None, 0, 0, A, A, 1, 0, None, A, None), INV,
         "gdx_locate_many_offsets_hits_compact_dev: null argument"),
        ("gdx_locate_many_offsets_hits_compact_dev", (h, A, None, 0, 0, A, A, 1, 1, A, None, None), INV,
         "gdx_locate_many_offsets_hits_compact_dev: d_workspace is null"),
        ("gdx_locate_many_offsets32_hits_compact_dev", (h, A, None, 0, 0, A, A, 1 << 32, 0, A, A, None), INV, NARROW),
        ("gdx_locate_many_offsets32_hits_compact_dev", (h, A, None, 0, 0, A, A, 1 << 32, 1, A, None, None), INV, NARROW),  # two faults
        ("gdx_locate_many_search_totals_compact_layout_dev", (h, A, A, 0, None, 0, A, A, None, A, None), INV,
         "gdx_locate_many_search_totals_compact_layout_dev: null argument"),
        ("gdx_locate_many_search_totals_compact_layout_dev", (h, A, A, 1, None, 0, A, None, None, A, None), INV, "d_compact is null"),  # two
        # the one-call step: records, null pointers, offsets width, narrow offsets, totals, and only then the layout
        step(rec=None) + (INV, REC),
        step(scan=None) + (INV, STEP + ": null argument"),
        step(totals=None) + (INV, STEP + ": null argument"),
        step(off=None) + (INV, STEP + ": null argument"),
        step(capacity=1, hits=A) + (INV, STEP + ": null argument"),
        step(width=48) + (INV, WIDTH),
        step(width=32, capacity=1 << 32, hits=A, ws=A) + (INV, NARROW),
        step(totals=A + 4) + (INV, "d_totals must be 8-byte aligned"),
        step(width=48, totals=A + 4) + (INV, WIDTH),  # two faults
        step(width=48, scan=None) + (INV, STEP + ": null argument"),  # two faults
        step(layout_=layout(struct_size=8), totals=A + 4) + (INV, "d_totals must be 8-byte aligned"),  # two faults
        step(layout_=layout(struct_size=8)) + (INV, LSIZE),
        step(qbuf=A + 1) + (INV, QBUF8),
        # the layout, through every entry that takes one
        ("gdx_count_many_layout_dev", (h, A, A, 0, layout(struct_size=8), A, None, None), INV, LSIZE),
        ("gdx_count_many_layout_dev", (h, A, A, 0, layout(struct_size=24), A, None, None), INV, LSIZE),
        ("gdx_count_many_layout_dev", (h, A, A, 0, layout(packed=2), A, None, None), INV, "gdx_query_layout_t.packed must be 0 or 1"),
        ("gdx_count_many_layout_dev", (h, A, A, 0, layout(uniform_len=1 << 21), A, None, None), INV,
         "gdx_query_layout_t.uniform_len must be below 2^21"),
        ("gdx_count_many_layout_dev", (h, A, A, 0, layout(packed=2, uniform_len=1 << 21), A, None, None), INV,
         "gdx_query_layout_t.packed must be 0 or 1"),  # two faults
        ("gdx_count_many_layout_dev", (h, A + 1, A, 0, None, A, None, None), INV, QBUF8),
        ("gdx_count_many_layout_dev", (h, A + 2, A, 0, layout(), A, None, None), INV, QBUF8),
        ("gdx_count_many_layout_dev", (h, A + 1, A, 0, layout(packed=1), A, None, None), INV, "d_qbuf (packed) must be 2-byte aligned"),
        ("gdx_count_many_layout_dev", (h, A + 2, A, 0, layout(packed=1, uniform_len=30), A, None, None), OK, ""),
        ("gdx_cursors_for_many_queries_layout_dev", (h, A + 4, A, 0, None, A, A, None, None), INV, QBUF8),
        ("gdx_locate_many_search_layout_dev", (h, A, A, 0, layout(struct_size=24), A, None), INV, LSIZE),
        ("gdx_locate_many_search_layout_dev", (h, A, A, 0, layout(struct_size=24), None, None), INV, REC),  # two faults
        ("gdx_locate_many_search_compact_layout_dev", (h, A, A, 0, layout(packed=2), A, A, None), INV,
         "gdx_query_layout_t.packed must be 0 or 1"),
        ("gdx_locate_many_search_compact_layout_dev", (h, A, A, 1, layout(packed=2), A, None, None), INV, "d_compact is null"),  # two
        ham(layout(struct_size=8)) + (INV, LSIZE),
        ham(layout(), qoff=None, nq=1) + (INV, "d_qoff is null and the layout is not uniform"),
        ham(None, qoff=None, nq=1) + (INV, "d_qoff is null and the layout is not uniform"),
        ham(layout(), qbuf=A + 1, qoff=None, nq=1) + (INV, QBUF8),  # two faults
        ham(layout(uniform_len=30), qoff=None, nq=1) + (OK, ""),
        # cursor extension
        ("gdx_cursor_extend_front_strings_dev", (h, None, None, A + 1, None, None, 0, None, None, None, None, None, None), INV, QBUF8),
        ("gdx_cursor_extend_front_strings_dev", (h, A, A, A, None, A, 1, None, None, None, None, None, None), INV, "null argument"),
        ("gdx_cursor_extend_front_strings_dev", (h, None, None, A, None, None, 0, None, None, None, A, None, None), INV, COUNTERS),
        ("gdx_cursor_extend_front_strings_dev", (h, None, None, A, None, None, 0, None, A, None, None, None, None), INV, COUNTERS),
        ("gdx_cursor_extend_front_strings_dev", (h, A, A, A, A, A, (1 << 32) - 1, None, A, A, None, None, None), UNS,
         "more than 2^32-2 cursors in one call"),
        ("gdx_cursor_extend_front_strings_dev", (h, A, A, A, A, A, (1 << 32) - 1, None, A, None, None, None, None), INV, COUNTERS),  # two
        ("gdx_cursor_extend_front_chunk_dev", (h, None, None, A + 4, None, 0, 1, 0, None, None, None, None, None, None), INV, QBUF8),
        ("gdx_cursor_extend_front_chunk_dev", (h, A, None, A, A, 1, 1, 0, None, None, None, None, None, None), INV, "null argument"),
        ("gdx_cursor_extend_front_chunk_dev", (h, None, None, A, None, 0, 0, 0, None, None, None, None, None, None), INV,
         "chunk_symbols must be positive"),
        ("gdx_cursor_extend_front_chunk_dev", (h, None, None, A, None, 0, 0, 0, None, None, None, None, A, None), INV,
         "chunk_symbols must be positive"),  # two faults
        ("gdx_cursor_extend_front_chunk_dev", (h, None, None, A, None, 0, 1, 0, None, None, None, None, A, None), INV, COUNTERS),
        ("gdx_cursor_extend_front_chunk_dev", (h, A, A, A, A, (1 << 32) - 1, 1, 0, None, A, A, None, None, None), UNS,
         "more than 2^32-2 cursors in one call"),
        # the secondary stages: the scalars first, then nothing to do, then the pointers
        ("gdx_suffix_segments_many_dev", (h, None, None, 0, 0, 0, None, None, None, None, None, None, None), INV,
         "max_segments must be at least 1"),
        ("gdx_suffix_segments_many_dev", (h, None, None, 0, 1, 2, None, None, None, None, None, None, None), INV, "unknown bit in flags"),
        ("gdx_suffix_segments_many_dev", (h, None, None, 0, 0, 2, None, None, None, None, None, None, None), INV,
         "max_segments must be at least 1"),  # two faults
        ("gdx_suffix_segments_many_dev", (h, None, None, 0, 1, 1, None, None, None, None, None, None, None), OK, ""),
        ("gdx_suffix_segments_many_dev", (h, A + 1, A, 1, 1, 0, None, None, None, None, None, None, None), INV, QBUF8),  # two faults
        ("gdx_suffix_segments_many_dev", (h, A, A, 1, 1, 0, A, A, A, A, None, None, None), INV, "null argument"),
        ("gdx_hamming_many_dev", (h, None, None, 0, None, None, None, None, 0, 1, None, None), OK, ""),
        ("gdx_hamming_many_dev", (h, A, A, 0, None, None, A, A, 1, 1, A, None), INV, "null argument"),
        ("gdx_edit_distance_many_dev", (h, None, None, 0, None, None, None, None, 0, 1, None, None, None), OK, ""),
        ("gdx_edit_distance_many_dev", (h, None, None, 1, layout(uniform_len=8), A, A, A, 1, 1, A, None, None), INV, "d_qbuf is null"),
        ("gdx_best_hits_many_dev", (h, 0, 1) + (None,) * 5 + (0,) + (None,) * 10, OK, ""),
        ("gdx_best_hits_many_dev", (h, 1, 1, A, A, A, None, None, 0) + (A,) * 9 + (None,), INV, "null argument"),
        ("gdx_pair_hits_many_dev", (h, 0, 1) + (None,) * 5 + (0, 0, 0) + (None,) * 12, OK, ""),
        ("gdx_seed_candidates_many_dev", (h, 0, 1) + (None,) * 5 + (1, 0, 1) + (None,) * 9, OK, ""),
        # align: the workspace, before the outputs and the candidates (which are null here)
        ("gdx_align_many_dev", (h, A, A, 0, None, None, None, None, 1, 1, None, None, None, None, None, A, 1, None, None), INV,
         "workspace of 1 bytes, at least %d are needed" % need[0]),
        ("gdx_align_many_dev", (h, A, A, 0, None, None, None, None, 1, 1, None, None, None, None, None, A + 8, need[0], None, None), INV,
         "d_workspace must be 16-byte aligned"),
        ("gdx_align_many_dev", (h, A, A, 0, None, None, None, None, 1, 1, None, None, None, None, None, A, need[0], None, None), INV,
         "null output"),
        ("gdx_align_many_dev", (h, A, A, 0, layout(struct_size=8), None, None, None, 1, 1, None, None, None, None, None, A, 1, None, None),
         INV, LSIZE),  # two faults
        ("gdx_align_many_dev", (h, A, A, 0, None, None, None, None, 0, 1, A, A, A, A, A, A, need[0], None, None), OK, ""),
        # both strands: mode, layout, outputs, the overlap
        ("gdx_strands_expand_dev", (h, A, A, 0, None, 0, None, 3, A + 4096, None, None), INV,
         "mode must be GDX_STRANDS_REVERSE or GDX_STRANDS_BOTH"),
        ("gdx_strands_expand_dev", (h, A, A, 0, layout(struct_size=8), 0, None, 0, A + 4096, None, None), INV,
         "mode must be GDX_STRANDS_REVERSE or GDX_STRANDS_BOTH"),  # two faults
        ("gdx_strands_expand_dev", (h, A, A, 0, layout(struct_size=8), 0, None, 1, A + 4096, None, None), INV, LSIZE),
        ("gdx_strands_expand_dev", (h, A, A, 0, None, 0, None, 1, None, None, None), INV, "null output"),
        ("gdx_strands_expand_dev", (h, A, A, 0, None, 0, None, 2, A + 4096, None, None), INV, "null output"),
        ("gdx_strands_expand_dev", (h, A, A, 0, None, 0, None, 1, A + 4100, None, None), INV, "d_out_qbuf must be 8-byte aligned"),
        ("gdx_strands_expand_dev", (h, A, None, 2, layout(uniform_len=8), 17, None, 1, A + 4096, None, None), INV,
         "a uniform batch of 2 queries of 8 symbols has 16 symbols, not 17"),
        ("gdx_strands_expand_dev", (h, A + 4096, A, 1, None, 8, None, 1, A + 4096, None, None), INV, "d_out_qbuf overlaps d_qbuf"),
        ("gdx_strands_expand_dev", (h, A + 4096, A, 1, None, 8, None, 2, A + 4088, A + 8192, None), INV, "d_out_qbuf overlaps d_qbuf"),
    ]
    for k, (name, args, status, text) in enumerate(cases):
        rc = getattr(lib, name)(*args)
        assert rc == status, (k, name, rc, _lib.last_error())
        if status != OK:
            assert _lib.last_error() == text, (k, name)
    # an index with 64-bit storage: every _dev entry says that it is not for it, before it looks at anything else
    lib.gdx_debug_force_wide(1)
    try:
        w = FmIndexConfig("i64").construct_index([b"ACGTTGCAACGT", b"GGA"], alph.ascii_dna_with_n())
    finally:
        lib.gdx_debug_force_wide(0)
    assert w.info.index_width == 64
    WIDE = ("this call is not available on an index with 64-bit storage (count, cursors_for_many_queries "
            "and locate on host pointers are)")
    for name, args in [("gdx_count_many_dev", (w._h, A + 1, A, 0, A, None, None)),
                       ("gdx_locate_many_search_dev", (w._h, A, A, 0, None, None)),
                       step()[:1] + ((w._h,) + step(width=48)[1][1:],),
                       ("gdx_suffix_segments_many_dev", (w._h, None, None, 0, 0, 0, None, None, None, None, None, None, None))]:
        assert getattr(lib, name)(*args) == UNS, name
        assert _lib.last_error() == WIDE, name
    assert lib.gdx_count_many_dev(None, A, A, 0, A, None, None) == INV and _lib.last_error() == "index handle is null"
    torch.cuda.synchronize()
    assert not bool(buf.any().item())  # nothing was written: no refused call got as far as a launch


def test_save_and_load_round_trip(setup, tmp_path):
    """FmIndex::save_to_file / load_from_file (lib.rs:296-327), own format around the reference's logical arrays."""
    from genedex_amd import FmIndex, GdxError

    _lib, lib, g, c, texts, rng = setup
    path = tmp_path / "index.gdx"
    g.save_to_file(path)
    h = FmIndex.load_from_file(path, alph.ascii_dna_with_n())
    assert h.total_text_len() == g.total_text_len() and h.num_texts() == g.num_texts()
    assert int(h.info.lookup_depth) == 3 and int(h.info.sa_rate) == 4
    qs = [texts[int(rng.integers(0, 3))][s:s + 35] for s in rng.integers(0, 19000, 2000)]
    qs = [q for q in qs if b"N" not in q[-3:]] + [b"", b"ACGTTGCA"]
    a = g.locate_raw(*pack_queries(qs))
    b = h.locate_raw(*pack_queries(qs))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert np.array_equal(h.export_bwt(), g.export_bwt())
    # a truncated or foreign file is an error, not a crash
    data = path.read_bytes()
    (tmp_path / "short.gdx").write_bytes(data[: len(data) // 2])
    (tmp_path / "junk.gdx").write_bytes(b"not an index" * 100)
    for name in ("short.gdx", "junk.gdx", "missing.gdx"):
        with pytest.raises(GdxError):
            FmIndex.load_from_file(tmp_path / name, alph.ascii_dna_with_n())


@pytest.mark.parametrize("chunk_queries,chunk_bytes", [(777, 0), (0, 4096), (1, 0)])
def test_host_calls_are_chunk_invariant(chunk_queries, chunk_bytes):
    """The host-pointer calls run as a pipeline over chunks (host_api.hip); chunk boundaries must be invisible:
    same counts, intervals, hit offsets and hits as the oracle whatever the chunk size, including a query longer
    than a chunk, empty queries, the sizing call, a too-small buffer and the allocating variant."""
    from genedex_amd import GdxError, _lib

    lib = _lib.load()
    rng = np.random.default_rng(77)
    a = alph.ascii_dna_with_n()
    texts = random_texts(rng, len_max=30000, symbols=b"ACGT")
    from genedex_amd import FmIndexConfig

    g = FmIndexConfig("u32").suffix_array_sampling_rate(3).lookup_table_depth(2).construct_index(texts, a)
    c = OracleIndex.build(texts, a.io_to_dense_table, 6, 4, sa_rate=3, lookup_depth=2, width=32)
    qs = [texts[0][10:10 + int(n)] for n in rng.integers(0, 90, 5000)] + [b"", texts[0][5:9000], b"ACGTTTGAC", b""]
    qs += [bytes(b"ACGT"[i] for i in rng.integers(0, 4, int(n))) for n in rng.integers(0, 40, 3000)]
    if chunk_queries == 1:
        qs = qs[:300] + qs[-300:]
    qbuf, qoff = pack_queries(qs)
    cs, ce = c.cursors_for_many(qbuf, qoff)
    co, ct, cp = c.locate_many(qs)
    lib.gdx_debug_set_host_chunking(chunk_queries, chunk_bytes)
    try:
        s, e, st = g.cursors_raw(qbuf, qoff)
        assert s.tolist() == cs.tolist() and e.tolist() == ce.tolist() and not st.any()
        counts, _ = g.count_raw(qbuf, qoff)
        assert counts.tolist() == (ce - cs).tolist()
        off, t, p, _ = g.locate_raw(qbuf, qoff)  # sizing call + fill
        assert off.tolist() == co.tolist() and t.tolist() == ct.tolist() and p.tolist() == cp.tolist()
        off2, t2, p2, _ = g.locate_alloc_raw(qbuf, qoff)  # one pass, library-owned buffer
        assert off2.tolist() == co.tolist() and t2.tolist() == ct.tolist() and p2.tolist() == cp.tolist()
        # a buffer that is too small: GDX_ERR_CAPACITY, the required size and the offsets are still reported
        nq = qoff.size - 1
        offs = np.zeros(nq + 1, dtype=np.uint64)
        small = np.zeros((int(co[-1]) // 2, 2), dtype=np.uint64)
        total = C.c_uint64(0)
        rc = lib.gdx_locate_many(g._h, qbuf.ctypes.data_as(_lib.u8p), qoff.ctypes.data_as(_lib.u64p), nq,
                                 offs.ctypes.data_as(_lib.u64p), small.ctypes.data_as(C.POINTER(_lib.HitStruct)),
                                 small.shape[0], C.byref(total), None)
        assert rc == _lib.GDX_ERR_CAPACITY and total.value == int(co[-1]) and offs.tolist() == co.tolist()
        # a bad symbol somewhere in the middle: its status alone is set, everything else stays valid
        bad = list(qs)
        bad[len(bad) // 2] = b"AC?T"
        bb, bo = pack_queries(bad)
        with pytest.raises(GdxError):
            g.count_raw(bb, bo)
        counts_b, st_b = g.count_raw(bb, bo, strict=False)
        assert st_b[len(bad) // 2] == _lib.GDX_Q_INVALID_SYMBOL and int(st_b.sum()) == _lib.GDX_Q_INVALID_SYMBOL
        keep = np.arange(nq) != len(bad) // 2
        assert counts_b[keep].tolist() == (ce - cs)[keep].tolist()
    finally:
        lib.gdx_debug_set_host_chunking(0, 0)


@pytest.mark.parametrize("mode", ["host-pack", "no-host-pack", "hit-limit", "uniform"])
def test_host_ascii_calls_pack_on_the_host(mode, monkeypatch):
    """ASCII batches of gdx_count_many / gdx_locate_many[_alloc] cross the link as 2-bit codes made by the pipeline's own workers,
    chunk by chunk (host_api.hip, pack_host.hpp); a chunk that holds a symbol 2 bits cannot name (N, an invalid byte) goes as
    ASCII.  Whatever a chunk went as, counts, statuses, offsets and hits are the oracle's -- with chunks small enough that both
    kinds occur, with packing switched off (GDX_HOST_PACK=0), with the batch declared uniform, and when a chunk's hits exceed
    what the fused step's 32-bit offsets hold (GDX_TEST_CHUNK_HIT_LIMIT stands in for 2^32 - 1: the wide call then runs again
    with 64-bit offsets instead of failing -- round-5 advisor)."""
    from genedex_amd import FmIndexConfig, _lib

    lib = _lib.load()
    rng = np.random.default_rng(1234)
    a = alph.ascii_dna_with_n()
    texts = [bytes(b"ACGTN"[i] for i in rng.choice(5, int(n), p=[0.2475, 0.2475, 0.2475, 0.2475, 0.01])) for n in (30000, 9000, 17000)]
    g = FmIndexConfig("u32").suffix_array_sampling_rate(4).construct_index(texts, a)
    c = OracleIndex.build(texts, a.io_to_dense_table, 6, 4, sa_rate=4, lookup_depth=0, width=32)
    if mode == "uniform":
        qs = [texts[0][int(p):int(p) + 40] for p in rng.integers(0, 29000, 6000)]  # (one in three holds an N)
    else:
        qs = [texts[int(t)][int(p):int(p) + int(n)] for t, p, n in zip(rng.integers(0, 3, 6000), rng.integers(0, 8000, 6000),
                                                                         rng.integers(0, 120, 6000))]
        qs += [b"", b"A", b"ACGTNNACGT", texts[1][100:4000]]
        qs += [bytes(b"ACGT"[i] for i in rng.integers(0, 4, int(n))) for n in rng.integers(1, 60, 2000)]
    qbuf, qoff = pack_queries(qs)
    nq = qoff.size - 1
    cs, ce = c.cursors_for_many(qbuf, qoff)
    co, ct, cp = c.locate_intervals(cs, ce)
    n_with_other = sum(1 for q in qs if any(ch not in b"ACGT" for ch in q))
    assert 100 < n_with_other < nq - 100  # chunks of both kinds
    if mode == "no-host-pack":
        monkeypatch.setenv("GDX_HOST_PACK", "0")
    if mode == "hit-limit":
        monkeypatch.setenv("GDX_TEST_CHUNK_HIT_LIMIT", "50")
    lib.gdx_debug_set_host_chunking(64 if mode != "hit-limit" else 512, 0)
    try:
        if mode == "uniform":
            counts, st = g.count_layout_raw(qbuf, None, nq, uniform_len=40)
            off, t, p, st2 = g.locate_layout_raw(qbuf, None, nq, uniform_len=40)
        else:
            counts, st = g.count_raw(qbuf, qoff)
            off, t, p, st2 = g.locate_alloc_raw(qbuf, qoff)
            off3, t3, p3, _ = g.locate_raw(qbuf, qoff)  # sizing call (offsets and total only) + fill
            assert off3.tolist() == co.tolist() and t3.tolist() == ct.tolist() and p3.tolist() == cp.tolist(), mode
        assert not st.any() and not st2.any()
        assert counts.tolist() == (ce - cs).tolist(), mode
        assert off.tolist() == co.tolist() and t.tolist() == ct.tolist() and p.tolist() == cp.tolist(), mode
    finally:
        lib.gdx_debug_set_host_chunking(0, 0)


def test_multi_handle_shards_equal_single_gpu(setup):
    """gdx_multi_*: replicas behind one handle (here: three replicas on the one GPU of the box), the batch cut into
    contiguous shards, one host thread and pipeline per replica; the output is bit for bit the one-handle output."""
    _lib, lib, g, c, texts, rng = setup
    a = alph.ascii_dna_with_n()
    tbuf, toff = pack_queries(texts)
    tab = np.ascontiguousarray(a.io_to_dense_table, dtype=np.uint8)
    devs = (C.c_int * 3)(0, 0, 0)
    m = C.c_void_p()
    _lib.check(lib.gdx_multi_build(tbuf.ctypes.data_as(_lib.u8p), toff.ctypes.data_as(_lib.u64p), len(texts),
                                   tab.ctypes.data_as(_lib.u8p), 6, 4, 4, 3, 32, devs, 3, None, C.byref(m)))
    try:
        assert lib.gdx_multi_replicas(m) == 3
        qs = [texts[int(rng.integers(0, 3))][s:s + int(rng.integers(0, 70))] for s in rng.integers(0, 19000, 4001)]
        qs = [q for q in qs if b"N" not in q[-3:]] + [b"", b"ACGT"]
        qbuf, qoff = pack_queries(qs)
        nq = qoff.size - 1
        cs, ce = c.cursors_for_many(qbuf, qoff)
        co, ct, cp = c.locate_many(qs)
        s_ = np.zeros(nq, dtype=np.uint64)
        e_ = np.zeros(nq, dtype=np.uint64)
        st = np.zeros(nq, dtype=np.uint8)
        _lib.check(lib.gdx_multi_cursors_for_many_queries(m, qbuf.ctypes.data_as(_lib.u8p), qoff.ctypes.data_as(_lib.u64p),
                                                          nq, s_.ctypes.data_as(_lib.u64p), e_.ctypes.data_as(_lib.u64p),
                                                          st.ctypes.data_as(_lib.u8p)))
        assert s_.tolist() == cs.tolist() and e_.tolist() == ce.tolist() and not st.any()
        cnt = np.zeros(nq, dtype=np.uint64)
        _lib.check(lib.gdx_multi_count_many(m, qbuf.ctypes.data_as(_lib.u8p), qoff.ctypes.data_as(_lib.u64p), nq,
                                            cnt.ctypes.data_as(_lib.u64p), None))
        assert cnt.tolist() == (ce - cs).tolist()
        off = np.zeros(nq + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        ptr = C.POINTER(_lib.HitStruct)()
        _lib.check(lib.gdx_multi_locate_many_alloc(m, qbuf.ctypes.data_as(_lib.u8p), qoff.ctypes.data_as(_lib.u64p), nq,
                                                   off.ctypes.data_as(_lib.u64p), C.byref(ptr), C.byref(total), None))
        n = total.value
        hits = np.ctypeslib.as_array(C.cast(ptr, _lib.u64p), shape=(2 * n,)).reshape(n, 2).copy()
        lib.gdx_free_hits(ptr)
        assert off.tolist() == co.tolist() and hits[:, 0].tolist() == ct.tolist() and hits[:, 1].tolist() == cp.tolist()
    finally:
        lib.gdx_multi_free(m)


def test_locate_takes_at_most_max_hits_per_query():
    """gdx_query_options_t.max_hits_per_query: the host-pointer locate calls return the first k hits of a query in
    suffix-array order -- locate(q).take(k) on the reference's lazy iterator (lib.rs:187-197) -- so one poly-A read does
    not materialise every occurrence.  Counts stay the reference's; hit_offsets count the hits returned."""
    from genedex_amd import FmIndexConfig, _lib

    lib = _lib.load()
    rng = np.random.default_rng(99)
    a = alph.ascii_dna_with_n()
    body = bytes(b"ACGT"[i] for i in rng.integers(0, 4, 30000))
    texts = [body[:15000] + b"A" * 60000 + body[15000:], b"A" * 5000 + body[:2000], body[100:9000]]
    g = FmIndexConfig("u32").construct_index(texts, a)
    c = OracleIndex.build(texts, a.io_to_dense_table, 6, 4, sa_rate=4, lookup_depth=0, width=32)
    qs = [b"A" * 20, body[200:260], b"A" * 50, body[5000:5030], b"AAAAAAAAAAAAAAAAAAAC", b"A" * 16, b""]
    qs += [body[s:s + 40] for s in rng.integers(0, 29000, 300)]
    qbuf, qoff = pack_queries(qs)
    cs, ce = c.cursors_for_many(qbuf, qoff)
    assert int((ce - cs)[0]) > 60000
    for k in (1, 7, 100, 100000):
        g.set_query_options(max_hits_per_query=k)
        take = np.minimum(ce - cs, k)
        co, ct, cp = c.locate_intervals(cs, cs + take)
        for call in (g.locate_raw, g.locate_alloc_raw):
            off, t, p, st = call(qbuf, qoff)
            assert not st.any()
            assert off.tolist() == co.tolist() and t.tolist() == ct.tolist() and p.tolist() == cp.tolist(), (k, call.__name__)
        counts, _ = g.count_raw(qbuf, qoff)  # counting is not limited
        assert counts.tolist() == (ce - cs).tolist()
    g.set_query_options()
    off, t, p, _ = g.locate_alloc_raw(qbuf, qoff)
    co, ct, cp = c.locate_intervals(cs, ce)
    assert off.tolist() == co.tolist() and t.tolist() == ct.tolist() and p.tolist() == cp.tolist()
    # the same limit through the multi handle (every replica takes the option)
    tbuf, toff = pack_queries(texts)
    tab = np.ascontiguousarray(a.io_to_dense_table, dtype=np.uint8)
    devs = (C.c_int * 2)(0, 0)
    m = C.c_void_p()
    _lib.check(lib.gdx_multi_build(tbuf.ctypes.data_as(_lib.u8p), toff.ctypes.data_as(_lib.u64p), len(texts),
                                   tab.ctypes.data_as(_lib.u8p), 6, 4, 4, 0, 32, devs, 2, None, C.byref(m)))
    try:
        o = _lib.QueryOptions()
        lib.gdx_query_options_init(C.byref(o))
        o.max_hits_per_query = 9
        _lib.check(lib.gdx_multi_set_query_options(m, C.byref(o)))
        nq = qoff.size - 1
        off = np.zeros(nq + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        ptr = C.POINTER(_lib.HitStruct)()
        _lib.check(lib.gdx_multi_locate_many_alloc(m, qbuf.ctypes.data_as(_lib.u8p), qoff.ctypes.data_as(_lib.u64p), nq,
                                                   off.ctypes.data_as(_lib.u64p), C.byref(ptr), C.byref(total), None))
        n = total.value
        hits = np.ctypeslib.as_array(C.cast(ptr, _lib.u64p), shape=(2 * n,)).reshape(n, 2).copy()
        lib.gdx_free_hits(ptr)
        co, ct, cp = c.locate_intervals(cs, cs + np.minimum(ce - cs, 9))
        assert off.tolist() == co.tolist() and hits[:, 0].tolist() == ct.tolist() and hits[:, 1].tolist() == cp.tolist()
    finally:
        lib.gdx_multi_free(m)


def test_query_options_struct_may_be_shorter_than_the_library_knows():
    """struct_size lets gdx_query_options_t grow: a caller built against an older header passes a shorter struct and the
    fields it does not know keep their defaults."""
    from genedex_amd import FmIndexConfig, _lib

    lib = _lib.load()
    g = FmIndexConfig("u32").construct_index([b"ACGTACGTTTGA"], alph.ascii_dna())
    o = _lib.QueryOptions()
    lib.gdx_query_options_init(C.byref(o))
    o.search_fast = 0
    o.max_hits_per_query = 5          # beyond the size the caller declares: must be ignored
    o.struct_size = 9 * 4             # the round-2 struct: struct_size + eight int32 fields
    _lib.check(lib.gdx_index_set_query_options(g._h, C.byref(o)))
    back = _lib.QueryOptions()
    _lib.check(lib.gdx_index_get_query_options(g._h, C.byref(back)))
    assert back.search_fast == 0 and back.max_hits_per_query == 0


def _gather_dev_case(n_replicas, devices, expect_rccl=None):
    """gdx_multi_locate_many_gather_dev: every replica locates the shard that sits in its own HBM, counts and hits are
    gathered on the root's device; the result must be the one-handle output of the concatenated batch."""
    import torch

    from genedex_amd import FmIndexConfig, _lib

    lib = _lib.load()
    rng = np.random.default_rng(314)
    a = alph.ascii_dna_with_n()
    texts = [bytes(b"ACGTN"[i] for i in rng.choice(5, 30000, p=[.2475, .2475, .2475, .2475, .01])) for _ in range(3)]
    c = OracleIndex.build(texts, a.io_to_dense_table, 6, 4, sa_rate=4, lookup_depth=0, width=32)
    tbuf, toff = pack_queries(texts)
    tab = np.ascontiguousarray(a.io_to_dense_table, dtype=np.uint8)
    devs = (C.c_int * n_replicas)(*devices)
    m = C.c_void_p()
    _lib.check(lib.gdx_multi_build(tbuf.ctypes.data_as(_lib.u8p), toff.ctypes.data_as(_lib.u64p), len(texts),
                                   tab.ctypes.data_as(_lib.u8p), 6, 4, 4, 0, 32, devs, n_replicas, None, C.byref(m)))
    try:
        qs = [texts[int(rng.integers(0, 3))][s:s + int(rng.integers(1, 70))] for s in rng.integers(0, 29000, 5000)]
        qs = [q for q in qs if b"N" not in q] + [b"", b"ACGT", b"A"]
        co, ct, cp = c.locate_many(qs)
        cs, ce = c.cursors_for_many(*pack_queries(qs))
        bounds = [len(qs) * r // n_replicas for r in range(n_replicas + 1)]
        shards = (_lib.DeviceShard * n_replicas)()
        keep = []
        for r in range(n_replicas):
            qb, qo = pack_queries(qs[bounds[r]:bounds[r + 1]])
            pad = np.zeros((qb.size + 16) // 8 * 8 + 8, dtype=np.uint8)
            pad[:qb.size] = qb
            d = torch.device("cuda", devices[r])
            tq, to = torch.from_numpy(pad).to(d), torch.from_numpy(qo.astype(np.int64)).to(d)
            keep += [tq, to]
            shards[r] = _lib.DeviceShard(tq.data_ptr(), to.data_ptr(), qo.size - 1)
        for root in sorted({0, n_replicas - 1}):
            out = _lib.Gathered()
            _lib.check(lib.gdx_multi_locate_many_gather_dev(m, shards, n_replicas, root, C.byref(out)))
            assert out.nq == len(qs) and out.total_hits == int(co[-1]) and out.device_id == devices[root]
            assert out.used_rccl == ((1 if len(set(devices)) > 1 else 0) if expect_rccl is None else expect_rccl)
            d = torch.device("cuda", out.device_id)

            class _Dev:  # a library-owned device buffer as a zero-copy torch tensor (__cuda_array_interface__)
                def __init__(self, ptr, shape, typestr):
                    self.__cuda_array_interface__ = {"data": (int(ptr), False), "shape": shape, "typestr": typestr, "version": 2}

            with torch.cuda.device(d):
                torch.cuda.synchronize()
                counts = torch.as_tensor(_Dev(out.d_counts, (out.nq,), "<i4"), device=d).clone()
                offs = torch.as_tensor(_Dev(out.d_hit_offsets, (out.nq + 1,), "<i8"), device=d).clone()
                hits = torch.as_tensor(_Dev(out.d_hits, (max(out.total_hits, 1), 2), "<i4"), device=d).clone()
                stat = torch.as_tensor(_Dev(out.d_status, (out.nq,), "|u1"), device=d).clone()
                torch.cuda.synchronize()
            assert (counts.cpu().numpy().astype(np.uint64) & 0xFFFFFFFF).tolist() == (ce - cs).tolist()
            assert offs.cpu().numpy().astype(np.uint64).tolist() == co.tolist()
            h = hits[: out.total_hits].cpu().numpy().astype(np.uint32)
            assert h[:, 0].tolist() == ct.tolist() and h[:, 1].tolist() == cp.tolist()
            assert not stat.any().item()
    finally:
        lib.gdx_multi_free(m)


def test_multi_gather_dev_three_replicas_on_one_device():
    _gather_dev_case(3, [0, 0, 0])


def test_multi_gather_dev_rccl_branch_through_a_recording_shim(tmp_path):
    """The RCCL branch of gdx_multi_locate_many_gather_dev (multi.hip: one group of ncclSend / ncclRecv per shard and array) has
    never met two GPUs.  Here it runs on ONE: tests/rccl_shim is loaded in librccl.so's place (GDX_RCCL_LIBRARY), replicas that
    share the device are made to exchange through it (GDX_MULTI_FORCE_RCCL), the shim pairs every receive with its send as RCCL
    would -- same peer, element count and type, or it fails -- moves the bytes, and records every call.  The gathered counts,
    offsets and hits must be the oracle's (checked in the child process by the same code as the plain test), and the record
    must show the sizes and destinations the shards call for: per non-root replica three sends to the root and three
    receives from it, counts as u32 at the shard's query base, statuses as bytes, hits as 2 u32 each at its hit base."""
    import subprocess
    import sys

    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shim = tmp_path / "librccl_shim.so"
    build = subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-shared", "-fPIC", "--offload-arch=gfx950",
                            os.path.join(root_dir, "tests", "rccl_shim", "rccl_shim.cpp"), "-o", str(shim)],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    log = tmp_path / "shim.log"
    env = dict(os.environ, GDX_RCCL_LIBRARY=str(shim), GDX_MULTI_FORCE_RCCL="1", GDX_RCCL_SHIM_LOG=str(log))
    code = ("import sys; sys.path.insert(0, 'tests'); import test_gpu_api_contract as t; "
            "t._gather_dev_case(3, [0, 0, 0], expect_rccl=1); print('child ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=root_dir, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    lines = log.read_text().splitlines()
    assert lines[0].startswith("init 3 ranks")
    ops = [ln.split() for ln in lines if ln.startswith(("send", "recv"))]
    # two calls (root 0, then root 2), each: 2 non-root replicas x 3 arrays x (send + recv)
    assert len(ops) == 2 * 2 * 3 * 2
    for call, root in enumerate((0, 2)):
        mine = ops[call * 12:(call + 1) * 12]
        sends = [o for o in mine if o[0] == "send"]
        recvs = [o for o in mine if o[0] == "recv"]
        assert all(int(o[3]) == root for o in sends) and all(int(o[1]) == root for o in recvs)
        base = {}
        for s_, r_ in zip(sends, recvs):
            assert s_[1] == r_[3] and s_[4:6] == r_[4:6]  # the same peer, element count and type on both sides
        for rep_ in sorted({int(o[1]) for o in sends}):
            cnt, st, hit = [o for o in sends if int(o[1]) == rep_]
            assert cnt[5] == "3" and st[5] == "1" and hit[5] == "3" and cnt[4] == st[4] and int(hit[4]) % 2 == 0
            base[rep_] = (int(cnt[4]), int(hit[4]) // 2)
            rc, rs, rh = [o for o in recvs if int(o[3]) == rep_]
            base[rep_] += (int(rc[6], 16), int(rs[6], 16), int(rh[6], 16))
        # destinations: shard r lands behind the shards before it -- between two senders the counts move on by 4 bytes per query
        # of what lies between them, statuses by 1, hits by 8 per hit
        a, b = sorted(base)
        assert b == a + 1
        nq_between, hits_between = base[a][0], base[a][1]  # (shard a is what lies between where a and a + 1 land)
        assert base[b][2] - base[a][2] == 4 * nq_between and base[b][3] - base[a][3] == nq_between
        assert base[b][4] - base[a][4] == 8 * hits_between


def test_multi_gather_dev_over_rccl():
    """The same with one replica per GPU: the transfers are ncclSend / ncclRecv over xGMI.  Needs two GPUs."""
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL point-to-point between devices)")
    n = min(torch.cuda.device_count(), 4)
    _gather_dev_case(n, list(range(n)))


@pytest.mark.parametrize("depth", [0, 3])
def test_partitioned_index_equals_one_index_on_counts_and_hit_sets(depth):
    """gdx_parts_*: a collection cut at text borders into several 32-bit indexes (what stands in for the reference's
    IndexStorage = i64 beyond 2^32 - 1 symbols).  Counts, statuses and hit SETS equal the oracle's single index over the
    whole collection; hits come part after part, suffix-array order inside a part."""
    from genedex_amd import GdxError, PartitionedFmIndex, _lib

    rng = np.random.default_rng(4242 + depth)
    a = alph.ascii_dna_with_n()
    texts = [bytes(b"ACGTN"[i] for i in rng.choice(5, int(rng.integers(0, 4000)), p=[.2475, .2475, .2475, .2475, .01]))
             for _ in range(23)]
    c = OracleIndex.build(texts, a.io_to_dense_table, 6, 4, sa_rate=4, lookup_depth=depth, width=64)
    g = PartitionedFmIndex.construct(texts, a, sa_rate=4, lookup_depth=depth, max_part_symbols=9000)
    assert g.num_parts >= 4 and g.num_texts() == len(texts) and g.total_text_len() == c.n
    qs = [texts[int(rng.integers(0, 23))] for _ in range(3)]  # whole texts as queries
    for _ in range(2500):
        t = texts[int(rng.integers(0, 23))]
        if len(t):
            pos = int(rng.integers(0, len(t)))
            qs.append(t[pos:pos + int(rng.integers(0, 40))])
        qs.append(bytes(b"ACGT"[i] for i in rng.integers(0, 4, int(rng.integers(0, 12)))))
    qs += [b"ACXGT", b"", b"NNN", b"GATTACA" * 3]
    qbuf, qoff = pack_queries(qs)
    cs, ce, cst = c.cursors_single(qbuf, qoff)
    counts, st = g.count_raw(qbuf, qoff, strict=False)
    assert st.tolist() == cst.tolist()
    ok = cst == 0
    assert counts[ok].tolist() == (ce - cs)[ok].tolist() and not counts[~ok].any()
    off, t, p, st2 = g.locate_raw(qbuf, qoff, strict=False)
    assert st2.tolist() == cst.tolist()
    co, ct, cp = c.locate_intervals(np.where(ok, cs, 0), np.where(ok, ce, 0))
    assert off.tolist() == co.tolist()
    for k in range(len(qs)):
        got = sorted(zip(t[off[k]:off[k + 1]].tolist(), p[off[k]:off[k + 1]].tolist()))
        want = sorted(zip(ct[co[k]:co[k + 1]].tolist(), cp[co[k]:co[k + 1]].tolist()))
        assert got == want, qs[k]
    # gdx_query_options_t.max_hits_per_query = k: locate(q).take(k) of the WHOLE collection -- the first k hits in part order,
    # not k per part; hit_offsets counts the hits returned
    g.set_query_options(max_hits_per_query=2)
    off_k, t_k, p_k, _ = g.locate_raw(qbuf, qoff, strict=False)
    assert np.diff(off_k).tolist() == np.minimum(np.diff(off), 2).tolist() and int(np.diff(off).max()) > 2 * g.num_parts
    for k in range(len(qs)):
        n_k = int(off_k[k + 1] - off_k[k])
        assert list(zip(t_k[off_k[k]:off_k[k + 1]].tolist(), p_k[off_k[k]:off_k[k + 1]].tolist())) == \
            list(zip(t[off[k]:off[k] + n_k].tolist(), p[off[k]:off[k] + n_k].tolist()))
    g.set_query_options()
    with pytest.raises(TypeError):  # (setattr on the ctypes struct would have taken any name and changed nothing)
        g.set_query_options(max_hits_per_querry=2)
    with pytest.raises(GdxError) as e:  # a single text must fit one part
        PartitionedFmIndex.construct([b"ACGT" * 5000, b"ACGT"], a, max_part_symbols=9000)
    assert e.value.status == _lib.GDX_ERR_TEXT_TOO_LONG
    one = PartitionedFmIndex.construct(texts, a, sa_rate=4, lookup_depth=depth)  # everything fits one part
    assert one.num_parts == 1
    off1, t1, p1, _ = one.locate_raw(qbuf, qoff, strict=False)
    assert off1.tolist() == co.tolist() and t1.tolist() == ct.tolist() and p1.tolist() == cp.tolist()


@pytest.mark.parametrize("build", [dict(), dict(jump_entry_bytes=32), dict(jump_entry_bytes=16), dict(pair_lines=False, jump_entry_bytes=0, top_table_depth=7,
                                                                           full_suffix_array=True, text_units=True),
                                   dict(pair_lines=False, jump_entry_bytes=0, top_table_depth=5, text_units=True)])
def test_the_whole_step_in_one_call(build):
    """gdx_locate_many_step_compact_layout_dev on the library's default shape and on indexes WITHOUT a seed table (records only,
    and with a compact array whose every word says "see the record"): search, totals, offsets and hits enqueued by one call, no host round trip -- the same
    offsets and hits as the oracle, for indexes with SA[row] at hand (32-byte entries, full suffix array: the stream kernel)
    and without (the queue kernel walks), with a hit buffer that is large enough and one that is too small (the totals tell,
    the offsets are right, what fits is stored)."""
    import torch

    from genedex_amd import FmIndexConfig
    from genedex_amd.device import DeviceEngine, DeviceQueries

    rng = np.random.default_rng(808)
    a = alph.ascii_dna_with_n()
    body = bytes(b"ACGT"[i] for i in rng.integers(0, 4, 40000))
    texts = [body[:30000], body[5000:9000] + b"NNNN" + body[100:3000], b"A" * 300 + body[200:6000]]
    g = FmIndexConfig("u32").acceleration_structures(**build).construct_index(texts, a)
    c = OracleIndex.build(texts, a.io_to_dense_table, 6, 4, sa_rate=4, lookup_depth=0, width=32)
    qs = [body[s:s + int(rng.integers(16, 70))] for s in rng.integers(0, 39000, 5000)]
    qs += [bytes(b"ACGT"[i] for i in rng.integers(0, 4, 20)) for _ in range(500)] + [b"A" * 20, b"", b"ACGTNACG"]
    qbuf, qoff = pack_queries(qs)
    co, ct, cp = c.locate_many(qs)
    dq = DeviceQueries.from_host(qbuf, qoff)
    eng = DeviceEngine(g)
    nq = dq.nq
    total = int(co[-1])
    for with_compact in (False, True):
        for capacity in (total + 7, total // 2):
            for dt in (torch.int64, torch.int32):
                rec = eng.alloc_records(nq)
                cw = eng.alloc_compact(nq) if with_compact else None
                off = torch.full((nq + 1,), -1, dtype=dt, device="cuda")
                hits = torch.full((max(capacity, 1), 2), -1, dtype=torch.int32, device="cuda")
                totals = torch.full((2,), -1, dtype=torch.int64, device="cuda")
                sws = torch.empty(max(eng.totals_workspace_bytes(nq), 16), dtype=torch.uint8, device="cuda")
                ws = torch.empty(max(eng.locate_workspace_bytes(hits.shape[0]), 16), dtype=torch.uint8, device="cuda")
                eng.locate_step(dq, rec, cw, sws, totals, off, hits, ws)
                torch.cuda.synchronize()
                tot = int(totals[0].item())
                assert tot == total and off.cpu().numpy().astype(np.uint64).tolist() == co.tolist(), (build, with_compact, capacity)
                if with_compact:
                    if build:  # no seed table: every word says "see"
                        assert int(totals[1].item()) == total and bool((cw[:nq] == -2).all().item())
                    else:      # the default shape has one: most reads are answered by their compact word
                        assert int(totals[1].item()) < total and int((cw[:nq] == -2).sum().item()) < nq // 2
                n = min(tot, capacity)
                h = hits[:n].cpu().numpy().astype(np.uint32)
                assert h[:, 0].tolist() == ct[:n].astype(np.uint32).tolist() and h[:, 1].tolist() == cp[:n].astype(np.uint32).tolist(), \
                    (build, with_compact, capacity)
                if tot > capacity:  # the caller finishes the step with a buffer of the size the totals name
                    hits = torch.empty((tot, 2), dtype=torch.int32, device="cuda")
                    ws = torch.empty(max(eng.locate_workspace_bytes(tot), 16), dtype=torch.uint8, device="cuda")
                    eng.locate_offsets_hits(rec, nq, sws, off, tot, int(totals[1].item()), hits, ws, compact=cw)
                    torch.cuda.synchronize()
                    h = hits.cpu().numpy().astype(np.uint32)
                    assert h[:, 0].tolist() == ct.astype(np.uint32).tolist() and h[:, 1].tolist() == cp.astype(np.uint32).tolist()


@pytest.mark.parametrize("seed", range(4))
def test_wide_index_equals_oracle_i64(seed):
    """Index storage beyond 32 bits (wide.hip; the reference's IndexStorage for i64): the 64-bit engine forced onto small
    inputs -- suffix sorter by plain prefix doubling on 64-bit ranks, u64 superblock offsets and samples -- must give the
    oracle's BWT, intervals (also frozen empty ones), statuses, counts and hits in the oracle's order."""
    from genedex_amd import FmIndexConfig, GdxError, _lib

    lib = _lib.load()
    rng = np.random.default_rng(9100 + seed)
    a = alph.ascii_dna_with_n()
    if seed == 0:
        texts = random_texts(rng, len_max=30000, symbols=b"ACGTN")
    elif seed == 1:  # repeats: many doubling rounds
        unit = bytes(b"ACGT"[i] for i in rng.integers(0, 4, 301))
        texts = [unit * 40, b"A" * 3000, unit[:100] * 7, b""]
    elif seed == 2:  # more than one superblock, sentinels inside
        texts = [bytes(b"ACGTN"[i] for i in rng.choice(5, 70000, p=[.2475, .2475, .2475, .2475, .01])) for _ in range(3)]
    else:
        texts = [b"", b"A", b"ACGT", b"", b"NNNN", bytes(b"ACGT"[i] for i in rng.integers(0, 4, 5000))]
    rate = [4, 1, 7, 3][seed]
    c = OracleIndex.build(texts, a.io_to_dense_table, 6, 4, sa_rate=rate, lookup_depth=0, width=64)
    lib.gdx_debug_force_wide(1)
    try:
        g = FmIndexConfig("i64").suffix_array_sampling_rate(rate).construct_index(texts, a)
    finally:
        lib.gdx_debug_force_wide(0)
    assert g.info.index_width == 64 and g.total_text_len() == c.n and g.num_texts() == len(texts)
    assert g.export_bwt().tobytes() == c.bwt.tobytes()
    qs = [b"", b"A", b"ACXGT", b"NN", b"TNA"]
    for _ in range(1500):
        t = texts[int(rng.integers(0, len(texts)))]
        if len(t):
            pos = int(rng.integers(0, len(t)))
            qs.append(t[pos:pos + int(rng.integers(0, 60))])
        qs.append(bytes(b"ACGTN"[i] for i in rng.integers(0, 5, int(rng.integers(0, 12)))))
    qbuf, qoff = pack_queries(qs)
    s, e, st = g.cursors_raw(qbuf, qoff, strict=False)
    cs, ce, cst = c.cursors_single(qbuf, qoff)
    assert st.tolist() == cst.tolist()
    ok = st == 0
    assert s[ok].tolist() == cs[ok].tolist() and e[ok].tolist() == ce[ok].tolist()
    counts, _ = g.count_raw(qbuf, qoff, strict=False)
    assert counts[ok].tolist() == (ce - cs)[ok].tolist()
    small = ok & ((ce - cs) < 5000)
    keep = [q for q, k in zip(qs, small) if k]
    kb, ko = pack_queries(keep)
    co, ct, cp = c.locate_intervals(cs[small], ce[small])
    for call in (g.locate_raw, g.locate_alloc_raw):
        off, t_, p_, _ = call(kb, ko)
        assert off.tolist() == co.tolist() and t_.tolist() == ct.tolist() and p_.tolist() == cp.tolist()
    assert g.cursor_empty().interval() == (0, c.n)
    # Cursor::extend_query_front one symbol at a time, Cursor::locate, and the operator level (rank / symbol_at)
    m = 300
    starts, ends = np.zeros(m, dtype=np.uint64), np.full(m, c.n, dtype=np.uint64)
    want = [(0, c.n)] * m
    for step in range(8):
        syms = np.frombuffer(bytes(b"ACGTNacgt"[i] for i in rng.integers(0, 9, m)), dtype=np.uint8)
        starts, ends, st2 = g.extend_front_raw(starts, ends, syms)
        want = [c.extend_front(s_, e_, int(sym))[:2] for (s_, e_), sym in zip(want, syms)]
        assert not st2.any() and list(zip(starts.tolist(), ends.tolist())) == want
    few = (ends - starts) < 3000
    off, t_, p_ = g.locate_intervals_raw(starts[few], ends[few])
    co, ct, cp = c.locate_intervals(starts[few], ends[few])
    assert off.tolist() == co.tolist() and t_.tolist() == ct.tolist() and p_.tolist() == cp.tolist()
    idx = np.unique(rng.integers(0, c.n + 1, 400)).astype(np.uint64)
    cols = naive_occurrence_columns(c.bwt, c.sigma)
    for sym in range(c.sigma):
        assert g.rank_many(np.full(idx.size, sym, dtype=np.uint8), idx).tolist() == cols[sym, idx.astype(np.int64)].tolist()
    pos = idx[idx < c.n]
    assert g.symbol_at_many(pos).tolist() == c.bwt[pos.astype(np.int64)].tolist()
    with pytest.raises(GdxError) as err:  # the rest of the ABI says so instead of misbehaving
        g.save_to_file("/tmp/should_not_exist.gdx")
    assert err.value.status == _lib.GDX_ERR_UNSUPPORTED
