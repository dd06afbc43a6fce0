"""Edge shapes of the offsets scan and store pass that ends every count + locate step (locate.hip: scan2_tile_sums_kernel ->
scan2_sums_kernel -> scan2_tile_scan_kernel<kStore, kWide>, then locate_by_query_kernel / locate_stream_kernel /
locate_queue_kernel), against the plain model of offsets_scan_model.py and the CPU oracle.  Exact equality everywhere.

The pass is driven WITHOUT a search: search records {start row, end row, 0xffffffff, 0} and compact words are made by hand from
real suffix-array intervals of one small collection and laid out at exactly the places under test (gdx_locate_many_totals_compact_dev
+ gdx_locate_many_offsets[32]_hits_compact_dev, gdx_locate_many_offsets_{capped,compact}_dev); batches of real reads tie the cases
back to the one-call step the benchmark times (gdx_locate_many_step_compact_layout_dev).  Two indexes of the same texts: the
library's default shape (SA[row] at hand: the store pass may locate inline, the stream / by-query kernels finish) and the
`verify-walk` shape of test_gpu_parity._VARIANTS (no full suffix array: the queue kernel walks).

The constants of locate.hip the shapes below are made from -- a change of one of them names the tests that need new shapes:"""
import numpy as np
import pytest

import offsets_scan_model as model
from genedex_amd import alphabet as alph
from oracle.oracle import OracleIndex, pack_queries

pytestmark = pytest.mark.gpu

ROW = 64             # lanes of a wavefront: one coalesced row of the scan
WAVE = 512           # kScan2Wave = 64 x kScan2Rows
TILE = 2048          # kScan2Tile (= kSumTile)
SWEEP = 16 * 1024    # tile sums one sweep of scan2_sums_kernel takes (kPer x 1024 threads)
CHUNK = 2048         # kLocateChunk
INLINE_MAX = 2048    # kScanInlineMax
SPARSE = 16          # open slots x 16 <= all slots: the store pass stores, flags and locates inline
POISON = 0x5A5A5A5A  # what outputs (and the records no kernel may read) hold beforehand
GUARD = 4            # elements behind off[nq] and hits[capacity] that must keep the poison

SHAPES = {
    # name: (build options, query options)
    "default": (dict(), dict()),
    "walk": (dict(pair_lines=False, jump_entry_bytes=0, top_table_depth=5, text_units=True), dict(search_kernel="pair")),
}
UNIT_A, COPIES_A = b"ACGTT", 2051   # reads of 3 / 4 / 5 units: 2049 / 2048 / 2047 rows
UNIT_B, COPIES_B = b"AACCGT", 5003  # a read of 4 units: 5000 rows
WIDTHS = (0, 1, 2, 3, 4, 2047, 2048, 2049, 5000)


class World:
    """the module's collection: oracle, the hit of every suffix-array row, real intervals by width, one engine per shape"""


@pytest.fixture(scope="module")
def world():
    from genedex_amd import FmIndexConfig
    from genedex_amd.device import DeviceEngine

    rng = np.random.default_rng(4242)
    a = alph.ascii_dna_with_n()
    body = bytes(b"ACGT"[i] for i in rng.integers(0, 4, 19300))
    seg2, seg3, seg4 = (bytes(b"ACGT"[i] for i in rng.integers(0, 4, 48)) for _ in range(3))
    texts = [
        body[:6000] + seg2 + body[6000:9000] + seg3 + body[9000:12000] + seg4 + body[12000:13000] + seg4 + body[13000:14000],
        body[14000:14500] + UNIT_A * COPIES_A + body[14500:15000],      # a tandem repeat: intervals of 2047 .. 2049 rows
        seg3 + body[15000:17000] + seg2 + body[17000:18000] + seg4,
        body[18000:18300] + UNIT_B * COPIES_B + body[18300:18600],      # ... and of 5000
        body[18600:19000] + seg4 + b"NNN" + seg3 + body[19000:19300],
    ]
    w = World()
    w.texts, w.body = texts, body
    w.oracle = o = OracleIndex.build(texts, a.io_to_dense_table, a.num_dense_symbols(), a.num_searchable_dense_symbols(),
                                     sa_rate=4, lookup_depth=0, width=32)
    w.n = o.n
    _, t, p = o.locate_intervals([0], [w.n])  # the hit of every row, once
    w.row_text, w.row_pos = t.astype(np.int64), p.astype(np.int64)
    w.sentinels = o.sentinel_indices.astype(np.int64)
    w.sa = o.full_sa.astype(np.int64)
    tid, pos = model.split_positions(w.sa, w.sentinels)  # (the compact words below are SA values: the same coordinates)
    assert np.array_equal(tid, w.row_text) and np.array_equal(pos, w.row_pos) and len(texts) >= 3
    w.reads = {0: bytes(b"ACGT"[i] for i in rng.integers(0, 4, 30)), 1: body[100:130], 2: seg2, 3: seg3, 4: seg4,
               2047: UNIT_A * 5, 2048: UNIT_A * 4, 2049: UNIT_A * 3, 5000: UNIT_B * 4}
    w.iv = {}
    for width, q in w.reads.items():
        s, e, st = o.cursor_for_query(q)
        assert st == 0 and e - s == width, (width, s, e)
        w.iv[width] = (s, e)
    w.engines, w.indexes = {}, {}
    for name, (build, query) in SHAPES.items():
        g = FmIndexConfig("u32").suffix_array_sampling_rate(4).acceleration_structures(**build).construct_index(texts, a)
        if query:
            g.set_query_options(**query)
        w.indexes[name], w.engines[name] = g, DeviceEngine(g)
    info = {name: e.aux_info() for name, e in w.engines.items()}
    assert info["default"]["default_shape"] and info["default"]["full_suffix_array"]      # SA[row] at hand: locate_entry_sa
    assert not info["walk"]["full_suffix_array"] and info["walk"]["jump_entry_bytes"] != 32  # the queue kernel walks
    return w


# ---- hand-made batches ------------------------------------------------------------------------------------------------------

def intervals(w, widths):
    """real row intervals of these widths: the text's own where it has one, else cut from the 5000-row interval"""
    widths = np.asarray(widths, dtype=np.int64)
    starts = np.zeros(widths.size, dtype=np.int64)
    wide = w.iv[5000][0]
    for width in np.unique(widths):
        sel = np.flatnonzero(widths == width)
        if int(width) in w.iv:
            starts[sel] = w.iv[int(width)][0]
        else:
            assert width < 5000
            starts[sel] = wide + (sel * 7) % (5000 - width)
    # reads of one row: different rows, so that neighbouring hits differ
    one = np.flatnonzero(widths == 1)
    starts[one] = (one * 131) % w.n
    return starts, starts + widths


def compact_words(w, starts, ends, salt=0):
    """compact words beside the records: every other read of one row is answered by its position, two in three of the reads
    without rows by "none", everything else says "see the record" """
    q = np.arange(starts.size) + salt
    width = ends - starts
    cw = np.full(starts.size, model.COMPACT_SEE, dtype=np.int32)
    cw[(width == 0) & (q % 3 != 0)] = model.COMPACT_NONE
    pos = (width == 1) & (q % 2 == 0)
    cw[pos] = w.sa[starts[pos]].astype(np.uint32).view(np.int32)
    return cw


def upload(eng, starts, ends, compact):
    import torch

    nq = starts.size
    if nq == 0:
        return eng.alloc_records(0), (eng.alloc_compact(0) if compact is not None else None)
    rec = model.record_words(starts, ends)
    if compact is not None:  # (kernels.hpp: the record slots of compactly answered reads are not written at all)
        rec[compact != model.COMPACT_SEE] = POISON
    return torch.from_numpy(rec).to(eng.dev), (torch.from_numpy(compact).to(eng.dev) if compact is not None else None)


def poisoned(n, dtype, dev, cols=None):
    import torch

    value = POISON if dtype == torch.int32 else (POISON << 32) | POISON
    return torch.full((n,) if cols is None else (n, cols), value, dtype=dtype, device=dev)


def check_offsets(off, nq, want, what):
    """off[0 .. nq] equal the model's (the narrow form: modulo 2^32), the guard behind off[nq] keeps the poison"""
    narrow = off.element_size() == 4
    got = off.cpu().numpy().view(np.uint32 if narrow else np.uint64).astype(np.uint64)
    assert got.size == nq + 1 + GUARD and np.all(got[nq + 1:] == (POISON if narrow else (POISON << 32) | POISON)), \
        (what, "something was written behind off[nq]")
    want = np.asarray(want, dtype=np.uint64) & np.uint64(0xFFFFFFFF if narrow else 0xFFFFFFFFFFFFFFFF)
    bad = np.flatnonzero(got[:nq + 1] != want)
    assert bad.size == 0, (what, "first wrong offset at read", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


def check_hits(hits, stored, want, what):
    """rows [0, stored) equal the model's, everything behind keeps the poison"""
    got = hits.cpu().numpy()
    assert np.all(got[stored:] == POISON), (what, "a hit was written at or beyond slot", stored)
    bad = np.flatnonzero(np.any(got[:stored].astype(np.int64) != want[:stored], axis=1))
    assert bad.size == 0, (what, "first wrong hit in slot", int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


def any_chunk_flagged(ws, total):
    """the word in front of a locate workspace's chunk flags (locate.hip: locate_chunk_flags_offset, kFlagsHead): set by the store
    pass when it leaves a read's slots to the locate kernel"""
    import torch

    at = (((total + CHUNK - 1) // CHUNK + 2) * 4 + 255) // 256 * 256
    return int(ws[at:at + 4].view(torch.int32).item()) != 0


def check_two_calls(w, shape, starts, ends, compact, max_hits=0, what="", flagged=None):
    """totals -> offsets + hits in both offset widths, and the plain offsets call, against the model; -> (offsets, hits).
    flagged: whether the store pass must have left something to the locate kernel"""
    import torch

    eng = w.engines[shape]
    nq = starts.size
    counts = model.slot_counts(starts, ends, compact, max_hits)
    want_off = model.offsets_of(counts)
    want_hits = model.expected_hits(starts, ends, compact, counts, w.row_text, w.row_pos, w.sentinels)
    total, rest = int(want_off[-1]), model.open_slots(counts, compact)
    rec, cw = upload(eng, starts, ends, compact)
    sws = torch.empty(max(eng.totals_workspace_bytes(nq), 16), dtype=torch.uint8, device=eng.dev)
    for dt in (torch.int64, torch.int32):
        tag = (what, shape, "compact" if compact is not None else "records", str(dt), "nq", nq, "max_hits", max_hits)
        totals = poisoned(2, torch.int64, eng.dev)
        eng.locate_totals(rec, nq, sws, totals, max_hits, cw)
        assert totals.tolist() == [total, rest], tag
        off = poisoned(nq + 1 + GUARD, dt, eng.dev)
        hits = poisoned(total + GUARD, torch.int32, eng.dev, 2)
        ws = torch.empty(max(eng.locate_workspace_bytes(total), 16), dtype=torch.uint8, device=eng.dev)
        eng.locate_offsets_hits(rec, nq, sws, off, total, rest, hits, ws, max_hits, cw)
        torch.cuda.synchronize()
        check_offsets(off, nq, want_off, tag)
        check_hits(hits, total, want_hits, tag)
        assert flagged is None or any_chunk_flagged(ws, total) == flagged, (tag, "the store pass and its chunk flags")
    off = poisoned(nq + 1 + GUARD, torch.int64, eng.dev)  # the offsets call of the three-call form: the same scan kernels
    eng.locate_offsets(rec, nq, off, max_hits, cw)
    torch.cuda.synchronize()
    check_offsets(off, nq, want_off, (what, shape, "offsets only", nq, max_hits))
    return want_off, want_hits


# ---- 1. query-count borders -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("nq", [1, ROW - 1, ROW, ROW + 1, WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE,
                                2 * TILE + 1, 3 * TILE + 1])
def test_query_count_on_row_wavefront_and_tile_borders(world, shape, nq):
    """Pins the q < m guards of scan2_load_counts / scan2_tile_scan_kernel, n_tiles = ceil(m / kScan2Tile), the chaining of rows
    (carry), wavefronts (s_part) and tiles (sums[tile]) and the one write of off[nq] (sums[n_tiles]) for a batch that ends one
    short of, on and one behind a row (64), a wavefront (512) and a tile (2048).  Four layouts of the counts: mixed; only the
    last read of every row (1 row), wavefront (2) and tile (4) has hits; only the first read (2049 rows); only the last."""
    w = world
    rng = np.random.default_rng(nq)
    q = np.arange(nq)
    mixed = rng.choice(WIDTHS + (7, 100), nq, p=[.3, .3, .1, .05, .1, .004, .004, .004, .003, .105, .03])
    ends_only = np.where(q % TILE == TILE - 1, 4, np.where(q % WAVE == WAVE - 1, 2, np.where(q % ROW == ROW - 1, 1, 0)))
    first_only = np.where(q == 0, 2049, 0)
    last_only = np.where(q == nq - 1, 3, 0)
    for name, widths in (("mixed", mixed), ("ends", ends_only), ("first", first_only), ("last", last_only)):
        starts, ends = intervals(w, widths)
        check_two_calls(w, shape, starts, ends, None, what=name)
        check_two_calls(w, shape, starts, ends, compact_words(w, starts, ends, salt=nq), what=name)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_no_reads_at_all(world, shape):
    """nq = 0 is accepted by every entry point of the pass (launch_scan_totals, launch_scan_offsets_store and launch_locate_step
    return before any kernel that would divide the batch into tiles): offsets [0], totals 0, nothing else written."""
    import torch

    from genedex_amd.device import DeviceQueries

    w = world
    none = np.zeros(0, dtype=np.int64)
    check_two_calls(w, shape, none, none, None)
    check_two_calls(w, shape, none, none, np.zeros(0, dtype=np.int32))
    eng = w.engines[shape]
    dq = DeviceQueries.from_host(np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    for dt in (torch.int64, torch.int32):
        for with_compact in (False, True):
            off, hits, totals, _ = run_step(eng, dq, dt, with_compact, capacity=3)
            check_offsets(off, 0, np.zeros(1, dtype=np.uint64), (shape, dt))
            check_hits(hits, 0, np.zeros((0, 2), dtype=np.int64), (shape, dt))
            assert totals == [0, 0]


# ---- 2. hit-total and chunk borders -----------------------------------------------------------------------------------------

def _runs(*parts):
    return np.concatenate([np.full(n, width, dtype=np.int64) for width, n in parts])


TOTALS = {
    # name: (widths of the reads, the total they must give)
    "nothing": (_runs((0, 3000)), 0),
    "one hit among empty reads": (_runs((0, 2500), (1, 1), (0, 2499)), 1),
    "one short of a chunk": (_runs((0, 70), (2047, 1), (0, 70)), CHUNK - 1),
    "one read fills a chunk": (_runs((0, 70), (2048, 1), (0, 70)), CHUNK),
    "a chunk of single hits": (_runs((1, 2048)), CHUNK),
    "one behind a chunk": (_runs((2048, 1), (0, 5), (1, 1)), CHUNK + 1),
    # the border between chunks 0 and 1 falls exactly between two reads, with nothing behind the second chunk
    "two chunks, the border between two reads": (_runs((2048, 1), (2048, 1)), 2 * CHUNK),
    # ... inside the slots of a read that starts at slot 1000 and ends in chunk 1
    "the border inside a read": (_runs((4, 250), (2049, 1), (2, 40)), 1000 + 2049 + 80),
    # ... in a run of thousands of reads without hits: slot 2048 belongs to the read BEHIND the run (chunk_first_query_kernel
    # takes the largest read whose offset is not beyond the slot)
    "the border in a run of empty reads": (_runs((1, 2048), (0, 5000), (1, 300), (4, 2)), 2048 + 308),
    "the border in a run of empty reads, a long read behind": (_runs((2, 1024), (0, 4097), (5000, 1)), 2048 + 5000),
}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", list(TOTALS))
def test_hit_totals_on_chunk_borders(world, shape, name):
    """Pins n_chunks = ceil(total / kLocateChunk), cnt of the last chunk, chunk_first_query_kernel's upper bound (entry n_chunks =
    the owner of the LAST slot), the head marks / s_carry of a read that goes on from an earlier chunk, and -- with compact words
    -- the chunk flags of the store pass, for totals of 0, 1, 2047, 2048, 2049 and 4096 slots."""
    widths, total = TOTALS[name]
    starts, ends = intervals(world, widths)
    for compact in (None, compact_words(world, starts, ends)):
        off, _ = check_two_calls(world, shape, starts, ends, compact, what=name)
        assert int(off[-1]) == total, name


def run_step(eng, dq, dt, with_compact, capacity, max_hits=0):
    """gdx_locate_many_step_compact_layout_dev into poisoned outputs with guards -> (offsets, hits, totals, compact words)"""
    import torch

    nq = dq.nq
    rec = eng.alloc_records(nq)
    cw = eng.alloc_compact(nq) if with_compact else None
    off = poisoned(nq + 1 + GUARD, dt, eng.dev)
    hits = poisoned(capacity + GUARD, torch.int32, eng.dev, 2)
    totals = poisoned(2, torch.int64, eng.dev)
    sws = torch.empty(max(eng.totals_workspace_bytes(nq), 16), dtype=torch.uint8, device=eng.dev)
    ws = torch.empty(max(eng.locate_workspace_bytes(capacity), 16), dtype=torch.uint8, device=eng.dev)
    eng.locate_step(dq, rec, cw, sws, totals, off, hits[:capacity], ws, max_hits)
    torch.cuda.synchronize()
    return off, hits, totals.tolist(), (cw[:nq].cpu().numpy() if with_compact and nq else None)


def oracle_hits(w, qbuf, qoff):
    s, e = w.oracle.cursors_for_many(qbuf, qoff)
    off, t, p = w.oracle.locate_intervals(s, e)
    return s.astype(np.int64), e.astype(np.int64), off, np.stack([t.astype(np.int64), p.astype(np.int64)], axis=1)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_hit_buffers_that_end_on_and_around_the_total(world, shape):
    """hits_capacity of the one-call step (gdx.h: 0 is allowed; what lies at or beyond the capacity is not stored, totals and
    offsets stay right): 0, 1, total - 1, total, total + 7, and 2048 slots for 2049 hits.  Pins `at < hits_capacity` of the store
    pass, `at + c <= hits_capacity` of the inline locate, `ch * kLocateChunk < hits_capacity` of the chunk flags and the
    min(*d_total, capacity) of the locate kernels -- the guard rows behind hits[capacity] keep their poison."""
    import torch

    from genedex_amd.device import DeviceQueries

    w = world
    eng = w.engines[shape]
    unique = [w.body[s:s + 32] for s in range(200, 5000, 40)]
    batches = {
        # 2049 hits: one, 2047 (ending on slot 2047), one -- a buffer of 2048 slots ends on the chunk border
        "2049": ([unique[0], w.reads[2047], unique[1]], (CHUNK,)),
        "mixed": (unique[:60] + [w.reads[2049], w.reads[0], b""] + unique[60:] + [w.reads[4], w.reads[2048], w.reads[3]], ()),
    }
    for name, (qs, extra) in batches.items():
        qbuf, qoff = pack_queries(qs)
        _, _, want_off, want_hits = oracle_hits(w, qbuf, qoff)
        total = int(want_off[-1])
        assert name != "2049" or total == CHUNK + 1
        dq = DeviceQueries.from_host(qbuf, qoff)
        for capacity in (0, 1, total - 1, total, total + 7) + extra:
            for dt in (torch.int64, torch.int32):
                for with_compact in (False, True):
                    tag = (shape, name, "capacity", capacity, str(dt), with_compact)
                    off, hits, totals, _ = run_step(eng, dq, dt, with_compact, capacity)
                    assert totals[0] == total, tag
                    check_offsets(off, dq.nq, want_off, tag)
                    check_hits(hits, min(total, capacity), want_hits, tag)


# ---- 3. the inline-locate cut-off -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [INLINE_MAX - 1, INLINE_MAX, INLINE_MAX + 1])
def test_inline_locate_cut_off_by_hand(world, rows):
    """Pins `c[j] <= ss.inline_max` (kScanInlineMax) of scan2_tile_scan_kernel<true, .> and `rest_hits * 16 <= total_hits` of
    launch_offsets_hits: ONE "see the record" read of 2047 / 2048 / 2049 rows among reads their compact words answer, the open
    share of the slots just under, on and just over one sixteenth.  On the default shape the read is located by the store pass
    itself (<= 2048 rows, sparse), by locate_stream_kernel through its chunk flags (2049 rows, sparse) or by
    locate_by_query_kernel (not sparse: no store pass); the walk shape has no inline locate.  The same arrays every way."""
    w = world
    for answered, sparse in ((15 * rows + 1, True), (15 * rows, True), (15 * rows - 1, False)):
        widths = np.ones(answered + 1, dtype=np.int64)
        widths[answered // 2 + 17] = rows
        widths = np.insert(widths, np.arange(5, answered, 301), 0)  # reads without occurrence in between: no slots
        at = int(np.flatnonzero(widths == rows)[0])
        starts, ends = intervals(w, widths)
        compact = np.where(widths == 0, model.COMPACT_NONE, w.sa[starts].astype(np.uint32).view(np.int32)).astype(np.int32)
        compact[at] = model.COMPACT_SEE
        counts = model.slot_counts(starts, ends, compact)
        total, open_ = int(counts.sum()), model.open_slots(counts, compact)
        assert open_ == rows and total == rows + answered and (open_ * SPARSE <= total) == sparse
        assert abs(open_ * SPARSE - total) <= 1  # ... and as close to the sixteenth as whole slots get
        # a sparse batch: the store pass flags the chunks of what it leaves open -- nothing when it located the read itself
        flagged = {"default": (rows > INLINE_MAX) if sparse else None, "walk": True if sparse else None}
        want = [check_two_calls(w, shape, starts, ends, compact, what=("answered", answered), flagged=flagged[shape])
                for shape in SHAPES]
        assert np.array_equal(want[0][0], want[1][0]) and np.array_equal(want[0][1], want[1][1])


@pytest.fixture(scope="module")
def answered_reads(world):
    """32-symbol reads of the first text's unique stretch that the default shape's search answers by their compact word"""
    import torch

    from genedex_amd.device import DeviceQueries

    w = world
    text = np.frombuffer(w.texts[0], dtype=np.uint8)
    pool = np.lib.stride_tricks.sliding_window_view(text[:5900], 32).copy()
    qoff = np.arange(pool.shape[0] + 1, dtype=np.uint64) * np.uint64(32)
    s, e = w.oracle.cursors_for_many(pool.reshape(-1), qoff)
    eng = w.engines["default"]
    dq = DeviceQueries.from_host(pool.reshape(-1), qoff)
    rec, cw = eng.alloc_records(dq.nq), eng.alloc_compact(dq.nq)
    eng.locate_search(dq, rec, cw)
    torch.cuda.synchronize()
    keep = (cw[:dq.nq].cpu().numpy() >= 0) & (e - s == 1)
    assert int(keep.sum()) > 5000
    return pool[keep]


def _one_long_read_among_answered(w, answered_reads, rows, answered):
    """`answered` reads of one hit with the tandem read of `rows` rows in their middle -> (qbuf, qoff, where it is)"""
    special = np.frombuffer(w.reads[rows], dtype=np.uint8)
    pool = answered_reads[np.arange(answered) % answered_reads.shape[0]]
    at = answered // 2 + 17
    qbuf = np.concatenate([pool[:at].reshape(-1), special, pool[at:].reshape(-1)])
    lens = np.full(answered + 1, 32, dtype=np.uint64)
    lens[at] = special.size
    qoff = np.zeros(answered + 2, dtype=np.uint64)
    np.cumsum(lens, out=qoff[1:])
    return qbuf, qoff, at


@pytest.mark.parametrize("rows", [INLINE_MAX - 1, INLINE_MAX, INLINE_MAX + 1])
def test_inline_locate_cut_off_in_the_one_call_step(world, answered_reads, rows):
    """The same through gdx_locate_many_step_compact_layout_dev on real reads, where the threshold is read on the device
    (`ss.d_totals[1] * 16 <= ss.d_totals[0]` in scan2_tile_scan_kernel): one read of the tandem repeat with 2047 / 2048 / 2049
    rows among reads of one hit that the search answers compactly.  Which reads a search answers by a compact word is its own
    choice (gdx_experimental.h: "nearly every read" -- the first read of a batch gets a resolved record, for one), so the open
    slots are not assumed: a first run tells how many reads of one hit are left to their records, the three batches are sized
    from that so that the open share sits one slot under, on and one slot over the sixteenth, and in every run totals[1] must
    be the sum over the reads whose word, as the call left it, says "see the record", the words must agree with the oracle's
    counts, and the ratio is asserted from the totals.  The walk shape (every word says "see the record": nothing inline,
    nothing sparse) gives the same offsets and hits."""
    import torch

    from genedex_amd.device import DeviceQueries

    w = world
    qbuf, qoff, at = _one_long_read_among_answered(w, answered_reads, rows, 15 * rows)
    _, _, _, cw = run_step(w.engines["default"], DeviceQueries.from_host(qbuf, qoff), torch.int64, True, 16 * rows)
    extra = int((cw == model.COMPACT_SEE).sum()) - 1
    assert cw[at] == model.COMPACT_SEE and 0 <= extra <= 16
    on = 15 * rows + SPARSE * extra  # 16 (rows + extra) == rows + answered
    for answered, sparse in ((on + 1, True), (on, True), (on - 1, False)):
        qbuf, qoff, at = _one_long_read_among_answered(w, answered_reads, rows, answered)
        s, e, want_off, want_hits = oracle_hits(w, qbuf, qoff)
        total = int(want_off[-1])
        assert total == answered + rows
        dq = DeviceQueries.from_host(qbuf, qoff)
        for dt in (torch.int64, torch.int32):
            tag = ("default", rows, answered, str(dt))
            off, hits, totals, cw = run_step(w.engines["default"], dq, dt, True, total)
            counts = model.slot_counts(s, e, cw)
            print(tag, "totals", totals, "reads of one hit left to their records:", int((cw == model.COMPACT_SEE).sum()) - 1)
            assert cw[at] == model.COMPACT_SEE and int((cw == model.COMPACT_SEE).sum()) == 1 + extra, tag
            assert np.array_equal(counts, (e - s).astype(np.uint64)), (tag, "a compact word contradicts the oracle's count")
            assert totals == [total, model.open_slots(counts, cw)] and totals[1] == rows + extra, tag
            assert (totals[1] * SPARSE <= totals[0]) == sparse and abs(totals[1] * SPARSE - totals[0]) <= 1, tag
            check_offsets(off, dq.nq, want_off, tag)
            check_hits(hits, total, want_hits, tag)
            off, hits, totals, _ = run_step(w.engines["walk"], dq, dt, True, total)
            assert totals == [total, total]
            check_offsets(off, dq.nq, want_off, ("walk", rows, answered, dt))
            check_hits(hits, total, want_hits, ("walk", rows, answered, dt))


# ---- 4. max_hits_per_query --------------------------------------------------------------------------------------------------

def _seams(n, specials):
    """a batch of n widths with `specials` on both sides of the first two tile seams"""
    rng = np.random.default_rng(n)
    widths = rng.choice([0, 1, 1, 2, 3, 4], n)
    for at, width in zip((TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 0, n - 1), specials * 3):
        widths[at] = width
    return widths


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("k", [1, 2, INLINE_MAX])
def test_max_hits_count_only(world, shape, k):
    """RecordSize with take == false, the meaning of max_hits in every device call (gdx_locate_many_offsets_capped_dev: "counted
    but not located"): reads of more than k rows get no slots, reads of exactly k rows keep theirs -- k and k + 1 rows on both
    sides of the tile seams (the two copies of the rule in scan2_load_counts and scan2_tile_scan_kernel and RecordSize itself
    must agree, or a tile's base and its own scan differ).  By hand through the two calls and the plain offsets call, and on
    real reads through the one-call step."""
    import torch

    from genedex_amd.device import DeviceQueries

    w = world
    widths = _seams(2 * TILE + 5, (k, k + 1))
    starts, ends = intervals(w, widths)
    for compact in (None, compact_words(w, starts, ends)):
        off, _ = check_two_calls(w, shape, starts, ends, compact, max_hits=k, what="count only")
        assert off[TILE] - off[TILE - 1] == k and off[TILE + 1] == off[TILE]  # (the read of k rows stays, the one of k + 1 goes)
    qs, qbuf, qoff, s, e = real_seam_reads(w, k)
    counts = model.slot_counts(s, e, None, k)
    want_off = model.offsets_of(counts)
    want_hits = model.expected_hits(s, e, None, counts, w.row_text, w.row_pos, w.sentinels)
    total = int(want_off[-1])
    dq = DeviceQueries.from_host(qbuf, qoff)
    for dt in (torch.int64, torch.int32):
        for with_compact in (False, True):
            off, hits, totals, _ = run_step(w.engines[shape], dq, dt, with_compact, total + 1, max_hits=k)
            assert totals[0] == total, (shape, k, dt, with_compact)
            check_offsets(off, dq.nq, want_off, (shape, k, dt, with_compact))
            check_hits(hits, total, want_hits, (shape, k, dt, with_compact))


def real_seam_reads(w, k):
    """real reads of 1 .. 4 rows and none, with reads of exactly k and k + 1 rows on both sides of the tile seams"""
    widths = _seams(2 * TILE + 5, (k, k + 1))
    unique = [w.body[s:s + 30] for s in range(150, 5900)]
    qs = [unique[i] if width == 1 else w.reads[int(width)] for i, width in enumerate(widths)]
    qbuf, qoff = pack_queries(qs)
    s, e = w.oracle.cursors_for_many(qbuf, qoff)
    assert np.array_equal(e - s, widths.astype(np.uint64))
    return qs, qbuf, qoff, s.astype(np.int64), e.astype(np.int64)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("k", [1, 2, INLINE_MAX])
def test_max_hits_take_k_on_the_host_call(world, shape, k):
    """RecordSize with take == true, what gdx_query_options_t.max_hits_per_query means to the host-pointer calls (every chunk of
    gdx_locate_many_alloc is the one-call step with LocateStep::take): offsets count min(n, k), the hits are a read's first k in
    suffix-array order.  The same real reads as above: k and k + 1 rows on both sides of the tile seams."""
    w = world
    g = w.indexes[shape]
    qs, qbuf, qoff, s, e = real_seam_reads(w, k)
    counts = model.slot_counts(s, e, None, k, take=True)
    assert counts.max() == k and np.array_equal(counts, np.minimum(e - s, k).astype(np.uint64))
    want_off = model.offsets_of(counts)
    want_hits = model.expected_hits(s, e, None, counts, w.row_text, w.row_pos, w.sentinels)
    g.set_query_options(max_hits_per_query=k, **SHAPES[shape][1])
    try:
        off, t, p, status = g.locate_alloc_raw(qbuf, qoff)
    finally:
        g.set_query_options(**SHAPES[shape][1])
    assert not status.any() and np.array_equal(off, want_off)
    assert np.array_equal(t.astype(np.int64), want_hits[:, 0]) and np.array_equal(p.astype(np.int64), want_hits[:, 1])


# ---- 5. the second sweep of the sums scan, the resident grid's stride --------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("width", [64, 32])
def test_more_tiles_than_one_sweep_of_the_sums_scan(world, shape, width):
    """nq = 16384 tiles + 2049 reads: scan2_sums_kernel goes round its loop twice (`base += 1024 * kPer`, the second sweep starts
    from a non-zero s_carry and holds two tiles, the last one a single read), and the blocks of scan2_tile_sums_kernel /
    scan2_tile_scan_kernel stride over the tiles many times (`tile += gridDim.x`, the next tile's base prefetched).  Records
    only, made on the device: all empty but a few hundred reads of 1 .. 5 rows -- in the first tiles, just before tile 16383,
    in tiles 16384 and 16385 and scattered in between.  Every offset is checked (on the device: the differences of neighbouring
    offsets are the counts, nothing else is non-zero), the offsets around every non-empty read, of the first and last 4096
    reads and off[nq] against the model on the host, totals and all hits against the oracle."""
    import torch

    w = world
    eng = w.engines[shape]
    if torch.cuda.mem_get_info(eng.dev)[0] < 4 << 30:
        pytest.skip("less than 4 GB of device memory free")
    nq = SWEEP * TILE + TILE + 1
    assert (nq + TILE - 1) // TILE == SWEEP + 2
    rng = np.random.default_rng(5)
    last_sweep = SWEEP * TILE
    at = np.unique(np.concatenate([
        [0, 1, ROW - 1, ROW, WAVE - 1, WAVE, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE], rng.integers(0, 3 * TILE, 60),
        last_sweep - 3 * TILE + rng.integers(0, 3 * TILE, 80), [last_sweep - TILE - 1, last_sweep - TILE, last_sweep - 1],
        [last_sweep, last_sweep + 1, last_sweep + WAVE, last_sweep + TILE - 1, last_sweep + TILE],  # (the last one = read nq - 1)
        last_sweep + rng.integers(0, TILE, 60), rng.integers(0, nq, 150)]).astype(np.int64))
    assert at[-1] == nq - 1 and 300 < at.size < 400
    widths = rng.integers(1, 6, at.size)
    starts, ends = intervals(w, widths)
    dt = torch.int64 if width == 64 else torch.int32
    rec = torch.zeros((nq, 4), dtype=torch.int32, device=eng.dev)
    rec[torch.from_numpy(at).to(eng.dev)] = torch.from_numpy(model.record_words(starts, ends)).to(eng.dev)
    counts = model.slot_counts(starts, ends)
    total = int(counts.sum())
    want_hits = model.expected_hits(starts, ends, None, counts, w.row_text, w.row_pos, w.sentinels)
    sws = torch.empty(eng.totals_workspace_bytes(nq), dtype=torch.uint8, device=eng.dev)
    totals = poisoned(2, torch.int64, eng.dev)
    eng.locate_totals(rec, nq, sws, totals)
    assert totals.tolist() == [total, total]
    off = poisoned(nq + 1 + GUARD, dt, eng.dev)
    hits = poisoned(total + GUARD, torch.int32, eng.dev, 2)
    ws = torch.empty(eng.locate_workspace_bytes(total), dtype=torch.uint8, device=eng.dev)
    eng.locate_offsets_hits(rec, nq, sws, off, total, total, hits, ws)
    torch.cuda.synchronize()
    # every offset: off[0] = 0 and the differences are the counts
    step = off[1:nq + 1] - off[:nq]
    where = torch.nonzero(step).reshape(-1)
    assert int(off[0].item()) == 0 and where.cpu().numpy().tolist() == at.tolist()
    assert step[where].cpu().numpy().tolist() == counts.astype(np.int64).tolist()
    del step
    look = np.unique(np.clip(np.concatenate([at - 1, at, at + 1, at + 2, np.arange(4096), nq - np.arange(4096), [nq]]), 0, nq))
    got = off[torch.from_numpy(look).to(eng.dev)].cpu().numpy()
    got = got.view(np.uint32 if width == 32 else np.uint64).astype(np.uint64)
    want = model.sparse_offsets(at, counts, look)
    assert np.array_equal(got, want), ("first wrong offset at read", int(look[np.flatnonzero(got != want)[0]]))
    assert int(want[-1]) == total
    guard = off[nq + 1:].cpu().numpy()
    assert np.all(guard == (POISON if width == 32 else (POISON << 32) | POISON))
    check_hits(hits, total, want_hits, (shape, width))


# ---- 6. real reads through the one call -------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES))
def test_real_reads_in_every_layout_through_the_one_call(world, shape):
    """gdx_locate_many_step_compact_layout_dev on batches of two tiles and one read (4097): reads of every length with random reads, an
    empty read and a read with N in the plain layout, and reads of 32 symbols in all four layouts (plain, uniform, packed, packed +
    uniform) -- both offset widths, with and without compact words, all equal to the oracle and therefore to each other.  The
    path the benchmark times, on the borders the cases above pin by hand."""
    import torch

    from genedex_amd.device import DeviceQueries

    w = world
    eng = w.engines[shape]
    rng = np.random.default_rng(66)
    n = 2 * TILE + 1
    flat = b"".join(t + b"$" for t in w.texts)
    qs = []
    for _ in range(n - 12):
        s = int(rng.integers(0, len(flat) - 80))
        q = flat[s:s + int(rng.integers(12, 70))]
        qs.append(q.split(b"$")[0])
    qs += [bytes(b"ACGT"[i] for i in rng.integers(0, 4, 24)) for _ in range(6)]
    qs += [b"", b"ACGTNACGTACG", w.reads[2049], w.reads[4], w.reads[5000], w.reads[2]]
    qs = [qs[i] for i in rng.permutation(n)]
    same = []
    for _ in range(n - 8):
        t = w.texts[int(rng.integers(0, len(w.texts)))]
        s = int(rng.integers(0, len(t) - 32))
        same.append(t[s:s + 32] if b"N" not in t[s:s + 32] else w.body[s % 9000:s % 9000 + 32])
    same += [(UNIT_A * 7)[:32], (UNIT_B * 6)[1:33], w.reads[2][:32], w.reads[3][:32], w.reads[4][8:40]]
    same += [bytes(b"ACGT"[i] for i in rng.integers(0, 4, 32)) for _ in range(3)]
    same = [same[i] for i in rng.permutation(n)]
    for name, batch in (("any length", qs), ("32 symbols", same)):
        assert len(batch) == n
        qbuf, qoff = pack_queries(batch)
        _, _, want_off, want_hits = oracle_hits(w, qbuf, qoff)
        total = int(want_off[-1])
        assert total > n
        plain = DeviceQueries.from_host(qbuf, qoff)
        forms = {"plain": plain}
        if name == "32 symbols":
            packed = plain.as_packed(w.indexes[shape])
            forms.update({"uniform": plain.as_uniform(32), "packed": packed, "packed + uniform": packed.as_uniform(32)})
        for form, dq in forms.items():
            for dt in (torch.int64, torch.int32):
                for with_compact in (False, True):
                    tag = (shape, name, form, str(dt), with_compact)
                    off, hits, totals, _ = run_step(eng, dq, dt, with_compact, total)
                    assert totals[0] == total, tag
                    check_offsets(off, n, want_off, tag)
                    check_hits(hits, total, want_hits, tag)
