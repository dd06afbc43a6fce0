"""The seed table's repeat records (IndexView::seed_pairs / seed_quads) and the reads they decide, on crafted texts that hold
the record path's edges on purpose (seed_record_model.py): every read a record decides gets exactly the 16-byte search record
the plain model says, and every consumer of those records -- the host calls, the device step calls with and without compact
results, hit caps, the 2-bit and uniform query forms, the locate kernels, the compact words and the wire -- gives the oracle's
counts, hits and hit order.

A read routed to the general kernel instead would still get the oracle's hits, but not the same raw records: the general
kernel writes a dead or single-row read as {row, row, ..} / {row, row + 1, ..}, a record {0, 0, ..} / {0, 1, ..}.  So the
raw-record checks below, which need reads of every kind, catch a record path that quietly goes unused.  (The seed kernels
load the 56 symbols in front of a read's end; a read that ends closer to the start of the query buffer is searched by the
verify kernel's own seed lookup, which does not read the records.  Every batch whose raw records are checked therefore
starts with reads no record decides.)"""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from genedex_amd import alphabet as alph
from seed_record_model import KINDS, LEAD, RecordModel, crafted_reads, crafted_texts
from test_gpu_parity import cpu_index, gpu_index, pack_queries
from test_gpu_seed import check_against_oracle, device_locate

pytestmark = pytest.mark.gpu

A = alph.ascii_dna_with_n()
# the default shape (k = 16 on these texts) and an odd k with the same structures; no jump table in either (with one, the
# seed kernel's list goes to search_fast_kernel4, which reads no records)
SHAPES = {"default": {}, "k11": dict(seed_symbols=11, jump_entry_bytes=0, full_suffix_array=True, inverse_suffix_array=True)}
MIN_PER_KIND = 20


@pytest.fixture(scope="module")
def crafted():
    texts, fams = crafted_texts()
    return texts, fams, cpu_index(texts, A)


def make_case(texts, fams, c, g):
    k = g.seed_info()["k"]
    model = RecordModel(texts, k, c)
    qs = crafted_reads(texts, fams, k)
    co, ct, cp = c.locate_many(qs)
    decided = {i: model.read(q) for i, q in enumerate(qs)}
    decided = {i: r for i, r in decided.items() if r is not None}
    return SimpleNamespace(texts=texts, fams=fams, c=c, g=g, k=k, model=model, qs=qs, co=co, ct=ct, cp=cp, decided=decided)


@pytest.fixture(scope="module", params=list(SHAPES))
def case(request, crafted):
    from genedex_amd.device import DeviceEngine

    texts, fams, c = crafted
    g = gpu_index(texts, A, **SHAPES[request.param])
    if request.param == "default":
        assert DeviceEngine(g).aux_info()["default_shape"] and g.seed_info()["k"] == 16
    else:
        assert g.seed_info()["k"] == 11
    return make_case(texts, fams, c, g)


def search_records(g, dq):
    """the 16-byte search records of a batch after locate_search (no compact results: every record is written)"""
    import torch

    from genedex_amd.device import DeviceEngine

    eng = DeviceEngine(g)
    rec = eng.alloc_records(dq.nq)
    rec.fill_(0x5a5a5a5a)
    eng.locate_search(dq, rec)
    torch.cuda.synchronize()
    return rec[:dq.nq].cpu().numpy().astype(np.uint32)


def assert_records(case, rec, idx=None):
    """the raw record of every read a record decides is the model's; returns the number of reads of each kind"""
    idx = range(len(case.qs)) if idx is None else idx
    kinds = dict.fromkeys(KINDS, 0)
    for row, i in enumerate(idx):
        r = case.decided.get(i)
        if r is None:
            continue
        kind, mask, want, _ = r
        got = tuple(int(x) for x in rec[row])
        assert got == want, (i, case.qs[i], kind, hex(mask), [hex(x) for x in got], [hex(x) for x in want])
        kinds[kind] += 1
    return kinds


def capped(co, ct, cp, max_hits):
    """offsets and hits of a batch when reads with more than max_hits hits get no slots (the device calls' max_hits)"""
    counts = np.diff(co).astype(np.int64)
    keep = np.ones(counts.size, dtype=bool) if max_hits == 0 else counts <= max_hits
    off = np.concatenate([[0], np.cumsum(np.where(keep, counts, 0))]).astype(np.uint64)
    sel = np.repeat(keep, counts)
    return off, ct[sel].astype(np.uint32), cp[sel].astype(np.uint32)


def step(g, dq, max_hits=0):
    """the whole locate step in one call (gdx_locate_many_step_compact_layout_dev): offsets and hits"""
    import torch

    from genedex_amd.device import DeviceEngine

    eng = DeviceEngine(g)
    rec, cw = eng.alloc_records(dq.nq), eng.alloc_compact(dq.nq)
    sws = torch.empty(max(eng.totals_workspace_bytes(dq.nq), 16), dtype=torch.uint8, device="cuda")
    totals = torch.zeros(2, dtype=torch.int64, device="cuda")
    off = torch.empty(dq.nq + 1, dtype=torch.int64, device="cuda")
    cap = 4 * dq.nq + 64
    hits = torch.full((cap, 2), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(eng.locate_workspace_bytes(cap), 16), dtype=torch.uint8, device="cuda")
    eng.locate_step(dq, rec, cw, sws, totals, off, hits, ws, max_hits=max_hits)
    torch.cuda.synchronize()
    tot = int(totals[0].item())
    assert tot <= cap
    return off.cpu().numpy().astype(np.uint64), hits[:tot].cpu().numpy().astype(np.uint32)


def assert_step(g, dq, co, ct, cp, max_hits=0):
    off, hits = step(g, dq, max_hits)
    want_off, want_t, want_p = capped(co, ct, cp, max_hits)
    assert off.tolist() == want_off.tolist()
    assert hits[:, 0].tolist() == want_t.tolist() and hits[:, 1].tolist() == want_p.tolist()


# ---- the records themselves ------------------------------------------------------------------------------------------

def test_record_counts_are_the_models(case):
    info = case.g.seed_info()
    assert info["pair_records"] == case.model.pair_records > 0
    assert info["quad_records"] == case.model.quad_records > 0


def test_raw_records_are_the_models(case):
    """Every read a record decides (1 .. 32 symbols in front of a seed on two to four rows with whole contexts): the record
    after locate_search is the model's, bit for bit -- with reads of every kind, so the path cannot go unused."""
    from genedex_amd.device import DeviceQueries

    rec = search_records(case.g, DeviceQueries.from_host(*pack_queries(case.qs)))
    kinds = assert_records(case, rec)
    assert all(v >= MIN_PER_KIND for v in kinds.values()), kinds


# ---- end to end --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("compact,fused", [(False, False), (True, False), (False, True), (True, True), (True, "search")])
def test_device_calls_equal_the_oracle(case, compact, fused):
    """search -> offsets -> hits on the device (separate calls, the fused totals, the search with totals, the one-call step
    inside device_locate) with hit caps of 0 .. 4: offsets, hits and hit order are the oracle's"""
    counts = np.diff(case.co).astype(np.uint32)
    for max_hits in range(5):
        off, hits, cnt, stat, _ = device_locate(case.g, case.qs, compact, max_hits=max_hits, fused=fused)
        want_off, want_t, want_p = capped(case.co, case.ct, case.cp, max_hits)
        assert off.tolist() == want_off.tolist(), max_hits
        assert hits[:, 0].tolist() == want_t.tolist() and hits[:, 1].tolist() == want_p.tolist(), max_hits
        assert cnt.tolist() == counts.tolist() and not stat.any()


def test_host_calls_compact_words_and_wire_equal_the_oracle(case):
    """the host locate / count calls; the compact words split into text id and position, their exception list, and the
    found-bitmap wire packed and split -- all as the oracle says"""
    import torch

    from genedex_amd import dist as gdist
    from genedex_amd.device import DeviceEngine, DeviceQueries

    check_against_oracle(case.g, case.c, case.qs, case.texts, fold=A.io_to_dense_table)
    g, co, ct, cp = case.g, case.co, case.ct, case.cp
    eng = DeviceEngine(g)
    dq = DeviceQueries.from_host(*pack_queries(case.qs))
    nq = dq.nq
    rec, cmp_ = eng.alloc_records(nq), eng.alloc_compact(nq)
    sws = torch.empty(max(eng.totals_workspace_bytes(nq), 16), dtype=torch.uint8, device="cuda")
    totals = torch.zeros(2, dtype=torch.int64, device="cuda")
    off = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
    hits = torch.empty((int(co[-1]) + 5, 2), dtype=torch.int32, device="cuda")
    ws = torch.empty(max(eng.locate_workspace_bytes(hits.shape[0]), 16), dtype=torch.uint8, device="cuda")
    eng.locate_step(dq, rec, cmp_, sws, totals, off, hits, ws)
    torch.cuda.synchronize()
    assert int(totals[0].item()) == int(co[-1])
    words = cmp_[:nq].cpu().numpy()
    counts = np.diff(co)
    ids = torch.full((nq,), 77, dtype=torch.uint8, device="cuda")
    pos = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
    eng.compact_split_hits(cmp_, nq, ids, pos)
    torch.cuda.synchronize()
    ids_h, pos_h = ids.cpu().numpy(), pos.cpu().numpy()
    for q in range(nq):
        if words[q] == -2:
            assert pos_h[q] == -2 and ids_h[q] == 0
        elif words[q] == -1:
            assert counts[q] == 0 and pos_h[q] == -1 and ids_h[q] == 0
        else:
            assert counts[q] == 1 and (int(ids_h[q]), int(pos_h[q])) == (int(ct[co[q]]), int(cp[co[q]])), q
    # the seed kernel lists the reads a record decides ("see the record") before the verify kernel decides them
    for i, (kind, _, _, _) in case.decided.items():
        assert words[i] == -2, (i, kind, words[i])
    want = np.flatnonzero(words == -2)
    listed = torch.full((len(want) + 3,), -5, dtype=torch.int32, device="cuda")
    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    eng.compact_exceptions(cmp_, nq, listed, n)
    torch.cuda.synchronize()
    assert int(n.item()) == len(want) and sorted(listed.cpu().numpy()[:len(want)].tolist()) == want.tolist()
    n_exc, n_exc_hits = gdist.exception_sizes(cmp_[:nq], off, nq)
    n_found = int(((cmp_[:nq] >= 0) | (cmp_[:nq] < -2)).sum().item())
    layout = gdist.WireLayout(nq, n_found, n_exc, n_exc_hits)
    buf = torch.full((layout.nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    v = layout.views(buf)
    wws = torch.empty(max(eng.wire_pack_workspace_bytes(nq), 16), dtype=torch.uint8, device="cuda")
    eng.wire_pack(cmp_, off, hits, nq, v, wws)
    torch.cuda.synchronize()
    assert v["meta"].tolist() == [n_exc, n_exc_hits, n_found, 0]
    ids2 = torch.full((nq,), 77, dtype=torch.uint8, device="cuda")
    pos2 = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
    eng.wire_split(v, nq, ids2, pos2)
    torch.cuda.synchronize()
    assert torch.equal(ids2, ids) and torch.equal(pos2, pos)
    cnt, hh = gdist.expand_split_results(ids2, pos2, v["exc_cnt"], v["exc_ids"], v["exc_pos"], v["meta"], nq)
    assert cnt.cpu().numpy().tolist() == counts.tolist()
    assert hh[:, 0].cpu().numpy().tolist() == ct.astype(np.int64).tolist()
    assert hh[:, 1].cpu().numpy().tolist() == cp.astype(np.int64).tolist()


# ---- the locate kernels -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("locate_kernel", ["queue", "lane", "pair"])
@pytest.mark.parametrize("jump_walk", [True, False])
def test_every_locate_kernel_decodes_the_records(case, locate_kernel, jump_walk):
    """the locate kernel option and the walk to sampled suffix-array values instead of SA[row] (locate_queue_kernel); the
    separate calls go through locate_by_query_kernel, the one-call step through the store pass's inline location"""
    from genedex_amd.device import DeviceQueries

    g = case.g
    g.set_query_options(locate_kernel=locate_kernel, locate_jump_walk=jump_walk)
    try:
        for compact, fused in ((False, False), (True, True)):
            off, hits, _, _, _ = device_locate(g, case.qs, compact, fused=fused, max_hits=3 if fused else 0)
            want_off, want_t, want_p = capped(case.co, case.ct, case.cp, 3 if fused else 0)
            assert off.tolist() == want_off.tolist()
            assert hits[:, 0].tolist() == want_t.tolist() and hits[:, 1].tolist() == want_p.tolist()
        assert_step(g, DeviceQueries.from_host(*pack_queries(case.qs)), case.co, case.ct, case.cp)
        check_against_oracle(g, case.c, case.qs)
    finally:
        g.set_query_options()


def hit_sparse_batch(case, n_absent=40000, seed=3):
    """the record-decided reads scattered among many absent ones: most hit chunks span thousands of reads"""
    rng = np.random.default_rng(seed)
    reads = [case.qs[i] for i in sorted(case.decided)]
    absent = [bytes(b"ACGT"[x] for x in rng.integers(0, 4, case.k + 20)) for _ in range(n_absent)]
    at = np.sort(rng.choice(n_absent + len(reads), size=len(reads), replace=False))
    out, j, r = [], 0, 0
    for i in range(n_absent + len(reads)):
        if r < len(reads) and at[r] == i:
            out.append(reads[r])
            r += 1
        else:
            out.append(absent[j])
            j += 1
    return out


def test_hit_sparse_batch(case):
    """a few record-decided reads among 40 000 absent ones through the one-call step (flagged chunks: locate_stream_kernel)
    and the separate calls"""
    from genedex_amd.device import DeviceQueries

    qs = hit_sparse_batch(case)
    co, ct, cp = case.c.locate_many(qs)
    assert int(co[-1]) < len(qs) // 10
    for max_hits in (0, 2):
        assert_step(case.g, DeviceQueries.from_host(*pack_queries(qs)), co, ct, cp, max_hits)
    off, hits, _, _, _ = device_locate(case.g, qs, True, fused=True)
    assert off.tolist() == co.tolist()
    assert hits[:, 0].tolist() == ct.astype(np.uint32).tolist() and hits[:, 1].tolist() == cp.astype(np.uint32).tolist()


def _by_query_off_child(shape):
    """(run in a child process with GDX_LOCATE_BY_QUERY=0, which the library reads once per process)"""
    texts, fams = crafted_texts()
    c = cpu_index(texts, A)
    case = make_case(texts, fams, c, gpu_index(texts, A, **SHAPES[shape]))
    from genedex_amd.device import DeviceQueries

    for compact, fused in ((False, False), (True, False), (True, True)):
        for max_hits in (0, 3):
            off, hits, _, _, _ = device_locate(case.g, case.qs, compact, max_hits=max_hits, fused=fused)
            want_off, want_t, want_p = capped(case.co, case.ct, case.cp, max_hits)
            assert off.tolist() == want_off.tolist()
            assert hits[:, 0].tolist() == want_t.tolist() and hits[:, 1].tolist() == want_p.tolist()
    check_against_oracle(case.g, case.c, case.qs)
    qs = hit_sparse_batch(case)
    co, ct, cp = c.locate_many(qs)
    assert_step(case.g, DeviceQueries.from_host(*pack_queries(qs)), co, ct, cp)
    off, hits, _, _, _ = device_locate(case.g, qs, False)
    assert off.tolist() == co.tolist() and hits[:, 1].tolist() == cp.astype(np.uint32).tolist()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_stream_kernel_instead_of_by_query(shape):
    """GDX_LOCATE_BY_QUERY=0: the separate calls' hits come from locate_stream_kernel too (the variable is read once per
    process, so a fresh child process runs the checks)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GDX_LOCATE_BY_QUERY="0")
    code = ("import sys; sys.path.insert(0, 'tests'); import test_gpu_seed_records as t; "
            f"t._by_query_off_child({shape!r}); print('child ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])


# ---- query forms --------------------------------------------------------------------------------------------------------

def test_every_alignment_of_the_query_starts(case):
    """the ASCII batch starting 0 .. 7 bytes into its buffer: every read starts at every residue of begin & 7 once"""
    import torch

    from genedex_amd.device import DeviceQueries

    qbuf, qoff = pack_queries(case.qs)
    total = int(qoff[-1])
    for base in range(8):
        buf = np.zeros((base + total + 8 + 7) // 8 * 8, dtype=np.uint8)
        buf[base:base + total] = qbuf[:total]
        off = torch.from_numpy(qoff.astype(np.int64) + base).cuda()
        dq = DeviceQueries(torch.from_numpy(buf).cuda(), off, len(case.qs), base + total)
        kinds = assert_records(case, search_records(case.g, dq))
        assert min(kinds.values()) >= MIN_PER_KIND, (base, kinds)
        assert_step(case.g, dq, case.co, case.ct, case.cp, max_hits=base % 5)


def test_uniform_and_packed_batches(case):
    """reads of one length (as_uniform: no offsets) in ASCII and as 2-bit codes, and the whole batch as 2-bit codes: the same
    records and the oracle's hits"""
    from genedex_amd.device import DeviceQueries

    dq = DeviceQueries.from_host(*pack_queries(case.qs)).as_packed(case.g)
    kinds = assert_records(case, search_records(case.g, dq))
    assert min(kinds.values()) >= MIN_PER_KIND, kinds
    assert_step(case.g, dq, case.co, case.ct, case.cp)
    lens = np.array([len(q) for q in case.qs])
    rng = np.random.default_rng(7)
    seen = dict.fromkeys(KINDS, 0)
    for n_v in (1, 2, 16, 31, 32, 33):
        idx = np.flatnonzero(lens == case.k + n_v)
        assert idx.size > 20, n_v
        ln = case.k + n_v
        lead = [bytes(b"ACGT"[x] for x in rng.integers(0, 4, ln)) for _ in range(-(-LEAD // ln))]
        qs = lead + [case.qs[i] for i in idx]
        idx = [-1] * len(lead) + idx.tolist()
        co, ct, cp = case.c.locate_many(qs)
        plain = DeviceQueries.from_host(*pack_queries(qs))
        for dq in (plain.as_uniform(case.k + n_v), plain.as_packed(case.g).as_uniform(case.k + n_v)):
            got = assert_records(case, search_records(case.g, dq), idx)
            assert n_v == 33 or sum(got.values()) > 0
            for kd, v in got.items():
                seen[kd] += v
            assert_step(case.g, dq, co, ct, cp)
            assert_step(case.g, dq, co, ct, cp, max_hits=2)
    assert min(seen.values()) >= MIN_PER_KIND, seen


# ---- A/B and other builds -----------------------------------------------------------------------------------------------

def test_records_switched_off_give_the_same_outputs(case, monkeypatch):
    """GDX_SEARCH_SEED_PAIRS=0 (read per call): the same reads take the general verify path -- their raw records show it --
    with the same outputs; switched back on, the raw records are the model's again"""
    from genedex_amd.device import DeviceQueries

    monkeypatch.setenv("GDX_SEARCH_SEED_PAIRS", "0")
    for compact, fused in ((False, False), (True, True), (True, "search")):
        off, hits, _, _, _ = device_locate(case.g, case.qs, compact, fused=fused)
        assert off.tolist() == case.co.tolist()
        assert hits[:, 0].tolist() == case.ct.astype(np.uint32).tolist()
        assert hits[:, 1].tolist() == case.cp.astype(np.uint32).tolist()
    check_against_oracle(case.g, case.c, case.qs)
    # ... and the other path was really taken: the general kernel writes a dead or single-row read as {row, row, ..} /
    # {row, row + 1, ..} where a record writes {0, 0, ..} / {0, 1, ..}
    dq = DeviceQueries.from_host(*pack_queries(case.qs))
    off_rec = search_records(case.g, dq)
    other = {kd: 0 for kd in ("none", "one")}
    for i, (kind, _, want, _) in case.decided.items():
        if kind in other and tuple(int(x) for x in off_rec[i]) != want:
            assert int(off_rec[i][0]) != 0, (i, kind)
            other[kind] += 1
    assert min(other.values()) >= MIN_PER_KIND, other
    monkeypatch.delenv("GDX_SEARCH_SEED_PAIRS")
    kinds = assert_records(case, search_records(case.g, dq))
    assert min(kinds.values()) >= MIN_PER_KIND


def test_loaded_index_has_the_same_records(crafted, tmp_path):
    """an index saved and loaded back with the default build options (gdx_index_load_ex) builds the same records"""
    from genedex_amd import FmIndex
    from genedex_amd.device import DeviceQueries

    texts, fams, c = crafted
    g = gpu_index(texts, A)
    path = tmp_path / "records.gdx"
    g.save_to_file(path)
    loaded = FmIndex.load_from_file(path, A)
    case = make_case(texts, fams, c, loaded)
    assert loaded.seed_info()["pair_records"] == g.seed_info()["pair_records"] == case.model.pair_records
    assert loaded.seed_info()["quad_records"] == g.seed_info()["quad_records"] == case.model.quad_records
    kinds = assert_records(case, search_records(loaded, DeviceQueries.from_host(*pack_queries(case.qs))))
    assert min(kinds.values()) >= MIN_PER_KIND
    check_against_oracle(loaded, c, case.qs)


def test_budget_that_admits_pair_records_only_or_neither(crafted):
    """aux_budget_bytes with room for the seed table and its pair records but not the quad records, then for neither.
    The default shape cannot be kept under such a budget: it is only chosen when the budget holds 1.25 times its estimate
    of the seed table (16 bytes per symbol over the load factor) beside 8.5 bytes per symbol, which always leaves room for
    both kinds of record.  So the same structures are asked for explicitly (k = 16, no jump or top table, whose shrinking
    would move the room), and the budgets are computed from the seed_info() of a build without a limit.

    A build whose placement turns an entry away starts over with a quarter more buckets, and whether it does depends on the
    order of the insert kernel's atomics.  So each budgeted build's records are checked against the rule of its own table
    (records fit when table + 32 bytes per pair record, then + 64 per quad record, fit the room beside the other structures);
    a load factor of 70 % keeps such retries rare, and the intended outcome is asserted where the tables are alike."""
    from genedex_amd.device import DeviceEngine, DeviceQueries

    texts, fams, c = crafted
    rng = np.random.default_rng(5)
    texts = texts + [bytes(b"ACGT"[i] for i in rng.integers(0, 4, 90000))]  # (unique k-mers: a larger table, room above the floor)
    c = cpu_index(texts, A)
    load = 70
    opts = dict(seed_symbols=16, seed_load_percent=load, jump_entry_bytes=0, top_table_depth=0, full_suffix_array=True,
                inverse_suffix_array=True)
    g = gpu_index(texts, A, **opts)
    info, aux = g.seed_info(), DeviceEngine(g).aux_info()
    table = info["buckets"] * 128
    assert info["bytes"] == table + 32 * info["pair_records"] + 64 * info["quad_records"]
    others = aux["aux_bytes"] - info["bytes"]  # suffix array, inverse suffix array, text units
    floor = 1.25 * 16 / (load / 100) * g.total_text_len()  # (an explicit k whose estimated table exceeds the budget is refused)
    pairs, quads = info["pair_records"], info["quad_records"]
    assert pairs > 0 and 64 * quads > 16 * pairs
    tables_alike = 0
    for budget, intended in ((others + table + 32 * pairs + 32 * quads, (pairs, 0)), (others + table + 16 * pairs, (0, 0))):
        assert budget >= floor, "the crafted texts no longer leave room above the seed table's floor"
        b = gpu_index(texts, A, aux_budget_bytes=budget, **opts)
        bi = b.seed_info()
        b_table = bi["buckets"] * 128
        room = budget - (DeviceEngine(b).aux_info()["aux_bytes"] - bi["bytes"])
        want_pairs = pairs if b_table + 32 * pairs <= room else 0
        want_quads = quads if b_table + 32 * want_pairs + 64 * quads <= room else 0
        assert (bi["pair_records"], bi["quad_records"]) == (want_pairs, want_quads), (budget, room, bi)
        assert bi["bytes"] == b_table + 32 * want_pairs + 64 * want_quads
        if bi["buckets"] == info["buckets"]:
            assert (want_pairs, want_quads) == intended
            tables_alike += 1
        case = make_case(texts, fams, c, b)
        # the reads of three- and four-copy k-mers (and of two-copy ones without pair records) take the general path now
        check_against_oracle(b, c, case.qs)
        dq = DeviceQueries.from_host(*pack_queries(case.qs))
        assert_step(b, dq, case.co, case.ct, case.cp)
        if want_pairs:
            rec = search_records(b, dq)
            pair_reads = [i for i, r in case.decided.items() if r[0] != "none" and
                          case.model.kmers[case.model.dense_of(case.qs[i][-case.k:])][2] == "pair"]
            assert len(pair_reads) >= MIN_PER_KIND
            for i in pair_reads:
                assert tuple(int(x) for x in rec[i]) == case.decided[i][2], i
    assert tables_alike > 0, "every budgeted build placed its table differently: neither intended budget case ran"


def test_records_at_k24():
    """the production k (21 tag bits, a 48-bit key) on the crafted texts: 2^27 buckets (17 GB), nearly all empty"""
    import torch

    from genedex_amd.device import DeviceQueries

    if torch.cuda.mem_get_info()[0] < 40e9:
        pytest.skip("needs 40 GB of free device memory")
    texts, fams = crafted_texts(seed=24)
    c = cpu_index(texts, A)
    g = gpu_index(texts, A, seed_symbols=24, jump_entry_bytes=0, full_suffix_array=True, inverse_suffix_array=True)
    info = g.seed_info()
    assert info["k"] == 24 and info["tag_bits"] == 21
    case = make_case(texts, fams, c, g)
    assert (info["pair_records"], info["quad_records"]) == (case.model.pair_records, case.model.quad_records)
    kinds = assert_records(case, search_records(g, DeviceQueries.from_host(*pack_queries(case.qs))))
    assert min(kinds.values()) >= MIN_PER_KIND, kinds
    check_against_oracle(g, c, case.qs)
    off, hits, _, _, _ = device_locate(g, case.qs, True, fused=True, max_hits=2)
    want_off, want_t, want_p = capped(case.co, case.ct, case.cp, 2)
    assert off.tolist() == want_off.tolist() and hits[:, 1].tolist() == want_p.tolist()
