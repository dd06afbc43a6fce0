"""The exhaustive sweep: the read ENDING at every text position of one small collection, at every length where the query kernels
change path, through every index shape and search variant of test_gpu_parity._VARIANTS -- so that no row, no text position and
no seed entry of an index stays unvisited, whatever a sample would have drawn.

Expected values come from sweep_model.py: the proved suffix array, neighbouring-row LCPs and nothing else (no rank structure, no
LF step, no backward search); reads with one substituted symbol are counted by a dictionary over the texts' windows.  Every
comparison goes through check(), which names the variant, the call, the length, the text and the position of the first offending
read.  N inside a read is a legal symbol here (lookup depth 0: an LF step consumes it)."""
import numpy as np
import pytest

from genedex_amd import alphabet as alph
from sweep_model import K, NEAR_MISS_KINDS, build_sweep_model, locate_lengths, near_miss_lengths, sweep_lengths
from test_gpu_parity import _VARIANTS, gpu_index

pytestmark = pytest.mark.gpu

A = alph.ascii_dna_with_n()
WALKING = ("verify-walk", "seed-walk", "pair-narrow")     # no SA[row] at hand: these walk to a sample
HEADLINE = ("default", "seed-sa", "seed-all", "seed-isa")  # the one-call count + locate step runs on these
KINDS = ("cursors", "count", "locate", "near-misses")


def has_seed_table(variant):
    """a seed table is asked for, or the build makes the default shape, which has one (aux_plan.hpp plan_aux_shape: none of its
    structures asked for or switched off, on the library's own table layout)"""
    build = _VARIANTS[variant][1]
    named = ("seed_symbols", "jump_entry_bytes", "full_suffix_array", "inverse_suffix_array", "text_units", "reference_table_layout")
    return bool(build.get("seed_symbols")) or (not any(o in build for o in named) and build.get("pair_lines") is not False)


CASES = [(v, kind) for v in _VARIANTS
         for kind in KINDS + (("seed-entries",) if has_seed_table(v) else ()) + (("step",) if v in HEADLINE else ())]


@pytest.fixture(scope="module")
def model():
    return build_sweep_model()


@pytest.fixture(scope="module")
def index_of(model):
    """variant -> (index, k): built once per variant (the cases of a variant follow each other; one index is kept)"""
    kept = {}

    def get(variant):
        if variant not in kept:
            kept.clear()
            query, build = _VARIANTS[variant]
            g = gpu_index(model.texts, A, sa_rate=5 if variant in WALKING else 4, **build)
            if query:
                g.set_query_options(**query)
            k = g.seed_info()["k"]
            assert (k > 0) == has_seed_table(variant), (variant, k)
            assert g.total_text_len() == model.n and g.num_texts() == len(model.texts)
            kept[variant] = (g, k if k else K)
        return kept[variant]

    yield get
    kept.clear()


def check(model, variant, call, length, what, want, got, read_of=None, subset=None):
    """THE comparison of the sweep: `got` equals `want` element for element, else an AssertionError that names the first
    offending read.  read_of: element -> read (elements that are hits); subset: read -> read of the whole sweep."""
    want, got = np.asarray(want).astype(np.int64), np.asarray(got).astype(np.int64)
    if want.shape == got.shape and np.array_equal(want, got):
        return
    m = min(want.size, got.size)
    differ = np.flatnonzero(want[:m] != got[:m])
    at = int(differ[0]) if differ.size else m
    where = f"{variant}: {call} at L = {length}, {what}"
    if at >= want.size or at >= got.size:
        raise AssertionError(f"{where}: {want.size} elements expected, {got.size} got (equal up to there)")
    read = int(read_of[at]) if read_of is not None else at
    if subset is not None:
        read = int(subset[read])
    raise AssertionError(f"{where}: {model.where(length, read)}: expected {int(want[at])}, got {int(got[at])} "
                         f"({int(differ.size)} of {m} elements differ)")


def check_hits(model, variant, call, length, want, got, subset=None):
    """offsets, text ids and positions of a batch, in the model's order"""
    (woff, wt, wp), (off, t, p) = want, got
    nq = woff.size - 1
    check(model, variant, call, length, "hit offsets", woff, off, read_of=np.maximum(np.arange(nq + 1) - 1, 0), subset=subset)
    owner = np.repeat(np.arange(nq), np.diff(woff))
    check(model, variant, call, length, "text ids of the hits", wt, t, read_of=owner, subset=subset)
    check(model, variant, call, length, "positions of the hits", wp, p, read_of=owner, subset=subset)


def subset_hits(model, length, keep):
    """the model's hits of the reads in `keep` (bool per read) as a batch of their own"""
    off, tid, pos = model.hits(length)
    counts = np.diff(off)
    sel = np.repeat(keep, counts)
    return np.concatenate([[0], np.cumsum(counts[keep])]).astype(np.int64), tid[sel], pos[sel]


# ---- the calls -----------------------------------------------------------------------------------------------------------

def sweep_cursors(model, variant, g, k):
    for length in sweep_lengths(k):
        lo, hi = model.intervals(length)
        s, e, st = g.cursors_raw(*model.reads(length))
        check(model, variant, "cursors_raw", length, "status", np.zeros_like(lo), st)
        check(model, variant, "cursors_raw", length, "interval start", lo, s)
        check(model, variant, "cursors_raw", length, "interval end", hi, e)


def sweep_counts(model, variant, g, k):
    for length in sweep_lengths(k):
        lo, hi = model.intervals(length)
        counts, st = g.count_raw(*model.reads(length))
        check(model, variant, "count_raw", length, "status", np.zeros_like(lo), st)
        check(model, variant, "count_raw", length, "count", hi - lo, counts)


def sweep_locate(model, variant, g, k):
    for length in locate_lengths(k):
        off, t, p, st = g.locate_raw(*model.reads(length))
        check(model, variant, "locate_raw", length, "status", np.zeros(st.size), st)
        check_hits(model, variant, "locate_raw", length, model.hits(length), (off, t, p))


_NEAR = {}  # (length, kind, k) -> (batch, counts): the dictionary's answers, computed once for all variants


def near_miss_batch(model, length, kind, k):
    key = (length, kind, k if kind == "before-seed" else 0)
    if key not in _NEAR:
        reads = model.near_misses(length, kind, k)
        _NEAR[key] = (model.as_batch(reads), model.window_counts(reads))
    return _NEAR[key]


def sweep_near_misses(model, variant, g, k):
    for length in near_miss_lengths(k):
        for kind in NEAR_MISS_KINDS:
            if kind == "before-seed" and length == k:
                continue  # (no symbol in front of the seed)
            (qbuf, qoff), want = near_miss_batch(model, length, kind, k)
            call = f"one symbol off ({kind})"
            counts, st = g.count_raw(qbuf, qoff)
            check(model, variant, "count_raw, " + call, length, "status", np.zeros_like(want), st)
            check(model, variant, "count_raw, " + call, length, "count", want, counts)
            s, e, st = g.cursors_raw(qbuf, qoff)
            check(model, variant, "cursors_raw, " + call, length, "status", np.zeros_like(want), st)
            # (where the frozen empty interval stands is the reference's business: the model does not define it)
            check(model, variant, "cursors_raw, " + call, length, "end - start", want, e.astype(np.int64) - s.astype(np.int64))


def seed_entries(model, variant, g, k):
    """the table holds every kind of entry and record, and the sweep at length k asks for every k-mer it holds"""
    info = g.seed_info()
    assert info["k"] == k
    for name in ("single_entries", "interval_entries", "pair_records", "quad_records"):
        assert info[name] > 0, (variant, name, info)
    if _VARIANTS[variant][1].get("seed_load_percent") == 100:
        assert info["overflowed_buckets"] > 0, (variant, info)
    code, start = model.kmer_codes(k)
    reads = model.gathered(k)[model.clean(k)]
    seeds = np.zeros(reads.shape[0], dtype=np.int64)
    for j in range(k):
        seeds = seeds * 4 + (A.io_to_dense_table[reads[:, j]].astype(np.int64) - 1)
    distinct, inverse, rows = np.unique(code, return_inverse=True, return_counts=True)
    assert np.array_equal(np.unique(seeds), distinct)
    # one entry per distinct k-mer; a record per k-mer on two (three or four) rows with 32 symbols A C G T in front of each
    assert info["single_entries"] + info["interval_entries"] == distinct.size, (variant, info)
    whole = np.bincount(inverse, weights=model.clean_symbols_in_front(32)[start] < 32, minlength=distinct.size) == 0
    assert info["pair_records"] == int(((rows == 2) & whole).sum()), (variant, info)
    assert info["quad_records"] == int((((rows == 3) | (rows == 4)) & whole).sum()), (variant, info)


def step(g, dq, capacity, max_hits=0):
    """gdx_locate_many_step_compact_layout_dev: (offsets, text ids, positions, counts, status) of the batch"""
    import torch

    from genedex_amd.device import DeviceEngine

    eng = DeviceEngine(g)
    nq = dq.nq
    rec, cw = eng.alloc_records(nq), eng.alloc_compact(nq)
    sws = torch.empty(max(eng.totals_workspace_bytes(nq), 16), dtype=torch.uint8, device="cuda")
    totals = torch.zeros(2, dtype=torch.int64, device="cuda")
    off = torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda")
    hits = torch.full((capacity, 2), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(eng.locate_workspace_bytes(capacity), 16), dtype=torch.uint8, device="cuda")
    eng.locate_step(dq, rec, cw, sws, totals, off, hits, ws, max_hits=max_hits)
    counts = torch.empty(nq, dtype=torch.int32, device="cuda")
    status = torch.empty(nq, dtype=torch.uint8, device="cuda")
    eng.unpack_records(rec, nq, counts, status, compact=cw)
    torch.cuda.synchronize()
    stored = min(int(totals[0].item()), capacity)
    h = hits[:stored].cpu().numpy()
    return off.cpu().numpy(), h[:, 0], h[:, 1], counts.cpu().numpy(), status.cpu().numpy()


def sweep_step(model, variant, g, k):
    """the headline path: search, totals, offsets and hits in one call, on ASCII reads with offsets, the same declared uniform,
    and the N-free reads as 2-bit codes of uniform length; once with a cap of two hits per read"""
    from genedex_amd.device import DeviceQueries

    for length in sorted({k, k + 32, k + 33, 50}):
        qbuf, qoff = model.reads(length)
        want = model.hits(length)
        clean = model.clean(length)
        plain = DeviceQueries.from_host(qbuf, qoff)
        forms = [("ASCII + offsets", plain, want, None),
                 ("ASCII, uniform", plain.as_uniform(length), want, None),
                 ("2-bit, uniform", DeviceQueries.from_host(*model.as_batch(model.gathered(length)[clean])).as_packed(g)
                  .as_uniform(length), subset_hits(model, length, clean), np.flatnonzero(clean))]
        for form, dq, (woff, wt, wp), subset in forms:
            call = f"locate_step ({form})"
            off, t, p, counts, st = step(g, dq, int(woff[-1]) + 8)
            check(model, variant, call, length, "status", np.zeros(dq.nq), st, subset=subset)
            check(model, variant, call, length, "count", np.diff(woff), counts, subset=subset)
            check_hits(model, variant, call, length, (woff, wt, wp), (off, t, p), subset=subset)
    woff, wt, wp = model.capped_hits(50, 2)
    off, t, p, counts, st = step(g, DeviceQueries.from_host(*model.reads(50)), int(woff[-1]) + 8, max_hits=2)
    call = "locate_step (ASCII + offsets, max_hits = 2)"
    check(model, variant, call, 50, "count", np.diff(model.hits(50)[0]), counts)  # (counted all the same)
    check_hits(model, variant, call, 50, (woff, wt, wp), (off, t, p))
    assert int(np.diff(model.hits(50)[0]).max()) > 2 and int(woff[-1]) > 0


_SWEEPS = {"cursors": sweep_cursors, "count": sweep_counts, "locate": sweep_locate, "near-misses": sweep_near_misses,
           "seed-entries": seed_entries, "step": sweep_step}


@pytest.fixture(scope="module")
def torch_started():
    """the first use of torch on the device takes seconds: not a part of any one case"""
    import torch

    torch.cuda.synchronize()


@pytest.mark.parametrize("variant,kind", CASES)
def test_sweep(model, index_of, torch_started, variant, kind):
    g, k = index_of(variant)
    _SWEEPS[kind](model, variant, g, k)


def test_every_variant_is_swept():
    for v in _VARIANTS:
        assert {kind for w, kind in CASES if w == v} >= set(KINDS), v
    assert {v for v, kind in CASES if kind == "step"} == set(HEADLINE)
    assert {v for v, kind in CASES if kind == "seed-entries"} >= {"default", "seed-sa", "seed-walk", "seed-all", "seed-isa",
                                                                  "seed-isa-nojump"}


def test_the_sweep_visits_every_row(model):
    """at length 1 the rows ISA[p] of the swept reads are all rows whose suffix does not start with a sentinel"""
    rows = np.sort(model.isa[model.windows(1)[0]])
    assert np.array_equal(rows, np.flatnonzero(model.dense[model.sa] != 0))
    assert model.n > 65_536 + 4_096


# ---- the other engines -----------------------------------------------------------------------------------------------------

def test_sweep_of_the_wide_engine(model):
    """the 64-bit engine (wide.hip) forced onto the collection: counts, intervals and hits of every read"""
    from genedex_amd import FmIndexConfig, _lib

    lib = _lib.load()
    lib.gdx_debug_force_wide(1)
    try:
        g = FmIndexConfig("i64").suffix_array_sampling_rate(4).construct_index(model.texts, A)
    finally:
        lib.gdx_debug_force_wide(0)
    assert g.info.index_width == 64 and g.total_text_len() == model.n
    sweep_counts(model, "wide", g, K)
    sweep_cursors(model, "wide", g, K)
    sweep_locate(model, "wide", g, K)


def test_sweep_of_the_partitioned_index(model):
    """several 32-bit indexes cut at text borders (parts.hip): counts are the model's; a read's hits come part after part, so
    they equal the model's as sets.  A text is never cut, so the tightest limit the collection admits is its longest text and
    the sentinel behind it."""
    from genedex_amd import PartitionedFmIndex

    g = PartitionedFmIndex.construct(model.texts, A, sa_rate=4, max_part_symbols=int(model.text_len.max()) + 1)
    assert g.num_parts >= 2 and g.total_text_len() == model.n and g.num_texts() == len(model.texts)
    for length in sweep_lengths(K):
        lo, hi = model.intervals(length)
        counts, st = g.count_raw(*model.reads(length))
        check(model, "parts", "count_raw", length, "status", np.zeros_like(lo), st)
        check(model, "parts", "count_raw", length, "count", hi - lo, counts)
    for length in locate_lengths(K):
        woff, wt, wp = model.hits(length)
        off, t, p, st = g.locate_raw(*model.reads(length))
        check(model, "parts", "locate_raw", length, "status", np.zeros(st.size), st)
        check(model, "parts", "locate_raw", length, "hit offsets", woff, off, read_of=np.maximum(np.arange(woff.size) - 1, 0))
        # the hits of a read as a set: sorted by (read, text, position) on both sides
        owner = np.repeat(np.arange(woff.size - 1), np.diff(woff))
        w_order = np.lexsort((wp, wt, owner))
        g_order = np.lexsort((p.astype(np.int64), t.astype(np.int64), owner))
        check(model, "parts", "locate_raw", length, "text ids of the sorted hits", wt[w_order], t[g_order], read_of=owner)
        check(model, "parts", "locate_raw", length, "positions of the sorted hits", wp[w_order], p[g_order], read_of=owner)
