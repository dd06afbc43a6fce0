"""gdx_mate_rescue_many[_dev] on the GPU against the CPU model of tests/test_mate_rescue_model.py (the definition of
include/gdx_experimental.h "mate rescue").  Outputs are integers: every comparison is exact, every output is filled with garbage
before the call."""
import ctypes as C

import numpy as np
import pytest

from genedex_amd import _lib, reversed_texts
from genedex_amd import alphabet as alph
from test_edit_distance_model import INVALID, NO_END, TOO_LONG
from test_gpu_candidates import GARBAGE
from test_gpu_parity import gpu_index
from test_mate_rescue_model import (A, NONE, NOT_TRIED, OUT_NAMES, PLANTED, RC, TEXT, _anchor_view, assert_same, attempts_of,
                                    planted_pairs, random_rescue_case, random_text, rescue_model)
from test_strands_model import join

pytestmark = pytest.mark.gpu

PER_MATE = ("resc_dist", "resc_end", "win_query", "win_begin")
PER_PAIR = ("resc_mate", "resc_pair_dist", "resc_span")
BLOCK, MAX_GRID = 256, 1024           # the kernel's workgroup (one sweep of a tile is 256 pairs) and the launcher's largest grid
_CASE = {}


def texts_and_engine():
    """three texts of a few thousand symbols with some N (a short one in the middle, so that windows are clipped at text ends that
    have neighbours on both sides) and the engine on their index, made once"""
    from genedex_amd.device import DeviceEngine

    if "eng" not in _CASE:
        rng = np.random.default_rng(22200)
        _CASE["texts"] = [random_text(rng, 3001, 0.01), random_text(rng, 41, 0), random_text(rng, 5500, 0.01)]
        _CASE["g"] = gpu_index(_CASE["texts"], A)
        _CASE["eng"] = DeviceEngine(_CASE["g"])
    return _CASE["texts"], _CASE["g"], _CASE["eng"]


def to_device(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(np.uint32)).view(np.int32)).cuda()


def garbage_rescue(n_pairs):
    import torch

    n = max(n_pairs, 1)
    out = {name: torch.full((2 * n,), GARBAGE, dtype=torch.int32, device="cuda") for name in PER_MATE}
    out.update({name: torch.full((n,), GARBAGE, dtype=torch.int32, device="cuda") for name in PER_PAIR})
    out["win_hits"] = torch.full((2 * n, 2), GARBAGE, dtype=torch.int32, device="cuda")
    return out


def rescue_from_device(out, n_pairs):
    """the nine arrays in the model's order"""
    import torch

    torch.cuda.synchronize()
    u32 = lambda name, n: out[name].cpu().numpy().view(np.uint32)[:n]  # noqa: E731
    hits = out["win_hits"].cpu().numpy().view(np.uint32).reshape(-1, 2)[:2 * n_pairs]
    return (u32("resc_dist", 2 * n_pairs), u32("resc_end", 2 * n_pairs)) + tuple(u32(name, n_pairs) for name in PER_PAIR) + \
        (u32("win_query", 2 * n_pairs), u32("win_begin", 2 * n_pairs), hits[:, 0], hits[:, 1])


def pairs_to_device(case):
    """the inputs behind the queries as the `pairs` dict of pair_hits() and the end tensor"""
    _, end, n_proper, mate_slot, mate_dist, wq, wb, wt, wp = case
    pairs = {"n_proper": to_device(n_proper), "mate_slot": to_device(mate_slot), "mate_dist": to_device(mate_dist),
             "win_query": to_device(wq), "win_begin": to_device(wb), "win_hits": to_device(np.stack([wt, wp], axis=1))}
    return pairs, to_device(end)


def device_call(eng, dq, case, n_pairs, ms, k, lo, hi, tile=None, grid=None):
    """gdx_mate_rescue_many_dev on host-made inputs, every output GARBAGE beforehand -> the nine arrays.  tile, grid: the
    launcher's shape for this call (gdx_debug_set_rescue_tiling; None = its default)"""
    pairs, end = pairs_to_device(case)
    out = garbage_rescue(n_pairs)
    lib = _lib.load()
    lib.gdx_debug_set_rescue_tiling(tile or 0, grid or 0)
    try:
        assert eng.mate_rescue(dq, end, pairs, n_pairs, ms, k, lo, hi, out=out) is out
    finally:
        lib.gdx_debug_set_rescue_tiling(0, 0)
    return rescue_from_device(out, n_pairs)


def batch(queries):
    from genedex_amd.device import DeviceQueries

    return DeviceQueries.from_host(*join(queries))


# ------------------------------------------------------------------------------------------------
# 1. read lengths, the four layouts, every W instance and the offsets instance, k

@pytest.mark.parametrize("length", (1, 63, 64, 65, 128, 129, 256, 257))
def test_read_lengths_in_all_four_layouts(length):
    texts, g, eng = texts_and_engine()
    rng = np.random.default_rng(22300 + length)
    n, ms, lo, hi = 70, 3, 100, 131
    for k in (0, 3, 256):
        case = random_rescue_case(rng, texts, n, ms, k, lo, hi, (length,), n_rate=0)     # (no N: the batch packs)
        want = rescue_model(texts, A, *case, n, ms, k, lo, hi)
        plain = batch(case[0])
        forms = {"plain": plain, "uniform": plain.as_uniform(length), "packed": plain.as_packed(g),
                 "packed + uniform": plain.as_uniform(length).as_packed(g)}
        for name, dq in forms.items():
            assert_same(device_call(eng, dq, case, n, ms, k, lo, hi), want, f"{name}, k = {k}")
        tried = want[0] != NOT_TRIED
        if length == 257:
            assert tried.any() and np.isin(want[0][tried], (TOO_LONG, INVALID)).all() and (want[2] == NONE).all()
        else:
            assert (want[0] <= k).any() and (want[0] == NOT_TRIED).any() and (k == 256 or (want[0] == k + 1).any())


def test_mixed_lengths_in_the_offsets_instance():
    texts, g, eng = texts_and_engine()
    rng = np.random.default_rng(22400)
    n, ms, lo, hi = 300, 5, 100, 131
    for k, n_rate in ((0, 0.02), (3, 0.02), (256, 0)):
        lengths = (0, 1, 31, 32, 33, 63, 64, 65, 128, 129, 191, 192, 193, 256, 257)
        case = random_rescue_case(rng, texts, n, ms, k, lo, hi, lengths, n_rate=n_rate)
        want = rescue_model(texts, A, *case, n, ms, k, lo, hi)
        assert_same(device_call(eng, batch(case[0]), case, n, ms, k, lo, hi), want, f"plain, k = {k}")
        if n_rate == 0:
            assert_same(device_call(eng, batch(case[0]).as_packed(g), case, n, ms, k, lo, hi), want, f"packed, k = {k}")
        d = want[0]
        assert (d == TOO_LONG).any() and (d == INVALID).any() and (d <= k).any() and (d == NOT_TRIED).any()
        # pass-through: a pair with a proper combination and a pair with both mates dead copy their winners and are not tried
        n_proper, slot = np.asarray(case[2]), np.asarray(case[3]).reshape(n, 2)
        quiet = (n_proper != 0) | (slot == NONE).all(axis=1)
        assert (n_proper != 0).any() and ((n_proper == 0) & (slot == NONE).all(axis=1)).any()
        both = np.repeat(quiet, 2)
        assert (d[both] == NOT_TRIED).all() and (want[1][both] == NO_END).all() and (want[2][quiet] == NONE).all()
        assert (want[3][quiet] == 2 * k + 2).all() and (want[4][quiet] == 0).all()
        for mine, theirs in zip(want[5:], case[5:]):
            assert np.array_equal(mine[both], np.asarray(theirs)[both])


# ------------------------------------------------------------------------------------------------
# 2. the spread (the text-unit edge, and the cap), every phase of the window's start in a text unit, windows clipped at text ends

@pytest.mark.parametrize("spread", (0, 1, 31, 32, 33, 4096))
def test_spreads_and_window_phases(spread):
    texts, g, eng = texts_and_engine()
    rng = np.random.default_rng(22500 + spread)
    n, ms, k, L, lo = (40 if spread == 4096 else 400), 2, 3, 50, 90
    case = random_rescue_case(rng, texts, n, ms, k, lo, lo + spread, (L,), bad=False)
    want = rescue_model(texts, A, *case, n, ms, k, lo, lo + spread)
    assert_same(device_call(eng, batch(case[0]), case, n, ms, k, lo, lo + spread), want, "plain")
    assert_same(device_call(eng, batch(case[0]).as_uniform(L), case, n, ms, k, lo, lo + spread), want, "uniform")
    # what the inputs show: windows that begin at every residue of a text unit (counted in the concatenation, as the kernel
    # does), windows cut at the start and at the end of a text, found and not found
    v = _anchor_view([len(q) for q in case[0]], *case[1:2], *case[3:4], *case[5:], n, ms, lo, lo + spread)
    tried = attempts_of(case[2], case[3], n)
    size = np.array([len(t) for t in texts])[v["T"]]
    t0 = np.concatenate([[0], np.cumsum([len(t) + 1 for t in texts])])[v["T"]]
    raw0, x1 = v["ylo"] - L - k, np.clip(v["yhi"], 0, size)
    x0 = np.clip(raw0, 0, size)
    if spread != 4096:
        assert set(((t0 + x0)[tried] % 32).tolist()) == set(range(32))
    assert (tried & (raw0 < 0) & (x1 > 0)).any() and (tried & (v["yhi"] > size) & (x0 < size)).any()
    assert (want[0] <= k).any() and (want[0] == k + 1).any()


def test_a_neighbouring_text_does_not_continue_the_alignment():
    from genedex_amd.device import DeviceEngine

    # pair 0: the read runs three symbols over the end of text 0 into what text 1 begins with; the anchor is mate 0, forward on
    # diagonal 40 of text 0, and [35, 60] admits ends up to 100 where the text has 80 symbols.  Pair 1: the read begins with the
    # last three symbols of text 0 and goes on with the first seven of text 1; the anchor is mate 1, reverse, ending at 42 in text 1
    texts = [TEXT, b"GGG" + TEXT[:40]]
    eng = DeviceEngine(gpu_index(texts, A))
    tail, head = TEXT[73:] + b"GGG", TEXT[-3:] + b"GGG" + TEXT[:4]
    queries = [b"A", b"T", RC(tail), tail, head, RC(head), b"C", b"G"]
    for k in (3, 2):
        case = (queries, np.array([70, 0, 0, 42]), np.zeros(2), np.array([0, NONE, NONE, 0]), np.array([0, k + 1, k + 1, 0]),
                np.array([0, NONE, NONE, 7]), np.zeros(4), np.array([0, 0, 0, 1]), np.array([40, 0, 0, 32]))
        want = rescue_model(texts, A, *case, 2, 1, k, 35, 60)
        assert_same(device_call(eng, batch(queries), case, 2, 1, k, 35, 60), want, f"k = {k}")
        assert want[0].tolist() == [NOT_TRIED, 3, 3, NOT_TRIED]
        assert want[1].tolist() == ([NO_END, 80, 7, NO_END] if k == 3 else [NO_END] * 4)


# ------------------------------------------------------------------------------------------------
# 3. compaction: attempts per tile, tiles per workgroup, the grid

def close_all_but(case, n_pairs, attempts_per_tile, tile):
    """the case with n_proper set so that tile t keeps exactly attempts_per_tile[t] attempts (an int: in its first pairs; ("last",
    c) / ("first", c): in its last or first pairs only); every pair of the case must come with two attempts"""
    queries, end, n_proper, slot, md, wq, wb, wt, wp = (np.array(x) if i else x for i, x in enumerate(case))
    n_proper[:] = 1
    for t, want in enumerate(attempts_per_tile):
        where, c = want if isinstance(want, tuple) else ("first", want)
        pairs = np.arange(t * tile, min((t + 1) * tile, n_pairs))
        pairs = pairs[::-1] if where == "last" else pairs
        chosen = pairs[:(c + 1) // 2]
        n_proper[chosen] = 0
        if c % 2:                                                                 # one pair with a single attempt: mate 1 unplaced
            m = 2 * chosen[-1] + 1
            slot[m], wq[m], wb[m], wt[m], wp[m] = NONE, NONE, 0, 0, 0
    return queries, end, n_proper, slot, md, wq, wb, wt, wp


def test_attempts_per_tile_tiles_and_grids():
    texts, g, eng = texts_and_engine()
    rng = np.random.default_rng(22600)
    tile, ms, k, lo, hi, L = 512, 2, 2, 60, 75, 20
    per_tile = [0, 1, 255, 256, 257, 513, ("last", 2), ("first", 2), 1024, ("last", 1), 154]
    n = (len(per_tile) - 1) * tile + 77                                           # the last tile is a partial one
    full = random_rescue_case(rng, texts, n, ms, k, lo, hi, (L,), p_open=1, p_placed=1, bad=False)
    case = close_all_but(full, n, per_tile, tile)
    tried = attempts_of(case[2], case[3], n)
    counts = [int(tried[2 * t * tile:2 * (t + 1) * tile].sum()) for t in range(len(per_tile))]
    assert counts == [0, 1, 255, 256, 257, 513, 2, 2, 1024, 1, 154]
    assert tried[2 * (7 * tile) - 2:2 * (7 * tile)].all() and tried[2 * 7 * tile:2 * 7 * tile + 2].all() and tried[2 * 10 * tile - 1]
    want = rescue_model(texts, A, *case, n, ms, k, lo, hi)
    dq = batch(case[0]).as_uniform(L)
    # a tile of 512 pairs on one workgroup each, on one workgroup in all, on three; tiles of one sweep; the default tile (every
    # pair in one tile: 3000 attempts behind each other); a tile that is no multiple of a sweep is rounded up
    for tile_pairs, grid in ((tile, None), (tile, 1), (tile, 3), (256, None), (256, 5), (None, None), (1, 2), (700, None)):
        assert_same(device_call(eng, dq, case, n, ms, k, lo, hi, tile=tile_pairs, grid=grid), want, f"tile {tile_pairs}, grid {grid}")
    assert (want[0][tried] <= k).sum() * 4 > tried.sum() and (want[0][~tried] == NOT_TRIED).all()


def test_more_pairs_than_one_stride_of_the_largest_grid():
    import torch

    from genedex_amd.device import DeviceQueries

    # tiles of one sweep: one stride of the largest grid is 1024 * 256 pairs.  A pair's results depend on that pair alone, so the
    # model runs on the few open pairs (the first, the last, those around the stride's end and a sample), numbered anew
    texts, g, eng = texts_and_engine()
    rng = np.random.default_rng(22700)
    n, ms, k, lo, hi, L = MAX_GRID * BLOCK + 1, 2, 2, 60, 75, 16
    chosen = np.unique(np.concatenate([[0, 1, 255, 256, MAX_GRID * BLOCK - 1, MAX_GRID * BLOCK], rng.integers(0, n, 300)]))
    few = chosen.size
    small = random_rescue_case(rng, texts, few, ms, k, lo, hi, (L,), p_open=1, bad=False)
    want = [np.array(x) for x in rescue_model(texts, A, *small, few, ms, k, lo, hi)]
    mates = (2 * chosen[:, None] + np.arange(2)[None, :]).reshape(-1)
    shift = 4 * np.repeat(chosen - np.arange(few), 2)                             # a query number holds its pair's
    # the big batch: every other pair has a proper combination and some winner to be copied
    qbuf = np.full(4 * n * L + 8, ord("A"), dtype=np.uint8)
    rows = (4 * chosen[:, None] + np.arange(4)[None, :]).reshape(-1)
    qbuf.reshape(-1)[:4 * n * L].reshape(4 * n, L)[rows] = np.frombuffer(b"".join(small[0]), dtype=np.uint8).reshape(4 * few, L)
    n_proper = np.ones(n, dtype=np.int64)
    n_proper[chosen] = 0
    big = {"end": rng.integers(0, 1 << 20, 2 * n * ms), "slot": rng.integers(0, ms, 2 * n), "md": rng.integers(0, k + 1, 2 * n),
           "wq": rng.integers(0, 1 << 20, 2 * n), "wb": rng.integers(0, 9, 2 * n), "wt": rng.integers(0, 3, 2 * n),
           "wp": rng.integers(0, 3000, 2 * n)}
    big["end"].reshape(2 * n, ms)[mates] = np.asarray(small[1]).reshape(2 * few, ms)
    for name, x in zip(("slot", "md", "wq", "wb", "wt", "wp"), small[3:]):
        big[name][mates] = np.asarray(x)
    placed = big["wq"][mates] != NONE
    big["wq"][mates] = np.where(placed, big["wq"][mates] + shift, NONE)
    case = (None, big["end"], n_proper, big["slot"], big["md"], big["wq"], big["wb"], big["wt"], big["wp"])
    dq = DeviceQueries(torch.from_numpy(qbuf).cuda(), torch.zeros(1, dtype=torch.int64, device="cuda"), 4 * n, 4 * n * L, False, L)
    got = device_call(eng, dq, case, n, ms, k, lo, hi, tile=BLOCK)
    expect = [np.full(2 * n, NOT_TRIED), np.full(2 * n, NO_END), np.full(n, NONE), np.full(n, 2 * k + 2), np.zeros(n, dtype=np.int64),
              big["wq"].copy(), big["wb"].copy(), big["wt"].copy(), big["wp"].copy()]
    for i, name in enumerate(OUT_NAMES):
        at = chosen if name in PER_PAIR else mates
        expect[i][at] = want[i]
    expect[5][mates] = np.where(want[5] == NONE, NONE, want[5] + shift)             # (the model numbered the open pairs anew)
    rescued = want[2] != NONE
    assert_same(got, expect, "one stride and one pair")
    assert rescued.any() and (got[0][mates] == k + 1).any()


def test_permuted_pairs_give_permuted_results():
    texts, g, eng = texts_and_engine()
    rng = np.random.default_rng(22800)
    n, ms, k, lo, hi, L = 1500, 3, 3, 80, 120, 30
    case = random_rescue_case(rng, texts, n, ms, k, lo, hi, (L,), p_open=0.3)
    dq = batch(case[0]).as_uniform(L)
    first = device_call(eng, dq, case, n, ms, k, lo, hi, tile=256)
    assert_same(first, rescue_model(texts, A, *case, n, ms, k, lo, hi), "as made")
    perm = rng.permutation(n)                                                     # new pair i is old pair perm[i]
    mates = (2 * perm[:, None] + np.arange(2)[None, :]).reshape(-1)
    queries = [case[0][4 * p + j] for p in perm for j in range(4)]
    move = 4 * np.repeat(np.arange(n) - perm, 2)
    wq = np.asarray(case[5])[mates]
    moved = (queries, np.asarray(case[1]).reshape(2 * n, ms)[mates].reshape(-1), np.asarray(case[2])[perm], np.asarray(case[3])[mates],
             np.asarray(case[4])[mates], np.where(wq == NONE, NONE, wq + move), *(np.asarray(x)[mates] for x in case[6:]))
    second = device_call(eng, batch(queries).as_uniform(L), moved, n, ms, k, lo, hi, tile=256, grid=7)
    back = np.argsort(perm)
    mates_back = (2 * back[:, None] + np.arange(2)[None, :]).reshape(-1)
    undone = [np.asarray(x)[back if name in PER_PAIR else mates_back].astype(np.int64) for x, name in zip(second, OUT_NAMES)]
    undone[5] = np.where(undone[5] == NONE, NONE, undone[5] - move[mates_back])
    assert_same(undone, first, "un-permuted")


# ------------------------------------------------------------------------------------------------
# 4. the host form and the refusals

def test_host_form_equals_the_device_form():
    texts, g, eng = texts_and_engine()
    rng = np.random.default_rng(22900)
    for n, ms, k, lo, hi, lengths in ((200, 4, 3, 100, 140, (0, 1, 40, 64, 65, 200, 257)), (33, 32, 0, 0, 0, (25,)),
                                      (1, 1, 256, 50, 4146, (256,))):
        case = random_rescue_case(rng, texts, n, ms, k, lo, hi, lengths)
        want = rescue_model(texts, A, *case, n, ms, k, lo, hi)
        assert_same(g.mate_rescue_raw(*join(case[0]), *case[1:], n, ms, k, lo, hi), want, "host")
        assert_same(device_call(eng, batch(case[0]), case, n, ms, k, lo, hi), want, "device")
    none = np.zeros(0, dtype=np.uint32)
    empty = g.mate_rescue_raw(np.zeros(8, dtype=np.uint8), np.zeros(1, dtype=np.uint64), *[none] * 8, 0, 2, 3, 0, 9)
    assert all(x.size == 0 for x in empty)


def test_refused_calls_write_nothing():
    import torch

    from genedex_amd import FmIndexConfig
    from genedex_amd.device import DeviceEngine

    texts, g, eng = texts_and_engine()
    lib = _lib.load()
    z = torch.full((1024,), 7, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    dq = batch([b"ACGT"] * 8)
    ins = [p(z)] * 7                          # end, n_proper, mate_slot, mate_dist, win_query, win_begin, win_hits
    outs = [p(z[64 * (i + 1):]) for i in range(8)]

    def dev(ms=2, k=3, lo=100, hi=200, n=2, nq=8, lay=None, ins_=ins, outs_=outs, h=g._h, qbuf=p(dq.qbuf), qoff=p(dq.qoff)):
        return lib.gdx_mate_rescue_many_dev(h, qbuf, qoff, nq, lay, n, ms, *ins_, k, lo, hi, *outs_, None)

    bad_layout = _lib.QueryLayout()
    lib.gdx_query_layout_init(C.byref(bad_layout))
    bad_layout.packed = 2
    invalid = (dict(ms=0), dict(ms=33), dict(ms=1 << 31), dict(k=257), dict(k=0xFFFFFFFF), dict(lo=201, hi=200), dict(lo=0, hi=1 << 31),
               dict(lo=0xFFFFFFFF - 10, hi=0xFFFFFFFF), dict(lo=100, hi=4197), dict(lo=0, hi=(1 << 31) - 1), dict(nq=7), dict(nq=12),
               dict(n=3), dict(n=0), dict(n=1 << 62, nq=0), dict(n=1 << 30, nq=1 << 32), dict(lay=C.byref(bad_layout)),
               dict(qoff=None), dict(qbuf=None))
    for kw in invalid:
        assert dev(**kw) == _lib.GDX_ERR_INVALID_ARGUMENT, kw
    for missing in range(7):
        assert dev(ins_=[None if i == missing else x for i, x in enumerate(ins)]) == _lib.GDX_ERR_INVALID_ARGUMENT, missing
    for missing in range(8):
        assert dev(outs_=[None if i == missing else x for i, x in enumerate(outs)]) == _lib.GDX_ERR_INVALID_ARGUMENT, missing
    torch.cuda.synchronize()
    assert (z.cpu().numpy() == 7).all()                                            # nothing was written so far
    assert dev(lo=100, hi=4196) == _lib.GDX_OK                                    # the spread at its cap (z = 7 everywhere: some pattern)
    torch.cuda.synchronize()
    z.fill_(7)
    assert dev(n=0, nq=0, ins_=[None] * 7, outs_=[None] * 8, qbuf=None, qoff=None) == _lib.GDX_OK   # n_pairs == 0 looks at nothing
    # unsupported: an index without text units, the packed form on an index that takes no packed queries, the 64-bit engine
    bare = gpu_index(texts, A, text_units=False, seed_symbols=0, full_suffix_array=False, inverse_suffix_array=False)
    assert not DeviceEngine(bare).aux_info()["text_units"]
    assert dev(h=bare._h) == _lib.GDX_ERR_UNSUPPORTED
    three = gpu_index([b"ACGACGGACA"], alph.Alphabet.from_io_symbols(b"ACG"), text_units=True)
    packed = _lib.QueryLayout()
    lib.gdx_query_layout_init(C.byref(packed))
    packed.packed = 1
    assert dev(h=three._h, lay=C.byref(packed)) == _lib.GDX_ERR_UNSUPPORTED
    lib.gdx_debug_force_wide(1)
    try:
        w = FmIndexConfig("i64").suffix_array_sampling_rate(4).construct_index([b"ACGTACGTTGCA"], A)
    finally:
        lib.gdx_debug_force_wide(0)
    assert w.info.index_width == 64
    assert dev(h=w._h) == _lib.GDX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (z.cpu().numpy() == 7).all()                                            # nothing was written by any refused call
    # the host form: the same causes; its outputs stay as they were
    qbuf, qoff = join([b"ACGT"] * 8)
    h_in = [np.zeros(8, dtype=np.uint32) for _ in range(6)]   # end, n_proper, mate_slot, mate_dist, win_query, win_begin
    h_out = [np.full(4, 7, dtype=np.uint32) for _ in range(7)]
    h_win = (_lib.HitStruct * 4)()
    u32 = lambda x: x.ctypes.data_as(_lib.u32p) if x is not None else None  # noqa: E731

    def host(ms=2, k=3, lo=100, hi=200, n=2, nq=8, h=g._h, ins_=h_in, outs_=h_out, hit=(0, 0), win=h_win, qo=qoff):
        hits = (_lib.HitStruct * 4)(hit, (0, 0), (0, 0), (0, 0))
        return lib.gdx_mate_rescue_many(h, qbuf.ctypes.data_as(_lib.u8p), qo.ctypes.data_as(_lib.u64p) if qo is not None else None, nq, n,
                                        ms, *(u32(x) for x in ins_), hits, k, lo, hi, *(u32(x) for x in outs_), win)

    for kw in (dict(ms=0), dict(ms=33), dict(k=257), dict(lo=201, hi=200), dict(lo=0, hi=1 << 31), dict(lo=100, hi=4197), dict(nq=7),
               dict(n=3), dict(n=0), dict(qo=None), dict(hit=(1 << 32, 0)), dict(hit=(0, 1 << 32)), dict(win=None)):
        assert host(**kw) == _lib.GDX_ERR_INVALID_ARGUMENT, kw
    for missing in range(6):
        assert host(ins_=[None if i == missing else x for i, x in enumerate(h_in)]) == _lib.GDX_ERR_INVALID_ARGUMENT, missing
    for missing in range(7):
        assert host(outs_=[None if i == missing else x for i, x in enumerate(h_out)]) == _lib.GDX_ERR_INVALID_ARGUMENT, missing
    assert host(h=bare._h) == _lib.GDX_ERR_UNSUPPORTED and host(h=w._h) == _lib.GDX_ERR_UNSUPPORTED
    assert all((x == 7).all() for x in h_out) and all(h_win[i].text_id == 0 and h_win[i].position == 0 for i in range(4))
    assert host() == _lib.GDX_OK and (h_out[0] != 7).all()                          # (and the same arguments, accepted, write)


# ------------------------------------------------------------------------------------------------
# 5. end to end on planted pairs: map_pairs(rescue=True) against the models chained

def test_planted_pairs_end_to_end():
    import torch

    from genedex_amd.device import DeviceEngine, DeviceQueries
    from test_align_model import align_model
    from test_best_hits_model import best_hits_model
    from test_candidates_model import A as DNA
    from test_candidates_model import candidates_model
    from test_pair_hits_model import pair_hits_model
    from test_smems_model import model_arrays, oracle_pair

    rng = np.random.default_rng(22100)
    text = random_text(rng, PLANTED["text_len"])
    n, k, ln, mc = 100, PLANTED["max_edits"], PLANTED["mate_len"], PLANTED["max_candidates"]
    lo, hi, ms = PLANTED["min_insert"], PLANTED["max_insert"], 2 * PLANTED["max_candidates"]
    reads, damaged, origin = planted_pairs(rng, text, n)
    texts = [text]
    # the models, chained
    qs = [q for r in reads for q in (r, RC(r))]
    F, R = oracle_pair(texts, DNA)
    n_smems, _, begin, length, start, end, status = model_arrays(F, R, qs, PLANTED["max_smems"], PLANTED["min_length"])
    assert not status.any()
    cands = candidates_model(F.full_sa.astype(np.int64), F.sentinel_indices.astype(np.int64), n_smems, begin, length, start, end,
                             PLANTED["max_smems"], PLANTED["max_occ"], PLANTED["band"], mc)
    _, _, _, cq, cb, ct, cp, _, _ = cands
    every = align_model(texts, DNA, qs, cq, cb, np.stack([ct, cp], axis=1), k)
    pairs = pair_hits_model(cq, cb, ct, cp, every[0], every[2], n, ms, k, lo, hi)
    model = rescue_model(texts, DNA, qs, every[2], pairs[0], pairs[6], pairs[7], pairs[8], pairs[9], pairs[10], pairs[11], n, ms, k, lo, hi)
    final = align_model(texts, DNA, qs, model[5], model[6], np.stack([model[7], model[8]], axis=1), k)
    # every planted pair is rescued: the damaged mate at distance 4, its end at the origin
    hurt = 2 * np.arange(n) + np.array(damaged)
    diag, strand = (np.array([o[i] for o in origin]) for i in (0, 1))
    assert (pairs[0] == 0).all() and (pairs[6][hurt] == NONE).all() and (pairs[6][hurt ^ 1] != NONE).all()
    assert (model[2] == np.array(damaged)).all() and (model[0][hurt] == 4).all() and (model[1][hurt] == diag[hurt] + ln).all()
    # the device
    g, r = gpu_index(texts, DNA), gpu_index(reversed_texts(texts), DNA)
    eng = DeviceEngine(g)
    dq = DeviceQueries.from_host(*join(reads))
    knobs = dict(max_smems=PLANTED["max_smems"], min_length=PLANTED["min_length"], max_occ=PLANTED["max_occ"], band=PLANTED["band"],
                 max_candidates=mc, max_edits=k, min_insert=lo, max_insert=hi)
    got = eng.map_pairs(dq, r, rescue=True, **knobs)
    plain, off = eng.map_pairs(dq, r, **knobs), eng.map_pairs(dq, r, rescue=False, **knobs)
    torch.cuda.synchronize()
    u32 = lambda t: t.cpu().numpy().view(np.uint32).astype(np.int64)  # noqa: E731
    assert set(plain) == set(off) and set(got) == set(plain) | {"rescued", "resc_mate", "resc_pair_dist", "resc_span"}
    used = np.arange(2 * k + 1)[None, :] < u32(plain["n_cigar"])[:, None]
    for name in plain:
        mine, theirs = (u32(x[name])[used] if name == "cigar" else u32(x[name]) for x in (plain, off))
        assert np.array_equal(mine, theirs), name
    rescued = np.zeros(2 * n, dtype=np.int64)
    rescued[hurt] = 1
    assert np.array_equal(u32(got["rescued"]), rescued) and np.array_equal(u32(got["resc_mate"]), model[2])
    assert np.array_equal(u32(got["resc_pair_dist"]), model[3]) and np.array_equal(u32(got["resc_span"]), model[4])
    assert np.array_equal(u32(got["strand"]), model[5] & 1) and np.array_equal(u32(got["text_id"]), model[7])
    assert np.array_equal(u32(got["dist"]), np.where(rescued != 0, final[0].astype(np.int64), pairs[7]))     # (align's own when rescued)
    for name, column in (("begin", 1), ("end", 2), ("n_cigar", 3)):
        assert np.array_equal(u32(got[name]), final[column].astype(np.int64)), name
    # the stage alone on the device's own slots: resc_dist and resc_end against the model
    sq = dq.with_strands(g, "both")
    seeds = eng.alloc_smems(sq.nq, PLANTED["max_smems"])
    eng.smems(sq, r, PLANTED["max_smems"], PLANTED["min_length"], seeds)
    dc = eng.seed_candidates(seeds, sq.nq, PLANTED["max_smems"], PLANTED["max_occ"], PLANTED["band"], mc)
    d_dist, d_end = eng.edit_distance(sq, dc["cand_query"], dc["cand_begin"], dc["cand_hits"], k)
    d_pairs = eng.pair_hits(dc, d_dist, d_end, n, ms, k, lo, hi)
    assert_same(rescue_from_device(eng.mate_rescue(sq, d_end, d_pairs, n, ms, k, lo, hi, out=garbage_rescue(n)), n), model, "the stage")
    # align's distance is at most resc_dist and its range overlaps [resc_end - L - k, resc_end]
    a_dist, a_begin, a_end = (u32(got[name])[hurt] for name in ("dist", "begin", "end"))
    assert (a_dist <= model[0][hurt]).all()
    assert (a_begin <= model[1][hurt]).all() and (a_end >= model[1][hurt] - ln - k).all() and (a_begin < a_end).all()
    single = best_hits_model(cq, cb, ct, cp, every[0], every[2], 2 * n, ms, k)
    assert np.array_equal(u32(got["mapq"]), single[5])                            # (the single-end figures stay those of the seeds)
