"""gdx_seed_candidates_many[_dev] on the GPU against the CPU model of tests/test_candidates_model.py (the definition of
include/gdx_experimental.h on a sort of tuples).  Outputs are integers: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_parity as parity
from genedex_amd import GdxError, _lib, reversed_texts
from test_align_model import align_model  # noqa: F401  (the reference of chain_alignments)
from test_candidates_model import (A, BAD_SEEDS, CHAIN, HAND_CASES, NONE, assert_same, candidates_model, chain_alignments,
                                   chain_case, hand_case_inputs, oracle_of, seed_arrays)
from test_edit_distance_model import INVALID, NO_END
from test_gpu_parity import _VARIANTS, gpu_index
from test_strands_model import join

pytestmark = pytest.mark.gpu

GARBAGE = 0x5A5A5A5A
PER_QUERY = ("n_candidates", "n_groups", "n_skipped")
PER_SLOT = ("cand_query", "cand_begin", "cand_weight")


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


def to_device(seeds):
    """the five seed arrays as the tensors smems() writes: u32 values in int32 tensors (start / end narrowed)"""
    import torch

    n_seeds, begin, length, start, end = seeds
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).astype(np.uint32).view(np.int32)).cuda()  # noqa: E731
    return {"n_seeds": dev(n_seeds), "begin": dev(begin), "length": dev(length), "start": dev(start), "end": dev(end)}


def garbage_outputs(nq, mc):
    import torch

    full = lambda shape, dtype=torch.int32, v=GARBAGE: torch.full(shape, v, dtype=dtype, device="cuda")  # noqa: E731
    out = {name: full((max(nq, 1),)) for name in PER_QUERY}
    out.update({name: full((max(nq * mc, 1),)) for name in PER_SLOT})
    out["cand_hits"] = full((max(nq * mc, 1), 2))
    out["status"] = full((max(nq, 1),), torch.uint8, 0x5A)
    return out


def from_device(out, nq, mc):
    """the nine arrays in the model's order and types"""
    import torch

    torch.cuda.synchronize()
    u32 = lambda t, n: t.cpu().numpy().view(np.uint32).reshape(-1)[:n]  # noqa: E731
    hits = out["cand_hits"].cpu().numpy().view(np.uint32).reshape(-1, 2)[:nq * mc].astype(np.uint64)
    return (u32(out["n_candidates"], nq), u32(out["n_groups"], nq), u32(out["n_skipped"], nq), u32(out["cand_query"], nq * mc),
            u32(out["cand_begin"], nq * mc), hits[:, 0], hits[:, 1], u32(out["cand_weight"], nq * mc),
            out["status"].cpu().numpy()[:nq])


def device_call(eng, seeds, ms, occ, band, mc):
    """gdx_seed_candidates_many_dev on host-made seed arrays, every output GARBAGE beforehand -> the nine arrays"""
    nq = len(seeds[0])
    out = garbage_outputs(nq, mc)
    got = eng.seed_candidates(to_device(seeds), nq, ms, occ, band, mc, out=out)
    assert got is out
    return from_device(out, nq, mc)


def host_call(g, seeds, ms, occ, band, mc, strict=True):
    return g.seed_candidates_raw(*seeds, ms, occ, band, mc, strict=strict)


def sa_in_one_fetch(eng):
    info = eng.aux_info()
    return info["full_suffix_array"] or info["jump_entry_bytes"] == 32


_MODELS = {}


def chain_model(copies, occ, band, mc):
    """candidates_model on the SMEMs of chain_case(copies), made once per knob set"""
    key = (copies, occ, band, mc)
    if key not in _MODELS:
        c = chain_case(copies)
        n_smems, _, begin, length, start, end, _ = c["seeds"]
        _MODELS[key] = candidates_model(c["sa"], c["sentinels"], n_smems, begin, length, start, end, CHAIN["max_smems"], occ, band, mc)
    return _MODELS[key]


def chain_seeds(copies):
    n_smems, _, begin, length, start, end, _ = chain_case(copies)["seeds"]
    return n_smems, begin, length, start, end


# ------------------------------------------------------------------------------------------------
# 1. random reads against the model, every index shape

KNOBS = [(occ, band, mc) for occ in (1, 8, 64) for band in (0, 8) for mc in (1, 4)]


@pytest.mark.parametrize("copies", (2, 6))
def test_random_reads_equal_the_model(copies, variant):
    from genedex_amd.device import DeviceEngine

    c = chain_case(copies)
    seeds, ms = chain_seeds(copies), CHAIN["max_smems"]
    nq = len(c["qs"])
    # the inputs: reads with several groups, reads cut by max_candidates, skipped seeds at the small limits and none at 64
    several = chain_model(copies, 8, 8, 4)
    assert (several[1] >= 2).sum() * 10 >= nq and (several[1] > 4).any() and (chain_model(copies, 1, 8, 4)[2] > 0).sum() * 10 >= nq
    assert copies == 2 or ((several[2] > 0).sum() * 10 >= nq and not chain_model(copies, 64, 8, 4)[2].any())
    g = gpu_index(c["texts"], A)
    eng = DeviceEngine(g)
    if not sa_in_one_fetch(eng):
        import torch

        out = garbage_outputs(nq, 4)
        assert status_of(lambda: eng.seed_candidates(to_device(seeds), nq, ms, 8, 8, 4, out=out)) == _lib.GDX_ERR_UNSUPPORTED
        assert status_of(lambda: host_call(g, seeds, ms, 8, 8, 4)) == _lib.GDX_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        for name, t in out.items():
            assert (t.cpu().numpy().view(np.uint8 if name == "status" else np.uint32) == (0x5A if name == "status" else GARBAGE)).all(), name
        return
    for occ, band, mc in KNOBS:
        assert_same(device_call(eng, seeds, ms, occ, band, mc), chain_model(copies, occ, band, mc), (variant, occ, band, mc))


def test_both_sources_of_sa_and_the_refusal():
    """SA[row] from the full suffix array, from word 6 of a 32-byte jump entry, and an index that has neither"""
    from genedex_amd.device import DeviceEngine

    c = chain_case(2)
    seeds, ms = chain_seeds(2), CHAIN["max_smems"]
    for shape, build in (("full", dict(full_suffix_array=True, jump_entry_bytes=0)), ("jump32", dict(jump_entry_bytes=32)),
                         ("none", dict(jump_entry_bytes=16))):
        g = gpu_index(c["texts"], A, **build)
        eng = DeviceEngine(g)
        info = eng.aux_info()
        assert info["full_suffix_array"] == (shape == "full") and (info["jump_entry_bytes"] == 32) == (shape == "jump32"), (shape, info)
        if shape == "none":
            assert status_of(lambda: device_call(eng, seeds, ms, 8, 8, 4)) == _lib.GDX_ERR_UNSUPPORTED
        else:
            assert_same(device_call(eng, seeds, ms, 8, 8, 4), chain_model(2, 8, 8, 4), shape)
            assert_same(host_call(g, seeds, ms, 8, 8, 4), chain_model(2, 8, 8, 4), shape + " (host form)")


# ------------------------------------------------------------------------------------------------
# 2. every hand-worked case of the model file through the device form

@pytest.mark.parametrize("name", list(HAND_CASES))
def test_hand_worked_case(name):
    from genedex_amd.device import DeviceEngine

    texts, seeds, (ms, occ, band, mc), want = hand_case_inputs(name)
    g = gpu_index(texts, A)
    assert_same(device_call(DeviceEngine(g), seeds, ms, occ, band, mc), want, name)
    if not name.startswith("bad"):
        assert_same(host_call(g, seeds, ms, occ, band, mc), want, name + " (host form)")


# ------------------------------------------------------------------------------------------------
# 3. anchor counts around the kernel's borders: a wavefront's 64 lanes, the sort's powers of two, the most anchors

RUN = [b"A" * 1100, b"C" * 40]                           # A^k begins 1101 - k suffixes
COUNTS = (0, 1, 2, 63, 64, 65, 128, 129, 1024)


def _rows_of_run(sa, k):
    """the rows of A^k in RUN's suffix array: the suffixes of text 0 of at least k symbols"""
    rows = [r for r in range(len(sa)) if int(sa[r]) + k <= 1100]
    assert rows == list(range(rows[0], rows[0] + 1101 - k))
    return rows[0], rows[-1] + 1


def test_anchor_counts_around_the_borders_one_seed_of_many_rows():
    from genedex_amd.device import DeviceEngine

    sa, sentinels = oracle_of(RUN)
    per_query = []
    for c in COUNTS:                                     # beside every count a query without anchors and one with one
        per_query += [[(5, 1101 - c) + _rows_of_run(sa, 1101 - c)] if c else [], [], [(0, 1100) + _rows_of_run(sa, 1100)]]
    seeds = seed_arrays(per_query, 1)
    assert [int(e - s) for s, e in zip(seeds[3][::3], seeds[4][::3])] == list(COUNTS)
    eng = DeviceEngine(gpu_index(RUN, A))
    for band, mc in ((0, 1024), (0, 3), (1, 1024), (62, 64), (63, 1), (5000, 2)):
        want = candidates_model(sa, sentinels, *seeds, 1, 1024, band, mc)
        if band == 0:
            assert want[1][::3].tolist() == list(COUNTS)                # every anchor is a group of its own
        assert_same(device_call(eng, seeds, 1, 1024, band, mc), want, (band, mc))
    want = candidates_model(sa, sentinels, *seeds, 1, 1023, 0, 4)         # ... and the one seed over the limit is skipped
    assert want[2][::3].tolist() == [0] * 8 + [1]
    assert_same(device_call(eng, seeds, 1, 1023, 0, 4), want, "max_occ 1023")


def test_anchor_counts_around_the_borders_many_seeds_of_many_rows():
    """max_seeds * max_occ == 1024 as 16 x 64, 64 x 16 and 1024 x 1: seeds of one length, each begin two further on, so that
    anchors of different seeds share diagonals and a group's weight is a union of many seeds"""
    from genedex_amd.device import DeviceEngine

    sa, sentinels = oracle_of(RUN)
    eng = DeviceEngine(gpu_index(RUN, A))
    for ms, occ in ((16, 64), (64, 16), (1024, 1)):
        k = 1101 - occ
        s, e = _rows_of_run(sa, k)
        full = [(2 * (ms - 1 - j), k, s, e) for j in range(ms)]
        per_query = [full, [], full[:1], full[: ms // 2 + 1], [(0, 1100) + _rows_of_run(sa, 1100)], full[3:]]
        seeds = seed_arrays(per_query, ms)
        for band, mc in ((0, 1024), (3, 5), (5000, 2)):
            want = candidates_model(sa, sentinels, *seeds, ms, occ, band, mc)
            assert (band != 0 or want[1][0] >= ms) and not want[8].any()
            assert_same(device_call(eng, seeds, ms, occ, band, mc), want, (ms, occ, band, mc))
        assert int(seeds[0][0]) * occ == 1024


# ------------------------------------------------------------------------------------------------
# 4. grid independence: one query, three, and more queries than the largest grid has wavefronts

def test_results_do_not_depend_on_the_batch():
    from genedex_amd.device import DeviceEngine

    c = chain_case(2)
    seeds, ms = chain_seeds(2), CHAIN["max_smems"]
    want = chain_model(2, 8, 8, 4)
    nq = len(c["qs"])
    eng = DeviceEngine(gpu_index(c["texts"], A))

    def pick(arrays, idx, per):
        return tuple(np.concatenate([x[i * per:(i + 1) * per] for i in idx]) for x in arrays)

    def want_of(idx):
        out = list(pick(want[:3], idx, 1) + pick(want[3:8], idx, 4) + pick(want[8:], idx, 1))
        out[3] = np.where(out[3] == NONE, NONE, np.repeat(np.arange(len(idx), dtype=np.uint32), 4)).astype(np.uint32)
        return out

    busiest = int(np.argmax(want[1]))
    for idx in ([busiest], [busiest, 0, 1], list(range(nq)) * 28):        # 8400 queries: the largest grid has 4096 wavefronts
        part = pick(seeds[:1], idx, 1) + pick(seeds[1:], idx, ms)
        assert_same(device_call(eng, part, ms, 8, 8, 4), want_of(idx), len(idx))
    assert nq * 28 > 4096


# ------------------------------------------------------------------------------------------------
# 5. the slots go straight into the verify calls: smems -> candidates -> align, no host visit in between

def test_smems_candidates_align_on_the_device():
    import torch

    from genedex_amd.device import DeviceEngine, DeviceQueries

    c = chain_case(2)
    texts, qs = c["texts"], c["qs"]
    nq, ms, ml, mc = len(qs), CHAIN["max_smems"], CHAIN["min_length"], CHAIN["max_candidates"]
    k, want = chain_alignments(2)
    g, r = gpu_index(texts, A), gpu_index(reversed_texts(texts), A)
    eng = DeviceEngine(g)
    dq = DeviceQueries.from_host(*join(qs))
    smems = eng.alloc_smems(nq, ms)
    cands = garbage_outputs(nq, mc)
    aligned = {name: torch.full((nq * mc,), GARBAGE, dtype=torch.int32, device="cuda") for name in ("dist", "begin", "end", "n_cigar")}
    aligned["cigar"] = torch.zeros((nq * mc, 2 * k + 1), dtype=torch.int32, device="cuda")
    workspace = torch.empty(eng.align_workspace_bytes(dq, nq * mc, k)[1], dtype=torch.uint8, device="cuda")
    # four device calls, the tensors of one handed to the next as they are
    eng.smems(dq, r, ms, ml, smems)
    eng.seed_candidates(smems, nq, ms, CHAIN["max_occ"], CHAIN["band"], mc, out=cands)
    eng.align(dq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], k, out=aligned, workspace=workspace)
    assert_same(from_device(cands, nq, mc), c["cands"], "candidates")
    got = [aligned[name].cpu().numpy().view(np.uint32) for name in ("dist", "begin", "end", "n_cigar", "cigar")]
    for x, w, name in zip(got, want, ("dist", "begin", "end", "n_cigar", "cigar")):
        assert np.array_equal(x, w), name
    unused = c["cands"][3] == NONE
    assert 0 < unused.sum() < nq * mc
    assert ((got[0] == INVALID) == unused).all() and (got[1][unused] == NO_END).all() and (got[2][unused] == NO_END).all()
    assert (got[3][unused] == 0).all() and (got[3][~unused & (got[2] != NO_END)] > 0).all()
    # ... and into the other two verify calls
    dist, end = eng.edit_distance(dq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], k)
    ham = eng.hamming(dq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], k)
    torch.cuda.synchronize()
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(end.cpu().numpy().view(np.uint32), want[2])
    assert ((ham.cpu().numpy().view(np.uint32) == 0xFFFFFFFF) == unused).all()


# ------------------------------------------------------------------------------------------------
# 6. the host form and the contract

def test_host_form_and_contract():
    import torch

    from genedex_amd import FmIndexConfig
    from genedex_amd.device import DeviceEngine

    c = chain_case(6)
    seeds, ms = chain_seeds(6), CHAIN["max_smems"]
    nq = len(c["qs"])
    g = gpu_index(c["texts"], A)
    eng = DeviceEngine(g)
    want = chain_model(6, 8, 8, 4)
    assert_same(host_call(g, seeds, ms, 8, 8, 4), want, "host")
    assert_same(device_call(eng, seeds, ms, 8, 8, 4), want, "device")
    # a bad query: GDX_ERR_QUERY_STATUS, every output written
    broken = [x.copy() for x in seeds]
    victim = int(np.flatnonzero((seeds[0] >= 2) & (want[0] > 0))[0])
    broken[2][victim * ms + 1] = 0                                           # a seed of length 0
    want_b = candidates_model(c["sa"], c["sentinels"], *broken, ms, 8, 8, 4)
    assert want_b[8].tolist() == [BAD_SEEDS if i == victim else 0 for i in range(nq)] and want[0][victim] > 0
    assert status_of(lambda: host_call(g, broken, ms, 8, 8, 4)) == _lib.GDX_ERR_QUERY_STATUS
    assert_same(host_call(g, broken, ms, 8, 8, 4, strict=False), want_b, "host, a bad query")
    assert_same(device_call(eng, broken, ms, 8, 8, 4), want_b, "device, a bad query")
    # the safe form on Smem lists
    small = gpu_index([b"ACGTTGCATT" + b"ACGTTGCA"], A)
    smems = small.smems_many([b"ACGTTGCA", b"GGGG"], gpu_index(reversed_texts([b"ACGTTGCATT" + b"ACGTTGCA"]), A), 4, 4)
    assert small.seed_candidates_many(smems, 8, 0, 4) == [[(0, 0, 0, 8), (0, 0, 10, 8)], []]
    assert small.seed_candidates_many(smems, 8, 10, 4) == [[(0, 0, 0, 8)], []]
    # refused calls write nothing: every listed cause, in both forms
    lib = _lib.load()
    z = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ins = [p(z)] * 5
    outs = [p(z[8 * i:]) for i in range(8)]

    def dev(ms_, occ, mc, ins_=ins, outs_=outs, h=g._h, nq_=1):
        return lib.gdx_seed_candidates_many_dev(h, nq_, ms_, *ins_, occ, 0, mc, *outs_, None)

    for ms_, occ, mc in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1025), (33, 32, 1), (1 << 31, 1 << 31, 1), (1 << 16, 1 << 16, 1)):
        assert dev(ms_, occ, mc) == _lib.GDX_ERR_INVALID_ARGUMENT, (ms_, occ, mc)
    for missing in range(5):
        assert dev(1, 1, 1, ins_=[None if i == missing else x for i, x in enumerate(ins)]) == _lib.GDX_ERR_INVALID_ARGUMENT
    for missing in range(7):                                                  # (d_status, the eighth, may be null)
        assert dev(1, 1, 1, outs_=[None if i == missing else x for i, x in enumerate(outs)]) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert dev(1, 1, 1, nq_=0xFFFFFFFF) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert dev(1, 1, 1, nq_=0, ins_=[None] * 5, outs_=[None] * 8) == _lib.GDX_OK        # nq == 0 looks at nothing
    h_out = [np.full(8, 7, dtype=np.uint32) for _ in range(6)]
    h_hits = (_lib.HitStruct * 8)()
    one = seed_arrays([[(0, 4, 0, 1)]], 1)
    u32, u64 = (lambda x: x.ctypes.data_as(_lib.u32p)), (lambda x: x.ctypes.data_as(_lib.u64p))

    def host(ms_, occ, mc, start=one[3], nq_=1, first_out=h_out[0]):
        return lib.gdx_seed_candidates_many(g._h, nq_, ms_, u32(one[0]), u32(one[1]), u32(one[2]), u64(start), u64(one[4]), occ, 0, mc,
                                            u32(first_out) if first_out is not None else None, u32(h_out[1]), u32(h_out[2]),
                                            u32(h_out[3]), u32(h_out[4]), h_hits, u32(h_out[5]), None)

    for ms_, occ, mc in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1025), (33, 32, 1), (1 << 16, 1 << 16, 1)):
        assert host(ms_, occ, mc) == _lib.GDX_ERR_INVALID_ARGUMENT, (ms_, occ, mc)
    assert host(1, 1, 1, start=np.array([1 << 32], dtype=np.uint64)) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert host(1, 1, 1, first_out=None) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert host(1, 1, 1, nq_=0) == _lib.GDX_OK
    assert all((x == 7).all() for x in h_out) and all(h.text_id == 0 and h.position == 0 for h in h_hits)
    assert host(1, 1, 1) == _lib.GDX_OK and h_out[0][0] == 1 and h_out[3][0] == 0 and h_out[5][0] == 4      # (and a call that is not refused)
    # the 64-bit engine
    lib.gdx_debug_force_wide(1)
    try:
        w = FmIndexConfig("i64").suffix_array_sampling_rate(4).construct_index([b"ACGTACGT"], A)
    finally:
        lib.gdx_debug_force_wide(0)
    assert w.info.index_width == 64
    assert dev(1, 1, 1, h=w._h) == _lib.GDX_ERR_UNSUPPORTED
    assert status_of(lambda: host_call(w, one, 1, 1, 0, 1)) == _lib.GDX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert z.cpu().tolist() == [7] * 64
