"""gdx_best_hits_many[_dev] on the GPU against the CPU model of tests/test_best_hits_model.py (the definition of
include/gdx_experimental.h "best hit per read").  Outputs are integers: every comparison is exact, every output is filled with
garbage before the call."""
import ctypes as C

import numpy as np
import pytest

from genedex_amd import _lib, alphabet, reversed_texts
from test_best_hits_model import EDIT_INVALID, MAPQ_NONE, NONE, assert_same, best_hits_model, random_slots
from test_candidates_model import A, CHAIN, chain_alignments, chain_case
from test_edit_distance_model import INVALID, NO_END
from test_gpu_candidates import GARBAGE, garbage_outputs, status_of
from test_gpu_parity import gpu_index
from test_strands_model import join

pytestmark = pytest.mark.gpu

PER_GROUP = ("best_slot", "best_dist", "sub_dist", "n_live", "n_best", "mapq", "win_query", "win_begin")
# the launcher's grid: at most 256 * 16 blocks of 256 lanes, a group on P lanes (P = the next power of two >= group_slots), so one
# stride of the largest grid covers 256 * 16 * 256 / P groups
MAX_GRID, BLOCK = 256 * 16, 256

_ENGINE = {}


def engine():
    """best hits never looks at the index: one small index serves every test that brings its own slots"""
    from genedex_amd.device import DeviceEngine

    if "eng" not in _ENGINE:
        _ENGINE["g"] = gpu_index([b"ACGTTGCAAGGCTTAGCCATGATCGGA"], A)
        _ENGINE["eng"] = DeviceEngine(_ENGINE["g"])
    return _ENGINE["g"], _ENGINE["eng"]


def lanes_of(group_slots):
    p = 1
    while p < group_slots:
        p *= 2
    return p


def garbage_best(n_groups):
    import torch

    out = {name: torch.full((max(n_groups, 1),), GARBAGE, dtype=torch.int32, device="cuda") for name in PER_GROUP}
    out["win_hits"] = torch.full((max(n_groups, 1), 2), GARBAGE, dtype=torch.int32, device="cuda")
    return out


def best_from_device(out, n_groups):
    """the ten arrays in the model's order"""
    import torch

    torch.cuda.synchronize()
    hits = out["win_hits"].cpu().numpy().view(np.uint32).reshape(-1, 2)[:n_groups]
    return tuple(out[name].cpu().numpy().view(np.uint32)[:n_groups] for name in PER_GROUP) + (hits[:, 0], hits[:, 1])


def slots_to_device(slots):
    import torch

    cq, cb, t, p, d, end = slots
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(np.uint32)).view(np.int32)).cuda()  # noqa: E731
    cands = {"cand_query": dev(cq), "cand_begin": dev(cb), "cand_hits": dev(np.stack([t, p], axis=1))}
    return cands, dev(d), (dev(end) if end is not None else None)


def device_call(eng, slots, n_groups, group_slots, k):
    """gdx_best_hits_many_dev on host-made slots, every output GARBAGE beforehand -> the ten arrays"""
    cands, dist, end = slots_to_device(slots)
    out = garbage_best(n_groups)
    assert eng.best_hits(cands, dist, end, n_groups, group_slots, k, out=out) is out
    return best_from_device(out, n_groups)


# ------------------------------------------------------------------------------------------------
# 1. random slots against the model: every P instance, powers of two and not, one group to more than one stride of the grid

@pytest.mark.parametrize("with_end", (True, False))
@pytest.mark.parametrize("group_slots", (1, 2, 3, 4, 5, 8, 16, 33, 64))
def test_random_slots_equal_the_model(group_slots, with_end):
    _, eng = engine()
    one_stride = MAX_GRID * BLOCK // lanes_of(group_slots)                    # 1048576 groups at P = 1, 16384 at P = 64
    rng = np.random.default_rng(16100 + 2 * group_slots + with_end)
    for n_groups in (1, 2, 63, 64, 65, 1000, one_stride + 1):
        for k in (0, 3, 1 << 31):
            slots = random_slots(rng, n_groups, group_slots, k, with_end)
            want = best_hits_model(*slots, n_groups, group_slots, k)
            assert_same(device_call(eng, slots, n_groups, group_slots, k), want, f"{n_groups} groups, k = {k}")
            if n_groups >= 1000 and group_slots >= 3 and k == 3:               # the inputs show something
                assert (want[3] < group_slots).any() and (want[4] >= 2).any() and (want[4] == 1).any() and (want[0] == NONE).any()


# ------------------------------------------------------------------------------------------------
# 2. edge groups, each as the first and as the last group of a wavefront

@pytest.mark.parametrize("group_slots", (1, 2, 3, 4, 5, 8, 16, 33, 64))
def test_edge_groups_at_the_borders_of_a_wavefront(group_slots):
    _, eng = engine()
    gs, k = group_slots, 3
    per_wave = 64 // lanes_of(gs)
    n_groups = 3 * per_wave + 1
    rng = np.random.default_rng(16200 + gs)
    for at in sorted({per_wave, 2 * per_wave - 1}):                            # first and last group of the second wavefront
        lo = at * gs
        for kind in ("all dead", "one locus", "last slot alone"):
            slots = [np.array(x, dtype=np.int64) for x in random_slots(rng, n_groups, gs, k, True)]
            cq, cb, t, p, d, end = slots
            j = np.arange(gs)
            cq[lo:lo + gs], t[lo:lo + gs], cb[lo:lo + gs], p[lo:lo + gs], end[lo:lo + gs] = 2 * at, 1, j, 1000 + j, 1150
            if kind == "all dead":
                d[lo:lo + gs] = np.where(j % 2 == 0, k + 1, EDIT_INVALID)
                expect = (NONE, k + 1, k + 1, 0, 0, MAPQ_NONE, NONE, 0, 0, 0)
            elif kind == "one locus":                                           # every slot ends at 1150; the least distance is last
                d[lo:lo + gs] = np.where(j == gs - 1, 1, 2)
                expect = (gs - 1, 1, k + 1, 1, 1, 45, 2 * at, gs - 1, 1, 1000 + gs - 1)
            else:
                d[lo:lo + gs] = k + 1
                end[lo:lo + gs] = 1150 + j
                d[lo + gs - 1] = 2
                expect = (gs - 1, 2, k + 1, 1, 1, 30, 2 * at, gs - 1, 1, 1000 + gs - 1)
            got = device_call(eng, slots, n_groups, gs, k)
            assert_same(got, best_hits_model(*slots, n_groups, gs, k), f"{kind} at group {at}")
            assert tuple(int(x[at]) for x in got) == expect, (kind, at)
        # the same three without ends: the diagonal 1000 is the one locus
        slots = [np.array(x, dtype=np.int64) for x in random_slots(rng, n_groups, gs, k, False)[:5]] + [None]
        cq, cb, t, p, d, _ = slots
        cq[lo:lo + gs], t[lo:lo + gs], cb[lo:lo + gs], p[lo:lo + gs], d[lo:lo + gs] = 2 * at, 1, j, 1000 + j, np.where(j == gs - 1, 1, 2)
        got = device_call(eng, slots, n_groups, gs, k)
        assert_same(got, best_hits_model(*slots, n_groups, gs, k), f"one diagonal at group {at}")
        assert tuple(int(x[at]) for x in got) == (gs - 1, 1, k + 1, 1, 1, 45, 2 * at, gs - 1, 1, 1000 + gs - 1)


# ------------------------------------------------------------------------------------------------
# 3. the chain on the device: smems -> candidates -> edit distance -> best hits -> align over the winners

def chain_on_device(copies):
    """the first three calls, made once per case -> (engine, reversed index, queries, candidates, dist, end)"""
    import torch

    from genedex_amd.device import DeviceEngine, DeviceQueries

    key = ("chain", copies)
    if key not in _ENGINE:
        c = chain_case(copies)
        nq, ms, ml, mc = len(c["qs"]), CHAIN["max_smems"], CHAIN["min_length"], CHAIN["max_candidates"]
        k, _ = chain_alignments(copies)
        g, r = gpu_index(c["texts"], A), gpu_index(reversed_texts(c["texts"]), A)
        eng = DeviceEngine(g)
        dq = DeviceQueries.from_host(*join(c["qs"]))
        smems = eng.alloc_smems(nq, ms)
        cands = garbage_outputs(nq, mc)
        eng.smems(dq, r, ms, ml, smems)
        eng.seed_candidates(smems, nq, ms, CHAIN["max_occ"], CHAIN["band"], mc, out=cands)
        dist, end = eng.edit_distance(dq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], k)
        torch.cuda.synchronize()
        _ENGINE[key] = (eng, r, dq, cands, dist, end)
    return _ENGINE[key]


# max_dist: the verify call's limit (band + the most edits of a read = 11), and the most edits of a read alone (3) -- a caller may
# ask best hits for less than it verified with.  Checked on the CPU with the model on chain_case's own arrays: unmapped / tied
# reads of 300 are 0 / 14 at (2, 11), 1 / 13 at (2, 3), 24 / 23 at (6, 11), 26 / 22 at (6, 3)
@pytest.mark.parametrize("copies,max_dist", ((2, 11), (2, 3), (6, 11), (6, 3)))
def test_the_chain_on_the_device(copies, max_dist):
    import torch

    c = chain_case(copies)
    nq, mc = len(c["qs"]), CHAIN["max_candidates"]
    k, want_aligned = chain_alignments(copies)
    eng, _, dq, cands, dist, end = chain_on_device(copies)
    best = garbage_best(nq)
    aligned = {name: torch.full((nq,), GARBAGE, dtype=torch.int32, device="cuda") for name in ("dist", "begin", "end", "n_cigar")}
    aligned["cigar"] = torch.zeros((nq, 2 * k + 1), dtype=torch.int32, device="cuda")
    workspace = torch.empty(eng.align_workspace_bytes(dq, nq, k)[1], dtype=torch.uint8, device="cuda")
    # two device calls, the tensors of one handed to the next as they are
    eng.best_hits(cands, dist, end, nq, mc, max_dist, out=best)
    eng.align(dq, best["win_query"], best["win_begin"], best["win_hits"], k, out=aligned, workspace=workspace)
    got = best_from_device(best, nq)
    d_h, e_h = dist.cpu().numpy().view(np.uint32)[:nq * mc], end.cpu().numpy().view(np.uint32)[:nq * mc]
    assert np.array_equal(d_h, want_aligned[0]) and np.array_equal(e_h, want_aligned[2])
    _, _, _, cq, cb, ct, cp, _, _ = c["cands"]
    want = best_hits_model(cq, cb, ct, cp, d_h, e_h, nq, mc, max_dist)
    assert_same(got, want, "best hits")
    unmapped = want[0] == NONE
    print(f"copies {copies}, max_dist {max_dist}: {int(unmapped.sum())} unmapped, {int((want[4] >= 2).sum())} tied of {nq} reads")
    assert (want[4] >= 2).any()
    if (copies, max_dist) != (2, 11):        # (every read of chain_case(2) has a candidate within 11 edits: counted above)
        assert unmapped.any()
    assert (~unmapped).sum() * 2 >= nq
    # the winners' alignments are those of their slots; an unmapped read gets the markers
    win_slot = np.arange(nq) * mc + np.where(unmapped, 0, want[0])
    a = [aligned[name].cpu().numpy().view(np.uint32) for name in ("dist", "begin", "end", "n_cigar", "cigar")]
    for x, w, name in zip(a, want_aligned, ("dist", "begin", "end", "n_cigar", "cigar")):
        assert np.array_equal(x[~unmapped], w[win_slot[~unmapped]]), name
    assert (a[0][unmapped] == INVALID).all() and (a[1][unmapped] == NO_END).all() and (a[2][unmapped] == NO_END).all()
    assert (a[3][unmapped] == 0).all() and (a[0][~unmapped] == want[1][~unmapped]).all() and (a[3][~unmapped] > 0).all()


# ------------------------------------------------------------------------------------------------
# 4. map_reads: both strands, the whole chain in one method

@pytest.mark.parametrize("copies", (2, 6))
def test_map_reads_on_both_strands(copies):
    import torch

    from genedex_amd.device import DeviceQueries

    c = chain_case(copies)
    qs = c["qs"]
    nq, ms, ml, mc = len(qs), CHAIN["max_smems"], CHAIN["min_length"], CHAIN["max_candidates"]
    k, _ = chain_alignments(copies)
    eng, r, dq_fwd, _, _, _ = chain_on_device(copies)
    mixed = [alphabet.reverse_complement(q) if i % 2 else q for i, q in enumerate(qs)]
    dq = DeviceQueries.from_host(*join(mixed))
    knobs = dict(max_smems=ms, min_length=ml, max_occ=CHAIN["max_occ"], band=CHAIN["band"], max_candidates=mc, max_edits=k)
    got = eng.map_reads(dq, r, **knobs)
    twin = eng.map_reads(dq_fwd, r, **knobs)
    # the stages one by one
    sq = dq.with_strands(eng.index, "both")
    smems = eng.alloc_smems(2 * nq, ms)
    eng.smems(sq, r, ms, ml, smems)
    cands = eng.seed_candidates(smems, 2 * nq, ms, CHAIN["max_occ"], CHAIN["band"], mc, out=garbage_outputs(2 * nq, mc))
    dist, end = eng.edit_distance(sq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], k)
    best = eng.best_hits(cands, dist, end, nq, 2 * mc, k, out=garbage_best(nq))
    aligned = eng.align(sq, best["win_query"], best["win_begin"], best["win_hits"], k)
    torch.cuda.synchronize()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    b = best_from_device(best, nq)
    model = best_hits_model(u32(cands["cand_query"]), u32(cands["cand_begin"]), u32(cands["cand_hits"])[:, 0], u32(cands["cand_hits"])[:, 1],
                            u32(dist), u32(end), nq, 2 * mc, k)
    assert_same(b, model, "best hits over both strands")
    mapped = b[0] != NONE
    stages = {"strand": b[6] & 1, "text_id": b[8], "begin": u32(aligned["begin"]), "end": u32(aligned["end"]), "dist": b[1],
              "sub_dist": b[2], "n_best": b[4], "mapq": b[5], "n_cigar": u32(aligned["n_cigar"])}
    assert set(got) == set(stages) | {"cigar"}
    for name, w in stages.items():
        assert np.array_equal(u32(got[name])[:nq], w), name
    n_cigar, cig, cig_w = stages["n_cigar"], u32(got["cigar"]), u32(aligned["cigar"])
    used = np.arange(2 * k + 1)[None, :] < n_cigar[:, None]                    # (the words from n_cigar on are not written)
    assert np.array_equal(cig[:nq][used], cig_w[:nq][used])
    assert ((b[6][mapped] >> 1) == np.flatnonzero(mapped)).all()               # win_query >> 1 is the read
    assert (u32(got["mapq"])[~mapped] == MAPQ_NONE).all() and (u32(got["begin"])[~mapped] == NO_END).all()
    # a read and its reverse complement map to the same place, the strand bit set
    t = {name: u32(twin[name])[:nq] for name in stages}
    both_unique = (stages["n_best"] == 1) & (t["n_best"] == 1)
    flipped = np.arange(nq) % 2 == 1
    assert (both_unique & flipped).sum() * 4 >= nq and (both_unique & ~flipped).sum() * 4 >= nq
    for name in ("text_id", "begin", "end", "dist", "sub_dist", "mapq"):
        assert np.array_equal(stages[name][both_unique], t[name][both_unique]), name
    assert (stages["strand"][both_unique] == (t["strand"][both_unique] ^ flipped[both_unique])).all()
    # (reads follow their text forwards: unless the reverse complement happens to align as well, the twin's strand is 0)
    assert (t["strand"][both_unique] == 0).sum() * 10 >= 9 * both_unique.sum()


# ------------------------------------------------------------------------------------------------
# 5. the host form and the contract

def test_host_form_and_contract():
    import torch

    from genedex_amd import FmIndexConfig

    g, eng = engine()
    rng = np.random.default_rng(16300)
    for gs, ng, k, with_end in ((4, 300, 3, True), (5, 77, 0, False), (64, 9, 1 << 31, True), (1, 5, 3, False)):
        slots = random_slots(rng, ng, gs, k, with_end)
        want = best_hits_model(*slots, ng, gs, k)
        assert_same(g.best_hits_raw(*slots, ng, gs, k), want, "host")
        assert_same(device_call(eng, slots, ng, gs, k), want, "device")
    # refused calls write nothing: every listed cause, in both forms
    lib = _lib.load()
    z = torch.full((256,), 7, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ins = [p(z)] * 5                                                            # cand_query, cand_begin, cand_hits, dist, end
    outs = [p(z[16 * i:]) for i in range(9)]

    def dev(gs, k, ng=1, ins_=ins, outs_=outs, h=g._h):
        return lib.gdx_best_hits_many_dev(h, ng, gs, *ins_, k, *outs_, None)

    for gs, k, ng in ((0, 3, 1), (65, 3, 1), (1 << 31, 3, 1), (1, (1 << 31) + 1, 1), (1, 0xFFFFFFFF, 1), (2, 3, 1 << 63), (64, 3, 1 << 58)):
        assert dev(gs, k, ng) == _lib.GDX_ERR_INVALID_ARGUMENT, (gs, k, ng)
    for missing in range(4):                                                    # (d_end, the fifth, may be null)
        assert dev(1, 3, ins_=[None if i == missing else x for i, x in enumerate(ins)]) == _lib.GDX_ERR_INVALID_ARGUMENT
    for missing in range(9):
        assert dev(1, 3, outs_=[None if i == missing else x for i, x in enumerate(outs)]) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert dev(1, 3, ng=0, ins_=[None] * 5, outs_=[None] * 9) == _lib.GDX_OK    # n_groups == 0 looks at nothing
    h_out = [np.full(4, 7, dtype=np.uint32) for _ in range(8)]
    h_win = (_lib.HitStruct * 4)()
    h_in = [np.array([0, 0], dtype=np.uint32), np.array([0, 0], dtype=np.uint32), np.array([1, 2], dtype=np.uint32),
            np.array([150, 160], dtype=np.uint32)]                               # cand_query, cand_begin, dist, end
    u32 = lambda x: x.ctypes.data_as(_lib.u32p) if x is not None else None  # noqa: E731

    def host(gs, k, ng=1, hit=(0, 10), first_in=h_in[0], first_out=h_out[0], end=h_in[3]):
        hits = (_lib.HitStruct * 2)((hit[0], hit[1]), (0, 20))
        return lib.gdx_best_hits_many(g._h, ng, gs, u32(first_in), u32(h_in[1]), hits, u32(h_in[2]), u32(end), k, u32(first_out),
                                      *(u32(x) for x in h_out[1:]), h_win)

    for gs, k, ng in ((0, 3, 1), (65, 3, 1), (2, (1 << 31) + 1, 1), (2, 3, 1 << 63)):
        assert host(gs, k, ng) == _lib.GDX_ERR_INVALID_ARGUMENT, (gs, k, ng)
    assert host(2, 3, hit=(0, 1 << 32)) == _lib.GDX_ERR_INVALID_ARGUMENT        # a position of 2^32
    assert host(2, 3, first_in=None) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert host(2, 3, first_out=None) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert host(2, 3, ng=0) == _lib.GDX_OK
    assert all((x == 7).all() for x in h_out) and all(h.text_id == 0 and h.position == 0 for h in h_win)
    assert host(2, 3, end=None) == _lib.GDX_OK and [int(x[0]) for x in h_out] == [0, 1, 2, 2, 1, 15, 0, 0]  # (a call that is not refused)
    assert (h_win[0].text_id, h_win[0].position) == (0, 10) and all(int(x[1]) == 7 for x in h_out)
    # the 64-bit engine
    lib.gdx_debug_force_wide(1)
    try:
        w = FmIndexConfig("i64").suffix_array_sampling_rate(4).construct_index([b"ACGTACGT"], A)
    finally:
        lib.gdx_debug_force_wide(0)
    assert w.info.index_width == 64
    assert dev(1, 3, h=w._h) == _lib.GDX_ERR_UNSUPPORTED
    one = random_slots(rng, 1, 2, 3, True)
    assert status_of(lambda: w.best_hits_raw(*one, 1, 2, 3)) == _lib.GDX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert z.cpu().tolist() == [7] * 256
