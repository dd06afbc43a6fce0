"""gdx_pair_hits_many[_dev] on the GPU against the CPU model of tests/test_pair_hits_model.py (the definition of
include/gdx_experimental.h "paired-end pairing").  Outputs are integers: every comparison is exact, every output is filled with
garbage before the call."""
import ctypes as C

import numpy as np
import pytest

from genedex_amd import _lib, reversed_texts
from test_best_hits_model import EDIT_INVALID
from test_candidates_model import A, CHAIN
from test_edit_distance_model import INVALID, NO_END
from test_gpu_best_hits import best_from_device, engine, garbage_best, lanes_of, slots_to_device
from test_gpu_candidates import GARBAGE, garbage_outputs, status_of
from test_gpu_parity import gpu_index
from test_pair_hits_model import (HI, LO, MAPQ_NONE, MAX_INSERT, NONE, PAIR_CHAIN, assert_same, kept_slots, pair_chain_case,
                                  pair_chain_counts, pair_hits_model, random_pair_slots)
from test_strands_model import join

pytestmark = pytest.mark.gpu

PER_PAIR = ("n_proper", "n_best", "pair_dist", "sub_dist", "mapq", "pair_span")
PER_MATE = ("mate_slot", "mate_dist", "win_query", "win_begin")
# the launcher's grid: at most 256 * 16 blocks of 256 lanes, a pair on 2P lanes (P = the next power of two >= mate_slots), so one
# stride of the largest grid covers 256 * 16 * 256 / 2P pairs
MAX_GRID, BLOCK = 256 * 16, 256


def garbage_pairs(n_pairs):
    import torch

    n = max(n_pairs, 1)
    out = {name: torch.full((n,), GARBAGE, dtype=torch.int32, device="cuda") for name in PER_PAIR}
    out.update({name: torch.full((2 * n,), GARBAGE, dtype=torch.int32, device="cuda") for name in PER_MATE})
    out["win_hits"] = torch.full((2 * n, 2), GARBAGE, dtype=torch.int32, device="cuda")
    return out


def pairs_from_device(out, n_pairs):
    """the twelve arrays in the model's order"""
    import torch

    torch.cuda.synchronize()
    hits = out["win_hits"].cpu().numpy().view(np.uint32).reshape(-1, 2)[:2 * n_pairs]
    return (tuple(out[name].cpu().numpy().view(np.uint32)[:n_pairs] for name in PER_PAIR) +
            tuple(out[name].cpu().numpy().view(np.uint32)[:2 * n_pairs] for name in PER_MATE) + (hits[:, 0], hits[:, 1]))


def device_call(eng, slots, n_pairs, mate_slots, k, lo=LO, hi=HI):
    """gdx_pair_hits_many_dev on host-made slots, every output GARBAGE beforehand -> the twelve arrays"""
    cands, dist, end = slots_to_device(slots)
    out = garbage_pairs(n_pairs)
    assert eng.pair_hits(cands, dist, end, n_pairs, mate_slots, k, lo, hi, out=out) is out
    return pairs_from_device(out, n_pairs)


# ------------------------------------------------------------------------------------------------
# 1. random slots against the model: every P instance, powers of two and not, one pair to more than one stride of the grid;
# 3a. where a pair has no proper combination the winners are those of gdx_best_hits_many_dev over the mates

@pytest.mark.parametrize("with_end", (True, False))
@pytest.mark.parametrize("mate_slots", (1, 2, 3, 4, 5, 8, 16, 17, 32))
def test_random_slots_equal_the_model(mate_slots, with_end):
    _, eng = engine()
    one_stride = MAX_GRID * BLOCK // (2 * lanes_of(mate_slots))               # 524288 pairs at P = 1, 16384 at P = 32
    assert mate_slots < 17 or one_stride + 1 == 16385
    rng = np.random.default_rng(17100 + 2 * mate_slots + with_end)
    for n_pairs in (1, 2, 31, 32, 33, 1000, one_stride + 1):
        for k in (0, 3, 1 << 30):
            slots = random_pair_slots(rng, n_pairs, mate_slots, k, with_end)
            want = pair_hits_model(*slots, n_pairs, mate_slots, k, LO, HI)
            got = device_call(eng, slots, n_pairs, mate_slots, k)
            assert_same(got, want, f"{n_pairs} pairs, k = {k}")
            if n_pairs == 1000:
                improper = np.repeat(got[0] == 0, 2)
                assert improper.any() and (~improper).any() and (want[1] == 1).any() and (want[6] == NONE).any()
                assert mate_slots < 3 or k != 3 or (want[1] >= 2).any()
                cands, dist, end = slots_to_device(slots)
                best = best_from_device(eng.best_hits(cands, dist, end, 2 * n_pairs, mate_slots, k, out=garbage_best(2 * n_pairs)), 2 * n_pairs)
                for mine, theirs in ((6, 0), (7, 1), (8, 6), (9, 7), (10, 8), (11, 9)):   # slot, dist, query, begin, text, position
                    assert np.array_equal(got[mine][improper], best[theirs][improper]), (mine, theirs)


# ------------------------------------------------------------------------------------------------
# 2. edge pairs, each as the first and as the last pair of the second wavefront

@pytest.mark.parametrize("mate_slots", (1, 2, 3, 4, 5, 8, 16, 17, 32))
def test_edge_pairs_at_the_borders_of_a_wavefront(mate_slots):
    _, eng = engine()
    ms, k = mate_slots, 3
    per_wave = 64 // (2 * lanes_of(ms))
    n_pairs = 3 * per_wave + 1
    rng = np.random.default_rng(17200 + ms)
    j = np.arange(ms)
    dead = np.where(j % 2 == 0, k + 1, EDIT_INVALID)
    none = (NONE, k + 1, NONE, 0, 0, 0)
    for at in sorted({per_wave, 2 * per_wave - 1}):                            # first and last pair of the second wavefront
        lo0, lo1 = 2 * at * ms, (2 * at + 1) * ms
        for kind in ("both dead", "one dead", "last slots alone", "rescue"):
            if kind == "rescue" and ms < 2:
                continue
            slots = [np.array(x, dtype=np.int64) for x in random_pair_slots(rng, n_pairs, ms, k, True)]
            cq, cb, t, p, d, end = slots
            # mate 0 forward on diagonal 1000 (ends 1100 + j: ms loci), mate 1 reverse on diagonal 1150, both on text 1
            cq[lo0:lo0 + ms], t[lo0:lo0 + ms], cb[lo0:lo0 + ms], p[lo0:lo0 + ms], end[lo0:lo0 + ms] = 4 * at, 1, j, 1000 + j, 1100 + j
            cq[lo1:lo1 + ms], t[lo1:lo1 + ms], cb[lo1:lo1 + ms], p[lo1:lo1 + ms] = 4 * at + 3, 1, j, 1150 + j
            if kind == "both dead":
                d[lo0:lo0 + ms], d[lo1:lo1 + ms], end[lo1:lo1 + ms] = dead, dead[::-1], 1300 + j
                expect = ((0, 0, 2 * k + 2, 2 * k + 2, MAPQ_NONE, 0), none, none)
            elif kind == "one dead":                                            # mate 1: ms loci in range, the least distance is last
                d[lo0:lo0 + ms], d[lo1:lo1 + ms], end[lo1:lo1 + ms] = dead, np.where(j == ms - 1, 1, 2), 1300 + j
                expect = ((0, 0, 2 * k + 2, 2 * k + 2, MAPQ_NONE, 0), none, (ms - 1, 1, 4 * at + 3, ms - 1, 1, 1150 + ms - 1))
            elif kind == "last slots alone":                                    # mate 1 all live, only its last slot ends in range
                d[lo0:lo0 + ms], d[lo1:lo1 + ms] = np.where(j == ms - 1, 1, k + 1), 0
                end[lo1:lo1 + ms] = np.where(j == ms - 1, 1300, 5000 + j)
                expect = ((1, 1, 1, 2 * k + 2, 52, 300), (ms - 1, 1, 4 * at, ms - 1, 1, 1000 + ms - 1),
                          (ms - 1, 0, 4 * at + 3, ms - 1, 1, 1150 + ms - 1))
            else:                                                               # mate 1 tied between two loci, the later one in range
                d[lo0:lo0 + ms], d[lo1:lo1 + ms] = np.where(j == 0, 1, k + 1), np.where(j < 2, 1, k + 1)
                end[lo1:lo1 + ms] = np.where(j == 1, 1300, 5000 + j)
                expect = ((1, 1, 2, 2 * k + 2, 45, 300), (0, 1, 4 * at, 0, 1, 1000), (1, 1, 4 * at + 3, 1, 1, 1151))
            got = device_call(eng, slots, n_pairs, ms, k)
            assert_same(got, pair_hits_model(*slots, n_pairs, ms, k, LO, HI), f"{kind} at pair {at}")
            assert tuple(int(x[at]) for x in got[:6]) == expect[0], (kind, at)
            for s in (0, 1):
                assert tuple(int(x[2 * at + s]) for x in got[6:]) == expect[1 + s], (kind, at, s)


# ------------------------------------------------------------------------------------------------
# 2b. both distances at the largest max_dist: the score 2^31 is the largest a combination can have

@pytest.mark.parametrize("mate_slots", (1, 3, 8, 32))
def test_both_distances_at_the_largest_max_dist(mate_slots):
    _, eng = engine()
    ms, k = mate_slots, 1 << 30
    n_pairs = 5
    rng = np.random.default_rng(17250 + ms)
    j = np.arange(ms)
    for with_end in (True, False):
        slots = [np.array(x, dtype=np.int64) if x is not None else None for x in random_pair_slots(rng, n_pairs, ms, k, with_end)]
        cq, cb, t, p, d, end = slots
        for at in (0, 3):
            # mate 0 forward on diagonals 1000 + 2j, mate 1 reverse on 1300 + 2j: only the LAST slot of mate 0 and the FIRST of
            # mate 1 are live, at distance k, so the lane of each mate with the other's slot number is dead
            lo0, lo1 = 2 * at * ms, (2 * at + 1) * ms
            cq[lo0:lo0 + ms], t[lo0:lo0 + ms], cb[lo0:lo0 + ms], p[lo0:lo0 + ms] = 4 * at, 1, j, 1000 + 3 * j
            cq[lo1:lo1 + ms], t[lo1:lo1 + ms], cb[lo1:lo1 + ms], p[lo1:lo1 + ms] = 4 * at + 3, 1, j, 1300 + 3 * j
            d[lo0:lo0 + ms], d[lo1:lo1 + ms] = np.where(j == ms - 1, k, k + 1), np.where(j == 0, k, k + 1)
            if with_end:
                end[lo0:lo0 + ms], end[lo1:lo1 + ms] = 1100 + 2 * j, 1400 + 2 * j
        span = (400 if with_end else 300) - 2 * (ms - 1)
        got = device_call(eng, slots, n_pairs, ms, k)
        assert_same(got, pair_hits_model(*slots, n_pairs, ms, k, LO, HI), f"at the limit, end = {with_end}")
        for at in (0, 3):
            assert tuple(int(x[at]) for x in got[:6]) == (1, 1, 1 << 31, (1 << 31) + 2, 0, span), at
            assert tuple(int(x[2 * at]) for x in got[6:]) == (ms - 1, k, 4 * at, ms - 1, 1, 1000 + 3 * (ms - 1)), at
            assert tuple(int(x[2 * at + 1]) for x in got[6:]) == (0, k, 4 * at + 3, 0, 1, 1300), at


# ------------------------------------------------------------------------------------------------
# 3b. the widest bounds on one text: every combination of opposite strands is proper

@pytest.mark.parametrize("mate_slots", (3, 8))
def test_with_the_widest_bounds_every_opposite_strand_combination_is_proper(mate_slots):
    _, eng = engine()
    rng = np.random.default_rng(17300 + mate_slots)
    n, k = 1000, 3
    for with_end in (True, False):
        # coordinates as for the bounds [6000, 100000]: every span is 5999 - 5000 or more, none is negative
        slots = random_pair_slots(rng, n, mate_slots, k, with_end, 6000, 100000, one_text=True)
        got = device_call(eng, slots, n, mate_slots, k, 0, MAX_INSERT)
        assert_same(got, pair_hits_model(*slots, n, mate_slots, k, 0, MAX_INSERT), "widest bounds")
        keep = kept_slots(*slots, 2 * n, mate_slots, k)
        reverse = (np.asarray(slots[0]).reshape(2 * n, mate_slots) & 1) == 1
        f, r = (keep & ~reverse).sum(axis=1).reshape(n, 2), (keep & reverse).sum(axis=1).reshape(n, 2)
        assert np.array_equal(got[0], f[:, 0] * r[:, 1] + r[:, 0] * f[:, 1]) and (got[0] >= 4).any()


# ------------------------------------------------------------------------------------------------
# 4. the chain on the device: map_pairs against the stages one by one, pair hits against the model on the device's own slots

# the counts of the inputs (test_pair_hits_model.test_the_chain_inputs_show_what_the_device_test_needs, CPU models): of 150
# pairs 148 proper, 3 with a mate tied single-end and one proper combination, 2 not proper at copies 2; 138, 7 and 12 at copies 6
@pytest.mark.parametrize("copies", (2, 6))
def test_the_chain_on_the_device(copies):
    import torch

    from genedex_amd.device import DeviceEngine, DeviceQueries

    c = pair_chain_case(copies)
    reads, k, ms = c["reads"], c["k"], c["mate_slots"]
    n_mates, n_pairs, mc, max_smems = len(reads), len(reads) // 2, CHAIN["max_candidates"], CHAIN["max_smems"]
    lo, hi = PAIR_CHAIN["min_insert"], PAIR_CHAIN["max_insert"]
    g, r = gpu_index(c["texts"], A), gpu_index(reversed_texts(c["texts"]), A)
    eng = DeviceEngine(g)
    dq = DeviceQueries.from_host(*join(reads))
    knobs = dict(max_smems=max_smems, min_length=CHAIN["min_length"], max_occ=CHAIN["max_occ"], band=CHAIN["band"], max_candidates=mc,
                 max_edits=k, min_insert=lo, max_insert=hi)
    got = eng.map_pairs(dq, r, **knobs)
    # the stages one by one
    sq = dq.with_strands(eng.index, "both")
    assert sq.nq == 2 * n_mates
    smems = eng.alloc_smems(sq.nq, max_smems)
    eng.smems(sq, r, max_smems, CHAIN["min_length"], smems)
    cands = eng.seed_candidates(smems, sq.nq, max_smems, CHAIN["max_occ"], CHAIN["band"], mc, out=garbage_outputs(sq.nq, mc))
    dist, end = eng.edit_distance(sq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], k)
    pairs = eng.pair_hits(cands, dist, end, n_pairs, ms, k, lo, hi, out=garbage_pairs(n_pairs))
    single = eng.best_hits(cands, dist, end, n_mates, ms, k, out=garbage_best(n_mates))
    aligned = eng.align(sq, pairs["win_query"], pairs["win_begin"], pairs["win_hits"], k)
    every = eng.align(sq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], k)     # (all slots, to pick the winners' from)
    torch.cuda.synchronize()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    b, s1 = pairs_from_device(pairs, n_pairs), best_from_device(single, n_mates)
    slots = (u32(cands["cand_query"]), u32(cands["cand_begin"]), u32(cands["cand_hits"])[:, 0], u32(cands["cand_hits"])[:, 1], u32(dist), u32(end))
    model = pair_hits_model(*slots, n_pairs, ms, k, lo, hi)
    assert_same(b, model, "pair hits on the device's slots")
    assert_same(b, c["pairs"], "pair hits against the CPU chain")
    # map_pairs is these stages
    stages = {"strand": b[8] & 1, "text_id": b[10], "begin": u32(aligned["begin"]), "end": u32(aligned["end"]), "dist": b[7],
              "n_cigar": u32(aligned["n_cigar"]), "mapq": s1[5], "n_best": s1[4], "sub_dist": s1[2]}
    per_pair = {"n_proper": b[0], "pair_n_best": b[1], "pair_dist": b[2], "pair_sub_dist": b[3], "pair_mapq": b[4], "pair_span": b[5]}
    assert set(got) == set(stages) | set(per_pair) | {"cigar"}
    for name, w in stages.items():
        assert np.array_equal(u32(got[name])[:n_mates], w), name
    for name, w in per_pair.items():
        assert np.array_equal(u32(got[name])[:n_pairs], w), name
    # the per-mate alignment is that of the winner's slot; an unmapped mate gets the markers
    mapped = b[6] != NONE
    win_slot = np.arange(n_mates) * ms + np.where(mapped, b[6], 0)
    n_cigar = stages["n_cigar"]
    for name in ("dist", "begin", "end", "n_cigar"):
        assert np.array_equal(u32(aligned[name])[:n_mates][mapped], u32(every[name])[win_slot[mapped]]), name
    used = np.arange(2 * k + 1)[None, :] < n_cigar[:, None]                    # (the words from n_cigar on are not written)
    assert np.array_equal(u32(got["cigar"])[:n_mates][used], u32(every["cigar"])[win_slot][used])
    assert np.array_equal(u32(aligned["dist"])[:n_mates][mapped], b[7][mapped]) and (n_cigar[mapped] > 0).all()
    a_dist, a_begin, a_end = (u32(aligned[name])[:n_mates] for name in ("dist", "begin", "end"))
    assert (a_dist[~mapped] == INVALID).all() and (a_begin[~mapped] == NO_END).all() and (a_end[~mapped] == NO_END).all()
    assert (n_cigar[~mapped] == 0).all() and (b[7][~mapped] == k + 1).all() and (s1[5][~mapped] == 255).all()
    # the conditions on the inputs, from the device's own results
    proper, rescued, improper, unique, at_origin = pair_chain_counts(dict(pairs=b, single=s1, origin=c["origin"]))
    print(f"copies {copies}: {proper} proper, {rescued} rescued, {improper} not proper, {at_origin} of {unique} unique at their origin, "
          f"{int((~mapped).sum())} mates unmapped")
    assert proper * 2 >= n_pairs and rescued >= 1 and improper >= 1 and at_origin == unique


# ------------------------------------------------------------------------------------------------
# 5. the host form and the contract

def test_host_form_and_contract():
    import torch

    from genedex_amd import FmIndexConfig
    from genedex_amd.device import DeviceQueries

    g, eng = engine()
    rng = np.random.default_rng(17300)
    for ms, n, k, with_end in ((4, 300, 3, True), (5, 77, 0, False), (32, 9, 1 << 30, True), (1, 5, 3, False)):
        slots = random_pair_slots(rng, n, ms, k, with_end)
        want = pair_hits_model(*slots, n, ms, k, LO, HI)
        assert_same(g.pair_hits_raw(*slots, n, ms, k, LO, HI), want, "host")
        assert_same(device_call(eng, slots, n, ms, k), want, "device")
    # refused calls write nothing: every listed cause, in both forms
    lib = _lib.load()
    z = torch.full((512,), 7, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ins = [p(z)] * 5                                                            # cand_query, cand_begin, cand_hits, dist, end
    outs = [p(z[32 * i:]) for i in range(11)]

    def dev(ms, k, n=1, lo=0, hi=500, ins_=ins, outs_=outs, h=g._h):
        return lib.gdx_pair_hits_many_dev(h, n, ms, *ins_, k, lo, hi, *outs_, None)

    refused = ((0, 3, 1, 0, 500), (33, 3, 1, 0, 500), (1 << 31, 3, 1, 0, 500), (1, (1 << 30) + 1, 1, 0, 500), (1, 0xFFFFFFFF, 1, 0, 500),
               (1, 3, 1, 501, 500), (1, 3, 1, 0, 1 << 31), (1, 3, 1, 0, 0xFFFFFFFF), (1, 3, 1 << 63, 0, 500), (32, 3, 1 << 58, 0, 500),
               (2, 3, 1 << 62, 0, 500))
    for ms, k, n, lo, hi in refused:
        assert dev(ms, k, n, lo, hi) == _lib.GDX_ERR_INVALID_ARGUMENT, (ms, k, n, lo, hi)
    for missing in range(4):                                                    # (d_end, the fifth, may be null)
        assert dev(1, 3, ins_=[None if i == missing else x for i, x in enumerate(ins)]) == _lib.GDX_ERR_INVALID_ARGUMENT
    for missing in range(11):
        assert dev(1, 3, outs_=[None if i == missing else x for i, x in enumerate(outs)]) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert dev(1, 3, n=0, ins_=[None] * 5, outs_=[None] * 11) == _lib.GDX_OK    # n_pairs == 0 looks at nothing
    h_out = [np.full(4, 7, dtype=np.uint32) for _ in range(10)]
    h_win = (_lib.HitStruct * 4)()
    # one pair of one slot per mate: forward on diagonal 10 (end 110), reverse ending at 310
    h_in = [np.array([0, 3], dtype=np.uint32), np.array([0, 0], dtype=np.uint32), np.array([1, 2], dtype=np.uint32),
            np.array([110, 310], dtype=np.uint32)]                               # cand_query, cand_begin, dist, end
    u32 = lambda x: x.ctypes.data_as(_lib.u32p) if x is not None else None  # noqa: E731

    def host(ms, k, n=1, lo=200, hi=500, hit=(0, 10), first_in=h_in[0], first_out=h_out[0], end=h_in[3]):
        hits = (_lib.HitStruct * 2)((hit[0], hit[1]), (0, 210))
        return lib.gdx_pair_hits_many(g._h, n, ms, u32(first_in), u32(h_in[1]), hits, u32(h_in[2]), u32(end), k, lo, hi, u32(first_out),
                                      *(u32(x) for x in h_out[1:]), h_win)

    for ms, k, n, lo, hi in ((0, 3, 1, 200, 500), (33, 3, 1, 200, 500), (1 << 31, 3, 1, 200, 500), (1, (1 << 30) + 1, 1, 200, 500),
                             (1, 0xFFFFFFFF, 1, 200, 500), (1, 3, 1, 501, 500), (1, 3, 1, 0, 1 << 31), (1, 3, 1, 0, 0xFFFFFFFF),
                             (1, 3, 1 << 63, 200, 500), (32, 3, 1 << 58, 200, 500), (2, 3, 1 << 62, 200, 500)):
        assert host(ms, k, n, lo, hi) == _lib.GDX_ERR_INVALID_ARGUMENT, (ms, k, n, lo, hi)
    # every required pointer of the host form: cand_query, cand_begin, cand_hits, dist (end, the fifth, may be null), ten u32
    # outputs and win_hits
    h_hits = (_lib.HitStruct * 2)((0, 10), (0, 210))
    h_args = [u32(h_in[0]), u32(h_in[1]), h_hits, u32(h_in[2]), u32(h_in[3])] + [u32(x) for x in h_out] + [h_win]
    for missing in [0, 1, 2, 3] + list(range(5, 16)):
        args = [None if i == missing else x for i, x in enumerate(h_args)]
        assert lib.gdx_pair_hits_many(g._h, 1, 1, *args[:5], 3, 200, 500, *args[5:]) == _lib.GDX_ERR_INVALID_ARGUMENT, missing
    assert host(1, 3, hit=(0, 1 << 32)) == _lib.GDX_ERR_INVALID_ARGUMENT        # a position of 2^32
    assert host(1, 3, hit=(1 << 32, 10)) == _lib.GDX_ERR_INVALID_ARGUMENT       # a text id of 2^32
    assert host(1, 3, first_in=None) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert host(1, 3, first_out=None) == _lib.GDX_ERR_INVALID_ARGUMENT
    assert host(1, 3, n=0) == _lib.GDX_OK
    assert all((x == 7).all() for x in h_out) and all(h.text_id == 0 and h.position == 0 for h in h_win)
    # (a call that is not refused) with ends the span is 310 - 10; without, 210 - 10
    assert host(1, 3) == _lib.GDX_OK and [int(x[0]) for x in h_out] == [1, 1, 3, 8, 37, 300, 0, 1, 0, 0]
    assert [int(x[1]) for x in h_out[6:]] == [0, 2, 3, 0] and all(int(x[1]) == 7 for x in h_out[:6])
    assert [(h.text_id, h.position) for h in h_win[:2]] == [(0, 10), (0, 210)] and all(int(x[2]) == 7 for x in h_out)
    assert host(1, 3, end=None) == _lib.GDX_OK and [int(x[0]) for x in h_out[:6]] == [1, 1, 3, 8, 37, 200]
    assert host(1, 3, lo=201, end=None) == _lib.GDX_OK and [int(x[0]) for x in h_out[:6]] == [0, 0, 8, 8, 255, 0]
    # the 64-bit engine
    lib.gdx_debug_force_wide(1)
    try:
        w = FmIndexConfig("i64").suffix_array_sampling_rate(4).construct_index([b"ACGTACGT"], A)
    finally:
        lib.gdx_debug_force_wide(0)
    assert w.info.index_width == 64
    assert dev(1, 3, h=w._h) == _lib.GDX_ERR_UNSUPPORTED
    one = random_pair_slots(rng, 1, 2, 3, True)
    assert status_of(lambda: w.pair_hits_raw(*one, 1, 2, 3, LO, HI)) == _lib.GDX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert z.cpu().tolist() == [7] * 512
    # map_pairs takes whole pairs
    with pytest.raises(ValueError):
        eng.map_pairs(DeviceQueries.from_host(*join([b"ACGTTGCA", b"GGCTTAGC", b"CATGATCG"])), g, max_smems=4, min_length=4, max_occ=4,
                      band=4, max_candidates=2, max_edits=3, min_insert=0, max_insert=100)
