"""The CPU model of gdx_best_hits_many[_dev]: the definition of include/gdx_experimental.h "best hit per read", step by step
on numpy arrays of shape (n_groups, group_slots), checked against a naive second implementation (sort the live slots, a dict
per locus), hand-made cases with the numbers written out, and the declarations a binding looks for.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gdx_best_hits_many", "gdx_best_hits_many_dev")
OUT_NAMES = ("best_slot", "best_dist", "sub_dist", "n_live", "n_best", "mapq", "win_query", "win_begin", "win_text_id", "win_position")
NONE = 0xFFFFFFFF            # GDX_CAND_NONE and GDX_BEST_NONE
MAPQ_NONE = 255
MAX_GROUP_SLOTS = 64
EDIT_INVALID, EDIT_TOO_LONG = 0xFFFFFFFF, 0xFFFFFFFE


def best_hits_model(cand_query, cand_begin, text_id, position, dist, end, n_groups, group_slots, max_dist):
    """-> the ten arrays of OUT_NAMES (the winner's hit as two), u32 values in int64"""
    ng, gs, k = int(n_groups), int(group_slots), int(max_dist)
    assert 1 <= gs <= MAX_GROUP_SLOTS and k <= 1 << 31
    shape = lambda x: np.asarray(x).astype(np.int64).reshape(ng, gs)  # noqa: E731
    cq, cb, t, p, d = (shape(x) for x in (cand_query, cand_begin, text_id, position, dist))
    j = np.broadcast_to(np.arange(gs, dtype=np.int64), (ng, gs))
    # 1. live
    live = (cq != NONE) & (d <= k)
    # 2. same locus: of the live slots with one key only the least (dist, j) stays
    e = shape(end) if end is not None else (p - cb) & 0xFFFFFFFF
    rank = d * gs + j                                   # (dist, j) as one number: j < gs
    keep = live.copy()
    for o in range(gs):                                 # slot o against every slot of its group
        same = live[:, o:o + 1] & (cq == cq[:, o:o + 1]) & (t == t[:, o:o + 1]) & (e == e[:, o:o + 1])
        keep &= ~(same & (rank[:, o:o + 1] < rank))
    # 3. results over the slots still live
    big = np.int64(1) << 62
    n_live = keep.sum(axis=1)
    ranked = np.where(keep, rank, big)
    best_slot = ranked.argmin(axis=1)                   # (the first of equals; ranks are distinct anyway)
    mapped = n_live > 0
    rows = np.arange(ng)
    best_dist = np.where(mapped, d[rows, best_slot], k + 1)
    n_best = (keep & (d == best_dist[:, None])).sum(axis=1)
    others = np.where(keep & (j != best_slot[:, None]), d, big).min(axis=1)
    sub_dist = np.where(others == big, k + 1, others)
    mapq = np.where(mapped, np.minimum(60, 60 * (sub_dist - best_dist) // (k + 1)), MAPQ_NONE)
    # 4. the winner
    pick = lambda x, none: np.where(mapped, x[rows, best_slot], none)  # noqa: E731
    return (np.where(mapped, best_slot, NONE), best_dist, sub_dist, n_live, n_best, mapq, pick(cq, NONE), pick(cb, 0), pick(t, 0),
            pick(p, 0))


def best_hits_naive(cand_query, cand_begin, text_id, position, dist, end, n_groups, group_slots, max_dist):
    """the same results group by group: the live slots sorted by (dist, j), the first of every locus kept"""
    gs, k = int(group_slots), int(max_dist)
    out = []
    for g in range(int(n_groups)):
        slots = range(g * gs, (g + 1) * gs)
        alive = sorted((int(dist[s]), s - g * gs) for s in slots if int(cand_query[s]) != NONE and int(dist[s]) <= k)
        loci = {}
        for d, j in alive:
            s = g * gs + j
            e = int(end[s]) if end is not None else (int(position[s]) - int(cand_begin[s])) % (1 << 32)
            loci.setdefault((int(cand_query[s]), int(text_id[s]), e), (d, j))
        kept = sorted(loci.values())
        if not kept:
            out.append((NONE, k + 1, k + 1, 0, 0, MAPQ_NONE, NONE, 0, 0, 0))
            continue
        (bd, bj), s = kept[0], g * gs + kept[0][1]
        sub = kept[1][0] if len(kept) > 1 else k + 1
        out.append((bj, bd, sub, len(kept), sum(1 for d, _ in kept if d == bd), min(60, 60 * (sub - bd) // (k + 1)),
                    int(cand_query[s]), int(cand_begin[s]), int(text_id[s]), int(position[s])))
    return tuple(np.array(col, dtype=np.int64).reshape(-1) for col in zip(*out)) if out else tuple(np.zeros(0, np.int64) for _ in OUT_NAMES)


def assert_same(got, want, what):
    assert len(got) == len(want) == len(OUT_NAMES)
    for g, w, name in zip(got, want, OUT_NAMES):
        g, w = np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64)
        assert g.shape == w.shape, f"{what}: {name}: shape {g.shape} != {w.shape}"
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what}: {name} differs in {bad.size} groups, first at {bad[0]}: {g[bad[0]]} != {w[bad[0]]}"


def random_slots(rng, n_groups, group_slots, max_dist, with_end, pool=4):
    """slots whose keys come from a pool of `pool` loci per group, so that most groups hold duplicates and ties; distances from
    {0 .. k + 1, GDX_EDIT_INVALID, GDX_EDIT_TOO_LONG}; some slots unused, some groups without a hit ->(cand_query, cand_begin, text_id, position, dist, end)"""
    ng, gs, k = int(n_groups), int(group_slots), int(max_dist)
    m = ng * gs
    group = np.repeat(np.arange(ng, dtype=np.int64), gs)
    locus = rng.integers(0, pool, m)
    # a locus of a group: one of two queries (the strands of a read), one of two texts, a diagonal, an end
    cq = (2 * group + (locus & 1)) & 0x7FFFFFFF
    t = (locus >> 1) & 1
    cb = rng.integers(0, 3, m) * 7
    diag = (locus * 1000 + group * 13) & 0xFFFFFFFF
    p = (diag + cb) & 0xFFFFFFFF                        # the same diagonal from another seed begin is the same locus
    end = (diag + 150) & 0xFFFFFFFF if with_end else None
    # every locus of a group has a distance of its own, mostly small so that ties between loci are common; a slot adds 0..2
    # to it, so that the copies of a locus differ and the least of them has to be found
    near = rng.integers(0, min(k, 3) + 2, (ng, pool))   # 0 .. min(k, 3) + 1
    far = rng.integers(0, k + 2, (ng, pool))
    own = np.where(rng.random((ng, pool)) < 0.7, near, far)
    d = np.minimum(own[group, locus] + rng.integers(0, 3, m), k + 1)
    d = np.where(rng.random(m) < 0.1, rng.choice([k + 1, EDIT_INVALID, EDIT_TOO_LONG], m), d)
    d = np.where(np.repeat(rng.random(ng) < 0.05, gs), k + 1, d)  # a group in twenty has no hit within k
    unused = rng.random(m) < 0.15
    cq = np.where(unused, NONE, cq)
    d = np.where(unused & (rng.random(m) < 0.5), 0, d)  # an unused slot may carry any distance
    return cq, cb, t, p, d, end


# ------------------------------------------------------------------------------------------------
# (a) the model against the naive implementation

@pytest.mark.parametrize("group_slots", (1, 2, 3, 5, 8, 33, 64))
def test_model_equals_the_naive_implementation(group_slots):
    rng = np.random.default_rng(16000 + group_slots)
    for k in (0, 3, 11, 1 << 31):
        for with_end in (True, False):
            slots = random_slots(rng, 200, group_slots, k, with_end)
            want = best_hits_naive(*slots, 200, group_slots, k)
            assert_same(best_hits_model(*slots, 200, group_slots, k), want, f"k = {k}, end = {with_end}")
            if group_slots >= 3 and k == 3:               # the inputs show something
                assert (want[3] < group_slots).any() and (want[4] >= 2).any() and (want[0] == NONE).any() and (want[4] == 1).any()


# ------------------------------------------------------------------------------------------------
# (b) hand-made cases, the expected numbers written out

def one_group(slots, k, with_end=True):
    """slots: (cand_query, cand_begin, text_id, position, dist, end) per slot -> both implementations' record of the one group"""
    cols = [np.array(c, dtype=np.int64) for c in zip(*slots)]
    args = (*cols[:5], cols[5] if with_end else None, 1, len(slots), k)
    got = best_hits_model(*args)
    assert_same(best_hits_naive(*args), got, "hand-made")
    return tuple(int(x[0]) for x in got)


def test_mapq_table():
    # (best_dist, sub_dist or None for a lone hit) -> mapq = min(60, 60 * (sub - best) // (k + 1))
    table = {0: {(0, None): 60, (0, 0): 0},
             3: {(0, None): 60, (0, 0): 0, (0, 1): 15, (0, 2): 30, (0, 3): 45, (1, None): 45, (1, 3): 30, (2, 3): 15, (3, None): 15,
                 (3, 3): 0},
             11: {(0, None): 60, (0, 1): 5, (0, 6): 30, (0, 11): 55, (5, 7): 10, (11, None): 5, (11, 11): 0, (4, None): 40}}
    for k, rows in table.items():
        for (bd, sd), mapq in rows.items():
            slots = [(0, 0, 0, 100, bd, 250)] + ([(0, 0, 1, 100, sd, 250)] if sd is not None else [(NONE, 0, 0, 0, 0, 0)])
            r = one_group(slots, k)
            assert r[:6] == (0, bd, sd if sd is not None else k + 1, 1 if sd is None else 2, 2 if sd == bd else 1, mapq), (k, bd, sd, r)


def test_a_duplicate_whose_better_copy_sits_in_the_later_slot():
    # slots 0 and 2 end at the same place of the same text: one locus, the copy of distance 1 stays; slot 1 is another locus
    r = one_group([(4, 10, 1, 500, 2, 640), (4, 0, 1, 900, 3, 1040), (4, 30, 1, 521, 1, 640)], 3)
    assert r == (2, 1, 3, 2, 1, 30, 4, 30, 1, 521)
    # without it the read would look like (best 1, sub 2); with equal distances the earlier slot stays
    r = one_group([(4, 10, 1, 500, 1, 640), (4, 30, 1, 521, 1, 640)], 3)
    assert r == (0, 1, 4, 1, 1, 45, 4, 10, 1, 500)
    # the same end in another text, or of the other strand's query, is another locus
    assert one_group([(4, 10, 1, 500, 1, 640), (4, 30, 2, 521, 1, 640)], 3)[:6] == (0, 1, 1, 2, 2, 0)
    assert one_group([(4, 10, 1, 500, 1, 640), (5, 30, 1, 521, 1, 640)], 3)[:6] == (0, 1, 1, 2, 2, 0)


def test_a_tie_between_the_first_and_the_last_slot():
    slots = [(0, 0, 0, 100, 2, 250)] + [(0, 0, 0, 1000 * j, 5, 1000 * j + 150) for j in range(1, 7)] + [(0, 0, 0, 9000, 2, 9150)]
    assert one_group(slots, 11) == (0, 2, 2, 8, 2, 0, 0, 0, 0, 100)


def test_an_unused_slot_carrying_distance_zero_is_dead():
    r = one_group([(NONE, 0, 0, 0, 0, 0), (7, 3, 2, 40, 2, 190)], 3)
    assert r == (1, 2, 4, 1, 1, 30, 7, 3, 2, 40)
    assert one_group([(NONE, 0, 0, 0, 0, 0), (NONE, 0, 0, 0, 0, 0)], 3) == (NONE, 4, 4, 0, 0, MAPQ_NONE, NONE, 0, 0, 0)
    # the markers and the capped value are dead without a special case
    r = one_group([(1, 0, 0, 5, EDIT_INVALID, NONE), (1, 0, 0, 6, EDIT_TOO_LONG, NONE), (1, 0, 0, 7, 4, NONE)], 3)
    assert r == (NONE, 4, 4, 0, 0, MAPQ_NONE, NONE, 0, 0, 0)


def test_without_ends_the_diagonal_wraps():
    # position 2 - begin 5 = 2^32 - 3 = position 7 - begin 10: one locus; position 3 - begin 5 is the next diagonal
    r = one_group([(0, 5, 0, 2, 1, 0), (0, 10, 0, 7, 0, 0), (0, 5, 0, 3, 1, 0)], 3, with_end=False)
    assert r == (1, 0, 1, 2, 1, 15, 0, 10, 0, 7)
    # with ends given the diagonal does not count: three different ends are three loci
    r = one_group([(0, 5, 0, 2, 1, 150), (0, 10, 0, 7, 0, 151), (0, 5, 0, 3, 1, 152)], 3)
    assert r[:6] == (1, 0, 1, 3, 1, 15)


# ------------------------------------------------------------------------------------------------
# (c) the two calls are declared everywhere a binding looks for them

def test_header_library_stub_and_rust_binding_have_both_calls():
    from genedex_amd import _lib
    from test_candidates_model import _header_arg_counts

    counts = _header_arg_counts("gdx_experimental.h")
    assert counts.get("gdx_best_hits_many") == 18 and counts.get("gdx_best_hits_many_dev") == 19
    assert "gdx_best_hits_many" not in _header_arg_counts("gdx.h")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    rust = open(os.path.join(ROOT, "bindings", "rust", "gdx.rs")).read()
    for name in NAMES:
        assert hasattr(lib, name), name + " is not exported by libgdx.so"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == counts[name], name
        assert re.search(r"pub fn " + name + r"\s*\(", rust), name
    assert re.search(r"pub fn best_hits_many\b", rust)  # the safe wrapper of GpuFmIndex
    header = open(os.path.join(ROOT, "include", "gdx_experimental.h")).read()
    for name, text, value in (("GDX_BEST_NONE", "0xFFFFFFFFu", NONE), ("GDX_BEST_MAPQ_NONE", "255u", MAPQ_NONE),
                              ("GDX_BEST_MAX_GROUP_SLOTS", "64u", MAX_GROUP_SLOTS)):
        assert re.search(r"#define\s+" + name + r"\s+" + text + r"\s", header), name
        assert getattr(_lib, name) == value, name
        assert re.search(r"pub const " + name + r": u\d+ = ", rust), name
