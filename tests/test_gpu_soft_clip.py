"""gdx_soft_clip_many[_dev] (soft_clip.hip) against the model of tests/test_soft_clip_model.py, every output prefilled with a
garbage pattern and the inputs compared before and after: the hand cases, random rows at strides below, at and above one
wavefront's width and batch sizes across workgroups, grids 1, 2, 3 and the default, the host form and every refusal, and
map_reads / map_pairs with `clip` end to end through DeviceEngine.sam_records."""
import re

import numpy as np
import pytest

from genedex_amd import _lib, reversed_texts
from test_candidates_model import A as DNA
from test_edit_distance_model import INVALID, NO_END, TOO_LONG
from test_gpu_parity import gpu_index
from test_mate_rescue_model import PLANTED, RC, planted_pairs, random_text
from test_sam_records_model import NONE, PAIRED, SINGLE, record_bound, sam_model
from test_soft_clip_model import (BAD_CIGAR, BAD_ROWS, DEFAULT, MARKER_ROWS, NO_SCORE, OUT_NAMES, SCORINGS, assert_hand_case, assert_invariants,
                                  assert_same, clip_model, hand_rows, random_rows, row_arrays)
from test_strands_model import join

pytestmark = pytest.mark.gpu

FILL = 0xA5A5A5A5
_CASE = {}
MS = (1, 63, 64, 65, 257, 5003)


def engine():
    """any index serves: the call looks at neither the queries nor the index's arrays"""
    from genedex_amd.device import DeviceEngine

    if "eng" not in _CASE:
        _CASE["g"] = gpu_index([b"ACGTACGTTGCA"], DNA)
        _CASE["eng"] = DeviceEngine(_CASE["g"])
    return _CASE["g"], _CASE["eng"]


def dev_u32(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(np.uint32)).view(np.int32)).cuda()


def prefilled(m, stride, status=True):
    import torch

    out = {name: torch.full((m,), FILL - (1 << 32), dtype=torch.int32, device="cuda") for name in OUT_NAMES[:7]}
    out["cigar"] = torch.full((m, stride), FILL - (1 << 32), dtype=torch.int32, device="cuda")
    out["status"] = torch.full((m,), 0xA5, dtype=torch.uint8, device="cuda") if status else None
    return out


def to_host(out):
    """the nine outputs as the model returns them (status None when none was asked for)"""
    got = [out["score"].cpu().numpy()] + [out[name].cpu().numpy().view(np.uint32) for name in OUT_NAMES[1:8]]
    return tuple(got) + (out["status"].cpu().numpy() if out["status"] is not None else None,)


def device_call(inputs, k, scoring, min_score=0, status=True, grid=None):
    """gdx_soft_clip_many_dev through DeviceEngine.soft_clip on prefilled outputs; the inputs must come back as they went in"""
    import torch

    g, eng = engine()
    names = ("dist", "begin", "end", "n_cigar", "cigar")
    m = len(inputs[0])
    aligned = {name: dev_u32(x) for name, x in zip(names, inputs)}
    aligned["cigar"] = aligned["cigar"].reshape(m, 2 * k + 1)
    lib = _lib.load()
    lib.gdx_debug_set_clip_grid(grid or 0)
    try:
        out = eng.soft_clip(aligned, k, tuple(scoring) + (min_score,), out=prefilled(m, 2 * k + 1, status))
        torch.cuda.synchronize()
    finally:
        lib.gdx_debug_set_clip_grid(0)
    for name, x in zip(names, inputs):
        assert np.array_equal(aligned[name].cpu().numpy().view(np.uint32).reshape(-1), np.asarray(x, dtype=np.uint32).reshape(-1)), name
    return to_host(out)


def assert_call(inputs, k, scoring, min_score, what, want=None, **kw):
    """the device's outputs equal the model's, the words from out_n_cigar on still hold the prefill -> the outputs"""
    got = device_call(inputs, k, scoring, min_score, **kw)
    if want is None:
        want = clip_model(*inputs, k, *scoring, min_score, fill=FILL, single_pass=k > 8)
    m = len(inputs[0])
    want = tuple(w[:m] for w in want)
    if got[8] is None:
        got, want = got[:8] + (want[8],), want
    assert_same(got, want, what)
    return got


# ------------------------------------------------------------------------------------------------
# 1. the hand cases

def test_hand_cases():
    names, rows, knobs = hand_rows()
    k = 3
    for knob in sorted(set(knobs)):                                               # one launch per (scoring, min_score)
        at = [c for c in range(len(rows)) if knobs[c] == knob]
        inputs = row_arrays([rows[c] for c in at], k)
        got = assert_call(inputs, k, knob[0], knob[1], ("hand cases", knob))
        for i, c in enumerate(at):
            assert_hand_case(names[c], tuple(x[i] for x in got))
            assert (got[7][i][int(got[6][i]):] == FILL).all(), names[c]            # words from out_n_cigar on hold the prefill


def test_markers_pass_through_and_every_bad_row_rule_on_its_own():
    k = 3
    got = assert_call(row_arrays(MARKER_ROWS, k), k, DEFAULT, 0, "markers")
    assert got[0].tolist() == [NO_SCORE] * 4 and got[1].tolist() == [INVALID, TOO_LONG, k + 1, k + 1] and not got[8].any()
    assert (got[2] == NO_END).all() and (got[3] == NO_END).all() and not got[6].any() and (got[7] == FILL).all()
    bad = list(BAD_ROWS.values())
    got = assert_call(row_arrays(bad, k), k, DEFAULT, 0, "bad rows")
    for c, name in enumerate(BAD_ROWS):
        assert (got[8][c], got[0][c], got[1][c], got[2][c], got[3][c], got[4][c], got[5][c], got[6][c]) == \
            (BAD_CIGAR, NO_SCORE, k + 1, NO_END, NO_END, 0, 0, 0), name
    assert (got[7] == FILL).all()
    # each of them alone in a batch of good rows: the neighbours of a group are not disturbed
    good = hand_rows()[1][:6]
    for name, row in BAD_ROWS.items():
        assert_call(row_arrays(good[:3] + [row] + good[3:], k), k, DEFAULT, 0, ("among good rows", name))


# ------------------------------------------------------------------------------------------------
# 2. random rows against the model: strides 1, 3, 17, 63, 65 and 513; m across groups, wavefronts and workgroups

def random_case(k):
    """5003 rows for this k and the model's outputs for each of the three scorings, made once"""
    if ("rows", k) not in _CASE:
        rng = np.random.default_rng(26300 + k)
        rows = random_rows(rng, MS[-1], k)
        min_scores = (7, 0, 3000)
        _CASE["rows", k] = (rows, min_scores, [clip_model(*rows, k, *s, ms, fill=FILL, single_pass=k > 8) for s, ms in zip(SCORINGS, min_scores)])
    return _CASE["rows", k]


@pytest.mark.parametrize("k", (0, 1, 8, 31, 32, 256))
def test_random_rows_against_the_model(k):
    rows, min_scores, wants = random_case(k)
    for scoring, min_score, want in zip(SCORINGS, min_scores, wants):
        assert_invariants(rows, want, k)
        for i, m in enumerate(MS):
            inputs = tuple(x[:m] for x in rows)
            got = assert_call(inputs, k, scoring, min_score, (k, m, scoring), want=want, status=m != 65)
            if m == MS[-1]:
                assert_invariants(rows, got, k)
        assert_call(tuple(x[:300] for x in rows), k, scoring, min_score, (k, "without status", scoring), want=want, status=False)
    kept = wants[0][3] != NO_END
    if k >= 8:                                                                    # the batch is not one the stage has nothing to do on
        assert kept.sum() > 2000 and ((wants[0][4] != 0) | (wants[0][5] != 0)).sum() > 300 and (wants[0][8] != 0).sum() > 100
        # a full row of one-symbol runs is kept whole by (1, 1, 0, 1): the tie rule; it is the row that crosses chunks of 64 runs
        assert (wants[1][6][wants[1][3] != NO_END] > 64).any() == (k >= 32)


# ------------------------------------------------------------------------------------------------
# 3. the grid

@pytest.mark.parametrize("k", (8, 32))
def test_results_do_not_depend_on_the_grid(k):
    rows, min_scores, wants = random_case(k)
    for grid in (1, 2, 3, None):
        assert_call(rows, k, SCORINGS[0], min_scores[0], (k, "grid", grid), want=wants[0], grid=grid)


# ------------------------------------------------------------------------------------------------
# 4. the host form and the refusals

def test_host_form_equals_the_device_form():
    g, eng = engine()
    for k in (3, 32):
        rows, min_scores, wants = random_case(8 if k == 3 else k)
        if k == 3:
            rng = np.random.default_rng(26400)
            rows = random_rows(rng, 301, k)
        inputs = tuple(x[:301] for x in rows)
        got = device_call(inputs, k, SCORINGS[0], 5)
        host = g.soft_clip_raw(*inputs, k, *SCORINGS[0], min_score=5)
        want = clip_model(*inputs, k, *SCORINGS[0], 5, fill=0, single_pass=True)    # (soft_clip_raw hands in rows of zeros)
        assert_same(host, want, ("host form", k))
        below = np.arange(2 * k + 1)[None, :] < got[6][:, None]
        assert_same(tuple(np.where(below, x, 0) if name == "cigar" else x for name, x in zip(OUT_NAMES, got)), host, ("device form", k))
    empty = g.soft_clip_raw(*[np.zeros(0, dtype=np.uint32)] * 4, np.zeros((0, 7), dtype=np.uint32), 3, *DEFAULT)
    assert all(x.size == 0 for x in empty)


def test_refused_calls_write_nothing():
    import ctypes as C

    import torch

    from genedex_amd import FmIndexConfig

    g, eng = engine()
    lib = _lib.load()
    k, m = 3, 4
    z = torch.full((4096,), 7, dtype=torch.int32, device="cuda")
    order = ("dist", "begin", "end", "n_cigar", "cigar", "out_score", "out_dist", "out_begin", "out_end", "out_clip_left", "out_clip_right",
             "out_n_cigar", "out_cigar", "out_status")

    def dev(h=g._h, m=m, k=k, scoring=DEFAULT, min_score=0, **kw):
        p = {name: z[128 * i:].data_ptr() for i, name in enumerate(order)}
        p.update(kw)
        return lib.gdx_soft_clip_many_dev(h, m, k, *scoring, min_score, *(p[name] for name in order), None)

    host_in = [np.full(m * 7, 7, dtype=np.uint32) for _ in range(5)]
    host_out = [np.full(m * 7, 7, dtype=np.uint32) for _ in range(8)] + [np.full(m, 7, dtype=np.uint8)]

    def host(h=g._h, m=m, k=k, scoring=DEFAULT, min_score=0, **kw):
        p = {name: x.ctypes.data_as(C.c_void_p) for name, x in zip(order, host_in + host_out)}
        p.update(kw)
        cast = lambda name: C.cast(p[name], dict(out_score=C.POINTER(C.c_int32), out_status=_lib.u8p).get(name, _lib.u32p))  # noqa: E731
        return lib.gdx_soft_clip_many(h, m, k, *scoring, min_score, *(cast(name) for name in order))

    invalid = [dict(k=257), dict(scoring=(0, 4, 6, 1)), dict(scoring=(1025, 4, 6, 1)), dict(scoring=(1, 0, 6, 1)), dict(scoring=(1, 1025, 6, 1)),
               dict(scoring=(1, 4, 6, 0)), dict(scoring=(1, 4, 6, 1025)), dict(scoring=(1, 4, 1025, 1)), dict(min_score=(1 << 30) + 1)]
    invalid += [{name: None} for name in order[:-1]]
    lib.gdx_debug_force_wide(1)
    try:
        w = FmIndexConfig("i64").suffix_array_sampling_rate(4).construct_index([b"ACGTACGTTGCA"], DNA)
    finally:
        lib.gdx_debug_force_wide(0)
    assert w.info.index_width == 64
    for call in (dev, host):
        for kw in invalid:
            assert call(**kw) == _lib.GDX_ERR_INVALID_ARGUMENT, (call.__name__, kw)
        assert call(h=None) == _lib.GDX_ERR_INVALID_ARGUMENT
        assert call(h=w._h) == _lib.GDX_ERR_UNSUPPORTED
        assert call(m=0) == _lib.GDX_OK                                           # and writes nothing
    torch.cuda.synchronize()
    assert (z.cpu().numpy() == 7).all() and all((x == 7).all() for x in host_out)
    # the same arguments, accepted: gap_open 0 and the largest parameters are inside the bounds; four rows whose n_cigar, 7, is
    # within the stride, whose words are not runs
    for call in (dev, host):
        assert call(scoring=(1024, 1024, 0, 1024), min_score=1 << 30, out_status=None) == _lib.GDX_OK
        assert call() == _lib.GDX_OK
    torch.cuda.synchronize()
    zz = z.cpu().numpy()
    status = zz[128 * 13:128 * 13 + 1].view(np.uint8)
    assert (status == BAD_CIGAR).all() and (zz[128 * 5:128 * 5 + m] == NO_SCORE).all() and (zz[128 * 6:128 * 6 + m] == k + 1).all()
    assert (zz[128 * 11:128 * 11 + m] == 0).all() and (zz[128 * 12:128 * 13] == 7).all() and (zz[128 * 5 + m:128 * 6] == 7).all()
    assert (host_out[8] == BAD_CIGAR).all() and (host_out[0][:m].view(np.int32) == NO_SCORE).all() and (host_out[7] == 7).all()


# ------------------------------------------------------------------------------------------------
# 5. through the chain: map_reads / map_pairs with clip, and the SAM records of the clipped result

CLIP = (1, 4, 6, 1, 0)
CHAIN_K = 24
KNOBS = dict(max_smems=PLANTED["max_smems"], min_length=PLANTED["min_length"], max_occ=PLANTED["max_occ"], band=PLANTED["band"],
             max_candidates=PLANTED["max_candidates"])
CLIP_NAMES = ("score", "dist", "begin", "end", "clip_left", "clip_right", "n_cigar")


def substituted(rng, piece, n):
    piece = bytearray(piece)
    for at in rng.choice(len(piece), n, replace=False):
        piece[at] = b"ACGT"[(b"ACGT".index(piece[at]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(piece)


def chain_case():
    """three texts, 64 junk-tail reads and 20 overhanging ones, mapped once without and once with clip"""
    import torch

    from genedex_amd.device import DeviceEngine, DeviceQueries

    if "chain" in _CASE:
        return _CASE["chain"]
    rng = np.random.default_rng(26500)
    texts = [random_text(rng, n) for n in (3000, 2000, 2500)]
    reads, kind = [], []
    for i in range(64):                    # 80 symbols of a text with 0..2 substitutions on either strand, then 20 random symbols
        t = i % 3
        at = int(rng.integers(100, len(texts[t]) - 200))
        piece = substituted(rng, texts[t][at:at + 80], i % 3)
        junk = bytes(b"ACGT"[x] for x in rng.integers(0, 4, 20))
        reads.append((piece if i % 2 == 0 else RC(piece)) + junk)
        kind.append(("junk", i % 2, t, 0))
    for h in range(1, 11):                 # 60 symbols that hang over the end / the start of a text by h
        t = h % 3
        over = bytes(b"ACGT"[x] for x in rng.integers(0, 4, h))
        reads.append(texts[t][len(texts[t]) - (60 - h):] + over)
        kind.append(("end", 0, t, h))
        reads.append(over + texts[t][:60 - h])
        kind.append(("start", 0, t, h))
    g, r = gpu_index(texts, DNA), gpu_index(reversed_texts(texts), DNA)
    eng = DeviceEngine(g)
    dq = DeviceQueries.from_host(*join(reads))
    plain = eng.map_reads(dq, r, max_edits=CHAIN_K, **KNOBS)
    clipped = eng.map_reads(dq, r, max_edits=CHAIN_K, clip=CLIP, **KNOBS)
    torch.cuda.synchronize()
    _CASE["chain"] = (texts, reads, kind, g, eng, dq, plain, clipped)
    return _CASE["chain"]


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def assert_clipped_equals_the_model(plain, clipped, k, clip, n):
    """the clipped fields are the model's over the unclipped result; everything else is the unclipped result's -> the model's"""
    cigar = u32(plain["cigar"]).reshape(-1, 2 * k + 1)[:n]
    want = clip_model(u32(plain["dist"])[:n], u32(plain["begin"])[:n], u32(plain["end"])[:n], u32(plain["n_cigar"])[:n], cigar, k, *clip,
                      single_pass=True)
    assert not want[8].any()
    for name, w in zip(CLIP_NAMES, want):
        got = clipped[name].cpu().numpy()[:n]
        assert np.array_equal(got if name == "score" else got.view(np.uint32), w), name
    below = np.arange(2 * k + 1)[None, :] < want[6][:, None]
    assert np.array_equal(np.where(below, u32(clipped["cigar"]).reshape(-1, 2 * k + 1)[:n], 0), want[7])
    assert np.array_equal(u32(clipped["edit_dist"])[:n], u32(plain["dist"])[:n])
    assert set(clipped) == set(plain) | {"score", "clip_left", "clip_right", "edit_dist"}
    for name in set(plain) - {"dist", "begin", "end", "n_cigar", "cigar"}:
        assert np.array_equal(u32(clipped[name]), u32(plain[name])), name
    return want


def test_junk_tails_and_overhangs_are_clipped():
    texts, reads, kind, g, eng, dq, plain, clipped = chain_case()
    n = len(reads)
    want = assert_clipped_equals_the_model(plain, clipped, CHAIN_K, CLIP, n)
    score, dist, begin, end, left, right, n_cigar = want[:7]
    strand, tid = u32(clipped["strand"])[:n], u32(clipped["text_id"])[:n]
    junk_clipped = 0
    for i, (what, rc, t, h) in enumerate(kind):
        if what == "junk":
            # the junk follows the piece in the read as given: behind the alignment on strand 0, in front of it on strand 1
            if end[i] != NO_END and strand[i] == rc and (left[i] if rc else right[i]) >= 10:
                junk_clipped += 1
            continue
        assert end[i] != NO_END and (strand[i], tid[i]) == (0, t), (i, what, h)
        # (an overhanging symbol that equals the text's last one may be matched to it, which clips one symbol more)
        assert end[i] <= len(texts[t]) and (right[i] if what == "end" else left[i]) >= h, (i, what, h)
    assert junk_clipped >= 48, junk_clipped
    assert (u32(plain["n_cigar"])[:n] > 0).sum() >= 70                            # (the chain had something to clip)


def rebuild_clipped_segment(line):
    """tests/test_sam_records_model.py::rebuild_segment for a CIGAR with S runs: text[begin:end] of a mapped record from SEQ,
    CIGAR and MD alone; an S run advances in SEQ as an I run does -> (text id field, begin, segment)"""
    f = line.rstrip(b"\n").split(b"\t")
    seq = b"" if f[9] == b"*" else f[9]
    md = [x for x in f[12:] if x.startswith(b"MD:Z:")][0][5:]
    runs = [] if f[5] == b"*" else [(int(n), op) for n, op in re.findall(rb"(\d+)([MIDNSHP=X])", f[5])]
    tokens = re.findall(rb"\d+|\^[^\d^]+|[^\d^]", md)
    at = [0]

    def next_token():
        at[0] += 1
        return tokens[at[0] - 1]

    out, x, left = bytearray(), 0, int(next_token())
    for n, op in runs:
        if op == b"=":
            assert left >= n
            out += seq[x:x + n]
            x, left = x + n, left - n
        elif op == b"X":
            for _ in range(n):
                assert left == 0
                out += next_token()
                left = int(next_token())
            x += n
        elif op == b"D":
            assert left == 0
            tok = next_token()
            assert tok[:1] == b"^" and len(tok) == n + 1
            out += tok[1:]
            left = int(next_token())
        elif op in (b"I", b"S"):
            x += n
        else:
            raise AssertionError(op)
    assert left == 0 and at[0] == len(tokens) and x == len(seq)
    return f[2], int(f[3]) - 1, bytes(out)


def parse(out, rec_off):
    data = out.cpu().numpy().tobytes()
    off = rec_off.cpu().numpy()
    assert off[0] == 0 and off[-1] == len(data)
    return [data[int(off[r]):int(off[r + 1])] for r in range(len(off) - 1)]


def assert_sam(texts, eng, reads, sq, result, mode, k, longest):
    """sam_records() of the clipped result equals sam_model fed the clipped arrays, byte for byte -> the records"""
    import torch

    n = len(reads)
    out, rec_off, status = eng.sam_records(sq, result, mode=mode)
    torch.cuda.synchronize()
    lines = parse(out, rec_off)
    end, strand = u32(result["end"])[:n], u32(result["strand"])[:n]
    wq = np.where(end != NO_END, 2 * np.arange(n) + (strand & 1), NONE)
    mapq, proper = u32(result["mapq"])[:n], None
    if mode == "paired":
        proper = (u32(result["n_proper"]) != 0) | (u32(result["resc_mate"]) != NONE)
        mapq = np.where(np.repeat(proper, 2), np.repeat(u32(result["pair_mapq"]), 2), mapq)
    queries = [q for r in reads for q in (r, RC(r))]
    recs, want_status = sam_model(texts, DNA, queries, 2, PAIRED if mode == "paired" else SINGLE, k, wq, u32(result["text_id"])[:n],
                                  u32(result["dist"])[:n], u32(result["begin"])[:n], end, u32(result["n_cigar"])[:n],
                                  u32(result["cigar"]).reshape(-1, 2 * k + 1)[:n], mapq, proper=proper)
    assert lines == recs and not status.cpu().numpy().any() and not any(want_status)
    bound = eng.sam_record_bound(longest, 0, 0, k)
    assert bound == record_bound(longest, 0, 0, k) and max(len(x) for x in lines) <= bound
    for i, line in enumerate(lines):
        if end[i] == NO_END:
            assert int(line.split(b"\t")[1]) & 4
            continue
        name, b, segment = rebuild_clipped_segment(line)
        t = int(name)
        assert b == u32(result["begin"])[i] and segment == texts[t][b:int(end[i])], (i, line)
    return lines


def test_sam_records_of_the_clipped_single_end_result():
    texts, reads, kind, g, eng, dq, plain, clipped = chain_case()
    sq = dq.with_strands(g, "both")
    lines = assert_sam(texts, eng, reads, sq, clipped, "single", CHAIN_K, 100)
    assert sum(b"S" in line.split(b"\t")[5] for line in lines) >= 60


def test_map_pairs_with_rescue_and_clip():
    import torch

    from genedex_amd.device import DeviceEngine, DeviceQueries

    rng = np.random.default_rng(26600)
    text = random_text(rng, PLANTED["text_len"])
    n_pairs, k = 12, PLANTED["max_edits"]
    reads, damaged, origin = planted_pairs(rng, text, n_pairs)
    # a junk tail on the intact mate of every third pair: something to clip besides something to clip away
    for p in range(0, n_pairs, 3):
        i = 2 * p + (1 - damaged[p])
        reads[i] = reads[i][:56] + reads[i][56:].translate(bytes.maketrans(b"ACGT", b"TGCA"))
    g, r = gpu_index([text], DNA), gpu_index(reversed_texts([text]), DNA)
    eng = DeviceEngine(g)
    dq = DeviceQueries.from_host(*join(reads))
    sq = dq.with_strands(g, "both")
    knobs = dict(max_edits=k, min_insert=PLANTED["min_insert"], max_insert=PLANTED["max_insert"], **KNOBS)
    plain = eng.map_pairs(dq, r, rescue=True, **knobs)
    # the damaged mate of a planted pair scores 7 - 4 + 14 - 4 + 14 - 4 + 14 - 4 + 7 = 40: a least score of 50 clips it away
    for clip in ((1, 4, 6, 1, 0), (1, 4, 6, 1, 50)):
        clipped = eng.map_pairs(dq, r, rescue=True, clip=clip, **knobs)
        torch.cuda.synchronize()
        want = assert_clipped_equals_the_model(plain, clipped, k, clip, 2 * n_pairs)
        lines = assert_sam([text], eng, reads, sq, clipped, "paired", k, PLANTED["mate_len"])
        gone = want[3] == NO_END
        if clip[4] == 0:
            assert not gone.any()
            continue
        hurt = 2 * np.arange(n_pairs) + np.array(damaged)
        assert gone[hurt].all() and not gone[hurt ^ 1].any() and (want[0][hurt] == 40).all() and (want[1][hurt] == k + 1).all()
        for i in hurt:                                                            # the clipped-away mate is unmapped, its partner says so
            mine, other = int(lines[i].split(b"\t")[1]), int(lines[i ^ 1].split(b"\t")[1])
            assert mine & 0x4 and not mine & 0x2 and other & 0x8 and not other & 0x4 and not other & 0x2, (i, mine, other)


def test_without_clip_the_results_have_todays_keys():
    texts, reads, kind, g, eng, dq, plain, clipped = chain_case()
    from genedex_amd.device import DeviceQueries

    assert set(plain) == {"strand", "text_id", "begin", "end", "dist", "sub_dist", "n_best", "mapq", "n_cigar", "cigar"}
    r = gpu_index(reversed_texts(texts), DNA)
    few = DeviceQueries.from_host(*join(reads[:8]))
    per_mate = {"strand", "text_id", "begin", "end", "dist", "n_cigar", "cigar", "mapq", "n_best", "sub_dist"}
    per_pair = {"n_proper", "pair_n_best", "pair_dist", "pair_sub_dist", "pair_mapq", "pair_span"}
    knobs = dict(max_edits=CHAIN_K, min_insert=100, max_insert=500, **KNOBS)
    assert set(eng.map_pairs(few, r, **knobs)) == per_mate | per_pair
    assert set(eng.map_pairs(few, r, rescue=True, clip=None, **knobs)) == per_mate | per_pair | {"rescued", "resc_mate", "resc_pair_dist", "resc_span"}
    assert set(eng.map_reads(few, r, max_edits=CHAIN_K, clip=None, **KNOBS)) == set(plain)
