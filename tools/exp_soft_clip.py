#!/usr/bin/env python3
"""gdx_soft_clip_many_dev behind the resident chain over read pairs: its time beside the traceback's over the same winners and
beside a device-to-device copy of the bytes it must read and write.

The workload of tools/exp_sam_records.py (profiles/r23) on the synthetic text: GDX_EXP_TOTAL symbols (default 2^30) with the
default-shape index and the companion over the reversed text; GDX_EXP_NQ (default 10 M) reads of 150 symbols with 0..3 edits as
interleaved pairs (fragments of 300 .. 600 symbols); the stages of map_pairs(rescue=True) one by one -- with_strands, smems,
seed_candidates, edit_distance, pair_hits, mate_rescue, align -- with max_smems 16, min_length 19, band 8, max_candidates 4,
max_occ 8, insert bounds [250, 650], then soft_clip with the scoring (1, 4, 6, 1) and min_score 0.  Two runs in one process:
  k11        max_edits 11, the reads as they are
  k24_junk   max_edits 24, the last 20 symbols of every eighth read replaced by random ones
Per run:
  clip_ms    the clip call;  align_ms  gdx_align_many_dev over the same winners
  copy_ms    torch's copy_ moving as many bytes as the call must read and write: four words per row in, seven and the status
             byte out, n_cigar words in and out_n_cigar words out (io_bytes, computed here); a copy reads and writes each of
             its bytes once, so it runs over io_bytes / 2
  medians of GDX_EXP_REPS (default 7) calls after two warm-up calls, events on the stream
  clipped / clipped_away: the share of the aligned reads that got an S run / that the stage dropped
Before anything is timed the first GDX_EXP_CHECK (default 2^16) rows of all eight outputs must equal the model of
tests/test_soft_clip_model.py over the traceback's rows.
usage: python tools/exp_soft_clip.py [report]   -> JSON lines on stderr, one JSON result line on stdout; report also writes
soft_clip.json into GDX_EXP_OUT (default profiles/r26)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from genedex_amd import alphabet  # noqa: E402
from genedex_amd.device import DeviceEngine, DeviceQueries, build_index_from_device_text, synth_text  # noqa: E402
from genedex_amd.index import build_options  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "report"
total = int(os.environ.get("GDX_EXP_TOTAL", 1 << 30))
nq = int(os.environ.get("GDX_EXP_NQ", 10_000_000)) & ~1
reps = int(os.environ.get("GDX_EXP_REPS", 7))
n_check = min(nq, int(os.environ.get("GDX_EXP_CHECK", 1 << 16)))
out_dir = os.environ.get("GDX_EXP_OUT", os.path.join(ROOT, "profiles", "r26"))
L, MAX_SMEMS, MIN_LENGTH, BAND, MAX_CANDIDATES, MAX_OCC = 150, 16, 19, 8, 4, 8
FRAGMENT, MIN_INSERT, MAX_INSERT = (300, 600), 250, 650
SCORING, JUNK = (1, 4, 6, 1, 0), 20
n_pairs = nq // 2
dev = torch.device("cuda", 0)
torch.manual_seed(7)
a = alphabet.ascii_dna_with_n()
acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
complement = torch.arange(256, dtype=torch.uint8, device=dev)
for x, y in (b"AT", b"TA", b"CG", b"GC"):
    complement[x] = y


def median_ms(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return sorted(out)[len(out) // 2]


def make_pairs(io_text):
    """tools/exp_sam_records.py's batch: the mates interleaved, the forward mate first in even pairs and second in odd ones"""
    start = torch.randint(0, total - FRAGMENT[1] - 8, (n_pairs,), device=dev)
    length = torch.randint(FRAGMENT[0], FRAGMENT[1] + 1, (n_pairs,), device=dev)
    read = torch.arange(nq, device=dev)
    reverse = ((read & 1) ^ ((read >> 1) & 1)).bool()
    origin = start[read >> 1] + torch.where(reverse, length[read >> 1] - L, torch.zeros_like(read))
    qbuf = torch.zeros(nq * L + 8, dtype=torch.uint8, device=dev)
    ar = torch.arange(L, device=dev)
    for lo in range(0, nq, 1 << 20):
        hi = min(nq, lo + (1 << 20))
        n = hi - lo
        src = origin[lo:hi, None] + ar[None, :]
        edits = []
        for _ in range(3):
            on = torch.rand(n, device=dev) < 0.5
            at = torch.randint(5, L - 5, (n,), device=dev)
            kind = torch.randint(0, 3, (n,), device=dev)
            skip, insert = (on & (kind == 2)).long(), (on & (kind == 1)).long()
            src = src + skip[:, None] * (ar[None, :] >= at[:, None]) - insert[:, None] * (ar[None, :] > at[:, None])
            edits.append((on & (kind != 2), at))
        block = io_text[src.reshape(-1)].reshape(n, L)
        for on, at in edits:
            rows = torch.nonzero(on).reshape(-1)
            block[rows, at[rows]] = acgt[torch.randint(0, 4, (rows.numel(),), device=dev)]
        block = torch.where(reverse[lo:hi, None], complement[block.flip(1).long()], block)
        qbuf[lo * L:hi * L] = block.reshape(-1)
    return qbuf


def batch(qbuf):
    return DeviceQueries(qbuf, torch.arange(0, nq + 1, dtype=torch.int64, device=dev) * L, nq, nq * L)


def run(eng, reng, dq, k):
    """the stages of map_pairs(rescue=True) up to the winners, then the traceback and the clip, checked and timed"""
    from test_soft_clip_model import OUT_NAMES, assert_same, clip_model

    mc = MAX_CANDIDATES
    sq = dq.with_strands(eng.index, "both")
    seeds = eng.alloc_smems(sq.nq, MAX_SMEMS)
    eng.smems(sq, reng, MAX_SMEMS, MIN_LENGTH, seeds)
    cands = eng.seed_candidates(seeds, sq.nq, MAX_SMEMS, MAX_OCC, BAND, mc)
    dist, end = eng.edit_distance(sq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], k)
    pairs = eng.pair_hits(cands, dist, end, n_pairs, 2 * mc, k, MIN_INSERT, MAX_INSERT)
    win = eng.mate_rescue(sq, end, pairs, n_pairs, 2 * mc, k, MIN_INSERT, MAX_INSERT)
    del seeds
    wq, wb, wh = win["win_query"][:nq], win["win_begin"][:nq], win["win_hits"][:nq]
    workspace = torch.empty(eng.align_workspace_bytes(sq, nq, k)[1], dtype=torch.uint8, device=dev)
    aligned = eng.align(sq, wq, wb, wh, k, workspace=workspace)
    clipped = eng.soft_clip(aligned, k, SCORING)
    torch.cuda.synchronize()
    # the first rows of all eight outputs (and the status) against the model
    u32 = lambda t: t[:n_check].cpu().numpy().view(np.uint32)  # noqa: E731
    rows = tuple(u32(aligned[name]) for name in ("dist", "begin", "end", "n_cigar", "cigar"))
    want = clip_model(*rows, k, *SCORING, single_pass=True)
    below = np.arange(2 * k + 1)[None, :] < want[6][:, None]
    got = tuple(clipped[name][:n_check].cpu().numpy() if name in ("score", "status") else u32(clipped[name]) for name in OUT_NAMES)
    got = got[:7] + (np.where(below, got[7], 0),) + got[8:]
    assert_same(got, want, ("PARITY FAILURE", k))
    has = aligned["end"][:nq] != -1
    kept = clipped["end"][:nq] != -1
    n_aligned = int(has.sum().item())
    words_in = int(aligned["n_cigar"][:nq][has].sum().item())
    words_out = int(clipped["n_cigar"][:nq].sum().item())
    io_bytes = 4 * (4 * nq + words_in) + 4 * (7 * nq + words_out) + nq
    res = {"max_edits": k, "aligned": n_aligned / nq, "checked_rows": n_check,
           "clipped": int(((clipped["clip_left"][:nq] != 0) | (clipped["clip_right"][:nq] != 0)).sum().item()) / max(n_aligned, 1),
           "clipped_away": int((has & ~kept).sum().item()) / max(n_aligned, 1), "status_bad": int(clipped["status"][:nq].sum().item()),
           "mean_runs_in": words_in / max(n_aligned, 1), "io_bytes": io_bytes, "io_bytes_per_read": io_bytes / nq}
    res["clip_ms"] = median_ms(lambda: eng.soft_clip(aligned, k, SCORING, out=clipped))
    res["align_ms"] = median_ms(lambda: eng.align(sq, wq, wb, wh, k, out=aligned, workspace=workspace))
    src = torch.empty(io_bytes // 2 // 16 * 16, dtype=torch.uint8, device=dev).fill_(7)   # a copy reads and writes each byte once
    dst = torch.empty_like(src)
    res["copy_ms"] = median_ms(lambda: dst.copy_(src))
    res["clip_over_copy"] = res["clip_ms"] / res["copy_ms"]
    res["clip_over_align"] = res["clip_ms"] / res["align_ms"]
    return res


io_text = synth_text(total, seed=42, n_per_million=0, device=dev)
t0 = time.time()
index = build_index_from_device_text(io_text, [total], a, index_storage="u32")
companion = build_index_from_device_text(io_text.flip(0).contiguous(), [total], a, index_storage="u32",
                                         options=build_options(seed_symbols=0, text_units=False, full_suffix_array=False,
                                                               inverse_suffix_array=False, jump_entry_bytes=0))
eng, reng = DeviceEngine(index), DeviceEngine(companion)
print(json.dumps({"build_s": time.time() - t0}), file=sys.stderr, flush=True)
qbuf = make_pairs(io_text)
res = {"total_symbols": total, "reads": nq, "read_length": L, "scoring": list(SCORING), "reps": reps}
res["k11"] = run(eng, reng, batch(qbuf), BAND + 3)
print(json.dumps(res["k11"]), file=sys.stderr, flush=True)
tails = qbuf[:nq * L].reshape(nq, L)[::8, L - JUNK:]
tails.copy_(acgt[torch.randint(0, 4, tuple(tails.shape), device=dev)])
res["k24_junk"] = run(eng, reng, batch(qbuf), 24)
res["k24_junk"]["junk_reads"] = 1 / 8
print(json.dumps(res))
if what == "report":
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "soft_clip.json"), "w") as f:
        f.write(json.dumps(res) + "\n")
