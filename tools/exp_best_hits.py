#!/usr/bin/env python3
"""gdx_best_hits_many_dev at the end of a resident chain: the time of the call beside gdx_edit_distance_many_dev over the same
slots, its achieved bytes per second against the streaming copy of the same run, and what it saves: gdx_align_many_dev over ALL
nq * max_candidates slots (the only route without the call) against best hits + gdx_align_many_dev over the nq winners.

The workload of tools/exp_candidates.py, so that the rows line up with profiles/r14: a synthetic A C G T text (GDX_EXP_TOTAL
symbols, default 2^30) and its genome-like variant, each with the default-shape index and the companion over the reversed text;
GDX_EXP_NQ (default 10 M) reads of 150 symbols with 0..3 edits made on the device; max_smems 16, min_length 19, band 8,
max_candidates 4, max_occ 8, max_edits = band + 3 = 11.  group_slots = max_candidates: a group is a read.  Per text:
  edit_ms            gdx_edit_distance_many_dev over all slots; best_ms the best-hits call over the same slots: medians of
                     GDX_EXP_REPS (default 7) calls after two warm-up calls, events on the stream
  best_GBps          (24 bytes per slot in + 40 bytes per group out) / best_ms, and stream_copy_GBps of measure_bandwidth()
  align_all_ms       gdx_align_many_dev over all slots with its CIGAR buffer and its best workspace (align_all_cigar_bytes,
                     align_all_workspace_bytes); winners_ms = best hits + gdx_align_many_dev over the winners, with theirs
  unmapped / tied / unique   the shares of reads with n_best 0, >= 2, 1
  winner_at_origin   the share of reads whose winner lies in their text within band + 3 diagonals of where the read was taken
Before anything is timed the nine outputs of the first GDX_EXP_CHECK (default 2^16) reads are held equal to a host model (numpy,
from the definition of include/gdx_experimental.h).
usage: python tools/exp_best_hits.py [report | profile]   -> JSON lines on stderr, one JSON result line on stdout; report also
writes best_hits.json and the measured table best_hits_table.md (embedded in profiles/r16/best_hits.md) into GDX_EXP_OUT
(default profiles/r16).  profile: a few calls only, for rocprofv3 --kernel-trace --stats, or for a --pmc run of its own"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from genedex_amd import alphabet  # noqa: E402
from genedex_amd.device import (DeviceEngine, DeviceQueries, build_index_from_device_text, genome_like_text,  # noqa: E402
                                measure_bandwidth, synth_text)
from genedex_amd.index import build_options  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "report"
total = int(os.environ.get("GDX_EXP_TOTAL", 1 << 30))
nq = int(os.environ.get("GDX_EXP_NQ", 10_000_000))
reps = int(os.environ.get("GDX_EXP_REPS", 7))
n_check = min(nq, int(os.environ.get("GDX_EXP_CHECK", 1 << 16)))
out_dir = os.environ.get("GDX_EXP_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r16"))
L, MAX_SMEMS, MIN_LENGTH, BAND, MAX_CANDIDATES, MAX_OCC = 150, 16, 19, 8, 4, 8
K = BAND + 3
NONE = 0xFFFFFFFF
dev = torch.device("cuda", 0)
torch.manual_seed(7)
a = alphabet.ascii_dna_with_n()
acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
res = {"total_symbols": total, "reads": nq, "read_length": L, "reps": reps, "max_smems": MAX_SMEMS, "min_length": MIN_LENGTH,
       "band": BAND, "max_candidates": MAX_CANDIDATES, "max_occ": MAX_OCC, "max_edits": K, "checked_reads": n_check, "rows": []}


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


def make_reads(io_text):
    """(the batch, origin[nq]): tools/exp_candidates.py's reads"""
    origin = torch.randint(0, total - L - 8, (nq,), device=dev)
    qbuf = torch.zeros(nq * L + 8, dtype=torch.uint8, device=dev)
    ar = torch.arange(L, device=dev)
    for lo in range(0, nq, 1 << 20):
        hi = min(nq, lo + (1 << 20))
        n = hi - lo
        src = origin[lo:hi, None] + ar[None, :]
        edits = []
        for _ in range(3):  # up to three edits (two draws may fall on the same offset)
            on = torch.rand(n, device=dev) < 0.5
            at = torch.randint(5, L - 5, (n,), device=dev)
            kind = torch.randint(0, 3, (n,), device=dev)  # 0 substitution, 1 inserted symbol, 2 skipped text symbol
            skip, insert = (on & (kind == 2)).long(), (on & (kind == 1)).long()
            src = src + skip[:, None] * (ar[None, :] >= at[:, None]) - insert[:, None] * (ar[None, :] > at[:, None])
            edits.append((on & (kind != 2), at))
        block = io_text[src.reshape(-1)].reshape(n, L)
        for on, at in edits:
            rows = torch.nonzero(on).reshape(-1)
            block[rows, at[rows]] = acgt[torch.randint(0, 4, (rows.numel(),), device=dev)]
        qbuf[lo * L:hi * L] = block.reshape(-1)
    return DeviceQueries(qbuf, torch.arange(0, nq + 1, dtype=torch.int64, device=dev) * L, nq, nq * L), origin


def host_model(cands, dist, end, n):
    """the ten output arrays of the first n groups, from the definition"""
    gs = MAX_CANDIDATES
    u32 = lambda t: t[:n * gs].cpu().numpy().view(np.uint32).astype(np.int64)  # noqa: E731
    cq, cb, d, e = (u32(x).reshape(n, gs) for x in (cands["cand_query"], cands["cand_begin"], dist, end))
    hits = u32(cands["cand_hits"]).reshape(n, gs, 2)
    t, p = hits[:, :, 0], hits[:, :, 1]
    j = np.broadcast_to(np.arange(gs), (n, gs))
    live = (cq != NONE) & (d <= K)
    rank = d * gs + j
    keep = live.copy()
    for o in range(gs):
        same = live[:, o:o + 1] & (cq == cq[:, o:o + 1]) & (t == t[:, o:o + 1]) & (e == e[:, o:o + 1])
        keep &= ~(same & (rank[:, o:o + 1] < rank))
    big = 1 << 62
    n_live = keep.sum(axis=1)
    mapped, rows = n_live > 0, np.arange(n)
    best = np.where(keep, rank, big).argmin(axis=1)
    bd = np.where(mapped, d[rows, best], K + 1)
    others = np.where(keep & (j != best[:, None]), d, big).min(axis=1)
    sub = np.where(others == big, K + 1, others)
    pick = lambda x, none: np.where(mapped, x[rows, best], none)  # noqa: E731
    return {"best_slot": np.where(mapped, best, NONE), "best_dist": bd, "sub_dist": sub, "n_live": n_live,
            "n_best": (keep & (d == bd[:, None])).sum(axis=1), "mapq": np.where(mapped, np.minimum(60, 60 * (sub - bd) // (K + 1)), 255),
            "win_query": pick(cq, NONE), "win_begin": pick(cb, 0), "win_text": pick(t, 0), "win_position": pick(p, 0)}


def check_against_model(cands, dist, end, best, where):
    want = host_model(cands, dist, end, n_check)
    got = {name: best[name][:n_check].cpu().numpy().view(np.uint32).astype(np.int64)
           for name in ("best_slot", "best_dist", "sub_dist", "n_live", "n_best", "mapq", "win_query", "win_begin")}
    hits = best["win_hits"][:n_check].cpu().numpy().view(np.uint32).astype(np.int64)
    got["win_text"], got["win_position"] = hits[:, 0], hits[:, 1]
    for name, w in want.items():
        if not np.array_equal(got[name], w):
            bad = int(np.flatnonzero(got[name] != w)[0])
            raise SystemExit(f"PARITY FAILURE: {name} differs from the host model at {bad}: {int(got[name][bad])} != {int(w[bad])} ({where})")


if what == "report":
    res["bandwidth"] = measure_bandwidth(dev)
    print(json.dumps(res["bandwidth"]), file=sys.stderr, flush=True)

for text_name in ("synthetic", "genome-like"):
    io_text = synth_text(total, seed=42, n_per_million=0, device=dev) if text_name == "synthetic" else genome_like_text(total, dev)
    t0 = time.time()
    index = build_index_from_device_text(io_text, [total], a, index_storage="u32")
    companion = build_index_from_device_text(io_text.flip(0).contiguous(), [total], a, index_storage="u32",
                                             options=build_options(seed_symbols=0, text_units=False, full_suffix_array=False,
                                                                   inverse_suffix_array=False, jump_entry_bytes=0))
    eng, reng = DeviceEngine(index), DeviceEngine(companion)
    print(json.dumps({"text": text_name, "build_s": time.time() - t0}), file=sys.stderr, flush=True)
    dq, origin = make_reads(io_text)
    smems = eng.alloc_smems(nq, MAX_SMEMS)
    eng.smems(dq, reng, MAX_SMEMS, MIN_LENGTH, smems)
    cands = eng.seed_candidates(smems, nq, MAX_SMEMS, MAX_OCC, BAND, MAX_CANDIDATES)
    del smems
    slots = nq * MAX_CANDIDATES
    dist, end = eng.edit_distance(dq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], K)
    best = eng.alloc_best_hits(nq)
    for t in best.values():
        t.fill_(0x55)
    eng.best_hits(cands, dist, end, nq, MAX_CANDIDATES, K, out=best)
    torch.cuda.synchronize()
    check_against_model(cands, dist, end, best, text_name)
    if what == "profile":
        continue
    n_best = best["n_best"][:nq]
    mapped = best["best_slot"][:nq] != -1
    diag = best["win_hits"][:nq, 1].long() - best["win_begin"][:nq].long()
    at_origin = mapped & (best["win_hits"][:nq, 0] == 0) & ((diag - origin).abs() <= BAND + 3)
    row = {"text": text_name, "equal_to_host_model": True, "slots": slots,
           "slots_in_use": float((cands["cand_query"] != -1).float().mean()),
           "unmapped": float((n_best == 0).float().mean()), "tied": float((n_best >= 2).float().mean()),
           "unique": float((n_best == 1).float().mean()), "winner_at_origin": float(at_origin.float().mean()),
           "mapq_60": float((best["mapq"][:nq] == 60).float().mean())}
    row["edit_ms"] = median_ms(lambda: eng.edit_distance(dq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], K, dist, end))
    row["best_ms"] = median_ms(lambda: eng.best_hits(cands, dist, end, nq, MAX_CANDIDATES, K, out=best))
    row["best_bytes"] = 24 * slots + 40 * nq
    row["best_GBps"] = row["best_bytes"] / row["best_ms"] / 1e6
    row["share_of_stream_copy"] = row["best_GBps"] / res["bandwidth"]["stream_copy_GBps"]
    row["times_edit_distance"] = row["best_ms"] / row["edit_ms"]

    def timed_align(cq, cb, ch, m):
        ws_bytes = eng.align_workspace_bytes(dq, m, K)[1]
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = {name: torch.empty(m, dtype=torch.int32, device=dev) for name in ("dist", "begin", "end", "n_cigar")}
        out["cigar"] = torch.empty((m, 2 * K + 1), dtype=torch.int32, device=dev)
        ms = median_ms(lambda: eng.align(dq, cq, cb, ch, K, out=out, workspace=workspace))
        return ms, out["cigar"].numel() * 4, ws_bytes

    row["align_all_ms"], row["align_all_cigar_bytes"], row["align_all_workspace_bytes"] = timed_align(
        cands["cand_query"], cands["cand_begin"], cands["cand_hits"], slots)
    row["align_winners_ms"], row["winners_cigar_bytes"], row["winners_workspace_bytes"] = timed_align(
        best["win_query"][:nq], best["win_begin"][:nq], best["win_hits"][:nq], nq)
    row["winners_ms"] = row["best_ms"] + row["align_winners_ms"]
    row["winners_over_all"] = row["winners_ms"] / row["align_all_ms"]
    res["rows"].append(row)
    print(json.dumps(row), file=sys.stderr, flush=True)
    del index, companion, eng, reng, dq, origin, cands, dist, end, best, io_text, n_best, mapped, diag, at_origin
    torch.cuda.empty_cache()

print(json.dumps(res))
if what == "report":
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "best_hits.json"), "w") as f:
        f.write(json.dumps(res) + "\n")
    mib = lambda b: "%.0f MiB" % (b / (1 << 20))  # noqa: E731
    head = ("text", "slots in use", "unmapped", "tied", "unique", "winner at origin", "edit distance, all slots", "best hits",
            "x edit distance", "GB/s", "of stream copy", "align, all slots", "its CIGAR buffer", "its workspace",
            "best hits + align, winners", "its CIGAR buffer", "its workspace", "x align, all slots")
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in res["rows"]:
        lines.append("| %s | %.3f | %.4f | %.4f | %.4f | %.4f | %.1f ms | %.2f ms | %.3f | %.0f | %.2f | %.1f ms | %s | %s | %.1f ms | %s | %s | %.2f |" % (
            r["text"], r["slots_in_use"], r["unmapped"], r["tied"], r["unique"], r["winner_at_origin"], r["edit_ms"], r["best_ms"],
            r["times_edit_distance"], r["best_GBps"], r["share_of_stream_copy"], r["align_all_ms"], mib(r["align_all_cigar_bytes"]),
            mib(r["align_all_workspace_bytes"]), r["winners_ms"], mib(r["winners_cigar_bytes"]), mib(r["winners_workspace_bytes"]),
            r["winners_over_all"]))
    with open(os.path.join(out_dir, "best_hits_table.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
