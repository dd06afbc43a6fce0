#!/usr/bin/env python3
"""gdx_pair_hits_many_dev at the end of a resident chain over read pairs: the time of the call beside gdx_best_hits_many_dev over
the same slots, its achieved bytes per second against the streaming copy of the same run, and what pairing decides: the share of
pairs that are proper, the share of reads tied single-end whose pair is unique, and the winners at their origin single-end
against paired.

The workload of tools/exp_best_hits.py (profiles/r16), its reads taken as pairs: a synthetic A C G T text (GDX_EXP_TOTAL symbols,
default 2^30) and its genome-like variant, each with the default-shape index and the companion over the reversed text;
GDX_EXP_NQ (default 10 M) reads of 150 symbols with 0..3 edits made on the device, reads 2p and 2p + 1 the mates of pair p: a
fragment of 300 .. 600 symbols (uniform) at a random place, one mate its first 150 symbols, the other the reverse complement of
its last 150, the forward mate first in even pairs and second in odd ones.  with_strands("both") in front; max_smems 16,
min_length 19, band 8, max_candidates 4, max_occ 8, max_edits = band + 3 = 11, mate_slots = 2 * max_candidates = 8, insert
bounds [250, 650].  Per text:
  pair_ms            gdx_pair_hits_many_dev; best_ms gdx_best_hits_many_dev over the same slots (n_groups = reads, group_slots =
                     8): medians of GDX_EXP_REPS (default 7) calls after two warm-up calls, events on the stream
  pair_GBps          (24 bytes per slot in + 24 per pair + 24 per mate out) / pair_ms, and stream_copy_GBps of measure_bandwidth()
  proper             the share of pairs with n_proper >= 1; unique_pairs those with n_proper >= 1 and n_best == 1
  tied_single_end    the share of reads with single-end n_best >= 2; rescued the share OF THOSE whose pair is unique
  at_origin_single / at_origin_paired   the share of reads whose single-end / paired winner lies in their text, on their strand,
                     within band + 3 diagonals of where the read was taken
Before anything is timed the outputs of the first GDX_EXP_CHECK (default 2^16) pairs are held equal to a host model (numpy, from
the definition of include/gdx_experimental.h).
usage: python tools/exp_pair_hits.py [report | profile]   -> JSON lines on stderr, one JSON result line on stdout; report also
writes pair_hits.json and the measured table pair_hits_table.md (embedded in profiles/r17/pair_hits.md) into GDX_EXP_OUT
(default profiles/r17).  profile: a few calls only, for rocprofv3 --kernel-trace --stats, or for a --pmc run of its own"""
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
nq = int(os.environ.get("GDX_EXP_NQ", 10_000_000)) & ~1
reps = int(os.environ.get("GDX_EXP_REPS", 7))
n_pairs = nq // 2
n_check = min(n_pairs, int(os.environ.get("GDX_EXP_CHECK", 1 << 16)))
out_dir = os.environ.get("GDX_EXP_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r17"))
L, MAX_SMEMS, MIN_LENGTH, BAND, MAX_CANDIDATES, MAX_OCC = 150, 16, 19, 8, 4, 8
K, MS = BAND + 3, 2 * MAX_CANDIDATES
FRAGMENT, MIN_INSERT, MAX_INSERT = (300, 600), 250, 650
NONE = 0xFFFFFFFF
dev = torch.device("cuda", 0)
torch.manual_seed(7)
a = alphabet.ascii_dna_with_n()
acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
complement = torch.arange(256, dtype=torch.uint8, device=dev)
for x, y in (b"AT", b"TA", b"CG", b"GC"):
    complement[x] = y
res = {"total_symbols": total, "reads": nq, "pairs": n_pairs, "read_length": L, "fragment": list(FRAGMENT), "min_insert": MIN_INSERT,
       "max_insert": MAX_INSERT, "reps": reps, "max_smems": MAX_SMEMS, "min_length": MIN_LENGTH, "band": BAND,
       "max_candidates": MAX_CANDIDATES, "max_occ": MAX_OCC, "max_edits": K, "mate_slots": MS, "checked_pairs": n_check, "rows": []}


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
    """(the batch with the mates interleaved, origin[nq]: where the forward form of a read was taken, reverse[nq]: its strand)"""
    start = torch.randint(0, total - FRAGMENT[1] - 8, (n_pairs,), device=dev)
    length = torch.randint(FRAGMENT[0], FRAGMENT[1] + 1, (n_pairs,), device=dev)
    read = torch.arange(nq, device=dev)
    reverse = ((read & 1) ^ ((read >> 1) & 1)).bool()           # the second mate of an even pair, the first of an odd one
    origin = start[read >> 1] + torch.where(reverse, length[read >> 1] - L, torch.zeros_like(read))
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
        block = torch.where(reverse[lo:hi, None], complement[block.flip(1).long()], block)
        qbuf[lo * L:hi * L] = block.reshape(-1)
    return DeviceQueries(qbuf, torch.arange(0, nq + 1, dtype=torch.int64, device=dev) * L, nq, nq * L), origin, reverse


def host_model(cands, dist, end, n):
    """the output arrays of the first n pairs, from the definition"""
    u32 = lambda t: t[:2 * n * MS].cpu().numpy().view(np.uint32).astype(np.int64)  # noqa: E731
    cq, cb, d, e = (u32(x).reshape(2 * n, MS) for x in (cands["cand_query"], cands["cand_begin"], dist, end))
    hits = u32(cands["cand_hits"]).reshape(2 * n, MS, 2)
    t, p = hits[:, :, 0], hits[:, :, 1]
    j = np.broadcast_to(np.arange(MS), (2 * n, MS))
    live = (cq != NONE) & (d <= K)
    rank = d * MS + j
    keep = live.copy()
    for o in range(MS):
        same = live[:, o:o + 1] & (cq == cq[:, o:o + 1]) & (t == t[:, o:o + 1]) & (e == e[:, o:o + 1])
        keep &= ~(same & (rank[:, o:o + 1] < rank))
    strand, diag = cq & 1, p - cb
    m0, m1 = (lambda x: x[0::2][:, :, None]), (lambda x: x[1::2][:, None, :])
    span = np.where(m0(strand) == 0, m1(e) - m0(diag), m0(e) - m1(diag))
    proper = m0(keep) & m1(keep) & (m0(t) == m1(t)) & (m0(strand) != m1(strand)) & (span >= MIN_INSERT) & (span <= MAX_INSERT)
    score = (m0(d) + m1(d)).reshape(n, -1)
    proper, span = proper.reshape(n, -1), span.reshape(n, -1)
    big, rows = 1 << 62, np.arange(n)
    n_proper = proper.sum(axis=1)
    paired = n_proper > 0
    at = np.where(proper, score * MS * MS + np.arange(MS * MS)[None, :], big).argmin(axis=1)
    pd = np.where(paired, score[rows, at], 2 * K + 2)
    others = np.where(proper, score, big)
    others[rows, at] = big
    others = others.min(axis=1)
    sub = np.where(others == big, 2 * K + 2, others)
    own = np.where(keep, rank, big)                             # the single-end best of every mate
    alone, has = own.argmin(axis=1), keep.any(axis=1)
    slot = np.where(np.repeat(paired, 2), np.stack([at // MS, at % MS], axis=1).reshape(-1), alone)
    mapped, mates = np.repeat(paired, 2) | has, np.arange(2 * n)
    pick = lambda x, none: np.where(mapped, x[mates, slot], none)  # noqa: E731
    return {"n_proper": n_proper, "n_best": (proper & (score == pd[:, None])).sum(axis=1), "pair_dist": pd, "sub_dist": sub,
            "mapq": np.where(paired, np.minimum(60, 60 * (sub - pd) // (2 * K + 2)), 255),
            "pair_span": np.where(paired, span[rows, at], 0), "mate_slot": np.where(mapped, slot, NONE), "mate_dist": pick(d, K + 1),
            "win_query": pick(cq, NONE), "win_begin": pick(cb, 0), "win_text": pick(t, 0), "win_position": pick(p, 0)}


def check_against_model(cands, dist, end, pairs, where):
    want = host_model(cands, dist, end, n_check)
    u32 = lambda t, n: t[:n].cpu().numpy().view(np.uint32).astype(np.int64)  # noqa: E731
    got = {name: u32(pairs[name], n_check) for name in ("n_proper", "n_best", "pair_dist", "sub_dist", "mapq", "pair_span")}
    got.update({name: u32(pairs[name], 2 * n_check) for name in ("mate_slot", "mate_dist", "win_query", "win_begin")})
    hits = u32(pairs["win_hits"], 2 * n_check)
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
    dq, origin, reverse = make_pairs(io_text)
    sq = dq.with_strands(index, "both")
    smems = eng.alloc_smems(sq.nq, MAX_SMEMS)
    eng.smems(sq, reng, MAX_SMEMS, MIN_LENGTH, smems)
    cands = eng.seed_candidates(smems, sq.nq, MAX_SMEMS, MAX_OCC, BAND, MAX_CANDIDATES)
    del smems
    slots = sq.nq * MAX_CANDIDATES
    dist, end = eng.edit_distance(sq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], K)
    pairs, single = eng.alloc_pair_hits(n_pairs), eng.alloc_best_hits(nq)
    for t in list(pairs.values()) + list(single.values()):
        t.fill_(0x55)
    eng.pair_hits(cands, dist, end, n_pairs, MS, K, MIN_INSERT, MAX_INSERT, out=pairs)
    eng.best_hits(cands, dist, end, nq, MS, K, out=single)
    torch.cuda.synchronize()
    check_against_model(cands, dist, end, pairs, text_name)
    if what == "profile":
        continue

    def at_origin(win_query, win_begin, win_hits):
        diag = win_hits[:nq, 1].long() - win_begin[:nq].long()
        return ((win_query[:nq] != -1) & (win_hits[:nq, 0] == 0) & ((win_query[:nq] & 1).bool() == reverse) &
                ((diag - origin).abs() <= BAND + 3))

    proper = pairs["n_proper"][:n_pairs] >= 1
    unique = proper & (pairs["n_best"][:n_pairs] == 1)
    tied = single["n_best"][:nq] >= 2
    rescued = tied & unique.repeat_interleave(2)
    row = {"text": text_name, "equal_to_host_model": True, "slots": slots,
           "slots_in_use": float((cands["cand_query"] != -1).float().mean()),
           "proper": float(proper.float().mean()), "unique_pairs": float(unique.float().mean()),
           "tied_pairs": float((pairs["n_best"][:n_pairs] >= 2).float().mean()),
           "unmapped_single_end": float((single["n_best"][:nq] == 0).float().mean()),
           "tied_single_end": float(tied.float().mean()),
           "rescued": float(rescued.float().sum() / tied.float().sum().clamp(min=1)),
           "rescued_at_origin": float((rescued & at_origin(pairs["win_query"], pairs["win_begin"], pairs["win_hits"])).float().sum() /
                                      rescued.float().sum().clamp(min=1)),
           "at_origin_single": float(at_origin(single["win_query"], single["win_begin"], single["win_hits"]).float().mean()),
           "at_origin_paired": float(at_origin(pairs["win_query"], pairs["win_begin"], pairs["win_hits"]).float().mean()),
           "pair_mapq_60": float((pairs["mapq"][:n_pairs] == 60).float().mean())}
    row["pair_ms"] = median_ms(lambda: eng.pair_hits(cands, dist, end, n_pairs, MS, K, MIN_INSERT, MAX_INSERT, out=pairs))
    row["best_ms"] = median_ms(lambda: eng.best_hits(cands, dist, end, nq, MS, K, out=single))
    row["pair_bytes"] = 24 * slots + 24 * n_pairs + 24 * nq
    row["best_bytes"] = 24 * slots + 40 * nq
    row["pair_GBps"] = row["pair_bytes"] / row["pair_ms"] / 1e6
    row["best_GBps"] = row["best_bytes"] / row["best_ms"] / 1e6
    row["share_of_stream_copy"] = row["pair_GBps"] / res["bandwidth"]["stream_copy_GBps"]
    row["times_best_hits"] = row["pair_ms"] / row["best_ms"]
    res["rows"].append(row)
    print(json.dumps(row), file=sys.stderr, flush=True)
    del index, companion, eng, reng, dq, sq, origin, reverse, cands, dist, end, pairs, single, io_text, proper, unique, tied, rescued
    torch.cuda.empty_cache()

print(json.dumps(res))
if what == "report":
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "pair_hits.json"), "w") as f:
        f.write(json.dumps(res) + "\n")
    head = ("text", "slots in use", "pairs proper", "pairs unique", "reads tied single-end", "of those: pair unique",
            "of those: at origin", "at origin, single-end", "at origin, paired", "best hits", "pair hits", "x best hits", "GB/s",
            "of stream copy")
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in res["rows"]:
        lines.append("| %s | %.3f | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.2f ms | %.2f ms | %.2f | %.0f | %.2f |" % (
            r["text"], r["slots_in_use"], r["proper"], r["unique_pairs"], r["tied_single_end"], r["rescued"], r["rescued_at_origin"],
            r["at_origin_single"], r["at_origin_paired"], r["best_ms"], r["pair_ms"], r["times_best_hits"], r["pair_GBps"],
            r["share_of_stream_copy"]))
    with open(os.path.join(out_dir, "pair_hits_table.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
