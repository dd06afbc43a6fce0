#!/usr/bin/env python3
"""gdx_seed_candidates_many_dev between its two neighbours in a resident chain: the time of the candidates call, of
gdx_smems_many_dev in front of it on the same batch and of gdx_edit_distance_many_dev behind it over ALL nq * max_candidates
slots, and what the candidates are worth.

Texts: a synthetic A C G T text (GDX_EXP_TOTAL symbols, default 2^30) and its genome-like variant (segmental duplications,
tandem repeats, poly-A, runs of N: genedex_amd.device.genome_like_text), each with the default-shape index and the companion
over the reversed text that gdx_smems_many needs.  Reads: GDX_EXP_NQ (default 10 M) reads of 150 symbols that follow the text
from a random origin with 0..3 edits at offsets in [5, L - 5), each a substitution, an inserted symbol or a skipped text symbol,
made on the device (the workload of tools/exp_align.py).  max_smems 16, min_length 19, band 8, max_candidates 4, max_occ 8 and
64.  Per text and max_occ:
  candidates_ms   median of GDX_EXP_REPS (default 7) calls after two warm-up calls, events on the stream
  smems_ms        the same for gdx_smems_many_dev on the batch, edit_ms for gdx_edit_distance_many_dev (max_edits = band + 3)
                  over all slots, unused ones included, and the two ratios
  slots_in_use    n_candidates summed over nq * max_candidates; anchors_per_read; reads_with_skipped_seeds
  origin_found    the share of reads with a candidate of their text whose diagonal is within band + 3 of the read's origin
Before anything is timed the outputs of the first GDX_EXP_CHECK (default 2^16) reads are held equal to a host model: the hits
of the seeds' rows from gdx_cursor_locate_many, then a sort of tuples, a linear scan for the groups, a coverage array for the
weight.
usage: python tools/exp_candidates.py [report | profile]   -> JSON lines on stderr, one JSON result line on stdout; report also
writes candidates.json and the measured table candidates_table.md (embedded in profiles/r14/candidates.md) into GDX_EXP_OUT
(default profiles/r14).  profile: a few calls only, for rocprofv3 --kernel-trace --stats, or for a --pmc run of its own"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from genedex_amd import alphabet  # noqa: E402
from genedex_amd.device import DeviceEngine, DeviceQueries, build_index_from_device_text, genome_like_text, synth_text  # noqa: E402
from genedex_amd.index import build_options  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "report"
total = int(os.environ.get("GDX_EXP_TOTAL", 1 << 30))
nq = int(os.environ.get("GDX_EXP_NQ", 10_000_000))
reps = int(os.environ.get("GDX_EXP_REPS", 7))
n_check = min(nq, int(os.environ.get("GDX_EXP_CHECK", 1 << 16)))
out_dir = os.environ.get("GDX_EXP_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r14"))
L, MAX_SMEMS, MIN_LENGTH, BAND, MAX_CANDIDATES = 150, 16, 19, 8, 4
K = BAND + 3
NONE = -1
dev = torch.device("cuda", 0)
torch.manual_seed(7)
a = alphabet.ascii_dna_with_n()
acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
res = {"total_symbols": total, "reads": nq, "read_length": L, "reps": reps, "max_smems": MAX_SMEMS, "min_length": MIN_LENGTH,
       "band": BAND, "max_candidates": MAX_CANDIDATES, "max_edits": K, "checked_reads": n_check, "rows": []}


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
    """(the batch, origin[nq]): tools/exp_align.py's reads at one length"""
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


def host_model(index, smems, max_occ, n):
    """the nine outputs for the first n reads, from the definition: located hits, a sort of tuples, a linear scan"""
    u32 = lambda t, k: t[:k].cpu().numpy().view(np.uint32).astype(np.int64)  # noqa: E731
    n_seeds = u32(smems["n_smems"], n)
    begin, length, start, end = (u32(smems[x], n * MAX_SMEMS) for x in ("begin", "length", "start", "end"))
    used = (np.arange(n * MAX_SMEMS) % MAX_SMEMS) < np.repeat(n_seeds, MAX_SMEMS)
    kept = used & (end - start <= max_occ)
    off, t_ids, pos = index.locate_intervals_raw(np.where(kept, start, 0), np.where(kept, end, 0))
    off, t_ids, pos = off.astype(np.int64), t_ids.astype(np.int64), pos.astype(np.int64)
    mc = MAX_CANDIDATES
    n_cand, n_groups = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    n_skipped = (used & ~kept).reshape(n, MAX_SMEMS).sum(axis=1)
    cq, cb, cw = np.full(n * mc, NONE, dtype=np.int64), np.zeros(n * mc, dtype=np.int64), np.zeros(n * mc, dtype=np.int64)
    ct, cp = np.zeros(n * mc, dtype=np.int64), np.zeros(n * mc, dtype=np.int64)
    for i in range(n):
        anchors = []
        for s in range(i * MAX_SMEMS, i * MAX_SMEMS + int(n_seeds[i])):
            anchors += [(int(t_ids[h]), int(pos[h] - begin[s]), int(begin[s]), int(length[s]), int(pos[h])) for h in range(off[s], off[s + 1])]
        anchors.sort()
        groups = []
        for an in anchors:
            if not groups or an[0] != groups[-1][0][0] or an[1] - groups[-1][0][1] > BAND:
                groups.append([])
            groups[-1].append(an)
        ranked = []
        for grp in groups:
            covered = np.zeros(L, dtype=bool)
            for _, _, b, ln, _ in grp:
                covered[b:b + ln] = True
            rep = grp[0]
            for an in grp[1:]:
                if an[3] > rep[3]:
                    rep = an
            ranked.append((-int(covered.sum()), grp[0][0], grp[0][1], rep))
        ranked.sort(key=lambda x: x[:3])
        n_groups[i], n_cand[i] = len(ranked), min(len(ranked), mc)
        for c, (neg_w, _, _, rep) in enumerate(ranked[:mc]):
            cq[i * mc + c], cb[i * mc + c], ct[i * mc + c], cp[i * mc + c], cw[i * mc + c] = i, rep[2], rep[0], rep[4], -neg_w
    return {"n_candidates": n_cand, "n_groups": n_groups, "n_skipped": n_skipped, "cand_query": cq, "cand_begin": cb,
            "cand_weight": cw, "text_id": ct, "position": cp}


def check_against_model(index, smems, cands, max_occ, where):
    want = host_model(index, smems, max_occ, n_check)
    hits = cands["cand_hits"][:n_check * MAX_CANDIDATES].cpu().numpy().view(np.uint32).astype(np.int64)
    got = {"text_id": hits[:, 0], "position": hits[:, 1]}
    for name in ("n_candidates", "n_groups", "n_skipped"):
        got[name] = cands[name][:n_check].cpu().numpy().view(np.uint32).astype(np.int64)
    for name in ("cand_begin", "cand_weight"):
        got[name] = cands[name][:n_check * MAX_CANDIDATES].cpu().numpy().view(np.uint32).astype(np.int64)
    got["cand_query"] = cands["cand_query"][:n_check * MAX_CANDIDATES].cpu().numpy().astype(np.int64)  # (-1: GDX_CAND_NONE)
    for name, w in want.items():
        if not np.array_equal(got[name], w):
            bad = int(np.flatnonzero(got[name] != w)[0])
            raise SystemExit(f"PARITY FAILURE: {name} differs from the host model at {bad}: {int(got[name][bad])} != {int(w[bad])} ({where})")
    if cands["status"][:n_check].any():
        raise SystemExit(f"PARITY FAILURE: a status is set ({where})")


for text_name in ("synthetic", "genome-like"):
    io_text = synth_text(total, seed=42, n_per_million=0, device=dev) if text_name == "synthetic" else genome_like_text(total, dev)
    t0 = time.time()
    index = build_index_from_device_text(io_text, [total], a, index_storage="u32")
    companion = build_index_from_device_text(io_text.flip(0).contiguous(), [total], a, index_storage="u32",
                                             options=build_options(seed_symbols=0, text_units=False, full_suffix_array=False,
                                                                   inverse_suffix_array=False, jump_entry_bytes=0))
    eng, reng = DeviceEngine(index), DeviceEngine(companion)
    print(json.dumps({"text": text_name, "build_s": time.time() - t0, "aux": eng.aux_info()}), file=sys.stderr, flush=True)
    dq, origin = make_reads(io_text)
    smems = eng.alloc_smems(nq, MAX_SMEMS)
    eng.smems(dq, reng, MAX_SMEMS, MIN_LENGTH, smems)
    torch.cuda.synchronize()
    slots = nq * MAX_CANDIDATES
    e_dist = torch.empty(slots, dtype=torch.int32, device=dev)
    e_end = torch.empty(slots, dtype=torch.int32, device=dev)
    occ = (smems["end"] - smems["start"]).reshape(nq, MAX_SMEMS)  # (rows < 2^31 here)
    in_use = torch.arange(MAX_SMEMS, device=dev)[None, :] < smems["n_smems"][:nq, None]
    for max_occ in (8, 64):
        cands = eng.alloc_seed_candidates(nq, MAX_CANDIDATES)
        for t in cands.values():
            t.fill_(0x55)
        eng.seed_candidates(smems, nq, MAX_SMEMS, max_occ, BAND, MAX_CANDIDATES, out=cands)
        torch.cuda.synchronize()
        check_against_model(index, smems, cands, max_occ, (text_name, max_occ))
        if what == "profile":
            continue
        used = cands["cand_query"] != NONE
        diag = cands["cand_hits"][:, 1].long() - cands["cand_begin"].long()
        near = used & (cands["cand_hits"][:, 0] == 0) & ((diag - origin.repeat_interleave(MAX_CANDIDATES)).abs() <= BAND + 3)
        row = {"text": text_name, "max_occ": max_occ, "equal_to_host_model": True,
               "smems_per_read": float(smems["n_smems"][:nq].float().mean()),
               "anchors_per_read": float((occ * (in_use & (occ <= max_occ))).sum().item() / nq),
               "reads_with_skipped_seeds": float((cands["n_skipped"][:nq] > 0).float().mean()),
               "groups_per_read": float(cands["n_groups"][:nq].float().mean()),
               "reads_cut_by_max_candidates": float((cands["n_groups"][:nq] > MAX_CANDIDATES).float().mean()),
               "slots_in_use": float(used.float().mean()),
               "origin_found": float(near.reshape(nq, MAX_CANDIDATES).any(dim=1).float().mean())}
        row["smems_ms"] = median_ms(lambda: eng.smems(dq, reng, MAX_SMEMS, MIN_LENGTH, smems))
        row["candidates_ms"] = median_ms(lambda: eng.seed_candidates(smems, nq, MAX_SMEMS, max_occ, BAND, MAX_CANDIDATES, out=cands))
        row["edit_ms"] = median_ms(lambda: eng.edit_distance(dq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], K,
                                                             e_dist, e_end))
        row["within_limit_of_used_slots"] = float(((e_dist >= 0) & (e_dist <= K))[used].float().mean())
        row["times_smems"] = row["candidates_ms"] / row["smems_ms"]
        row["times_edit_distance"] = row["candidates_ms"] / row["edit_ms"]
        row["reads_per_s"] = nq / row["candidates_ms"] * 1e3
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del cands, used, diag, near
    del index, companion, eng, reng, dq, origin, smems, e_dist, e_end, occ, in_use, io_text
    torch.cuda.empty_cache()

print(json.dumps(res))
if what == "report":
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "candidates.json"), "w") as f:
        f.write(json.dumps(res) + "\n")
    head = ("text", "max_occ", "SMEMs / read", "anchors / read", "reads with skipped seeds", "groups / read", "cut by max_candidates",
            "slots in use", "origin found", "smems", "candidates", "edit distance, all slots", "x smems", "x edit distance", "reads/s")
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in res["rows"]:
        lines.append("| %s | %d | %.2f | %.2f | %.3f | %.2f | %.3f | %.3f | %.4f | %.1f ms | %.1f ms | %.1f ms | %.2f | %.2f | %.0f M |" % (
            r["text"], r["max_occ"], r["smems_per_read"], r["anchors_per_read"], r["reads_with_skipped_seeds"], r["groups_per_read"],
            r["reads_cut_by_max_candidates"], r["slots_in_use"], r["origin_found"], r["smems_ms"], r["candidates_ms"], r["edit_ms"],
            r["times_smems"], r["times_edit_distance"], r["reads_per_s"] / 1e6))
    with open(os.path.join(out_dir, "candidates_table.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
