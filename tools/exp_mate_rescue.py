#!/usr/bin/env python3
"""gdx_mate_rescue_many_dev behind gdx_pair_hits_many_dev on the resident chain over read pairs: how many pairs it adds to the
proper ones, where the rescued mates land, the time of the call beside the edit-distance and the pairing call of the same run,
and how full the rounds of its Myers lanes are.

The workload of tools/exp_pair_hits.py (profiles/r17): a synthetic A C G T text (GDX_EXP_TOTAL symbols, default 2^30) and its
genome-like variant, each with the default-shape index and the companion over the reversed text; GDX_EXP_NQ (default 10 M) reads of
150 symbols with 0..3 edits made on the device, reads 2p and 2p + 1 the mates of pair p: a fragment of 300 .. 600 symbols (uniform)
at a random place, one mate its first 150 symbols, the other the reverse complement of its last 150, the forward mate first in even
pairs and second in odd ones.  with_strands("both") in front; max_smems 16, min_length 19, band 8, max_candidates 4, max_occ 8,
max_edits = band + 3 = 11, mate_slots = 2 * max_candidates = 8, insert bounds [250, 650].  Per text:
  proper_before      the share of pairs with n_proper >= 1; proper_or_rescued those and the pairs with resc_mate != GDX_RESCUE_NONE
  attempts           the share of mates with an attempt; found the share OF THOSE with resc_dist <= max_edits
  rescued_near_origin  the share of rescued mates whose resc_end lies within max_edits of where the read's forward form ends
                     (right text, right strand), and what stands behind it: anchor_at_origin, the share of rescued mates whose
                     ANCHOR lies on its own strand within band + 3 diagonals of where it was taken; near_given_anchor, the share near
                     their origin among those; left_of_origin, the share of rescued mates that end more than max_edits LEFT of their
                     origin (the smallest admissible end of the least distance wins); end_offset, the quantiles 5, 25, 50, 75 and 95
                     of resc_end - the origin's end over the rescued mates with their anchor at its origin
  rescue_ms          gdx_mate_rescue_many_dev; edit_ms gdx_edit_distance_many_dev over all slots; pair_ms gdx_pair_hits_many_dev:
                     medians of GDX_EXP_REPS (default 7) calls after two warm-up calls, events on the stream
  lane_occupancy     attempts / (rounds * 256), the rounds counted on the host from the flags with the launcher's default tile
                     (ceil(n_pairs / 1024) pairs, at least 2048, rounded up to 256: a tile runs ceil(its attempts / 256) rounds);
                     lane_per_mate_occupancy: attempts / (64 * the wavefronts of 64 consecutive mates that hold an attempt)
Before anything is timed the outputs of the first GDX_EXP_CHECK (default 2^16) pairs are held equal to a host model (numpy, from
the definition of include/gdx_experimental.h).
usage: python tools/exp_mate_rescue.py [report | profile]   -> JSON lines on stderr, one JSON result line on stdout; report also
writes mate_rescue.json into GDX_EXP_OUT (default profiles/r22).  profile: a few calls
only, for rocprofv3 --kernel-trace --stats"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from genedex_amd import alphabet  # noqa: E402
from genedex_amd.device import (DeviceEngine, DeviceQueries, build_index_from_device_text, genome_like_text,  # noqa: E402
                                synth_text)
from genedex_amd.index import build_options  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "report"
total = int(os.environ.get("GDX_EXP_TOTAL", 1 << 30))
nq = int(os.environ.get("GDX_EXP_NQ", 10_000_000)) & ~1
reps = int(os.environ.get("GDX_EXP_REPS", 7))
n_pairs = nq // 2
n_check = min(n_pairs, int(os.environ.get("GDX_EXP_CHECK", 1 << 16)))
text_names = os.environ.get("GDX_EXP_TEXTS", "synthetic,genome-like").split(",")
out_dir = os.environ.get("GDX_EXP_OUT", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r22"))
L, MAX_SMEMS, MIN_LENGTH, BAND, MAX_CANDIDATES, MAX_OCC = 150, 16, 19, 8, 4, 8
K, MS = BAND + 3, 2 * MAX_CANDIDATES
FRAGMENT, MIN_INSERT, MAX_INSERT = (300, 600), 250, 650
NONE, NOT_TRIED, NO_END = 0xFFFFFFFF, 0xFFFFFFFD, 0xFFFFFFFF
BLOCK, MAX_GRID, MIN_TILE = 256, 1024, 2048          # copies of mate_rescue.hip's kBlock, kMaxGrid and kMinTile: keep them equal
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
    """tools/exp_pair_hits.py's: (the batch with the mates interleaved, origin[nq]: where the forward form of a read was taken,
    reverse[nq]: its strand)"""
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


def host_model(io_text, sq, end, pairs, n):
    """the output arrays of the first n pairs, from the definition (one text, every read L symbols long)"""
    u32 = lambda t, m: t[:m].cpu().numpy().view(np.uint32).astype(np.int64)  # noqa: E731
    n_proper = u32(pairs["n_proper"], n)
    slot, md, wq, wb = (u32(pairs[name], 2 * n) for name in ("mate_slot", "mate_dist", "win_query", "win_begin"))
    hits = u32(pairs["win_hits"], 2 * n)
    wt, wp = hits[:, 0], hits[:, 1]
    e = u32(end, 2 * n * MS).reshape(2 * n, MS)
    mate = np.arange(2 * n)
    swap = mate ^ 1
    tried = (np.repeat(n_proper, 2) == 0) & (slot[swap] != NONE)
    strand_a, diag_a = wq[swap] & 1, wp[swap] - wb[swap]
    right_a = e[swap, np.where(slot[swap] == NONE, 0, slot[swap])]
    rq = 4 * (mate >> 1) + 2 * (mate & 1) + (1 - strand_a)
    ylo = np.where(strand_a == 0, diag_a + MIN_INSERT, right_a - MAX_INSERT + L)
    yhi = np.where(strand_a == 0, diag_a + MAX_INSERT, right_a - MIN_INSERT + L)
    x0, x1 = np.clip(ylo - L - K, 0, total), np.clip(yhi, 0, total)
    dense = np.asarray(a.io_to_dense_table, dtype=np.uint8)
    resc_dist, resc_end = np.where(tried, K + 1, NOT_TRIED), np.full(2 * n, NO_END)
    todo = np.flatnonzero(tried)
    assert (wt[swap][todo] == 0).all()
    width_max = MAX_INSERT - MIN_INSERT + L + K
    idx = np.arange(L + 1)
    for lo in range(0, todo.size, 2048):
        m = todo[lo:lo + 2048]
        r = m.size
        reads = sq.qbuf[(torch.from_numpy(rq[m] * L).to(dev)[:, None] + torch.arange(L, device=dev)[None, :]).reshape(-1)]
        Q = dense[reads.cpu().numpy()].astype(np.int64).reshape(r, L)
        cols = torch.from_numpy(x0[m]).to(dev)[:, None] + torch.arange(width_max, device=dev)[None, :]
        W = dense[io_text[cols.clamp(max=total - 1).reshape(-1)].cpu().numpy()].astype(np.int64).reshape(r, width_max)
        searchable = (Q >= 1) & (Q <= 4)
        col = np.broadcast_to(idx, (r, L + 1)).copy()
        last = np.zeros((r, width_max + 1), dtype=np.int64)
        last[:, 0] = L
        tmp = np.zeros_like(col)
        for j in range(width_max):
            mismatch = 1 - (searchable & (Q == W[:, j:j + 1]))
            tmp[:, 1:] = np.minimum(col[:, :-1] + mismatch, col[:, 1:] + 1)
            tmp[:, 0] = 0
            col = np.minimum.accumulate(tmp - idx, axis=1) + idx
            last[:, j + 1] = col[:, L]
        y = x0[m][:, None] + np.arange(width_max + 1)[None, :]
        ok = (y <= x1[m][:, None]) & (y >= ylo[m][:, None]) & (y <= yhi[m][:, None])
        last = np.where(ok, last, 1 << 30)
        best, best_j = last.min(axis=1), last.argmin(axis=1)
        resc_dist[m] = np.where(best <= K, best, K + 1)
        resc_end[m] = np.where(best <= K, x0[m] + best_j, NO_END)
    success = resc_dist <= K
    score = np.where(success, md[swap] + resc_dist, 1 << 40).reshape(n, 2)
    pick = np.where(score[:, 1] < score[:, 0], 1, 0)
    any_ = success.reshape(n, 2).any(axis=1)
    at = 2 * np.arange(n) + pick
    yy = resc_end[at]
    span = np.where(strand_a[at] == 0, yy - diag_a[at], right_a[at] - (yy - L))
    out_q, out_b, out_t, out_p = wq.copy(), wb.copy(), wt.copy(), wp.copy()
    r = at[any_]
    out_q[r], out_b[r], out_t[r], out_p[r] = rq[r], np.maximum(0, L - yy)[any_], wt[swap][r], np.maximum(0, yy - L)[any_]
    return {"resc_dist": resc_dist, "resc_end": resc_end, "resc_mate": np.where(any_, pick, NONE),
            "resc_pair_dist": np.where(any_, score[np.arange(n), pick], 2 * K + 2), "resc_span": np.where(any_, span, 0),
            "win_query": out_q, "win_begin": out_b, "win_text": out_t, "win_position": out_p}


def check_against_model(io_text, sq, end, pairs, resc, where):
    want = host_model(io_text, sq, end, pairs, n_check)
    u32 = lambda t, n: t[:n].cpu().numpy().view(np.uint32).astype(np.int64)  # noqa: E731
    got = {name: u32(resc[name], n_check) for name in ("resc_mate", "resc_pair_dist", "resc_span")}
    got.update({name: u32(resc[name], 2 * n_check) for name in ("resc_dist", "resc_end", "win_query", "win_begin")})
    hits = u32(resc["win_hits"], 2 * n_check)
    got["win_text"], got["win_position"] = hits[:, 0], hits[:, 1]
    for name, w in want.items():
        if not np.array_equal(got[name], w):
            bad = int(np.flatnonzero(got[name] != w)[0])
            raise SystemExit(f"PARITY FAILURE: {name} differs from the host model at {bad}: {int(got[name][bad])} != {int(w[bad])} "
                             f"({where})")


def occupancy(tried):
    """(attempts / (rounds * 256) with the launcher's default tile, attempts / (64 * wavefronts of a lane-per-mate grid at work))"""
    tile = max((n_pairs + MAX_GRID - 1) // MAX_GRID, MIN_TILE)
    tile = (tile + BLOCK - 1) // BLOCK * BLOCK
    t = tried[:2 * n_pairs].long()
    pad = (-t.numel()) % (2 * tile)
    per_tile = torch.nn.functional.pad(t, (0, pad)).reshape(-1, 2 * tile).sum(dim=1)
    rounds = int(((per_tile + BLOCK - 1) // BLOCK).sum())
    waves = int((torch.nn.functional.pad(t, (0, (-t.numel()) % 64)).reshape(-1, 64).sum(dim=1) > 0).sum())
    attempts = int(t.sum())
    return tile, rounds, attempts / max(rounds * BLOCK, 1), attempts / max(64 * waves, 1)


for text_name in text_names:
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
    dist, end = eng.edit_distance(sq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], K)
    pairs, resc = eng.alloc_pair_hits(n_pairs), eng.alloc_mate_rescue(n_pairs)
    for t in list(pairs.values()) + list(resc.values()):
        t.fill_(0x55)
    eng.pair_hits(cands, dist, end, n_pairs, MS, K, MIN_INSERT, MAX_INSERT, out=pairs)
    eng.mate_rescue(sq, end, pairs, n_pairs, MS, K, MIN_INSERT, MAX_INSERT, out=resc)
    torch.cuda.synchronize()
    check_against_model(io_text, sq, end, pairs, resc, text_name)
    if what == "profile":
        continue
    proper = pairs["n_proper"][:n_pairs] >= 1
    rescued_pair = resc["resc_mate"][:n_pairs] != -1
    tried = resc["resc_dist"][:nq] != -3                                          # GDX_RESCUE_NOT_TRIED
    found = tried & (resc["resc_dist"][:nq] >= 0) & (resc["resc_dist"][:nq] <= K)
    mate = torch.arange(nq, device=dev)
    rescued_mate = rescued_pair.repeat_interleave(2) & (resc["resc_mate"][:n_pairs].repeat_interleave(2) == (mate & 1))
    near = ((resc["resc_end"][:nq].long() - (origin + L)).abs() <= K) & (resc["win_hits"][:nq, 0] == 0) & \
        ((resc["win_query"][:nq] & 1).bool() == reverse)
    offset = resc["resc_end"][:nq].long() - (origin + L)
    a_diag = pairs["win_hits"][:nq, 1].long() - pairs["win_begin"][:nq].long()
    a_ok = (pairs["win_query"][:nq] != -1) & (pairs["win_hits"][:nq, 0] == 0) & ((pairs["win_query"][:nq] & 1).bool() == reverse) & \
        ((a_diag - origin).abs() <= BAND + 3)
    anchor_ok = a_ok[mate ^ 1] & rescued_mate                                     # the rescued mate's anchor is the other mate
    share = lambda x, of: float(x.float().sum() / of.float().sum().clamp(min=1))  # noqa: E731
    q = torch.tensor([0.05, 0.25, 0.5, 0.75, 0.95], device=dev)
    end_offset = torch.quantile(offset[anchor_ok].float(), q).tolist() if bool(anchor_ok.any()) else []
    tile, rounds, occ, occ_mate = occupancy(tried)
    row = {"text": text_name, "equal_to_host_model": True, "proper_before": float(proper.float().mean()),
           "proper_or_rescued": float((proper | rescued_pair).float().mean()), "rescued_pairs": float(rescued_pair.float().mean()),
           "attempts": float(tried.float().mean()), "found": float(found.float().sum() / tried.float().sum().clamp(min=1)),
           "rescued_near_origin": float((rescued_mate & near).float().sum() / rescued_mate.float().sum().clamp(min=1)),
           "anchor_at_origin": share(anchor_ok, rescued_mate), "near_given_anchor": share(anchor_ok & near, anchor_ok),
           "left_of_origin": share(rescued_mate & (offset < -K), rescued_mate), "end_offset": end_offset,
           "tile_pairs": tile, "rounds": rounds, "lane_occupancy": occ, "lane_per_mate_occupancy": occ_mate}
    row["edit_ms"] = median_ms(lambda: eng.edit_distance(sq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], K,
                                                         out_dist=dist, out_end=end))
    row["pair_ms"] = median_ms(lambda: eng.pair_hits(cands, dist, end, n_pairs, MS, K, MIN_INSERT, MAX_INSERT, out=pairs))
    row["rescue_ms"] = median_ms(lambda: eng.mate_rescue(sq, end, pairs, n_pairs, MS, K, MIN_INSERT, MAX_INSERT, out=resc))
    res["rows"].append(row)
    print(json.dumps(row), file=sys.stderr, flush=True)
    del index, companion, eng, reng, dq, sq, origin, reverse, cands, dist, end, pairs, resc, io_text
    torch.cuda.empty_cache()

print(json.dumps(res))
if what == "report":
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "mate_rescue.json"), "w") as f:
        f.write(json.dumps(res) + "\n")
