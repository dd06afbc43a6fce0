#!/usr/bin/env python3
"""gdx_align_many_dev: time and candidates per second of the alignment traceback for two workspace sizes, and its ratio to
gdx_edit_distance_many_dev (the same forward pass without history and walk) on the same candidates.

Index: a synthetic A C G T text (GDX_EXP_TOTAL symbols, default 2^30) in the default shape.  Reads: GDX_EXP_NQ (default 10 M)
reads of 50, 150 and 250 symbols that follow the text from a random origin with 0..3 edits at offsets in [5, L - 5), each a
substitution, an inserted symbol or a skipped text symbol, made on the device (the workload of tools/exp_edit_distance.py).
Candidates: GDX_EXP_CANDIDATES (default 10 M); candidate c belongs to read c mod nq and names the read's TRUE origin through a
seed that begins in the read's first five symbols: traceback is what this call is for.  For plain + offsets and packed + uniform
batches and max_edits 2 and 8:
  time        median of GDX_EXP_REPS (default 7) runs after two warm-up runs, events on the stream, with a workspace of the best
              size ([1] of the size query) and of a quarter of it
  edit        the time of gdx_edit_distance_many_dev on the same candidates, and the ratio
Before anything is timed, dist and end are held equal to gdx_edit_distance_many_dev on every candidate, the two layouts and the
two workspace sizes are compared on all five outputs, and the first 2^16 alignments are replayed on the host: the runs consume
exactly the read and text[begin, end), '=' sits on equal and 'X' on unequal symbols, the ops other than '=' number dist, adjacent
runs differ and there are at most 2 dist + 1 of them.
usage: python tools/exp_align.py [report | profile]   -> JSON lines on stderr, one JSON result line on stdout
(profile: a few calls only, for rocprofv3 --kernel-trace --stats, or for a --pmc run of its own)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from genedex_amd import alphabet  # noqa: E402
from genedex_amd.device import DeviceEngine, DeviceQueries, build_index_from_device_text, synth_text  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "report"
total = int(os.environ.get("GDX_EXP_TOTAL", 1 << 30))
nq = int(os.environ.get("GDX_EXP_NQ", 10_000_000))
reps = int(os.environ.get("GDX_EXP_REPS", 7))
m = int(os.environ.get("GDX_EXP_CANDIDATES", 10_000_000))
lengths = [int(x) for x in os.environ.get("GDX_EXP_LENGTHS", "50,150,250").split(",")]
NO_END = -1
NAMES = ("dist", "begin", "end", "n_cigar", "cigar")
dev = torch.device("cuda", 0)
torch.manual_seed(7)
a = alphabet.ascii_dna()

io_text = synth_text(total, seed=42, n_per_million=0, device=dev)
t0 = time.time()
index = build_index_from_device_text(io_text, [total], a, index_storage="u32")
eng = DeviceEngine(index)
res = {"total_symbols": total, "reads": nq, "candidates": m, "reps": reps, "build_s": time.time() - t0, "aux": eng.aux_info(),
       "rows": []}
print(json.dumps(res), file=sys.stderr, flush=True)
acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)


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


def replay(q, window, x0, out):
    """the first rows of a result replayed on the host.  q: [n, L] read bytes, window: [n, w] text bytes from x0[i] on"""
    dist, begin, end, n_cigar, cigar = out
    for i in range(q.shape[0]):
        if end[i] == NO_END:
            assert begin[i] == NO_END and n_cigar[i] == 0, i
            continue
        r, y, cost, last = 0, int(begin[i] - x0[i]), 0, 0
        for w in cigar[i, :n_cigar[i]]:
            n, op = int(w) >> 4, int(w) & 15
            assert n > 0 and op != last and op in (1, 2, 7, 8), (i, n, op)
            if op in (7, 8):
                same = q[i, r:r + n] == window[i, y:y + n]
                assert same.size == n and (same.all() if op == 7 else not same.any()), (i, r, y, n, op)
                r, y = r + n, y + n
            elif op == 1:
                r += n
            else:
                y += n
            cost += n if op != 7 else 0
            last = op
        assert r == q.shape[1] and y == int(end[i] - x0[i]) and cost == dist[i] and n_cigar[i] <= 2 * dist[i] + 1, i


for L in lengths:
    # the reads and where they come from: read symbol j is text symbol origin + j + (skips in front of or at j) - (insertions
    # in front of j), then the inserted and substituted symbols are overwritten
    origin = torch.randint(0, total - L - 8, (nq,), device=dev)
    qmat = torch.empty((nq, L), dtype=torch.uint8, device=dev)
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
        qmat[lo:hi] = block
    qbuf = torch.zeros(nq * L + 8, dtype=torch.uint8, device=dev)
    qbuf[: nq * L] = qmat.reshape(-1)
    plain = DeviceQueries(qbuf, torch.arange(0, nq + 1, dtype=torch.int64, device=dev) * L, nq, nq * L)
    forms = {"plain+offsets": plain, "packed+uniform": plain.as_uniform(L).as_packed(index)}
    c = torch.arange(m, device=dev)
    cq = (c % nq).to(torch.int32)
    begin = torch.randint(0, 5, (m,), device=dev)
    start = origin[cq.long()]
    hits = torch.stack([torch.zeros_like(start), start + begin], dim=1).to(torch.int32).contiguous()  # (positions < 2^31 here)
    cb = begin.to(torch.int32)
    del c, begin
    e_dist = torch.empty(m, dtype=torch.int32, device=dev)
    e_end = torch.empty(m, dtype=torch.int32, device=dev)
    for k in (2, 8):
        outs, sizes = {}, {}
        for name, dq in forms.items():
            least, best = eng.align_workspace_bytes(dq, m, k)
            quarter = max(least, best // 4 // least * least)
            sizes[name] = {"least": least, "best": best, "quarter": quarter}
            for tag, size in (("best", best), ("quarter", quarter)):
                out = {x: torch.full((m,), -7, dtype=torch.int32, device=dev) for x in NAMES[:4]}
                out["cigar"] = torch.zeros((m, 2 * k + 1), dtype=torch.int32, device=dev)  # zero: words from n_cigar on stay so
                ws = torch.empty(size, dtype=torch.uint8, device=dev)
                eng.align(dq, cq, cb, hits, k, out=out, workspace=ws)
                outs[name, tag] = (out, ws)
            eng.edit_distance(dq, cq, cb, hits, k, e_dist, e_end)
            torch.cuda.synchronize()
            if not (torch.equal(outs[name, "best"][0]["dist"], e_dist) and torch.equal(outs[name, "best"][0]["end"], e_end)):
                raise SystemExit(f"PARITY FAILURE: dist / end differ from gdx_edit_distance_many_dev ({name}, L {L}, max_edits {k})")
        first = outs["plain+offsets", "best"][0]
        for key, (out, _) in outs.items():
            if not all(torch.equal(out[x], first[x]) for x in NAMES):
                raise SystemExit(f"PARITY FAILURE: {key} differs from plain+offsets with the best workspace (L {L}, max_edits {k})")
        n = min(m, 1 << 16)
        x0 = (start[:n] - k).clamp(0, total)
        window = io_text[(x0[:, None] + torch.arange(L + 2 * k, device=dev)[None, :]).clamp(max=total - 1).reshape(-1)].reshape(n, -1)
        replay(qmat[cq[:n].long()].cpu().numpy(), window.cpu().numpy(), x0.cpu().numpy(), [first[x][:n].cpu().numpy() for x in NAMES])
        within = float((first["dist"] <= k).float().mean())
        runs = float(first["n_cigar"].float().mean())
        with_indel = float((((first["cigar"] & 15) == 1) | ((first["cigar"] & 15) == 2)).any(dim=1).float().mean())
        columns = ((start + L + k).clamp(0, total) - (start - k).clamp(0, total)).double().mean().item()
        if what == "profile":
            continue
        for name, dq in forms.items():
            edit_ms = median_ms(lambda: eng.edit_distance(dq, cq, cb, hits, k, e_dist, e_end))
            row = {"read_length": L, "candidates": m, "layout": name, "max_edits": k, "blocks": (L + 63) // 64,
                   "columns_per_candidate": columns, "workspace_bytes": sizes[name], "edit_distance_ms": edit_ms,
                   "candidates_within_limit": within, "runs_per_candidate": runs, "candidates_with_indel": with_indel,
                   "equal_to_edit_distance": True, "replayed": n}
            for tag in ("best", "quarter"):
                out, ws = outs[name, tag]
                ms = median_ms(lambda: eng.align(dq, cq, cb, hits, k, out=out, workspace=ws))
                row[f"ms_{tag}"] = ms
                row[f"candidates_per_s_{tag}"] = m / ms * 1e3
                row[f"times_edit_distance_{tag}"] = ms / edit_ms
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        del outs, first
    del cq, cb, hits, start, e_dist, e_end, qmat, qbuf, plain, forms, origin
print(json.dumps(res))
