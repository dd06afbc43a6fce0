#!/usr/bin/env python3
"""gdx_edit_distance_many_dev: time, candidates per second and cell updates per second of the edit-distance verification,
against a VALU floor counted from the kernel's ISA and against gdx_hamming_many_dev on the same candidates.

Index: a synthetic A C G T text (GDX_EXP_TOTAL symbols, default 2^30) in the default shape.  Reads: GDX_EXP_NQ (default 10 M)
reads of 50, 150 and 250 symbols that follow the text from a random origin with 0..3 edits at offsets in [5, L - 5), each a
substitution, an inserted symbol or a skipped text symbol, made on the device.  Candidates: GDX_EXP_CANDIDATES (default 10 M);
candidate c belongs to read c mod nq; an even c names the read's true origin through a seed that begins in the read's first
five symbols, an odd c a random position of the text.  For plain + offsets and packed + uniform batches and max_edits 2 and 8:
  time        median of GDX_EXP_REPS (default 7) runs after two warm-up runs, events on the stream
  cells       L x window columns per candidate (counted from the candidates), per second
  VALU floor  block steps (ceil(L / 64) per column; 4 slots per column of which ceil(L / 64) run in the offsets instance) x the
              VALU instructions of one column of that instance / its blocks, counted from the ISA given in GDX_EXP_ISA (the
              .s of edit_distance.hip: hipcc -S --cuda-device-only), over 256 CUs x 4 SIMDs at one wave64 VALU instruction per
              2 cycles and GDX_EXP_CLOCK_HZ (default 2.4e9).  Without GDX_EXP_ISA the floor is left out.
  hamming     the time of gdx_hamming_many_dev with max_mismatches = max_edits on the same candidates
Before anything is timed the first 2^16 results are compared with a torch restatement of the column recurrence batched over
candidates, and the two layouts with each other on all candidates.
usage: python tools/exp_edit_distance.py [report | profile]   -> JSON lines on stderr, one JSON result line on stdout
(profile: a few calls only, for rocprofv3 --kernel-trace --stats)"""
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from genedex_amd import _lib, alphabet  # noqa: E402
from genedex_amd.device import DeviceEngine, DeviceQueries, build_index_from_device_text, synth_text  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "report"
total = int(os.environ.get("GDX_EXP_TOTAL", 1 << 30))
nq = int(os.environ.get("GDX_EXP_NQ", 10_000_000))
reps = int(os.environ.get("GDX_EXP_REPS", 7))
m = int(os.environ.get("GDX_EXP_CANDIDATES", 10_000_000))
lengths = [int(x) for x in os.environ.get("GDX_EXP_LENGTHS", "50,150,250").split(",")]
clock_hz = float(os.environ.get("GDX_EXP_CLOCK_HZ", 2.4e9))
VALU_PER_S = 256 * 4 * clock_hz / 2  # wave64 VALU instructions per second of the whole device
NO_END = -1
dev = torch.device("cuda", 0)
torch.manual_seed(7)
lib = _lib.load()
a = alphabet.ascii_dna()


def column_loop_valu(isa_text):
    """{(xlate, uniform, W): VALU instructions in the column loop (the loop at depth 2) of that instance of edit_kernel}"""
    out = {}
    for f in re.finditer(r"^_ZN3gdx\S*edit_kernelILi(\d)ELb(\d)ELi(\d)E\S*:.*?^\.Lfunc_end", isa_text, flags=re.S | re.M):
        inside, n = False, 0
        for line in f.group(0).split("\n"):
            if re.match(r"\.LBB\d+_\d+:", line):
                inside = "Depth=2" in line
                continue
            t = line.strip()
            if t.startswith(";"):
                inside = inside or "Loop Header: Depth=2" in t
            elif inside and t.startswith("v_"):
                n += 1
        out[(int(f.group(1)), bool(int(f.group(2))), int(f.group(3)))] = n
    return out


isa = os.environ.get("GDX_EXP_ISA")
valu = column_loop_valu(open(isa).read()) if isa else {}
io_text = synth_text(total, seed=42, n_per_million=0, device=dev)
t0 = time.time()
index = build_index_from_device_text(io_text, [total], a, index_storage="u32")
eng = DeviceEngine(index)
res = {"total_symbols": total, "reads": nq, "candidates": m, "reps": reps, "build_s": time.time() - t0, "aux": eng.aux_info(),
       "valu_per_s": VALU_PER_S, "valu_per_column": {f"{k[0]},{int(k[1])},{k[2]}": v for k, v in valu.items()}, "rows": []}
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


def model(q, t, width, x0, k):
    """the column recurrence batched over candidates.  q: [n, L] read bytes; t: [n, w] window bytes (anything behind the
    candidate's own `width`); x0: [n] -> (min(dist, k + 1), smallest end or NO_END).  A C G T only: equal bytes match."""
    n, L = q.shape
    idx = torch.arange(L + 1, device=dev, dtype=torch.int32)
    col = idx.repeat(n, 1)
    best = torch.full((n,), L, dtype=torch.int32, device=dev)
    end = x0.to(torch.int32).clone()
    tmp = torch.zeros_like(col)
    for j in range(t.shape[1]):
        active = j < width
        mismatch = (q != t[:, j:j + 1]).to(torch.int32)
        tmp[:, 1:] = torch.minimum(col[:, :-1] + mismatch, col[:, 1:] + 1)
        new = torch.cummin(tmp - idx, dim=1).values + idx
        col = torch.where(active[:, None], new, col)
        better = active & (col[:, L] < best)
        best = torch.where(better, col[:, L], best)
        end = torch.where(better, (x0 + j + 1).to(torch.int32), end)
    within = best <= k
    return torch.where(within, best, torch.full_like(best, k + 1)), torch.where(within, end, torch.full_like(end, NO_END))


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
    start = torch.where(c % 2 == 0, origin[cq.long()], torch.randint(0, total - L, (m,), device=dev))
    hits = torch.stack([torch.zeros_like(start), start + begin], dim=1).to(torch.int32).contiguous()  # (positions < 2^31 here)
    cb = begin.to(torch.int32)
    del c, begin
    dist = {name: torch.empty(m, dtype=torch.int32, device=dev) for name in forms}
    end = {name: torch.empty(m, dtype=torch.int32, device=dev) for name in forms}
    ham = torch.empty(m, dtype=torch.int32, device=dev)
    W = (L + 63) // 64
    for k in (2, 8):
        for name, dq in forms.items():
            dist[name].fill_(-7)
            end[name].fill_(-7)
            eng.edit_distance(dq, cq, cb, hits, k, dist[name], end[name])
        torch.cuda.synchronize()
        if not (torch.equal(dist["plain+offsets"], dist["packed+uniform"]) and torch.equal(end["plain+offsets"], end["packed+uniform"])):
            raise SystemExit(f"PARITY FAILURE: the two layouts differ (L {L}, max_edits {k})")
        n = min(m, 1 << 16)
        x0 = (start[:n] - k).clamp(0, total)
        x1 = (start[:n] + L + k).clamp(0, total)
        window = io_text[(x0[:, None] + torch.arange(L + 2 * k, device=dev)[None, :]).clamp(max=total - 1).reshape(-1)].reshape(n, -1)
        want_dist, want_end = model(qmat[cq[:n].long()], window, x1 - x0, x0, k)
        if not (torch.equal(dist["plain+offsets"][:n], want_dist) and torch.equal(end["plain+offsets"][:n], want_end)):
            raise SystemExit(f"PARITY FAILURE: the call and the torch model differ (L {L}, max_edits {k})")
        within = float((dist["plain+offsets"] <= k).float().mean())
        columns = ((start + L + k).clamp(0, total) - (start - k).clamp(0, total)).double().mean().item()
        if what == "profile":
            continue
        for name, dq in forms.items():
            ms = median_ms(lambda: eng.edit_distance(dq, cq, cb, hits, k, dist[name], end[name]))
            ham_ms = median_ms(lambda: eng.hamming(dq, cq, cb, hits, k, ham))
            per_column = valu.get((2, True, W) if name == "packed+uniform" else (1, False, 4))
            # the offsets instance walks four block slots per column and runs ceil(L / 64) of them: its count per column is
            # scaled to the blocks that run
            floor_valu = None if per_column is None else columns * per_column * (1.0 if name == "packed+uniform" else W / 4) * m / 64
            row = {"read_length": L, "candidates": m, "layout": name, "max_edits": k, "ms": ms,
                   "candidates_per_s": m / ms * 1e3, "columns_per_candidate": columns, "blocks": W,
                   "cell_updates_per_s": L * columns * m / ms * 1e3,
                   "valu_per_column": per_column, "valu_per_block_step": None if per_column is None else per_column / (W if name == "packed+uniform" else 4),
                   "valu_floor_ms": None if floor_valu is None else floor_valu / VALU_PER_S * 1e3,
                   "share_of_valu_floor": None if floor_valu is None else floor_valu / VALU_PER_S * 1e3 / ms,
                   "hamming_ms": ham_ms, "times_hamming": ms / ham_ms,
                   "candidates_within_limit": within, "equal_to_model": True}
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    del cq, cb, hits, start, dist, end, ham, qmat, qbuf, plain, forms, origin
print(json.dumps(res))
