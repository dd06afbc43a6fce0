#!/usr/bin/env python3
"""gdx_hamming_many_dev: time, candidates per second and achieved bytes per second of the Hamming verification against its
byte floor and against the random-gather ceiling of the device (0.72 of the 8 TB/s HBM peak, DESIGN.md: the locate walk).

Index: a synthetic A C G T text (GDX_EXP_TOTAL symbols, default 2^30) in the default shape.  Reads: GDX_EXP_NQ (default 10 M)
reads of 50 and of 150 symbols sampled from the text on the device with 0..3 substitutions.  Candidates: 10 M and 100 M;
candidate c belongs to read c mod nq; an even c names the read's true origin through a seed that begins somewhere in the
read, an odd c a random position of the text.  For plain + offsets and packed + uniform batches and max_mismatches 2 and L:
  time       median of GDX_EXP_REPS (default 7) runs after two warm-up runs, events on the stream
  floor      per candidate the 128-byte lines its text window touches (counted from the candidates, 256 symbols per line),
             plus the read's bytes in that layout (L + 8 plain with offsets, L / 4 packed + uniform), plus 12 bytes of
             candidate and 4 of result
  achieved   floor bytes / time, beside the gather ceiling
Before anything is timed the first million results are compared with a torch model (text gather + compare), and the two
layouts with each other on all candidates.
usage: python tools/exp_hamming.py [report | profile]   -> JSON lines on stderr, one JSON result line on stdout
(profile: a few calls only, for rocprofv3 --kernel-trace --stats)"""
import json
import os
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
sizes = [int(x) for x in os.environ.get("GDX_EXP_CANDIDATES", "10000000,100000000").split(",")]
HBM_PEAK, GATHER_SHARE = 8.0e12, 0.72
dev = torch.device("cuda", 0)
torch.manual_seed(7)
lib = _lib.load()
a = alphabet.ascii_dna()
io_text = synth_text(total, seed=42, n_per_million=0, device=dev)
t0 = time.time()
index = build_index_from_device_text(io_text, [total], a, index_storage="u32")
eng = DeviceEngine(index)
res = {"total_symbols": total, "reads": nq, "reps": reps, "build_s": time.time() - t0, "aux": eng.aux_info(),
       "gather_ceiling_Bps": HBM_PEAK * GATHER_SHARE, "rows": []}
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


for L in (50, 150):
    # the reads and where they come from
    origin = torch.randint(0, total - L, (nq,), device=dev)
    qmat = torch.empty((nq, L), dtype=torch.uint8, device=dev)
    ar = torch.arange(L, device=dev)
    for lo in range(0, nq, 1 << 20):
        hi = min(nq, lo + (1 << 20))
        block = io_text[(origin[lo:hi, None] + ar[None, :]).reshape(-1)].reshape(hi - lo, L)
        for _ in range(3):  # up to three substitutions (a draw may repeat the symbol or the place)
            hit = torch.rand(hi - lo, device=dev) < 0.5
            at = torch.randint(0, L, (hi - lo,), device=dev)
            rows = torch.nonzero(hit).reshape(-1)
            block[rows, at[rows]] = acgt[torch.randint(0, 4, (rows.numel(),), device=dev)]
        qmat[lo:hi] = block
    qbuf = torch.zeros(nq * L + 8, dtype=torch.uint8, device=dev)
    qbuf[: nq * L] = qmat.reshape(-1)
    plain = DeviceQueries(qbuf, torch.arange(0, nq + 1, dtype=torch.int64, device=dev) * L, nq, nq * L)
    forms = {"plain+offsets": plain, "packed+uniform": plain.as_uniform(L).as_packed(index)}
    for m in sizes:
        c = torch.arange(m, device=dev)
        cq = (c % nq).to(torch.int32)
        begin = torch.randint(0, L - 11, (m,), device=dev)
        start = torch.where(c % 2 == 0, origin[cq.long()], torch.randint(0, total - L, (m,), device=dev))
        hits = torch.stack([torch.zeros_like(start), start + begin], dim=1).to(torch.int32).contiguous()  # (positions < 2^31 here)
        cb = begin.to(torch.int32)
        lines = ((start + L - 1) // 256 - start // 256 + 1).double().mean().item()
        del c, begin
        out = {name: torch.empty(m, dtype=torch.int32, device=dev) for name in forms}
        for k in (2, L):
            for name, dq in forms.items():
                out[name].fill_(-7)
                eng.hamming(dq, cq, cb, hits, k, out[name])
            torch.cuda.synchronize()
            if not torch.equal(out["plain+offsets"], out["packed+uniform"]):
                raise SystemExit(f"PARITY FAILURE: the two layouts differ (L {L}, m {m}, max_mismatches {k})")
            n = min(m, 1 << 20)
            want = (qmat[cq[:n].long()] != io_text[(start[:n, None] + ar[None, :]).reshape(-1)].reshape(n, L)).sum(1).clamp(max=k + 1)
            if not torch.equal(out["plain+offsets"][:n].long(), want):
                raise SystemExit(f"PARITY FAILURE: the call and the torch model differ (L {L}, m {m}, max_mismatches {k})")
            within = float((out["plain+offsets"] <= k).float().mean())
            if what == "profile":
                continue
            for name, dq in forms.items():
                read_bytes = L + 8 if name == "plain+offsets" else L / 4
                floor_bytes = (128 * lines + read_bytes + 12 + 4) * m
                ms = median_ms(lambda: eng.hamming(dq, cq, cb, hits, k, out[name]))
                row = {"read_length": L, "candidates": m, "layout": name, "max_mismatches": k, "ms": ms,
                       "candidates_per_s": m / ms * 1e3, "lines_per_candidate": lines,
                       "floor_bytes_per_candidate": floor_bytes / m, "achieved_Bps": floor_bytes / ms * 1e3,
                       "share_of_gather_ceiling": floor_bytes / ms * 1e3 / (HBM_PEAK * GATHER_SHARE),
                       "floor_ms_at_gather_ceiling": floor_bytes / (HBM_PEAK * GATHER_SHARE) * 1e3,
                       "candidates_within_limit": within, "equal_to_model": True}
                res["rows"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
        del cq, cb, hits, start, out
    del qmat, qbuf, plain, forms, origin
print(json.dumps(res))
