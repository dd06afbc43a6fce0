#!/usr/bin/env python3
"""gdx_smems_many_dev against its emulation with the calls that existed before it, and its own rates.

Indexes: a synthetic A C G T text (GDX_EXP_TOTAL symbols, default 2^30) in the default shape, and the companion over the
reversed text with the build options include/gdx.h recommends (occurrence table, pair lines, top table).  Reads:
GDX_EXP_NQ (default 10 M) reads of 100 symbols sampled from the text on the device, three sets: no substitution, one,
three per read.  max_smems = 16, min_length = 1.
  gate    the walk emulated round by round over the live reads: gdx_suffix_segments_many_dev(max_segments = 1) on the
          companion over the reversed q[p, m) gives e, the same call on the forward index over q[0, e) gives s and the
          interval; the per-round query buffers and the bookkeeping are torch ops on the device.  Checked once against the
          fused call on all reads of every set, then both timed alternately in windows of at least a second.
  report  reads/s and cursor steps/s of the fused call (steps: the symbols both passes consumed, the blocking one
          included, counted by the emulation), SMEMs per read, and the same reads through
          gdx_suffix_segments_many_dev(max_segments = 8, GDX_SEGMENTS_LF_ONLY) as a neighbouring data point.
usage: python tools/exp_smems.py [gate,report | profile]   -> JSON lines on stderr, one JSON result line on stdout
(profile: a few calls of the fused kernel only, for rocprofv3 runs)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from genedex_amd import alphabet  # noqa: E402
from genedex_amd.device import DeviceEngine, DeviceQueries, build_index_from_device_text, synth_text  # noqa: E402
from genedex_amd.index import build_options  # noqa: E402

what = (sys.argv[1] if len(sys.argv) > 1 else "gate,report").split(",")
total = int(os.environ.get("GDX_EXP_TOTAL", 1 << 30))
nq = int(os.environ.get("GDX_EXP_NQ", 10_000_000))
window_s = float(os.environ.get("GDX_EXP_WINDOW_S", 1.0))
LEN, MAX_SMEMS, MIN_LENGTH = 100, 16, 1
dev = torch.device("cuda", 0)
torch.manual_seed(7)
io_text = synth_text(total, seed=42, n_per_million=0, device=dev)


def make_reads(n_subst):
    """nq reads of LEN symbols sampled from the text, n_subst substitutions each (A->C->G->T->A at random places):
    (the batch, the reads as one flat buffer, the reads each reversed as one flat buffer)"""
    rot = torch.arange(256, dtype=torch.uint8, device=dev)
    for a, b in zip(b"ACGT", b"CGTA"):
        rot[a] = b
    qmat = torch.empty((nq, LEN), dtype=torch.uint8, device=dev)
    ar = torch.arange(LEN, device=dev)
    for lo in range(0, nq, 1 << 20):
        hi = min(nq, lo + (1 << 20))
        pos = torch.randint(0, total - LEN, (hi - lo,), device=dev)
        block = io_text[(pos[:, None] + ar[None, :]).reshape(-1)].reshape(hi - lo, LEN)
        for _ in range(n_subst):
            col = torch.randint(0, LEN, (hi - lo, 1), device=dev)
            block.scatter_(1, col, rot[block.gather(1, col).long()])
        qmat[lo:hi] = block
    qbuf = torch.zeros(nq * LEN + 8, dtype=torch.uint8, device=dev)
    qbuf[: nq * LEN] = qmat.reshape(-1)
    qoff = torch.arange(0, nq + 1, dtype=torch.int64, device=dev) * LEN
    return DeviceQueries(qbuf, qoff, nq, nq * LEN), qmat.reshape(-1), qmat.flip(1).contiguous().reshape(-1)


def windows(fn, reps=3):
    """reps windows of at least window_s seconds each -> ms per call of every window"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        calls, t0 = 0, time.perf_counter()
        while True:
            fn()
            calls += 1
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= window_s:
                break
        out.append((time.perf_counter() - t0) / calls * 1e3)
    return out


def spread(ms):
    return (max(ms) - min(ms)) / sorted(ms)[len(ms) // 2]


def longest_suffix_of_prefixes(eng, flat, rows, lens):
    """gdx_suffix_segments_many_dev(max_segments = 1) over the prefixes flat[row * LEN : row * LEN + len] as a batch of their
    own -> (length, start, end) per prefix"""
    n = rows.numel()
    qoff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=qoff[1:])
    nbytes = int(qoff[-1])
    row_of = torch.repeat_interleave(torch.arange(n, device=dev), lens, output_size=nbytes)
    src = rows[row_of] * LEN + (torch.arange(nbytes, device=dev) - qoff[row_of])
    qbuf = torch.zeros(nbytes + 8, dtype=torch.uint8, device=dev)
    qbuf[:nbytes] = flat[src]
    out = eng.alloc_segments(n, 1)
    eng.suffix_segments(DeviceQueries(qbuf, qoff, n, nbytes), 1, out)
    return out["length"].long(), out["start"], out["end"]


def emulate(eng_f, eng_r, flat, rev_flat):
    """the walk of include/gdx.h, one round per pass pair over the reads that are still live"""
    p = torch.full((nq,), LEN - 1, dtype=torch.int64, device=dev)
    n = torch.zeros(nq, dtype=torch.int64, device=dev)
    out = {k: torch.zeros(nq * MAX_SMEMS, dtype=torch.int32, device=dev) for k in ("begin", "length", "start", "end")}
    steps = torch.zeros((), dtype=torch.int64, device=dev)
    while True:
        live = ((p >= 0) & (n < MAX_SMEMS)).nonzero().squeeze(1)
        if live.numel() == 0:
            break
        pl = p[live]
        fwd, _, _ = longest_suffix_of_prefixes(eng_r, rev_flat, live, LEN - pl)  # the reversed q[p, m) is a prefix of the reversed read
        e = pl + fwd
        steps += fwd.sum() + (e < LEN).sum()
        hit = fwd > 0
        p[live[~hit]] -= 1
        rows, e = live[hit], e[hit]
        if rows.numel() == 0:
            continue
        back, start, end = longest_suffix_of_prefixes(eng_f, flat, rows, e)
        s = e - back
        steps += back.sum() + (s > 0).sum()
        rec = back >= MIN_LENGTH
        slot = rows[rec] * MAX_SMEMS + n[rows[rec]]
        out["begin"][slot] = s[rec].int()
        out["length"][slot] = back[rec].int()
        out["start"][slot] = start[rec]
        out["end"][slot] = end[rec]
        n[rows[rec]] += 1
        p[rows] = s - 1
    out["n_smems"] = n.int()
    out["remaining"] = (p + 1).clamp(min=0).int()
    return out, int(steps)


res = {"total_symbols": total, "reads": nq, "read_length": LEN, "max_smems": MAX_SMEMS, "min_length": MIN_LENGTH,
       "window_s": window_s, "free_hbm_gb_at_start": torch.cuda.mem_get_info()[0] / 1e9}
a = alphabet.ascii_dna_with_n()
t0 = time.time()
forward = build_index_from_device_text(io_text, [total], a, index_storage="u32")
res["build_forward_s"] = time.time() - t0
free_before = torch.cuda.mem_get_info()[0]
t0 = time.time()
companion = build_index_from_device_text(io_text.flip(0).contiguous(), [total], a, index_storage="u32",
                                         options=build_options(seed_symbols=0, text_units=False, full_suffix_array=False,
                                                               inverse_suffix_array=False, jump_entry_bytes=0))
res["build_companion_s"] = time.time() - t0
torch.cuda.synchronize()
res["companion_hbm_gb"] = (free_before - torch.cuda.mem_get_info()[0]) / 1e9
eng, reng = DeviceEngine(forward), DeviceEngine(companion)
res["aux_forward"], res["aux_companion"] = eng.aux_info(), reng.aux_info()
print(json.dumps({k: res[k] for k in ("total_symbols", "reads", "build_forward_s", "build_companion_s", "companion_hbm_gb",
                                      "aux_forward", "aux_companion")}), file=sys.stderr, flush=True)
sets = {}
for name, k in (("subst0", 0), ("subst1", 1), ("subst3", 3)):
    sets[name] = make_reads(k)

if "profile" in what:
    out = eng.alloc_smems(nq, MAX_SMEMS)
    for name, (q, _, _) in sets.items():
        for _ in range(2):
            eng.smems(q, reng, MAX_SMEMS, MIN_LENGTH, out)
        torch.cuda.synchronize()
    print(json.dumps({"profile": "done"}))
    sys.exit(0)

steps_of = {}
if "gate" in what:
    res["gate"] = {}
    out = eng.alloc_smems(nq, MAX_SMEMS)
    for name, (q, flat, rev_flat) in sets.items():
        for t in out.values():
            t.fill_(0x55)
        eng.smems(q, reng, MAX_SMEMS, MIN_LENGTH, out)
        emu, steps_of[name] = emulate(eng, reng, flat, rev_flat)
        torch.cuda.synchronize()
        differ = [k for k in emu if not torch.equal(out[k], emu[k])]
        if differ or out["status"].any():
            raise SystemExit(f"PARITY FAILURE ({name}): the fused call and its emulation differ in {differ}")
        fused_ms, emu_ms = [], []
        for _ in range(3):  # the two sides alternately, in the same process
            fused_ms += windows(lambda: eng.smems(q, reng, MAX_SMEMS, MIN_LENGTH, out), reps=1)
            emu_ms += windows(lambda: emulate(eng, reng, flat, rev_flat), reps=1)
        g = {"equal": True, "fused_ms": fused_ms, "emulation_ms": emu_ms, "fused_spread": spread(fused_ms),
             "emulation_spread": spread(emu_ms), "speedup_worst_case": min(emu_ms) / max(fused_ms)}
        # faster by more than the larger of the two spreads: the slowest fused window against the fastest emulation window
        g["passes"] = min(emu_ms) > max(fused_ms) * (1.0 + max(g["fused_spread"], g["emulation_spread"]))
        res["gate"][name] = g
        print(json.dumps({name: g}), file=sys.stderr, flush=True)
        del emu

if "report" in what:
    res["report"] = []
    out = eng.alloc_smems(nq, MAX_SMEMS)
    seg = eng.alloc_segments(nq, 8)
    for name, (q, flat, rev_flat) in sets.items():
        if name not in steps_of:
            steps_of[name] = emulate(eng, reng, flat, rev_flat)[1]
        t = windows(lambda: eng.smems(q, reng, MAX_SMEMS, MIN_LENGTH, out), reps=3)
        t_seg = windows(lambda: eng.suffix_segments(q, 8, seg, lf_only=True), reps=2)
        row = {"reads": name, "ms": t, "reads_per_s": nq / (min(t) / 1e3), "cursor_steps": steps_of[name],
               "cursor_steps_per_read_symbol": steps_of[name] / (nq * LEN), "cursor_steps_per_s": steps_of[name] / (min(t) / 1e3),
               "smems_per_read": float(out["n_smems"].float().mean()), "cut_reads": int((out["remaining"] > 0).sum()),
               "mean_smem_length": float(out["length"].long().sum()) / max(int(out["n_smems"].long().sum()), 1),
               "suffix_segments_8_lf_only_ms": t_seg, "suffix_segments_8_lf_only_reads_per_s": nq / (min(t_seg) / 1e3),
               "segments_per_read": float(seg["n_segments"].float().mean())}
        res["report"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
print(json.dumps(res))
