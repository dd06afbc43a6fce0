#!/usr/bin/env python3
"""gdx_suffix_segments_many_dev against its emulation with the calls that existed before it, and its own rates.

Index: a synthetic A C G T text (GDX_EXP_TOTAL symbols, default 2^30), the default shape and -- for the table at the
end -- a pair-lines-only index.  Reads: GDX_EXP_NQ (default 10 M) reads of 100 symbols sampled from the text on the
device, three sets: no substitution, one, three per read.
  gate    longest suffix match (max_segments = 1) emulated with gdx_cursor_extend_front_many_dev, one launch per symbol,
          the last non-empty interval and the length kept with torch ops on the device: checked once against the fused
          call, then both timed alternately in windows of at least a second.
  report  reads/s and matched symbols/s (LF steps the walk stands for) of max_segments 1 and 8, with and without
          GDX_SEGMENTS_LF_ONLY, on both indexes.
usage: python tools/exp_suffix_segments.py [gate,report | profile]   -> JSON lines on stderr, one JSON result line on stdout
(profile: a few calls of the fused kernel only, for rocprofv3 runs)"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from genedex_amd import _lib, alphabet  # noqa: E402
from genedex_amd.device import DeviceEngine, DeviceQueries, build_index_from_device_text, synth_text  # noqa: E402
from genedex_amd.index import build_options  # noqa: E402

what = (sys.argv[1] if len(sys.argv) > 1 else "gate,report").split(",")
total = int(os.environ.get("GDX_EXP_TOTAL", 1 << 30))
nq = int(os.environ.get("GDX_EXP_NQ", 10_000_000))
window_s = float(os.environ.get("GDX_EXP_WINDOW_S", 1.0))
LEN = 100
dev = torch.device("cuda", 0)
torch.manual_seed(7)
io_text = synth_text(total, seed=42, n_per_million=0, device=dev)


def make_reads(n_subst):
    """nq reads of LEN symbols sampled from the text, n_subst substitutions each (A->C->G->T->A at random places)"""
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
    return DeviceQueries(qbuf, qoff, nq, nq * LEN), qmat.t().contiguous()  # columns: the symbols of one launch of the emulation


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


def emulate(eng, cols, n_rows):
    """longest suffix match with the one-symbol cursor call: one launch per symbol"""
    start = torch.zeros(nq, dtype=torch.int32, device=dev)
    end = torch.full((nq,), n_rows, dtype=torch.int64, device=dev).to(torch.int32)  # (u32 values in int32 tensors)
    length = torch.zeros(nq, dtype=torch.int32, device=dev)
    alive = torch.ones(nq, dtype=torch.bool, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for j in range(LEN - 1, -1, -1):
        s2, e2 = start.clone(), end.clone()
        _lib.check(eng.lib.gdx_cursor_extend_front_many_dev(eng.h, C.c_void_p(s2.data_ptr()), C.c_void_p(e2.data_ptr()),
                                                            C.c_void_p(cols[j].data_ptr()), nq, None, stream))
        alive = alive & (s2 != e2)
        start = torch.where(alive, s2, start)
        end = torch.where(alive, e2, end)
        length += alive
    return length, start, end


res = {"total_symbols": total, "reads": nq, "read_length": LEN, "window_s": window_s,
       "free_hbm_gb_at_start": torch.cuda.mem_get_info()[0] / 1e9}
indexes = {}
t0 = time.time()
indexes["default"] = build_index_from_device_text(io_text, [total], alphabet.ascii_dna_with_n(), index_storage="u32")
res["build_default_s"] = time.time() - t0
eng = DeviceEngine(indexes["default"])
res["aux_default"] = eng.aux_info()
print(json.dumps({k: res[k] for k in ("total_symbols", "reads", "build_default_s", "aux_default")}), file=sys.stderr, flush=True)
sets = {}
for name, k in (("subst0", 0), ("subst1", 1), ("subst3", 3)):
    sets[name] = make_reads(k)

if "profile" in what:
    for name, (q, _) in sets.items():
        for ms in (1, 8):
            out = eng.alloc_segments(nq, ms)
            for lf_only in (False, True):
                eng.suffix_segments(q, ms, out, lf_only=lf_only)
            torch.cuda.synchronize()
    print(json.dumps({"profile": "done"}))
    sys.exit(0)

if "gate" in what:
    n_rows = indexes["default"].total_text_len()
    res["gate"] = {}
    for name, (q, cols) in sets.items():
        out = eng.alloc_segments(nq, 1)
        eng.suffix_segments(q, 1, out)
        length, start, end = emulate(eng, cols, n_rows)
        torch.cuda.synchronize()
        hit = length > 0
        same = (torch.equal(out["length"], length) and torch.equal(out["start"][hit], start[hit]) and torch.equal(out["end"][hit], end[hit])
                and not out["start"][~hit].any() and not out["status"].any())
        if not same:
            raise SystemExit(f"PARITY FAILURE ({name}): the fused call and its emulation differ")
        fused, emu = [], []
        for _ in range(3):  # the two sides alternately, in the same process
            fused += windows(lambda: eng.suffix_segments(q, 1, out), reps=1)
            emu += windows(lambda: emulate(eng, cols, n_rows), reps=1)
        g = {"equal": True, "fused_ms": fused, "emulation_ms": emu, "fused_spread": spread(fused), "emulation_spread": spread(emu),
             "speedup_worst_case": min(emu) / max(fused), "mean_length": float(length.float().mean())}
        g["passes"] = min(emu) > max(fused)  # faster by more than both spreads: the slowest fused window beats the fastest emulation
        res["gate"][name] = g
        print(json.dumps({name: g}), file=sys.stderr, flush=True)
        del out, length, start, end

if "report" in what:
    opts = build_options(jump_entry_bytes=0, top_table_depth=0)  # pair lines and nothing else (aux_pair_lines_only says what was built)
    indexes["pair_lines_only"] = build_index_from_device_text(io_text, [total], alphabet.ascii_dna_with_n(), index_storage="u32",
                                                              options=opts)
    res["aux_pair_lines_only"] = DeviceEngine(indexes["pair_lines_only"]).aux_info()
    res["report"] = []
    for iname, ix in indexes.items():
        e2 = DeviceEngine(ix)
        for name, (q, _) in sets.items():
            for ms in (1, 8):
                out = e2.alloc_segments(nq, ms)
                for lf_only in (False, True):
                    t = windows(lambda: e2.suffix_segments(q, ms, out, lf_only=lf_only), reps=2)
                    matched = int(out["length"].long().sum())
                    row = {"index": iname, "reads": name, "max_segments": ms, "lf_only": lf_only, "ms": t,
                           "reads_per_s": nq / (min(t) / 1e3), "matched_symbols_per_s": matched / (min(t) / 1e3),
                           "segments_per_read": float(out["n_segments"].float().mean())}
                    res["report"].append(row)
                    print(json.dumps(row), file=sys.stderr, flush=True)
                del out
print(json.dumps(res))
