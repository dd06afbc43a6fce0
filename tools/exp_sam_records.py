#!/usr/bin/env python3
"""gdx_sam_records_many_dev behind the resident chain over read pairs: the time of its steps beside a device-to-device copy of as
many bytes as it writes.

The workload of tools/exp_mate_rescue.py (profiles/r22) on the synthetic text: GDX_EXP_TOTAL symbols (default 2^30) with the
default-shape index and the companion over the reversed text; GDX_EXP_NQ (default 10 M) reads of 150 symbols with 0..3 edits as
interleaved pairs (fragments of 300 .. 600 symbols); map_pairs(rescue=True) with max_smems 16, min_length 19, band 8,
max_candidates 4, max_occ 8, max_edits 11, insert bounds [250, 650].  Its result goes through DeviceEngine.sam_inputs into
sam_records_dev, paired mode, numbers for names (GDX_EXP_NAMES=1: a 24-byte name per read and a text name).
  sizing_ms    the call with out = NULL: lengths, scan of the workgroup sums, offsets
  call_ms      the call with out: the same three and the fill;  fill_ms = call_ms - sizing_ms
  copy_ms      a device-to-device copy of rec_off[n_reads] bytes (torch's copy_) in the same process; stream_copy_ms the library's
               own streaming copy kernel (gdx_bench_stream_copy) over the same bytes
  medians of GDX_EXP_REPS (default 7) calls after two warm-up calls, events on the stream
Before anything is timed the first GDX_EXP_CHECK (default 2^14) records are parsed on the host and every mapped one must rebuild
text[begin:end] from SEQ, CIGAR and MD (tests/test_sam_records_model.py's rebuild_segment).
usage: python tools/exp_sam_records.py [report | profile]   -> JSON lines on stderr, one JSON result line on stdout; report also
writes sam_records.json into GDX_EXP_OUT (default profiles/r23).  profile: a few calls only, for rocprofv3 --kernel-trace --stats"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from genedex_amd import _lib, alphabet  # noqa: E402
from genedex_amd.device import DeviceEngine, DeviceQueries, build_index_from_device_text, synth_text  # noqa: E402
from genedex_amd.index import build_options  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "report"
total = int(os.environ.get("GDX_EXP_TOTAL", 1 << 30))
nq = int(os.environ.get("GDX_EXP_NQ", 10_000_000)) & ~1
reps = int(os.environ.get("GDX_EXP_REPS", 7))
n_check = min(nq, int(os.environ.get("GDX_EXP_CHECK", 1 << 14)))
with_names = os.environ.get("GDX_EXP_NAMES", "0") == "1"
out_dir = os.environ.get("GDX_EXP_OUT", os.path.join(ROOT, "profiles", "r23"))
L, MAX_SMEMS, MIN_LENGTH, BAND, MAX_CANDIDATES, MAX_OCC = 150, 16, 19, 8, 4, 8
K = BAND + 3
FRAGMENT, MIN_INSERT, MAX_INSERT = (300, 600), 250, 650
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
    """tools/exp_mate_rescue.py's batch: the mates interleaved, the forward mate first in even pairs and second in odd ones"""
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
    return DeviceQueries(qbuf, torch.arange(0, nq + 1, dtype=torch.int64, device=dev) * L, nq, nq * L)


io_text = synth_text(total, seed=42, n_per_million=0, device=dev)
t0 = time.time()
index = build_index_from_device_text(io_text, [total], a, index_storage="u32")
companion = build_index_from_device_text(io_text.flip(0).contiguous(), [total], a, index_storage="u32",
                                         options=build_options(seed_symbols=0, text_units=False, full_suffix_array=False,
                                                               inverse_suffix_array=False, jump_entry_bytes=0))
eng, reng = DeviceEngine(index), DeviceEngine(companion)
print(json.dumps({"build_s": time.time() - t0}), file=sys.stderr, flush=True)
dq = make_pairs(io_text)
sq = dq.with_strands(index, "both")
result = eng.map_pairs(dq, reng, rescue=True, max_smems=MAX_SMEMS, min_length=MIN_LENGTH, max_occ=MAX_OCC, band=BAND,
                       max_candidates=MAX_CANDIDATES, max_edits=K, min_insert=MIN_INSERT, max_insert=MAX_INSERT)
torch.cuda.synchronize()
names = [b"read.%012d/%d...." % (r >> 1, r & 1) for r in range(nq)] if with_names else None
args, kw, n = eng.sam_inputs(sq, result, mode="paired", names=names, text_names=[b"chrSynthetic1"] if with_names else None)
rec_off = args[-1]
eng.sam_records_dev(*args, None, **kw)
total_bytes = int(rec_off[n].item())
out = torch.full((total_bytes + 16,), 0xA5, dtype=torch.uint8, device=dev)
eng.sam_records_dev(*args, out, out_capacity=total_bytes, **kw)
torch.cuda.synchronize()
assert int(out[total_bytes].item()) == 0xA5

# the first records, parsed: every mapped one rebuilds its piece of the text
from test_sam_records_model import rebuild_segment  # noqa: E402

off = rec_off[:n_check + 1].cpu().numpy()
data = out[:int(off[-1])].cpu().numpy().tobytes()
begin, end = (result[name][:n_check].cpu().numpy().astype("int64") & 0xFFFFFFFF for name in ("begin", "end"))
mapped = 0
for r in range(n_check):
    line = data[int(off[r]):int(off[r + 1])]
    if end[r] == 0xFFFFFFFF:
        assert line.split(b"\t")[2] == b"*", line
        continue
    mapped += 1
    _, b, segment = rebuild_segment(line)
    want = io_text[int(begin[r]):int(end[r])].cpu().numpy().tobytes()
    if b != begin[r] or segment != want:
        raise SystemExit(f"PARITY FAILURE: record {r} does not rebuild its text: {line!r} != {want!r}")
res = {"total_symbols": total, "reads": nq, "read_length": L, "max_edits": K, "names": with_names, "reps": reps, "checked_records": n_check,
       "checked_mapped": mapped, "mapped": float((result["end"][:nq] != -1).float().mean()), "bytes": total_bytes,
       "bytes_per_record": total_bytes / nq, "status_bad": int(kw["status"][:n].sum().item())}
print(json.dumps(res), file=sys.stderr, flush=True)
if what == "profile":
    for _ in range(3):
        eng.sam_records_dev(*args, out, out_capacity=total_bytes, **kw)
    torch.cuda.synchronize()
    sys.exit(0)
src = torch.empty(total_bytes // 16 * 16, dtype=torch.uint8, device=dev).fill_(7)
dst = torch.empty_like(src)
lib = _lib.load()
res["sizing_ms"] = median_ms(lambda: eng.sam_records_dev(*args, None, **kw))
res["call_ms"] = median_ms(lambda: eng.sam_records_dev(*args, out, out_capacity=total_bytes, **kw))
res["fill_ms"] = res["call_ms"] - res["sizing_ms"]
res["copy_ms"] = median_ms(lambda: dst.copy_(src))
stream = torch.cuda.current_stream().cuda_stream
res["stream_copy_ms"] = median_ms(lambda: _lib.check(lib.gdx_bench_stream_copy(dst.data_ptr(), src.data_ptr(), src.numel(), stream)))
res["fill_over_copy"] = res["fill_ms"] / res["copy_ms"]
for tile in (1024, 2048):  # smaller tiles than the default (4096, the largest), the default grid
    lib.gdx_debug_set_sam_tiling(tile, 0)
    res[f"call_ms_tile_{tile}"] = median_ms(lambda: eng.sam_records_dev(*args, out, out_capacity=total_bytes, **kw))
lib.gdx_debug_set_sam_tiling(0, 0)
print(json.dumps(res))
if what == "report":
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "sam_records.json" if not with_names else "sam_records_names.json"), "w") as f:
        f.write(json.dumps(res) + "\n")
