#!/usr/bin/env python3
"""gdx_strands_expand_dev: what a both-strand count + locate step costs with the expand on the device, against the route
that existed before it (a reverse-complement batch prepared on the host and uploaded a second time).

Index: a synthetic A C G T text (GDX_EXP_TOTAL symbols, default 2^30) in the default shape.  Reads: GDX_EXP_NQ (default 10 M)
reads of 50 symbols sampled from the text on the device, every second one reverse-complemented (so half come from the reverse
strand).  For each of the four layouts (plain / packed x offsets / uniform):
  expand     the expand alone, modes REVERSE and BOTH, beside its traffic floor: bytes read + bytes written over the measured
             copy rate of the device (6.29 TB/s, a float4 copy)
  step       the one-call count + locate step on the expanded batch of 2 nq rows; expand + step = the both-strand step
  baseline   two steps, on the forward batch and on a reverse-complement batch that is already resident (kernels only), and
             the same plus the second host preparation (numpy reverse complement, gdx_pack_queries for the packed forms) and
             upload of that batch
The two routes' results are compared (counts and status of every row, the number of hits, the position of every row with
one hit) before anything is timed.  Times: medians of GDX_EXP_REPS (default 7) runs after two warm-up runs, events on the
stream; host preparation by perf_counter.
usage: python tools/exp_strands.py [report | profile]   -> JSON lines on stderr, one JSON result line on stdout
(profile: a few expands and steps only, for rocprofv3 --kernel-trace --stats)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from genedex_amd import _lib, alphabet  # noqa: E402
from genedex_amd.device import DeviceEngine, DeviceQueries, build_index_from_device_text, synth_text  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "report"
total = int(os.environ.get("GDX_EXP_TOTAL", 1 << 30))
nq = int(os.environ.get("GDX_EXP_NQ", 10_000_000))
reps = int(os.environ.get("GDX_EXP_REPS", 7))
LEN = 50
COPY_RATE = 6.29e12  # bytes per second, read + written
dev = torch.device("cuda", 0)
torch.manual_seed(7)
lib = _lib.load()
a = alphabet.ascii_dna()
io_text = synth_text(total, seed=42, n_per_million=0, device=dev)
t0 = time.time()
index = build_index_from_device_text(io_text, [total], a, index_storage="u32")
eng = DeviceEngine(index)
res = {"total_symbols": total, "reads": nq, "read_length": LEN, "reps": reps, "build_s": time.time() - t0, "aux": eng.aux_info()}
print(json.dumps(res), file=sys.stderr, flush=True)

comp = torch.from_numpy(alphabet.dna_complement_table()).to(dev)
qmat = torch.empty((nq, LEN), dtype=torch.uint8, device=dev)
ar = torch.arange(LEN, device=dev)
for lo in range(0, nq, 1 << 20):
    hi = min(nq, lo + (1 << 20))
    pos = torch.randint(0, total - LEN, (hi - lo,), device=dev)
    block = io_text[(pos[:, None] + ar[None, :]).reshape(-1)].reshape(hi - lo, LEN)
    block[1::2] = comp[block[1::2].flip(1).long()]  # every second read comes from the reverse strand
    qmat[lo:hi] = block
del io_text


def plain_batch(mat):
    n = mat.shape[0]
    qbuf = torch.zeros(n * LEN + 8, dtype=torch.uint8, device=dev)
    qbuf[: n * LEN] = mat.reshape(-1)
    return DeviceQueries(qbuf, torch.arange(0, n + 1, dtype=torch.int64, device=dev) * LEN, n, n * LEN)


def in_layout(dq, packed, uniform):
    if uniform:
        dq = dq.as_uniform(LEN)
    return dq.as_packed(index) if packed else dq


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


class Step:
    """the buffers of one count + locate step of m rows, and the step"""

    def __init__(self, m):
        self.m, self.cap = m, m + m // 4 + 4096
        self.rec, self.cw = eng.alloc_records(m), eng.alloc_compact(m)
        self.off = torch.empty(m + 1, dtype=torch.int32, device=dev)
        self.hits = torch.empty((self.cap, 2), dtype=torch.int32, device=dev)
        self.totals = torch.zeros(2, dtype=torch.int64, device=dev)
        self.sws = torch.empty(max(eng.totals_workspace_bytes(m), 16), dtype=torch.uint8, device=dev)
        self.ws = torch.empty(max(eng.locate_workspace_bytes(self.cap), 16), dtype=torch.uint8, device=dev)

    def run(self, dq):
        eng.locate_step(dq, self.rec, self.cw, self.sws, self.totals, self.off, self.hits, self.ws)

    def results(self):
        counts = torch.empty(self.m, dtype=torch.int32, device=dev)
        status = torch.empty(self.m, dtype=torch.uint8, device=dev)
        eng.unpack_records(self.rec, self.m, counts, status, compact=self.cw)
        torch.cuda.synchronize()
        assert int(self.totals[0]) <= self.cap, "hit buffer too small for this text"
        one = counts == 1
        first = self.hits[self.off[:-1].long().clamp(max=self.cap - 1), 1]
        return counts, status, int(self.totals[0]), torch.where(one, first, torch.full_like(first, -1))


def host_reverse_batch(h_mat, packed):
    """the second host preparation: numpy reverse complement (+ gdx_pack_queries) and the upload"""
    t = alphabet.dna_complement_table()
    rc = np.ascontiguousarray(t[h_mat[:, ::-1]])
    if not packed:
        buf = np.zeros(rc.size + 8, dtype=np.uint8)
        buf[: rc.size] = rc.reshape(-1)
    else:
        off = np.arange(rc.shape[0] + 1, dtype=np.uint64) * np.uint64(LEN)
        buf = np.zeros(int(lib.gdx_packed_bytes(rc.size)), dtype=np.uint8)
        n_exc = C.c_uint64(0)
        _lib.check(lib.gdx_pack_queries(index._h, rc.ctypes.data_as(_lib.u8p), off.ctypes.data_as(_lib.u64p), rc.shape[0],
                                        buf.ctypes.data_as(_lib.u8p), None, 0, C.byref(n_exc)))
    d = torch.from_numpy(buf).to(dev)
    torch.cuda.synchronize()
    return d


fwd_plain = plain_batch(qmat)
rev_plain = plain_batch(comp[qmat.flip(1).long()])
h_mat = qmat.cpu().numpy() if what != "profile" else None
del qmat
both_step, one_step = Step(2 * nq), Step(nq)
res["layouts"] = []
for packed in (False, True):
    for uniform in (False, True):
        name = ("packed" if packed else "plain") + "+" + ("uniform" if uniform else "offsets")
        fwd, rev = in_layout(fwd_plain, packed, uniform), in_layout(rev_plain, packed, uniform)
        both = fwd.with_strands(index, "both")
        if what == "profile":
            for _ in range(2):
                fwd.with_strands(index, "reverse")
                fwd.with_strands(index, "both")
                both_step.run(both)
            torch.cuda.synchronize()
            continue
        # the two routes agree
        both_step.run(both)
        bc, bs, bt, bp = both_step.results()
        one_step.run(fwd)
        fc, fs, ft, fp = one_step.results()
        fc, fs, fp = fc.clone(), fs.clone(), fp.clone()
        one_step.run(rev)
        rc_, rs, rt, rp = one_step.results()
        ok = (torch.equal(bc[0::2], fc) and torch.equal(bc[1::2], rc_) and torch.equal(bs[0::2], fs) and torch.equal(bs[1::2], rs)
              and bt == ft + rt and torch.equal(bp[0::2], fp) and torch.equal(bp[1::2], rp))
        if not ok:
            raise SystemExit(f"PARITY FAILURE ({name}): the expanded batch and the two host-made batches give different results")
        found = float((bc.reshape(-1, 2) > 0).any(1).float().mean())
        # times
        n_sym = nq * LEN
        in_bytes = n_sym / 4 if packed else n_sym
        off_bytes = 0 if uniform else 8 * nq
        row = {"layout": name, "equal": True, "reads_found_on_a_strand": found, "hits": bt}
        for mode, k in (("reverse", 1), ("both", 2)):
            ms = median_ms(lambda: lib.gdx_strands_expand_dev(
                index._h, C.c_void_p(fwd.qbuf.data_ptr()), fwd.layout()[1], nq, C.byref(fwd.layout()[0]) if fwd.layout()[0] is not None else None,
                n_sym, None, k, C.c_void_p(both.qbuf.data_ptr()), C.c_void_p(both.qoff.data_ptr()) if not uniform else None,
                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            traffic = in_bytes + off_bytes + k * in_bytes + (off_bytes * 2 if k == 2 else 0)
            row[f"expand_{mode}_ms"] = ms
            row[f"expand_{mode}_floor_ms"] = traffic / COPY_RATE * 1e3
            row[f"expand_{mode}_fraction_of_floor_rate"] = traffic / COPY_RATE * 1e3 / ms
            row[f"expand_{mode}_bytes_per_read"] = traffic / nq
        fwd.with_strands(index, "both")  # (the timed REVERSE runs wrote into `both`: make it again)
        both = fwd.with_strands(index, "both")
        row["step_on_expanded_ms"] = median_ms(lambda: both_step.run(both))
        row["both_strand_step_ms"] = row["expand_both_ms"] + row["step_on_expanded_ms"]
        row["baseline_two_steps_ms"] = median_ms(lambda: (one_step.run(fwd), one_step.run(rev)))
        prep = []
        for _ in range(3):
            t0 = time.perf_counter()
            d = host_reverse_batch(h_mat, packed)
            prep.append((time.perf_counter() - t0) * 1e3)
            del d
        row["baseline_host_prepare_and_upload_ms"] = sorted(prep)[1]
        row["baseline_with_host_ms"] = row["baseline_two_steps_ms"] + row["baseline_host_prepare_and_upload_ms"]
        row["expand_share_of_both_strand_step"] = row["expand_both_ms"] / row["both_strand_step_ms"]
        row["both_strand_step_over_baseline_kernels"] = row["both_strand_step_ms"] / row["baseline_two_steps_ms"]
        res["layouts"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
print(json.dumps(res))
