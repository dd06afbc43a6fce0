"""benchlib.dump -- --dump-outputs: what the timed path computed in its last step, as .npy files, so that two builds of the
project can be compared output for output on the same inputs (bench.py's inputs are seeded: the same arguments give the same
text and the same batch)."""
from __future__ import annotations

import os

from .common import log

__all__ = ['DUMP_LIMIT_BYTES', 'DUMP_SAMPLE', 'DUMP_SEED', 'dump_outputs']

DUMP_LIMIT_BYTES = 64 << 20  # every file together
DUMP_SAMPLE = 1 << 19        # queries, and hits, in the fixed sample of a larger batch
DUMP_SEED = 20240917         # the sample is the same from run to run and from build to build


def _sample(np, n, k, rng):
    """sorted distinct indices in [0, n): all of them when n <= k, else a seeded draw"""
    if n <= k:
        return np.arange(n, dtype=np.int64)
    return np.sort(rng.choice(n, size=k, replace=False)).astype(np.int64)


def dump_outputs(np, torch, runner, slot, out_dir):
    """The arrays a caller of the timed step receives, for a fixed sample of the queries and of the hits:

        query_index   the sampled queries (indices into the batch)
        counts        their numbers of occurrences
        status        their status codes (0 = searched)
        hit_offsets   where their hits start in the hit array (count + locate only)
        hit_index     the sampled hits (indices into the hit array)
        hit_text_id   their text ids
        hit_position  their positions in the text
        totals        [number of queries, number of hits (count only: the sum of the counts)]

    Integers up to 2^53 in float64 (text ids and status codes in float32): exact.  -> {name: shape}"""
    o = runner.outs[slot]
    nq = runner.nq
    dev = o["status"].device
    rng = np.random.default_rng(DUMP_SEED)
    qi = _sample(np, nq, DUMP_SAMPLE, rng)
    qt = torch.from_numpy(qi).to(dev)
    arrays = {"query_index": qi.astype(np.float64),
              "counts": runner.counts(o).to(torch.int64).index_select(0, qt).cpu().numpy().astype(np.float64),
              "status": runner.status(o).to(torch.int64).index_select(0, qt).cpu().numpy().astype(np.float32)}
    total_hits = runner.total_hits  # (count only: the sum of the counts, from the sizing pass)
    if runner.do_locate:
        arrays["hit_offsets"] = o["hit_offsets"][:nq].index_select(0, qt).cpu().numpy().astype(np.float64)
        hi = _sample(np, total_hits, DUMP_SAMPLE, rng)
        h = runner.hits[slot][:total_hits].index_select(0, torch.from_numpy(hi).to(dev)).to(torch.int64).cpu().numpy()
        arrays["hit_index"] = hi.astype(np.float64)
        arrays["hit_text_id"] = h[:, 0].astype(np.float32)
        arrays["hit_position"] = (h[:, 1] & 0xFFFFFFFF).astype(np.float64)
    arrays["totals"] = np.array([nq, total_hits], dtype=np.float64)
    size = sum(a.nbytes for a in arrays.values())
    if size > DUMP_LIMIT_BYTES:
        raise SystemExit(f"--dump-outputs: {size} bytes, more than {DUMP_LIMIT_BYTES}")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    log(f"[bench] outputs of the last timed step ({size / 1e6:.1f} MB) written to {out_dir}: {sorted(arrays)}")
    return {name: a.shape for name, a in arrays.items()}
