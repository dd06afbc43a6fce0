"""Device-resident use of libgdx.so: indexes built from text that already sits in HBM, query sets
generated in HBM, and the `_dev` entry points of include/gdx.h driven on a torch stream.

torch is used for device memory, streams and events only (plumbing); every computation is a HIP
kernel of libgdx.so.  torch must be imported before libgdx.so is loaded so that both share one HIP
runtime (torch bundles its own libamdhip64.so.7).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .alphabet import Alphabet
from .index import FmIndex, _WIDTHS, _p
from .synth import split_lengths

u8p, u64p = _lib.u8p, _lib.u64p


def _ptr(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


def _layout_arg(lay):
    """the layout pointer of a _dev call: NULL for a batch in the plain form"""
    return C.byref(lay) if lay is not None else None


def _check_candidates(cand_query: torch.Tensor, cand_begin: torch.Tensor, cand_hits: torch.Tensor) -> int:
    """the candidate tensors of the verify calls (hamming, edit_distance, align) -> m"""
    m = cand_query.numel()
    if cand_begin.numel() != m or cand_hits.numel() != 2 * m:
        raise ValueError("cand_query, cand_begin and cand_hits differ in length")
    for t in (cand_query, cand_begin, cand_hits):
        if t.element_size() != 4 or not t.is_contiguous():
            raise ValueError("candidates are contiguous 32-bit tensors")
    return m


def _check_slots(cands: dict, dist: torch.Tensor, end, slots: int, what: str) -> None:
    """the candidate dict, dist and end (or None) of best_hits / pair_hits hold at least `slots` slots (`what` in words)"""
    m = _check_candidates(cands["cand_query"], cands["cand_begin"], cands["cand_hits"])
    if slots > m or dist.numel() < slots or (end is not None and end.numel() < slots):
        raise ValueError(f"candidates, dist and end hold {what} slots")


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def synth_text(total: int, seed: int = 42, n_per_million: int = 10_000, device="cuda") -> torch.Tensor:
    """IO symbols of the synthetic text, generated in HBM (gdx_synth_text_dev)."""
    lib = _lib.load()
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
    _lib.check(lib.gdx_synth_text_dev(_ptr(out), total, seed, n_per_million, _stream()))
    return out


def build_index_from_device_text(io_text: torch.Tensor, text_lengths, alphabet: Alphabet, sa_rate=4, lookup_depth=0,
                                 index_storage="u32", options=None) -> FmIndex:
    lib = _lib.load()
    toff = np.zeros(len(text_lengths) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(text_lengths, dtype=np.uint64), out=toff[1:])
    tab = np.ascontiguousarray(alphabet.io_to_dense_table, dtype=np.uint8)
    handle = C.c_void_p()
    torch.cuda.synchronize()
    from .index import build_options

    opts = options if options is not None else build_options()
    st = lib.gdx_index_build_dev_ex(_ptr(io_text), _p(toff, u64p), len(text_lengths), _p(tab, u8p),
                                    alphabet.num_dense_symbols(), alphabet.num_searchable_dense_symbols(), sa_rate,
                                    lookup_depth, _WIDTHS[index_storage], io_text.device.index or 0, C.byref(opts),
                                    C.byref(handle))
    _lib.check(st)
    return FmIndex(handle, alphabet)


class DeviceQueries:
    """A query set resident in HBM: qbuf (u8, padded to 8 bytes) + qoff (u64[nq+1]).
    packed: qbuf holds 2-bit codes, four symbols per byte (gdx.h "packed queries"; qoff still counts symbols);
    uniform_len != 0: every query has that many symbols and query i starts at symbol i * uniform_len (the search calls then
    pass no offsets: gdx_query_layout_t).  total_bytes = the bytes of qbuf the queries occupy in this form."""

    def __init__(self, qbuf: torch.Tensor, qoff: torch.Tensor, nq: int, total_bytes: int, packed: bool = False,
                 uniform_len: int = 0):
        self.qbuf, self.qoff, self.nq, self.total_bytes = qbuf, qoff, nq, total_bytes
        self.packed, self.uniform_len = packed, uniform_len

    def layout(self):
        """(gdx_query_layout_t or None, offsets pointer) for the *_layout_dev calls"""
        if not self.packed and not self.uniform_len:
            return None, _ptr(self.qoff)
        lay = _lib.QueryLayout()
        _lib.load().gdx_query_layout_init(C.byref(lay))
        lay.packed = 1 if self.packed else 0
        lay.uniform_len = int(self.uniform_len)
        return lay, (C.c_void_p(0) if self.uniform_len else _ptr(self.qoff))

    def total_symbols(self) -> int:
        return self.total_bytes * 4 if self.packed else self.total_bytes  # (packed: rounded up to whole bytes)

    def as_uniform(self, length: int) -> "DeviceQueries":
        """the same batch declared uniform (every query `length` symbols, back to back from symbol 0): checked on the device"""
        n = self.nq
        if n:
            want = torch.arange(0, n + 1, device=self.qoff.device, dtype=torch.int64) * length
            if not torch.equal(self.qoff[: n + 1], want):
                raise ValueError("the batch is not uniform: query i must span [i * length, (i + 1) * length)")
        return DeviceQueries(self.qbuf, self.qoff, n, self.total_bytes, self.packed, length)

    def as_packed(self, index: FmIndex) -> "DeviceQueries":
        """2-bit form of the batch made on the device (gdx_pack_queries_dev); raises if a query has a symbol outside the
        four searchable ones (such queries are the packed form's exceptions and go through the ASCII calls)"""
        lib = _lib.load()
        n_sym = int(self.qoff[self.nq].item()) if self.nq else 0
        nbytes = int(lib.gdx_packed_bytes(n_sym))
        packed = torch.zeros(nbytes, dtype=torch.uint8, device=self.qbuf.device)
        bad = torch.zeros(1, dtype=torch.int64, device=self.qbuf.device)
        _lib.check(lib.gdx_pack_queries_dev(index._h, _ptr(self.qbuf), n_sym, _ptr(packed), C.c_void_p(0), _ptr(bad), _stream()))
        if int(bad.item()):
            raise ValueError(f"{int(bad.item())} symbols outside the four searchable ones: not expressible in 2 bits")
        return DeviceQueries(packed, self.qoff, self.nq, (n_sym + 3) // 4, True, self.uniform_len)

    def with_strands(self, index: FmIndex, mode: str = "both", complement=None) -> "DeviceQueries":
        """A new batch in the same form, made on the device (gdx_strands_expand_dev): mode "reverse" -- query i is the reverse
        complement of query i; "both" -- 2 nq queries, query 2i as given and query 2i + 1 its reverse complement.  complement:
        256 bytes, None = the stock table (alphabet.dna_complement_table)."""
        lib = _lib.load()
        m = {"reverse": _lib.GDX_STRANDS_REVERSE, "both": _lib.GDX_STRANDS_BOTH}[mode]
        if self.uniform_len:
            n_sym = self.nq * int(self.uniform_len)
        else:
            n_sym = int(self.qoff[self.nq].item()) if self.nq else 0
        dev = self.qbuf.device
        out = torch.empty(int(lib.gdx_strands_out_bytes(n_sym, 1 if self.packed else 0, m)), dtype=torch.uint8, device=dev)
        lay, qoff = self.layout()
        if self.uniform_len:
            out_off = self.qoff
        elif m == _lib.GDX_STRANDS_BOTH:
            out_off = torch.empty(2 * self.nq + 1, dtype=torch.int64, device=dev)
        else:
            out_off = self.qoff
        comp_arr = None if complement is None else np.ascontiguousarray(complement, dtype=np.uint8)  # (read during the call)
        if comp_arr is not None and comp_arr.size != 256:
            raise ValueError("a complement table has 256 entries")
        comp = None if comp_arr is None else comp_arr.ctypes.data_as(u8p)
        _lib.check(lib.gdx_strands_expand_dev(index._h, _ptr(self.qbuf), qoff, self.nq, C.byref(lay) if lay is not None else None,
                                              n_sym, comp, m, _ptr(out), _ptr(out_off) if not self.uniform_len else C.c_void_p(0),
                                              _stream()))
        nq = self.nq * m
        if self.uniform_len:
            n_out = nq * int(self.uniform_len)
        elif m == _lib.GDX_STRANDS_BOTH:
            n_out = 2 * (n_sym - (int(self.qoff[0].item()) if self.nq else 0))
        else:
            n_out = n_sym
        return DeviceQueries(out, out_off, nq, (n_out + 3) // 4 if self.packed else n_out, self.packed, self.uniform_len)

    @classmethod
    def synth(cls, io_text: torch.Tensor, text_lengths, nq: int, len_min: int, len_max: int,
              sampled_per_million: int, seed: int = 43) -> "DeviceQueries":
        lib = _lib.load()
        dev = io_text.device
        toff_h = np.zeros(len(text_lengths) + 1, dtype=np.int64)
        np.cumsum(np.asarray(text_lengths, dtype=np.int64), out=toff_h[1:])
        toff = torch.from_numpy(toff_h).to(dev)
        cap = (nq * len_max + 8 + 7) // 8 * 8
        qbuf = torch.zeros(cap, dtype=torch.uint8, device=dev)
        qoff = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        total = C.c_uint64(0)
        _lib.check(lib.gdx_synth_queries_dev(_ptr(io_text), _ptr(toff), len(text_lengths), nq, len_min, len_max,
                                             sampled_per_million, seed, _ptr(qoff), _ptr(qbuf), cap,
                                             C.byref(total), _stream()))
        return cls(qbuf, qoff, nq, total.value)

    @classmethod
    def from_host(cls, qbuf: np.ndarray, qoff: np.ndarray, device="cuda") -> "DeviceQueries":
        nq = qoff.size - 1
        total = int(qoff[-1])
        pad = np.zeros((total + 8 + 7) // 8 * 8, dtype=np.uint8)
        pad[:total] = qbuf[:total]
        return cls(torch.from_numpy(pad).to(device), torch.from_numpy(qoff.astype(np.int64)).to(device), nq, total)

    def slice(self, lo: int, hi: int) -> "DeviceQueries":
        """queries [lo, hi) as a view: the same byte buffer, a window of the offsets (no copy)"""
        if self.packed or self.uniform_len:
            raise ValueError("slice(): plain batches only (a packed / uniform shard is packed from the sliced plain batch)")
        off = self.qoff[lo:hi + 1]
        nbytes = int((off[-1] - off[0]).item()) if hi > lo else 0
        return DeviceQueries(self.qbuf, off, hi - lo, nbytes)

    def copy_slice(self, lo: int, hi: int) -> "DeviceQueries":
        """queries [lo, hi) as a batch of their own (bytes copied, offsets from 0): what a rank holds of a sharded batch"""
        if self.packed or self.uniform_len:
            raise ValueError("copy_slice(): plain batches only")
        off = self.qoff[lo:hi + 1]
        b0, b1 = (int(off[0].item()), int(off[-1].item())) if hi > lo else (0, 0)
        buf = torch.zeros((b1 - b0 + 8 + 7) // 8 * 8, dtype=torch.uint8, device=self.qbuf.device)
        buf[: b1 - b0] = self.qbuf[b0:b1]
        return DeviceQueries(buf, off - off[0] if hi > lo else off.clone(), hi - lo, b1 - b0)

    def host_slice(self, first: int, count: int):
        """(qbuf, qoff) of queries [first, first+count) as numpy arrays (for the CPU baseline / checks)."""
        off = self.qoff[first:first + count + 1].cpu().numpy().astype(np.uint64)
        b0, b1 = int(off[0]), int(off[-1])
        buf = self.qbuf[b0:b1].cpu().numpy() if b1 > b0 else np.zeros(1, dtype=np.uint8)
        return buf, off - off[0]


class DeviceEngine:
    """count / locate passes over a DeviceQueries set, everything staying in HBM."""

    def __init__(self, index: FmIndex):
        self.index = index
        self.lib = _lib.load()
        self.h = index._h
        self.dev = torch.device("cuda", int(index.info.device_id))

    def alloc_outputs(self, nq: int, hint: bool = False):
        """hint=True adds the opaque locate-hint array: search() then fills it and locate() uses it (the device form
        of the fused locate_many; only valid while start / end stay as search() wrote them)."""
        d = self.dev
        out = {
            "start": torch.empty(nq, dtype=torch.int32, device=d),
            "end": torch.empty(nq, dtype=torch.int32, device=d),
            "status": torch.empty(nq, dtype=torch.uint8, device=d),
            "hit_offsets": torch.empty(nq + 1, dtype=torch.int64, device=d),
        }
        if hint:
            out["hint"] = torch.empty(nq, dtype=torch.int64, device=d)
        return out

    def search(self, q: DeviceQueries, out) -> None:
        """cursors_for_many_queries: intervals + status (the dominant kernel)."""
        lay, qoff = q.layout()
        if lay is not None:
            if "hint" in out:
                raise ValueError("hints go with plain batches")
            _lib.check(self.lib.gdx_cursors_for_many_queries_layout_dev(self.h, _ptr(q.qbuf), qoff, q.nq, C.byref(lay),
                                                                        _ptr(out["start"]), _ptr(out["end"]),
                                                                        _ptr(out["status"]), _stream()))
            return
        if "hint" in out:
            _lib.check(self.lib.gdx_cursors_for_many_queries_hint_dev(self.h, _ptr(q.qbuf), _ptr(q.qoff), q.nq,
                                                                      _ptr(out["start"]), _ptr(out["end"]),
                                                                      _ptr(out["status"]), _ptr(out["hint"]),
                                                                      _stream()))
            return
        _lib.check(self.lib.gdx_cursors_for_many_queries_dev(self.h, _ptr(q.qbuf), _ptr(q.qoff), q.nq,
                                                             _ptr(out["start"]), _ptr(out["end"]),
                                                             _ptr(out["status"]), _stream()))

    def count(self, q: DeviceQueries, counts: torch.Tensor, status: torch.Tensor) -> None:
        lay, qoff = q.layout()
        if lay is not None:
            _lib.check(self.lib.gdx_count_many_layout_dev(self.h, _ptr(q.qbuf), qoff, q.nq, C.byref(lay), _ptr(counts),
                                                          _ptr(status), _stream()))
            return
        _lib.check(self.lib.gdx_count_many_dev(self.h, _ptr(q.qbuf), _ptr(q.qoff), q.nq, _ptr(counts),
                                               _ptr(status), _stream()))

    def hit_offsets(self, out, m: int) -> None:
        _lib.check(self.lib.gdx_hit_offsets_dev(self.h, _ptr(out["start"]), _ptr(out["end"]), m,
                                                _ptr(out["hit_offsets"]), _stream()))

    def locate_workspace_bytes(self, total: int) -> int:
        return int(self.lib.gdx_locate_workspace_bytes(total))

    def locate(self, out, m: int, total: int, hits: torch.Tensor, workspace: torch.Tensor) -> None:
        """hits: int32[total, 2] = (text_id, position) per hit, in suffix-array order per query."""
        if "hint" in out:
            _lib.check(self.lib.gdx_locate_intervals_hint_dev(self.h, _ptr(out["start"]), _ptr(out["end"]), m,
                                                              _ptr(out["hit_offsets"]), total, _ptr(hits),
                                                              _ptr(workspace), _ptr(out["hint"]), _stream()))
            return
        _lib.check(self.lib.gdx_locate_intervals_dev(self.h, _ptr(out["start"]), _ptr(out["end"]), m,
                                                     _ptr(out["hit_offsets"]), total, _ptr(hits), _ptr(workspace),
                                                     _stream()))

    # ---- fused count + locate over 16-byte search records (gdx_locate_many_*_dev) -------------------------
    def alloc_records(self, nq: int) -> torch.Tensor:
        return torch.empty((max(nq, 1), 4), dtype=torch.int32, device=self.dev)

    def alloc_compact(self, nq: int) -> torch.Tensor:
        """compact results beside the records (gdx.h): int32[nq], the position of the only hit / -1 none / -2 see the record"""
        return torch.empty(max(nq, 1), dtype=torch.int32, device=self.dev)

    def locate_search(self, q: DeviceQueries, rec: torch.Tensor, compact: torch.Tensor = None) -> None:
        lay, qoff = q.layout()
        if lay is not None:
            if compact is not None:
                _lib.check(self.lib.gdx_locate_many_search_compact_layout_dev(self.h, _ptr(q.qbuf), qoff, q.nq, C.byref(lay),
                                                                              _ptr(rec), _ptr(compact), _stream()))
            else:
                _lib.check(self.lib.gdx_locate_many_search_layout_dev(self.h, _ptr(q.qbuf), qoff, q.nq, C.byref(lay), _ptr(rec),
                                                                      _stream()))
            return
        if compact is not None:
            _lib.check(self.lib.gdx_locate_many_search_compact_dev(self.h, _ptr(q.qbuf), _ptr(q.qoff), q.nq, _ptr(rec),
                                                                   _ptr(compact), _stream()))
            return
        _lib.check(self.lib.gdx_locate_many_search_dev(self.h, _ptr(q.qbuf), _ptr(q.qoff), q.nq, _ptr(rec), _stream()))

    def locate_search_totals(self, q: DeviceQueries, rec: torch.Tensor, compact: torch.Tensor, scan_ws: torch.Tensor,
                             totals: torch.Tensor, max_hits: int = 0) -> None:
        """gdx_locate_many_search_totals_compact_layout_dev: the compact search and the hit totals in one call"""
        lay, qoff = q.layout()
        _lib.check(self.lib.gdx_locate_many_search_totals_compact_layout_dev(
            self.h, _ptr(q.qbuf), qoff, q.nq, C.byref(lay) if lay is not None else None, max_hits, _ptr(rec), _ptr(compact),
            _ptr(scan_ws), _ptr(totals), _stream()))

    def locate_step(self, q: DeviceQueries, rec: torch.Tensor, compact, scan_ws: torch.Tensor, totals: torch.Tensor,
                    hit_offsets: torch.Tensor, hits: torch.Tensor, workspace: torch.Tensor, max_hits: int = 0,
                    event_after_search=None) -> None:
        """gdx_locate_many_step_compact_layout_dev: search, totals, offsets and hits in one call, no host round trip; hits
        beyond hits.shape[0] are not stored (totals[0], read later, tells); hit_offsets int32 = the narrow form;
        event_after_search: a torch.cuda.Event that has been recorded once (so that its handle exists)"""
        lay, qoff = q.layout()
        _lib.check(self.lib.gdx_locate_many_step_compact_layout_dev(
            self.h, _ptr(q.qbuf), qoff, q.nq, C.byref(lay) if lay is not None else None, max_hits, _ptr(rec),
            _ptr(compact) if compact is not None else None, _ptr(scan_ws), _ptr(totals), _ptr(hit_offsets),
            32 if hit_offsets.dtype == torch.int32 else 64, _ptr(hits), hits.shape[0], _ptr(workspace),
            C.c_void_p(event_after_search.cuda_event) if event_after_search is not None else None, _stream()))

    def locate_offsets(self, rec: torch.Tensor, nq: int, hit_offsets: torch.Tensor, max_hits: int = 0,
                       compact: torch.Tensor = None) -> None:
        """max_hits != 0: queries with more occurrences are counted but get no hit slots"""
        if compact is not None:
            _lib.check(self.lib.gdx_locate_many_offsets_compact_dev(self.h, _ptr(rec), _ptr(compact), nq, max_hits,
                                                                    _ptr(hit_offsets), _stream()))
            return
        _lib.check(self.lib.gdx_locate_many_offsets_capped_dev(self.h, _ptr(rec), nq, max_hits, _ptr(hit_offsets),
                                                               _stream()))

    def locate_hits(self, rec: torch.Tensor, nq: int, hit_offsets: torch.Tensor, total: int, hits: torch.Tensor,
                    workspace: torch.Tensor, compact: torch.Tensor = None) -> None:
        if compact is not None:
            _lib.check(self.lib.gdx_locate_many_hits_compact_dev(self.h, _ptr(rec), _ptr(compact), nq, _ptr(hit_offsets), total,
                                                                 _ptr(hits), _ptr(workspace), _stream()))
            return
        _lib.check(self.lib.gdx_locate_many_hits_dev(self.h, _ptr(rec), nq, _ptr(hit_offsets), total, _ptr(hits),
                                                     _ptr(workspace), _stream()))

    def totals_workspace_bytes(self, nq: int) -> int:
        return int(self.lib.gdx_locate_many_totals_workspace_bytes(nq))

    def locate_totals(self, rec: torch.Tensor, nq: int, scan_ws: torch.Tensor, totals: torch.Tensor, max_hits: int = 0,
                      compact: torch.Tensor = None) -> None:
        """gdx_locate_many_totals_compact_dev: totals = int64[2] (all hit slots, slots behind "see the record")"""
        _lib.check(self.lib.gdx_locate_many_totals_compact_dev(self.h, _ptr(rec), _ptr(compact) if compact is not None else None,
                                                               nq, max_hits, _ptr(scan_ws), _ptr(totals), _stream()))

    def locate_offsets_hits(self, rec: torch.Tensor, nq: int, scan_ws: torch.Tensor, hit_offsets: torch.Tensor, total: int,
                            rest: int, hits: torch.Tensor, workspace: torch.Tensor, max_hits: int = 0,
                            compact: torch.Tensor = None) -> None:
        """gdx_locate_many_offsets_hits_compact_dev: offsets + the hits the compact results answer in one pass, then the rest
        (hit_offsets of dtype int32: the narrow form, gdx_locate_many_offsets32_hits_compact_dev)"""
        call = (self.lib.gdx_locate_many_offsets32_hits_compact_dev if hit_offsets.dtype == torch.int32
                else self.lib.gdx_locate_many_offsets_hits_compact_dev)
        _lib.check(call(
            self.h, _ptr(rec), _ptr(compact) if compact is not None else None, nq, max_hits, _ptr(scan_ws), _ptr(hit_offsets),
            total, rest, _ptr(hits), _ptr(workspace) if workspace is not None else None, _stream()))

    def unpack_records(self, rec: torch.Tensor, nq: int, counts=None, status=None, compact=None) -> None:
        if compact is not None:
            _lib.check(self.lib.gdx_locate_many_unpack_compact_dev(self.h, _ptr(rec), _ptr(compact), nq,
                                                                   _ptr(counts) if counts is not None else None,
                                                                   _ptr(status) if status is not None else None, _stream()))
            return
        _lib.check(self.lib.gdx_locate_many_unpack_dev(self.h, _ptr(rec), nq,
                                                       _ptr(counts) if counts is not None else None,
                                                       _ptr(status) if status is not None else None, _stream()))

    def compact_split_hits(self, compact: torch.Tensor, nq: int, text_ids: torch.Tensor, positions: torch.Tensor) -> None:
        """gdx_compact_split_hits_dev: compact results -> uint8 text ids + int32 positions in the text (-1 none, -2 see the
        record); what the root of a multi-GPU gather turns a received shard into"""
        _lib.check(self.lib.gdx_compact_split_hits_dev(self.h, _ptr(compact), nq, _ptr(text_ids), _ptr(positions), _stream()))

    def wire_pack_workspace_bytes(self, nq: int) -> int:
        return int(self.lib.gdx_wire_pack_workspace_bytes(nq))

    def wire_pack(self, compact: torch.Tensor, hit_offsets: torch.Tensor, hits: torch.Tensor, nq: int, v: dict,
                  workspace: torch.Tensor) -> None:
        """gdx_wire_pack_dev: a located shard into its "found bitmap" wire form; v = dist.WireLayout.views(buffer)"""
        _lib.check(self.lib.gdx_wire_pack_dev(
            self.h, _ptr(compact), _ptr(hit_offsets), 32 if hit_offsets.dtype == torch.int32 else 64, _ptr(hits), nq,
            _ptr(v["bitmap"]), _ptr(v["tile_found"]), _ptr(v["found_pos"]), v["found_pos"].numel(), _ptr(v["exc_q"]),
            _ptr(v["exc_cnt"]), v["exc_q"].numel(), _ptr(v["exc_ids"]), _ptr(v["exc_pos"]), v["exc_ids"].numel(), _ptr(v["meta"]),
            _ptr(workspace), _stream()))

    def wire_split(self, v: dict, nq: int, text_ids: torch.Tensor, positions: torch.Tensor) -> None:
        """gdx_wire_split_dev: a received shard -> uint8 text ids + int32 positions (-1 none, -2 exception)"""
        _lib.check(self.lib.gdx_wire_split_dev(self.h, _ptr(v["bitmap"]), _ptr(v["tile_found"]), _ptr(v["found_pos"]),
                                               v["found_pos"].numel(), nq, _ptr(v["exc_q"]), _ptr(v["meta"]), v["exc_q"].numel(),
                                               _ptr(text_ids), _ptr(positions), _stream()))

    def compact_exceptions(self, compact: torch.Tensor, nq: int, queries: torch.Tensor, n: torch.Tensor) -> None:
        """gdx_compact_exceptions_dev: the queries that say "see the record" into `queries` (int32 / uint32 view, unordered, as
        many as it holds); n (int64[1]) = how many there are"""
        _lib.check(self.lib.gdx_compact_exceptions_dev(self.h, _ptr(compact), nq, _ptr(queries), queries.numel(), _ptr(n),
                                                       _stream()))

    # ---- batched cursor extension by strings (gdx_cursor_extend_front_strings_dev) ------------------------
    def cursor_extend_strings(self, start, end, qbuf, qbeg, qend, m, status=None, active_in=None, n_active_in=None,
                              active_out=None, n_active_out=None) -> None:
        opt = lambda t: _ptr(t) if t is not None else None  # noqa: E731
        _lib.check(self.lib.gdx_cursor_extend_front_strings_dev(self.h, _ptr(start), _ptr(end), _ptr(qbuf), _ptr(qbeg),
                                                                _ptr(qend), m, opt(status), opt(active_in),
                                                                opt(n_active_in), opt(active_out), opt(n_active_out),
                                                                _stream()))

    def cursor_extend_chunk(self, start, end, qbuf, qoff, m, chunk_symbols, chunk_index, status=None, active_in=None,
                            n_active_in=None, active_out=None, n_active_out=None) -> None:
        """gdx_cursor_extend_front_chunk_dev: chunk `chunk_index` (from the right) of every query, no edge arrays."""
        opt = lambda t: _ptr(t) if t is not None else None  # noqa: E731
        _lib.check(self.lib.gdx_cursor_extend_front_chunk_dev(self.h, _ptr(start), _ptr(end), _ptr(qbuf), _ptr(qoff), m,
                                                              int(chunk_symbols), int(chunk_index), opt(status),
                                                              opt(active_in), opt(n_active_in), opt(active_out),
                                                              opt(n_active_out), _stream()))

    # ---- longest matching suffix segments (gdx_suffix_segments_many_dev) -----------------------------------
    def alloc_segments(self, nq: int, max_segments: int):
        d = self.dev
        slots = max(nq * max_segments, 1)
        return {
            "n_segments": torch.empty(max(nq, 1), dtype=torch.int32, device=d),
            "remaining": torch.empty(max(nq, 1), dtype=torch.int32, device=d),
            "length": torch.empty(slots, dtype=torch.int32, device=d),
            "start": torch.empty(slots, dtype=torch.int32, device=d),
            "end": torch.empty(slots, dtype=torch.int32, device=d),
            "status": torch.empty(max(nq, 1), dtype=torch.uint8, device=d),
        }

    def suffix_segments(self, q: DeviceQueries, max_segments: int, out, lf_only: bool = False) -> None:
        """One fused launch: per query its longest matching suffix segments into `out` (alloc_segments; u32 values in int32
        tensors, segment j of query i in slot i * max_segments + j).  Plain batches only."""
        if q.packed or q.uniform_len:
            raise ValueError("suffix_segments(): plain batches only")
        _lib.check(self.lib.gdx_suffix_segments_many_dev(
            self.h, _ptr(q.qbuf), _ptr(q.qoff), q.nq, int(max_segments), _lib.GDX_SEGMENTS_LF_ONLY if lf_only else 0,
            _ptr(out["n_segments"]), _ptr(out["remaining"]), _ptr(out["length"]), _ptr(out["start"]), _ptr(out["end"]),
            _ptr(out["status"]) if out.get("status") is not None else None, _stream()))

    # ---- super-maximal exact matches (gdx_smems_many_dev) ---------------------------------------------------
    def alloc_smems(self, nq: int, max_smems: int):
        d = self.dev
        slots = max(nq * max_smems, 1)
        out = {name: torch.empty(max(nq, 1), dtype=torch.int32, device=d) for name in ("n_smems", "remaining")}
        out.update({name: torch.empty(slots, dtype=torch.int32, device=d) for name in ("begin", "length", "start", "end")})
        out["status"] = torch.empty(max(nq, 1), dtype=torch.uint8, device=d)
        return out

    def smems(self, q: DeviceQueries, reversed_index, max_smems: int, min_length: int, out) -> None:
        """One fused launch: per query its super-maximal exact matches into `out` (alloc_smems; u32 values in int32 tensors,
        SMEM j of query i in slot i * max_smems + j).  reversed_index: the DeviceEngine or FmIndex of the same texts, each
        reversed.  Plain batches only."""
        if q.packed or q.uniform_len:
            raise ValueError("smems(): plain batches only")
        r = reversed_index.h if isinstance(reversed_index, DeviceEngine) else reversed_index._h
        _lib.check(self.lib.gdx_smems_many_dev(
            self.h, r, _ptr(q.qbuf), _ptr(q.qoff), q.nq, int(max_smems), int(min_length), _ptr(out["n_smems"]),
            _ptr(out["remaining"]), _ptr(out["begin"]), _ptr(out["length"]), _ptr(out["start"]), _ptr(out["end"]),
            _ptr(out["status"]) if out.get("status") is not None else None, _stream()))

    def _alloc_u32(self, *columns, hits=None):
        """{name: int32[max(n, 1)]} for every (n, names) of columns, and int32[max(n, 1), 2] under hits = (n, name)"""
        out = {name: torch.empty(max(n, 1), dtype=torch.int32, device=self.dev) for n, names in columns for name in names}
        if hits is not None:
            out[hits[1]] = torch.empty((max(hits[0], 1), 2), dtype=torch.int32, device=self.dev)
        return out

    # ---- seed-hit candidates (gdx_seed_candidates_many_dev) --------------------------------------------------
    def alloc_seed_candidates(self, nq: int, max_candidates: int):
        slots = nq * max_candidates
        out = self._alloc_u32((nq, ("n_candidates", "n_groups", "n_skipped")), (slots, ("cand_query", "cand_begin", "cand_weight")),
                              hits=(slots, "cand_hits"))
        out["status"] = torch.empty(max(nq, 1), dtype=torch.uint8, device=self.dev)
        return out

    def seed_candidates(self, seeds: dict, nq: int, max_seeds: int, max_occ: int, band: int, max_candidates: int, out: dict = None):
        """One launch: the seed slots of nq queries -> ranked, de-duplicated candidates in `out` (alloc_seed_candidates; made
        here when None) -> out.  seeds: the `out` dict of smems() as it is ("n_smems", "begin", "length", "start", "end";
        max_seeds = its max_smems), or one with "n_seeds" / "n_segments" in its place.  out["cand_query"], ["cand_begin"] and
        ["cand_hits"] go straight into hamming() / edit_distance() / align() with all nq * max_candidates slots: an unused slot
        has cand_query -1 (GDX_CAND_NONE) and gets the verify call's INVALID marker."""
        n_seeds = next(seeds[name] for name in ("n_seeds", "n_smems", "n_segments") if seeds.get(name) is not None)
        if out is None:
            out = self.alloc_seed_candidates(nq, int(max_candidates))
        _lib.check(self.lib.gdx_seed_candidates_many_dev(
            self.h, int(nq), int(max_seeds), _ptr(n_seeds), _ptr(seeds["begin"]), _ptr(seeds["length"]), _ptr(seeds["start"]),
            _ptr(seeds["end"]), int(max_occ), int(band), int(max_candidates), _ptr(out["n_candidates"]), _ptr(out["n_groups"]),
            _ptr(out["n_skipped"]), _ptr(out["cand_query"]), _ptr(out["cand_begin"]), _ptr(out["cand_hits"]),
            _ptr(out["cand_weight"]), _ptr(out["status"]) if out.get("status") is not None else None, _stream()))
        return out

    # ---- Hamming verification of located seeds (gdx_hamming_many_dev) ---------------------------------------
    def hamming(self, q: DeviceQueries, cand_query: torch.Tensor, cand_begin: torch.Tensor, cand_hits: torch.Tensor,
                max_mismatches: int, out: torch.Tensor = None) -> torch.Tensor:
        """One launch: per candidate the mismatches of the whole query against its text on the seed's diagonal, capped at
        max_mismatches + 1, into `out` (u32 values in an int32 tensor of m entries; made here when None).  q in any of the four
        forms (a batch made by with_strands goes straight in); cand_query / cand_begin: int32[m] holding u32 values; cand_hits:
        int32[m, 2] = (text_id, position), the hits tensor of locate().  A candidate whose query or text id is out of range
        gets -1 (GDX_HAMMING_INVALID)."""
        m = _check_candidates(cand_query, cand_begin, cand_hits)
        if out is None:
            out = torch.empty(max(m, 1), dtype=torch.int32, device=self.dev)
        lay, qoff = q.layout()
        _lib.check(self.lib.gdx_hamming_many_dev(self.h, _ptr(q.qbuf), qoff, q.nq, _layout_arg(lay),
                                                 _ptr(cand_query), _ptr(cand_begin), _ptr(cand_hits), m, int(max_mismatches),
                                                 _ptr(out), _stream()))
        return out

    # ---- edit-distance verification of located seeds (gdx_edit_distance_many_dev) ----------------------------
    def edit_distance(self, q: DeviceQueries, cand_query: torch.Tensor, cand_begin: torch.Tensor, cand_hits: torch.Tensor,
                      max_edits: int, out_dist: torch.Tensor = None, out_end: torch.Tensor = None, want_end: bool = True):
        """One launch: per candidate of hamming() the infix edit distance of the whole query (at most 256 symbols) against its
        text within max_edits of the seed's diagonal, capped at max_edits + 1, into out_dist, and the exclusive end of the
        leftmost best alignment into out_end (u32 values in int32 tensors of m entries; made here when None; want_end=False
        with out_end None passes NULL).  -> (out_dist, out_end).  Out-of-range candidates get -1 (GDX_EDIT_INVALID), longer
        queries -2 (GDX_EDIT_TOO_LONG); out_end is -1 (GDX_EDIT_NO_END) wherever out_dist is not a distance <= max_edits."""
        m = _check_candidates(cand_query, cand_begin, cand_hits)
        if out_dist is None:
            out_dist = torch.empty(max(m, 1), dtype=torch.int32, device=self.dev)
        if out_end is None and want_end:
            out_end = torch.empty(max(m, 1), dtype=torch.int32, device=self.dev)
        lay, qoff = q.layout()
        _lib.check(self.lib.gdx_edit_distance_many_dev(self.h, _ptr(q.qbuf), qoff, q.nq, _layout_arg(lay),
                                                       _ptr(cand_query), _ptr(cand_begin), _ptr(cand_hits), m, int(max_edits),
                                                       _ptr(out_dist), _ptr(out_end) if out_end is not None else None, _stream()))
        return out_dist, out_end

    # ---- alignment traceback of verified seed hits (gdx_align_many_dev) ---------------------------------------
    def align_workspace_bytes(self, q: DeviceQueries, m: int, max_edits: int):
        """(least, best): the workspace sizes of align() for m candidates of q's layout -- the least that works and the one
        beyond which more memory does not help.  Launches nothing."""
        lay, _ = q.layout()
        sizes = (C.c_uint64 * 2)()
        _lib.check(self.lib.gdx_align_many_dev(self.h, None, None, 0, _layout_arg(lay), None, None, None,
                                               int(m), int(max_edits), None, None, None, None, None, None, 0, sizes, None))
        return int(sizes[0]), int(sizes[1])

    def align(self, q: DeviceQueries, cand_query: torch.Tensor, cand_begin: torch.Tensor, cand_hits: torch.Tensor, max_edits: int,
              out: dict = None, workspace: torch.Tensor = None):
        """One launch: per candidate of edit_distance() the distance and end it gives, where the canonical best alignment begins
        and its run-length CIGAR.  -> {"dist", "begin", "end", "n_cigar": int32[m], "cigar": int32[m, 2 max_edits + 1]} (u32
        values; tensors of `out` are used where given, the others made here).  cigar words are run_length << 4 | GDX_CIGAR_*;
        the words of a row from n_cigar on are not written.  begin and end are -1 (GDX_EDIT_NO_END) and n_cigar 0 wherever dist
        is not a distance <= max_edits.  workspace: a contiguous 16-byte aligned tensor of at least align_workspace_bytes()[0]
        bytes, scratch for the call; None takes the best size from torch's allocator.  The result does not depend on its size."""
        m = _check_candidates(cand_query, cand_begin, cand_hits)
        if workspace is None:
            workspace = torch.empty(self.align_workspace_bytes(q, m, max_edits)[1], dtype=torch.uint8, device=self.dev)
        if not workspace.is_contiguous():
            raise ValueError("the workspace is a contiguous tensor")
        out = dict(out) if out else {}
        for name in ("dist", "begin", "end", "n_cigar"):
            if out.get(name) is None:
                out[name] = torch.empty(max(m, 1), dtype=torch.int32, device=self.dev)
        if out.get("cigar") is None:
            out["cigar"] = torch.empty((max(m, 1), 2 * int(max_edits) + 1), dtype=torch.int32, device=self.dev)
        lay, qoff = q.layout()
        _lib.check(self.lib.gdx_align_many_dev(self.h, _ptr(q.qbuf), qoff, q.nq, _layout_arg(lay),
                                               _ptr(cand_query), _ptr(cand_begin), _ptr(cand_hits), m, int(max_edits),
                                               _ptr(out["dist"]), _ptr(out["begin"]), _ptr(out["end"]), _ptr(out["n_cigar"]),
                                               _ptr(out["cigar"]), _ptr(workspace), workspace.numel() * workspace.element_size(),
                                               None, _stream()))
        return out

    # ---- soft clipping (gdx_soft_clip_many_dev) -----------------------------------------------------------------
    def soft_clip(self, aligned: dict, max_edits: int, scoring, out: dict = None):
        """One launch: per candidate of align() the best-scoring contiguous part of its runs, S runs (op 4) in place of what lies
        outside, begin and end moved inwards.  aligned: the dict of align() as it is; scoring = (match, mismatch, gap_open,
        gap_extend) or with min_score as a fifth.  -> {"score", "dist", "begin", "end", "clip_left", "clip_right", "n_cigar":
        int32[m], "cigar": int32[m, 2 max_edits + 1], "status": uint8[m]} (tensors of `out` are used where given, the others
        made here; the words of a cigar row from n_cigar on are not written).  score is signed: the best score, GDX_CLIP_NO_SCORE
        for a candidate without an alignment.  A candidate whose best score is below max(1, min_score) is clipped away and looks
        like an unmapped one: end -1, n_cigar 0, dist max_edits + 1.  status 1 (GDX_CLIP_BAD_CIGAR): runs that fail the check."""
        match, mismatch, gap_open, gap_extend, *rest = (int(x) for x in scoring)
        min_score = rest[0] if rest else 0
        m, stride = int(aligned["dist"].numel()), 2 * int(max_edits) + 1
        if any(aligned[name].numel() != m for name in ("begin", "end", "n_cigar")) or aligned["cigar"].numel() != m * stride:
            raise ValueError("aligned holds the outputs of align() with this max_edits")
        if not all(aligned[name].is_contiguous() for name in ("dist", "begin", "end", "n_cigar", "cigar")):
            raise ValueError("the tensors of aligned are contiguous")
        out = dict(out) if out else {}
        for name in ("score", "dist", "begin", "end", "clip_left", "clip_right", "n_cigar"):
            if out.get(name) is None:
                out[name] = torch.empty(m, dtype=torch.int32, device=self.dev)
        if out.get("cigar") is None:
            out["cigar"] = torch.empty((m, stride), dtype=torch.int32, device=self.dev)
        if "status" not in out:
            out["status"] = torch.empty(m, dtype=torch.uint8, device=self.dev)
        _lib.check(self.lib.gdx_soft_clip_many_dev(
            self.h, m, int(max_edits), match, mismatch, gap_open, gap_extend, min_score, _ptr(aligned["dist"]), _ptr(aligned["begin"]),
            _ptr(aligned["end"]), _ptr(aligned["n_cigar"]), _ptr(aligned["cigar"]), _ptr(out["score"]), _ptr(out["dist"]),
            _ptr(out["begin"]), _ptr(out["end"]), _ptr(out["clip_left"]), _ptr(out["clip_right"]), _ptr(out["n_cigar"]),
            _ptr(out["cigar"]), _ptr(out["status"]) if out["status"] is not None else None, _stream()))
        return out

    def _clipped(self, result: dict, aligned: dict, max_edits: int, clip) -> dict:
        """map_reads / map_pairs with clip given: the clipped alignment in the place of the traced one"""
        c = self.soft_clip(aligned, max_edits, clip)
        # (where nothing was aligned the stage's own dist stays; elsewhere the edits that are left, k + 1 for a read clipped away)
        dist = torch.where(aligned["end"] == -1, result["dist"][:c["dist"].numel()], c["dist"])
        return {**result, "edit_dist": result["dist"], "dist": dist, "begin": c["begin"], "end": c["end"], "n_cigar": c["n_cigar"],
                "cigar": c["cigar"], "score": c["score"], "clip_left": c["clip_left"], "clip_right": c["clip_right"]}

    # ---- best hit per read (gdx_best_hits_many_dev) -----------------------------------------------------------
    def alloc_best_hits(self, n_groups: int):
        return self._alloc_u32((n_groups, ("best_slot", "best_dist", "sub_dist", "n_live", "n_best", "mapq", "win_query", "win_begin")),
                               hits=(n_groups, "win_hits"))

    def best_hits(self, cands: dict, dist: torch.Tensor, end, n_groups: int, group_slots: int, max_dist: int, out: dict = None):
        """One launch: every group of group_slots consecutive candidate slots and the distances a verify call gave them -> the
        group's best hit in `out` (alloc_best_hits; made here when None) -> out.  cands: the `out` dict of seed_candidates() as
        it is ("cand_query", "cand_begin", "cand_hits"); dist / end: what edit_distance() returned for all its slots, end None
        after hamming().  group_slots = max_candidates makes a group a query; after with_strands(mode="both") group_slots =
        2 * max_candidates makes it a read.  out["win_query"], ["win_begin"] and ["win_hits"] go straight into align() /
        edit_distance() / hamming() as n_groups candidates: an unmapped read (best_slot -1, GDX_BEST_NONE; mapq 255) has
        win_query -1 (GDX_CAND_NONE) and gets the verify call's INVALID marker."""
        n_groups, group_slots = int(n_groups), int(group_slots)
        _check_slots(cands, dist, end, n_groups * group_slots, "n_groups * group_slots")
        if out is None:
            out = self.alloc_best_hits(n_groups)
        _lib.check(self.lib.gdx_best_hits_many_dev(
            self.h, n_groups, group_slots, _ptr(cands["cand_query"]), _ptr(cands["cand_begin"]), _ptr(cands["cand_hits"]), _ptr(dist),
            _ptr(end) if end is not None else None, int(max_dist), _ptr(out["best_slot"]), _ptr(out["best_dist"]),
            _ptr(out["sub_dist"]), _ptr(out["n_live"]), _ptr(out["n_best"]), _ptr(out["mapq"]), _ptr(out["win_query"]),
            _ptr(out["win_begin"]), _ptr(out["win_hits"]), _stream()))
        return out

    def map_reads(self, q: DeviceQueries, reversed_index, *, max_smems: int, min_length: int, max_occ: int, band: int,
                  max_candidates: int, max_edits: int, both_strands: bool = True, clip=None) -> dict:
        """The seed-and-verify chain on resident reads, every stage reading what the one before left in HBM: with_strands ->
        smems -> seed_candidates -> edit_distance -> best_hits -> align over the winners, one slot per read.  q: a plain batch;
        reversed_index as in smems().
        -> per-read tensors (u32 values in int32): "strand" (1 = the reverse complement; 0 without both_strands), "text_id",
        "begin", "end" (the alignment's text range), "dist", "sub_dist", "n_best", "mapq", "n_cigar" and "cigar" (int32[reads,
        2 max_edits + 1]).  An unmapped read has mapq 255 (GDX_BEST_MAPQ_NONE), n_best 0, n_cigar 0, begin and end -1, dist and
        sub_dist max_edits + 1; its strand and text_id say nothing.  The align workspace is sized for one candidate per read.
        No result crosses to the host in between (with_strands reads the batch's symbol count once to size its output).
        clip = (match, mismatch, gap_open, gap_extend, min_score) puts soft_clip() behind align: "begin", "end", "n_cigar", "cigar"
        and "dist" are then the clipped ones, and "score", "clip_left", "clip_right" and "edit_dist" (what "dist" is without
        clip) are added.  A read that is clipped away looks like an unmapped one (end -1, n_cigar 0, dist max_edits + 1), and
        sam_records() writes it as unmapped.  A caller who expects junk tails raises max_edits."""
        n_reads = q.nq
        sq = q.with_strands(self.index, "both") if both_strands else q
        nq, mc = sq.nq, int(max_candidates)
        seeds = self.alloc_smems(nq, int(max_smems))
        self.smems(sq, reversed_index, int(max_smems), int(min_length), seeds)
        cands = self.seed_candidates(seeds, nq, int(max_smems), max_occ, band, mc)
        dist, end = self.edit_distance(sq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], max_edits)
        best = self.best_hits(cands, dist, end, n_reads, mc * (2 if both_strands else 1), max_edits)
        aligned = self.align(sq, best["win_query"][:n_reads], best["win_begin"][:n_reads], best["win_hits"][:n_reads], max_edits)
        strand = best["win_query"] & 1 if both_strands else torch.zeros_like(best["win_query"])  # (win_query = 2 read + strand)
        result = {"strand": strand, "text_id": best["win_hits"][:, 0], "begin": aligned["begin"], "end": aligned["end"],
                  "dist": best["best_dist"], "sub_dist": best["sub_dist"], "n_best": best["n_best"], "mapq": best["mapq"],
                  "n_cigar": aligned["n_cigar"], "cigar": aligned["cigar"]}
        return result if clip is None else self._clipped(result, aligned, max_edits, clip)

    # ---- paired-end pairing (gdx_pair_hits_many_dev) -----------------------------------------------------------
    def alloc_pair_hits(self, n_pairs: int):
        n_mates = 2 * max(n_pairs, 1)
        return self._alloc_u32((n_pairs, ("n_proper", "n_best", "pair_dist", "sub_dist", "mapq", "pair_span")),
                               (n_mates, ("mate_slot", "mate_dist", "win_query", "win_begin")), hits=(n_mates, "win_hits"))

    def pair_hits(self, cands: dict, dist: torch.Tensor, end, n_pairs: int, mate_slots: int, max_dist: int, min_insert: int,
                  max_insert: int, out: dict = None):
        """One launch: the slots are 2 * n_pairs mates of mate_slots consecutive candidate slots, mates 2p and 2p + 1 making pair
        p; per pair the best combination of one live slot of each mate on one text, on opposite strands and with min_insert <=
        span <= max_insert, in `out` (alloc_pair_hits; made here when None) -> out.  cands, dist, end as best_hits() takes them;
        after with_strands(mode="both") on a batch with the mates interleaved mate_slots = 2 * max_candidates.  Per pair
        "n_proper", "n_best", "pair_dist", "sub_dist", "mapq" (255, GDX_PAIR_MAPQ_NONE, without a proper combination) and
        "pair_span"; per mate "mate_slot" (-1, GDX_PAIR_NONE, without a live slot), "mate_dist" and the winner "win_query",
        "win_begin", "win_hits" -- the pair's slot, or the mate's single-end best when the pair has no proper combination --
        which go straight into align() as 2 * n_pairs candidates."""
        n_pairs, mate_slots = int(n_pairs), int(mate_slots)
        _check_slots(cands, dist, end, 2 * n_pairs * mate_slots, "2 * n_pairs * mate_slots")
        if out is None:
            out = self.alloc_pair_hits(n_pairs)
        _lib.check(self.lib.gdx_pair_hits_many_dev(
            self.h, n_pairs, mate_slots, _ptr(cands["cand_query"]), _ptr(cands["cand_begin"]), _ptr(cands["cand_hits"]), _ptr(dist),
            _ptr(end) if end is not None else None, int(max_dist), int(min_insert), int(max_insert), _ptr(out["n_proper"]),
            _ptr(out["n_best"]), _ptr(out["pair_dist"]), _ptr(out["sub_dist"]), _ptr(out["mapq"]), _ptr(out["pair_span"]),
            _ptr(out["mate_slot"]), _ptr(out["mate_dist"]), _ptr(out["win_query"]), _ptr(out["win_begin"]), _ptr(out["win_hits"]),
            _stream()))
        return out

    # ---- mate rescue (gdx_mate_rescue_many_dev) -------------------------------------------------------------------
    def alloc_mate_rescue(self, n_pairs: int):
        n_mates = 2 * max(n_pairs, 1)
        return self._alloc_u32((n_mates, ("resc_dist", "resc_end", "win_query", "win_begin")),
                               (n_pairs, ("resc_mate", "resc_pair_dist", "resc_span")), hits=(n_mates, "win_hits"))

    def mate_rescue(self, q: DeviceQueries, end: torch.Tensor, pairs: dict, n_pairs: int, mate_slots: int, max_edits: int,
                    min_insert: int, max_insert: int, out: dict = None):
        """One launch: for every pair without a proper combination each placed mate is the anchor from which the other mate's
        opposite strand is searched in the window of the text that min_insert <= span <= max_insert implies, within max_edits
        (at most 256) edits; max_insert - min_insert is at most 4096 (GDX_RESCUE_MAX_SPREAD).  q: the batch with_strands("both")
        made of the interleaved mates, 4 * n_pairs queries in any form; end: what edit_distance() returned for all 2 * n_pairs *
        mate_slots slots; pairs: the `out` dict of pair_hits() as it is.  Results in `out` (alloc_mate_rescue; made here when
        None) -> out.  Per mate "resc_dist" (-3, GDX_RESCUE_NOT_TRIED, without an attempt; max_edits + 1 when nothing was found)
        and "resc_end"; per pair "resc_mate" (the rescued mate, -1 = GDX_RESCUE_NONE), "resc_pair_dist" and "resc_span"; and the
        merged winners "win_query", "win_begin", "win_hits", which go into align() in place of those of pair_hits()."""
        n_pairs, mate_slots = int(n_pairs), int(mate_slots)
        if end is None or end.numel() < 2 * n_pairs * mate_slots:
            raise ValueError("end holds 2 * n_pairs * mate_slots slots")
        if any(pairs[name].numel() < n for n, names in ((n_pairs, ("n_proper",)), (2 * n_pairs, ("mate_slot", "mate_dist", "win_query",
               "win_begin")), (4 * n_pairs, ("win_hits",))) for name in names):
            raise ValueError("pairs holds the outputs of pair_hits() for n_pairs pairs")
        if out is None:
            out = self.alloc_mate_rescue(n_pairs)
        lay, qoff = q.layout()
        _lib.check(self.lib.gdx_mate_rescue_many_dev(
            self.h, _ptr(q.qbuf), qoff, q.nq, _layout_arg(lay), n_pairs, mate_slots, _ptr(end), _ptr(pairs["n_proper"]),
            _ptr(pairs["mate_slot"]), _ptr(pairs["mate_dist"]), _ptr(pairs["win_query"]), _ptr(pairs["win_begin"]),
            _ptr(pairs["win_hits"]), int(max_edits), int(min_insert), int(max_insert), _ptr(out["resc_dist"]), _ptr(out["resc_end"]),
            _ptr(out["resc_mate"]), _ptr(out["resc_pair_dist"]), _ptr(out["resc_span"]), _ptr(out["win_query"]),
            _ptr(out["win_begin"]), _ptr(out["win_hits"]), _stream()))
        return out

    # ---- SAM records (gdx_sam_records_many_dev) --------------------------------------------------------------------
    def sam_workspace_bytes(self, n_reads: int) -> int:
        return int(self.lib.gdx_sam_workspace_bytes(int(n_reads)))

    def sam_record_bound(self, max_read_len: int, max_name_len: int, max_text_name_len: int, max_edits: int) -> int:
        """an upper bound of one record's bytes (gdx_sam_record_bound): sizes `out` without a look at the device"""
        return int(self.lib.gdx_sam_record_bound(int(max_read_len), int(max_name_len), int(max_text_name_len), int(max_edits)))

    def sam_records_dev(self, q: DeviceQueries, n_reads: int, strands: int, mode: int, max_edits: int, win_query, win_hits, dist,
                        begin, end, n_cigar, cigar, mapq, rec_off: torch.Tensor, out: torch.Tensor = None, *, proper=None,
                        names=None, name_off=None, text_names=None, text_name_off=None, dense_to_io: bytes = None,
                        status: torch.Tensor = None, workspace: torch.Tensor = None, out_capacity: int = None):
        """gdx_sam_records_many_dev as it is: lengths, scan, offsets and -- with `out` -- the fill, on the current stream, without a
        synchronisation.  rec_off: int64[n_reads + 1]; out: uint8 or None (the sizing call); out_capacity: out.numel() unless
        given.  workspace: at least sam_workspace_bytes(n_reads) bytes, made here when None."""
        n_reads = int(n_reads)
        if workspace is None:
            workspace = torch.empty(self.sam_workspace_bytes(n_reads), dtype=torch.uint8, device=self.dev)
        lay, qoff = q.layout()
        a = _lib.SamInputs()
        opt = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        a.qbuf, a.qoff, a.nq, a.layout = q.qbuf.data_ptr(), qoff.value, q.nq, (C.pointer(lay) if lay is not None else None)
        a.n_reads, a.strands, a.mode, a.max_edits = n_reads, int(strands), int(mode), int(max_edits)
        a.win_query, a.win_hits, a.dist, a.begin, a.end = opt(win_query), opt(win_hits), opt(dist), opt(begin), opt(end)
        a.n_cigar, a.cigar, a.mapq, a.proper = opt(n_cigar), opt(cigar), opt(mapq), opt(proper)
        a.names, a.name_off, a.text_names, a.text_name_off = opt(names), opt(name_off), opt(text_names), opt(text_name_off)
        table = (C.c_uint8 * 16).from_buffer_copy(bytes(dense_to_io)) if dense_to_io is not None else None
        a.dense_to_io = C.addressof(table) if table is not None else None
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
        a.rec_off, a.out, a.status = opt(rec_off), opt(out), opt(status)
        a.out_capacity = int(out_capacity) if out_capacity is not None else (out.numel() if out is not None else 0)
        _lib.check(self.lib.gdx_sam_records_many_dev(self.h, C.byref(a), _stream()))

    def _name_table(self, names, n: int, what: str):
        """names: a sequence of n str / bytes -> (uint8 tensor, int64 offsets tensor) on the device"""
        names = [x.encode() if isinstance(x, str) else bytes(x) for x in names]
        if len(names) != n:
            raise ValueError(f"{what}: {len(names)} names for {n}")
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(x) for x in names], out=off[1:])
        buf = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8)  # (never empty)
        return torch.from_numpy(buf.copy()).to(self.dev), torch.from_numpy(off).to(self.dev)

    def sam_inputs(self, q_strands: DeviceQueries, result: dict, *, mode: str, names=None, text_names=None, dense_to_io: bytes = None):
        """what sam_records() hands to sam_records_dev() for a result of map_reads / map_pairs: (args up to rec_off, keyword
        arguments, n_reads) -- sam_records_dev(*args, out, out_capacity=..., **kw).  Tools that time the call use it as it is."""
        if mode not in ("single", "paired"):
            raise ValueError("mode is 'single' or 'paired'")
        n = int(result["begin"].numel())
        strands = q_strands.nq // n if n else 1
        if strands not in (1, 2) or strands * n != q_strands.nq:
            raise ValueError("q_strands holds one or two queries per read of the result")
        cigar = result["cigar"]
        max_edits = (int(cigar.shape[1]) - 1) // 2
        reads = torch.arange(max(n, 1), dtype=torch.int64, device=self.dev)[:n]
        has = result["end"][:n] != -1
        win_query = torch.where(has, reads * strands + (result["strand"][:n].to(torch.int64) & (strands - 1)),
                                torch.full_like(reads, 0xFFFFFFFF)).to(torch.int32)  # (wraps to the u32 pattern)
        win_hits = torch.stack([result["text_id"][:n], torch.zeros_like(result["text_id"][:n])], dim=1).contiguous()
        mapq, proper = result["mapq"][:n], None
        if mode == "paired":
            proper = result["n_proper"] != 0
            if "resc_mate" in result:
                proper = proper | (result["resc_mate"] != -1)
            proper = proper.to(torch.int32).contiguous()
            pm = result["pair_mapq"].repeat_interleave(2)
            mapq = torch.where(proper.repeat_interleave(2) != 0, pm, mapq)
        d_names = self._name_table(names, n, "names") if names is not None else (None, None)
        d_tnames = self._name_table(text_names, self.index.num_texts(), "text_names") if text_names is not None else (None, None)
        rec_off = torch.empty(n + 1, dtype=torch.int64, device=self.dev)
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=self.dev)
        workspace = torch.empty(self.sam_workspace_bytes(n), dtype=torch.uint8, device=self.dev)
        args = (q_strands, n, strands, _lib.GDX_SAM_PAIRED if mode == "paired" else _lib.GDX_SAM_SINGLE, max_edits, win_query.contiguous(),
                win_hits, result["dist"][:n].contiguous(), result["begin"][:n].contiguous(), result["end"][:n].contiguous(),
                result["n_cigar"][:n].contiguous(), cigar.contiguous(), mapq.contiguous(), rec_off)
        kw = dict(proper=proper, names=d_names[0], name_off=d_names[1], text_names=d_tnames[0], text_name_off=d_tnames[1],
                  dense_to_io=dense_to_io, status=status, workspace=workspace)
        return args, kw, n

    def sam_records(self, q_strands: DeviceQueries, result: dict, *, mode: str, names=None, text_names=None, sizing="exact",
                    dense_to_io: bytes = None):
        """The SAM records of a batch that map_reads() / map_pairs() has mapped, made on the device.  q_strands: the batch the
        alignment ran over -- q.with_strands(index, "both") of the mapped batch, or the batch itself when it was mapped with
        both_strands=False; result: the dict of map_reads (mode "single") or map_pairs (mode "paired"), as it is.  The winners'
        query numbers are rebuilt on the device from "strand" and the read number (a read with end -1 has none); a mate of a
        proper pair ("n_proper" != 0, or rescued) gets the pair's "pair_mapq", every other read its own "mapq".
        names / text_names: one str or bytes per read / per text, or None for numbers.  sizing: "exact" runs the sizing call and
        reads the total once (one synchronisation); a number is the capacity of `out` in bytes, taken as it is (no
        synchronisation; records that do not fit whole are left out -- sam_record_bound() gives a safe size).
        -> (out: uint8 tensor, rec_off: int64[n_reads + 1], status: uint8[n_reads]); record r is out[rec_off[r] : rec_off[r + 1]]."""
        args, kw, n = self.sam_inputs(q_strands, result, mode=mode, names=names, text_names=text_names, dense_to_io=dense_to_io)
        rec_off, status = args[-1], kw["status"]
        if sizing == "exact":
            self.sam_records_dev(*args, None, **kw)
            capacity = int(rec_off[n].item())
        else:
            capacity = int(sizing)
        out = torch.empty(max(capacity, 1), dtype=torch.uint8, device=self.dev)
        self.sam_records_dev(*args, out, out_capacity=capacity, **kw)
        return out[:capacity], rec_off, status[:n]

    def map_pairs(self, q: DeviceQueries, reversed_index, *, max_smems: int, min_length: int, max_occ: int, band: int,
                  max_candidates: int, max_edits: int, min_insert: int, max_insert: int, rescue: bool = False, clip=None) -> dict:
        """map_reads for paired reads.  q: a plain batch with the mates interleaved, reads 2p and 2p + 1 being the mates of pair p
        (an odd q.nq raises ValueError).  with_strands("both") -> smems -> seed_candidates -> edit_distance -> pair_hits ->
        best_hits per mate (for the single-end figures) -> align over the 2 * n_pairs winners of pair_hits.
        -> per-mate tensors (u32 values in int32, index 2p + s): "strand", "text_id", "begin", "end", "dist" (the winner's),
        "n_cigar", "cigar" (int32[mates, 2 max_edits + 1]) and the single-end "mapq", "n_best", "sub_dist" of map_reads;
        per-pair tensors: "n_proper", "pair_n_best", "pair_dist", "pair_sub_dist", "pair_mapq" (255 without a proper
        combination), "pair_span".  A mate of a pair without a proper combination is placed as map_reads places it; an unmapped
        mate has n_cigar 0, begin and end -1 and dist max_edits + 1.  No result crosses to the host in between.
        rescue=True puts mate_rescue() between pair_hits and align, which then runs over the merged winners, and adds the per-mate
        "rescued" (1 for a mate placed from its partner, else 0) and the per-pair "resc_mate", "resc_pair_dist", "resc_span"; for
        a rescued mate "strand" and "text_id" are the rescue candidate's and "dist" is align's own distance.
        clip as in map_reads: the per-mate "begin", "end", "n_cigar", "cigar" and "dist" are the clipped ones and the per-mate
        "score", "clip_left", "clip_right" and "edit_dist" are added; the pairing itself is not done again."""
        if q.nq % 2:
            raise ValueError("map_pairs takes the mates interleaved: an even number of reads")
        n_mates, n_pairs, mc = q.nq, q.nq // 2, int(max_candidates)
        sq = q.with_strands(self.index, "both")
        seeds = self.alloc_smems(sq.nq, int(max_smems))
        self.smems(sq, reversed_index, int(max_smems), int(min_length), seeds)
        cands = self.seed_candidates(seeds, sq.nq, int(max_smems), max_occ, band, mc)
        dist, end = self.edit_distance(sq, cands["cand_query"], cands["cand_begin"], cands["cand_hits"], max_edits)
        pairs = self.pair_hits(cands, dist, end, n_pairs, 2 * mc, max_edits, min_insert, max_insert)
        single = self.best_hits(cands, dist, end, n_mates, 2 * mc, max_edits)
        win, dist_of = pairs, pairs["mate_dist"]
        if rescue:
            win = self.mate_rescue(sq, end, pairs, n_pairs, 2 * mc, max_edits, min_insert, max_insert)
        aligned = self.align(sq, win["win_query"][:n_mates], win["win_begin"][:n_mates], win["win_hits"][:n_mates], max_edits)
        per_mate = {"strand": win["win_query"] & 1, "text_id": win["win_hits"][:, 0], "begin": aligned["begin"],
                    "end": aligned["end"], "dist": dist_of, "n_cigar": aligned["n_cigar"], "cigar": aligned["cigar"],
                    "mapq": single["mapq"], "n_best": single["n_best"], "sub_dist": single["sub_dist"]}
        per_pair = {"n_proper": pairs["n_proper"], "pair_n_best": pairs["n_best"], "pair_dist": pairs["pair_dist"],
                    "pair_sub_dist": pairs["sub_dist"], "pair_mapq": pairs["mapq"], "pair_span": pairs["pair_span"]}
        if rescue:
            # mate 2p + o is rescued when resc_mate[p] == o (resc_mate is -1 without a rescue)
            mate_of = torch.arange(2 * max(n_pairs, 1), dtype=torch.int32, device=self.dev)
            rescued = (win["resc_mate"].repeat_interleave(2) == (mate_of & 1)).to(torch.int32)
            per_mate["rescued"] = rescued
            per_mate["dist"] = torch.where(rescued != 0, aligned["dist"], dist_of)
            per_pair.update({name: win[name] for name in ("resc_mate", "resc_pair_dist", "resc_span")})
        if clip is not None:
            per_mate = self._clipped(per_mate, aligned, max_edits, clip)
        # (the buffers hold at least one entry: an empty batch gets empty tensors, not that unwritten row)
        return {**{name: t[:n_mates] for name, t in per_mate.items()}, **{name: t[:n_pairs] for name, t in per_pair.items()}}

    def search_step_stats(self, q: DeviceQueries):
        """(LF steps, line fetches of all queries, fetch slots their wavefronts spent)"""
        steps = torch.zeros(3, dtype=torch.int64, device=self.dev)
        _lib.check(self.lib.gdx_search_step_stats_dev(self.h, _ptr(q.qbuf), _ptr(q.qoff), q.nq, _ptr(steps),
                                                      _stream()))
        return [int(x) for x in steps.tolist()]

    def aux_info(self) -> dict:
        """Acceleration structures of the index (gdx_index_aux_info)."""
        import ctypes

        out = (ctypes.c_uint32 * 4)()
        _lib.check(self.lib.gdx_index_aux_info(self.h, out))
        a = self.index.aux()
        return {"pair_lines": bool(out[0]), "jump_entry_bytes": int(out[1]), "top_table_depth": int(out[2]),
                "full_suffix_array": bool(out[3] & 1), "text_units": bool(out[3] & 2), "inverse_suffix_array": bool(out[3] & 4),
                "default_shape": bool(out[3] & 8),  # the library chose it: every option was left at its default
                "aux_bytes": a["aux_bytes"], "aux_budget_bytes": a["aux_budget_bytes"], "wide_permille": a["wide_permille"],
                "shrunk_by_budget": (a["wanted_jump_entry_bytes"], a["wanted_top_table_depth"])
                != (a["jump_entry_bytes"], a["top_table_depth"]),
                "seed": self.index.seed_info()}

    def search_lf_steps(self, q: DeviceQueries) -> int:
        return self.search_step_stats(q)[0]

    def locate_record_walks(self, rec, nq: int, hit_offsets, total: int, hits, workspace):
        """(walk steps executed with the records' hints, hits that walked)"""
        steps = torch.zeros(2, dtype=torch.int64, device=self.dev)
        _lib.check(self.lib.gdx_locate_many_hits_stats_dev(self.h, _ptr(rec), nq, _ptr(hit_offsets), total, _ptr(hits),
                                                           _ptr(workspace), _ptr(steps), _stream()))
        return [int(x) for x in steps.tolist()]

    def locate_walk_steps(self, out, m: int, total: int, hits: torch.Tensor, workspace: torch.Tensor) -> int:
        steps = torch.zeros(2, dtype=torch.int64, device=self.dev)
        _lib.check(self.lib.gdx_locate_step_stats_dev(self.h, _ptr(out["start"]), _ptr(out["end"]), m,
                                                      _ptr(out["hit_offsets"]), total, _ptr(hits), _ptr(workspace),
                                                      _ptr(steps), _stream()))
        return int(steps[0].item())


def measure_bandwidth(device="cuda", gib: float = 4.0, reps: int = 3):
    """Roofline denominators measured on this GPU: streaming copy and random line gathers (GB/s)."""
    lib = _lib.load()
    nbytes = int(gib * (1 << 30)) // 4096 * 4096
    src = torch.empty(nbytes, dtype=torch.uint8, device=device)
    src.random_(0, 255)
    dst = torch.empty_like(src)
    sink = torch.zeros(1, dtype=torch.int32, device=device)
    res = {}

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        best = None
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b)
            best = ms if best is None or ms < best else best
        return best / 1e3

    t = timed(lambda: _lib.check(lib.gdx_bench_stream_copy(_ptr(dst), _ptr(src), nbytes, _stream())))
    res["stream_copy_GBps"] = 2 * nbytes / t / 1e9
    t = timed(lambda: _lib.check(lib.gdx_bench_stream_read(_ptr(src), nbytes, _ptr(sink), _stream())))
    res["stream_read_GBps"] = nbytes / t / 1e9
    n_acc = 1 << 27
    names = {0: "lane", 1: "group", 2: "lane_dependent"}
    for line in (64, 128):
        for mode in (0, 1, 2):
            t = timed(lambda: _lib.check(lib.gdx_bench_random_gather(_ptr(src), nbytes // line, line, n_acc, 7, mode,
                                                                     _ptr(sink), _stream())))
            res[f"gather{line}_{names[mode]}_GBps"] = n_acc * line / t / 1e9
            res[f"gather{line}_{names[mode]}_Glines_per_s"] = n_acc / t / 1e9
    return res


def genome_like_text(total: int, dev, seed: int = 7) -> torch.Tensor:
    """A text with the repeat structure of a genome instead of i.i.d. symbols: random base sequence, then copies --
    30 % of the text is made of duplicated segments (1 k .. 2 M symbols, 0.5 % substitutions), 3 % tandem repeats
    (unit 2..60), 1 % poly-A, 2 % runs of N (assembly gaps, up to total / 100)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rng = np.random.default_rng(seed)
    text = synth_text(total, seed=seed, n_per_million=100, device=dev)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)

    def place(n_symbols, make):
        done = 0
        while done < n_symbols:
            done += make()

    def duplication():
        ln = int(min(rng.integers(1_000, 2_000_000), total // 8))
        src, dst = int(rng.integers(0, total - ln)), int(rng.integers(0, total - ln))
        seg = text[src:src + ln].clone()
        n_mut = max(1, ln // 200)
        # distinct positions: a scatter with duplicate indices has no defined winner, and the text must be the same
        # text in every run
        at = torch.unique(torch.randint(0, ln, (n_mut,), device=dev, generator=g))
        seg[at] = acgt[torch.randint(0, 4, (at.numel(),), device=dev, generator=g)]
        text[dst:dst + ln] = seg
        return ln

    def tandem():
        unit = int(rng.integers(2, 61))
        ln = int(rng.integers(unit * 5, unit * 2000))
        dst = int(rng.integers(0, total - ln))
        u = acgt[torch.randint(0, 4, (unit,), device=dev, generator=g)]
        text[dst:dst + ln] = u.repeat(ln // unit + 1)[:ln]
        return ln

    def poly_a():
        ln = int(rng.integers(20, 5000))
        dst = int(rng.integers(0, total - ln))
        text[dst:dst + ln] = ord("A")
        return ln

    def gap():
        ln = int(rng.integers(1000, max(2000, total // 100)))
        dst = int(rng.integers(0, total - ln))
        text[dst:dst + ln] = ord("N")
        return ln

    place(int(0.30 * total), duplication)
    place(int(0.03 * total), tandem)
    place(int(0.01 * total), poly_a)
    place(int(0.02 * total), gap)
    return text


def hg38_text_lengths(total: int, n_texts: int = 24):
    return split_lengths(total, n_texts)


def build_parts_from_device_text(io_text: torch.Tensor, text_lengths, alphabet: Alphabet, sa_rate=4, lookup_depth=0,
                                 max_part_symbols=0, options=None):
    """gdx_parts_build on a text that already sits in HBM: a collection beyond 2^32 - 1 symbols as several 32-bit
    indexes cut at text borders (index.PartitionedFmIndex)."""
    from .index import PartitionedFmIndex

    toff = np.zeros(len(text_lengths) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(text_lengths, dtype=np.uint64), out=toff[1:])
    torch.cuda.synchronize()
    return PartitionedFmIndex._build(_ptr(io_text), 1, toff, len(text_lengths), alphabet, sa_rate, lookup_depth,
                                     io_text.device.index or 0, max_part_symbols, options)
