"""Host-side mirror of the reference's public API for the query path.

Names, argument meaning and error behaviour follow feldroop/genedex v0.2.2:
``FmIndexConfig`` (src/config.rs:17-70), ``FmIndex`` (src/lib.rs:117-327), ``Cursor``
(src/cursor.rs:16-73), ``Hit`` (src/lib.rs:331-335).  Every query runs in the HIP kernels of
libgdx.so; a panic of the reference becomes a Python exception.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import GdxError, u8p, u16p, u32p, u64p
from .alphabet import Alphabet


class Hit(NamedTuple):
    """src/lib.rs:331-335"""
    text_id: int
    position: int


class Segment(NamedTuple):
    """One longest matching suffix segment of a query (FmIndex.suffix_segments_many): query[query_end - length : query_end]"""
    query_end: int
    length: int
    cursor: "Cursor"


class Smem(NamedTuple):
    """One super-maximal exact match of a query (FmIndex.smems_many): query[query_begin : query_end], cursor its interval"""
    query_begin: int
    query_end: int
    cursor: "Cursor"


class Alignment(NamedTuple):
    """One candidate's alignment (FmIndex.align_many): query against text[begin : end] with `dist` edits; cigar is a SAM string
    of = X I D runs.  begin, end and cigar are None where there is none (dist is then max_edits + 1 or a GDX_EDIT_* marker)."""
    dist: int
    begin: int
    end: int
    cigar: str


class SeedCandidate(NamedTuple):
    """One verification candidate of a query (FmIndex.seed_candidates_many): the seed query[begin:] lies at `position` of text
    `text_id`; weight = the query symbols covered by the seeds that agree with it."""
    begin: int
    text_id: int
    position: int
    weight: int


_CIGAR_CHAR = {_lib.GDX_CIGAR_INS: "I", _lib.GDX_CIGAR_DEL: "D", _lib.GDX_CIGAR_EQ: "=", _lib.GDX_CIGAR_DIFF: "X"}


def cigar_string(words) -> str:
    """the cigar words of one candidate (run_length << 4 | op) as a SAM string such as 37=1X12=2I98="""
    return "".join("%d%s" % (int(w) >> 4, _CIGAR_CHAR[int(w) & 15]) for w in words)


def _p(a, t):
    return a.ctypes.data_as(t)


def _complement_table(table):
    table = np.ascontiguousarray(table, dtype=np.uint8)
    if table.size != 256:
        raise ValueError("a complement table has 256 entries")
    return table


def pack_queries(queries):
    """list of bytes-like -> (qbuf u8[...], qoff u64[nq+1])"""
    queries = [bytes(q) for q in queries]
    lens = np.fromiter((len(q) for q in queries), dtype=np.uint64, count=len(queries))
    qoff = np.zeros(len(queries) + 1, dtype=np.uint64)
    np.cumsum(lens, out=qoff[1:])
    joined = b"".join(queries)
    qbuf = np.frombuffer(joined, dtype=np.uint8).copy() if joined else np.zeros(1, dtype=np.uint8)
    return qbuf, qoff


_WIDTHS = {"u32": 32, "i32": -32, "i64": 64}


def build_options(pair_lines=None, jump_entry_bytes=None, top_table_depth=None, aux_budget_bytes=None,
                  full_suffix_array=None, text_units=None, seed_symbols=None, seed_load_percent=None,
                  inverse_suffix_array=None, reference_table_layout=None):
    """gdx_build_options_t (include/gdx.h); None = the library's default for that field."""
    o = _lib.BuildOptions()
    _lib.load().gdx_build_options_init(C.byref(o))
    if pair_lines is not None:
        o.pair_lines = int(bool(pair_lines))
    if jump_entry_bytes is not None:
        o.jump_entry_bytes = int(jump_entry_bytes)
    if top_table_depth is not None:
        o.top_table_depth = int(top_table_depth)
    if aux_budget_bytes is not None:
        o.aux_budget_bytes = int(aux_budget_bytes)
    if full_suffix_array is not None:
        o.full_suffix_array = int(bool(full_suffix_array))
    if text_units is not None:
        o.text_units = int(bool(text_units))
    if seed_symbols is not None:
        o.seed_symbols = 1 if seed_symbols is True else int(seed_symbols)  # True = k chosen from the text length
    if seed_load_percent is not None:
        o.seed_load_percent = int(seed_load_percent)
    if inverse_suffix_array is not None:
        o.inverse_suffix_array = int(bool(inverse_suffix_array))
    if reference_table_layout is not None:
        names = {"condensed64": 1, "condensed512": 2, "flat64": 3, "flat512": 4}
        o.reference_table_layout = names.get(reference_table_layout, reference_table_layout)
    return o


class FmIndexConfig:
    """Builder for the index (src/config.rs:17-82).  `index_storage` is the reference's generic `I`."""

    def __init__(self, index_storage: str = "i32"):
        if index_storage not in _WIDTHS:
            raise ValueError("index_storage must be one of 'i32', 'u32', 'i64'")
        self.index_storage = index_storage
        self._sa_rate = 4    # config.rs:75
        self._depth = 0      # config.rs:76
        self._device = 0
        self._build = {}     # gdx_build_options_t fields (this implementation's own knobs)

    def suffix_array_sampling_rate(self, rate: int) -> "FmIndexConfig":
        assert rate > 0  # config.rs:28
        self._sa_rate = int(rate)
        return self

    def lookup_table_depth(self, depth: int) -> "FmIndexConfig":
        self._depth = int(depth)
        return self

    def construction_performance_priority(self, _priority) -> "FmIndexConfig":
        # config.rs:53-61: selects CPU construction sub-algorithms; the built index is identical, so the
        # GPU builder has nothing to choose.
        return self

    def device(self, device_id: int) -> "FmIndexConfig":
        self._device = int(device_id)
        return self

    def acceleration_structures(self, pair_lines=None, jump_entry_bytes=None, top_table_depth=None,
                                aux_budget_bytes=None, full_suffix_array=None, text_units=None, seed_symbols=None,
                                seed_load_percent=None, inverse_suffix_array=None, reference_table_layout=None) -> "FmIndexConfig":
        """gdx_build_options_t: which derived structures the index carries beside the reference's arrays
        (results are identical with any combination); None keeps the default."""
        self._build = dict(pair_lines=pair_lines, jump_entry_bytes=jump_entry_bytes, top_table_depth=top_table_depth,
                           aux_budget_bytes=aux_budget_bytes, full_suffix_array=full_suffix_array, text_units=text_units,
                           seed_symbols=seed_symbols, seed_load_percent=seed_load_percent,
                           inverse_suffix_array=inverse_suffix_array, reference_table_layout=reference_table_layout)
        return self

    def construct_index(self, texts, alphabet: Alphabet) -> "FmIndex":
        """src/config.rs:63-69"""
        texts = [bytes(t) for t in texts]
        tbuf, toff = pack_queries(texts)
        lib = _lib.load()
        handle = C.c_void_p()
        tab = np.ascontiguousarray(alphabet.io_to_dense_table, dtype=np.uint8)
        opts = build_options(**self._build)
        st = lib.gdx_index_build_ex(_p(tbuf, u8p), _p(toff, u64p), len(texts), _p(tab, u8p),
                                    alphabet.num_dense_symbols(), alphabet.num_searchable_dense_symbols(),
                                    self._sa_rate, self._depth, _WIDTHS[self.index_storage], self._device,
                                    C.byref(opts), C.byref(handle))
        _lib.check(st)
        return FmIndex(handle, alphabet)


class FmIndex:
    """src/lib.rs:89-100.  Owns a handle to the index in HBM."""

    def __init__(self, handle, alphabet: Alphabet):
        self._h = handle
        self._lib = _lib.load()
        self._alphabet = alphabet
        info = _lib.IndexInfo()
        _lib.check(self._lib.gdx_index_info(self._h, C.byref(info)))
        self.info = info

    def __del__(self):
        try:
            if self._h:
                self._lib.gdx_index_free(self._h)
                self._h = None
        except Exception:
            pass

    @classmethod
    def from_parts(cls, count, interleaved_blocks, n, sa_samples, sa_rate, border_keys, border_vals,
                   sentinel_indices, alphabet: Alphabet, lookup_depth=0, index_storage="u32", device=0,
                   table_kind="condensed", block_bits=64, options=None):
        """Import of the reference's logical arrays (include/gdx.h gdx_index_from_parts[_ex]); table_kind
        'condensed' | 'flat' and block_bits 64 | 512 select one of the reference's four table variants."""
        lib = _lib.load()
        count = np.ascontiguousarray(count, dtype=np.uint64)
        blocks = np.ascontiguousarray(interleaved_blocks, dtype=np.uint64)
        sa_samples = np.ascontiguousarray(sa_samples, dtype=np.uint32)
        bk = np.ascontiguousarray(border_keys, dtype=np.uint64)
        bv = np.ascontiguousarray(border_vals, dtype=np.uint64)
        si = np.ascontiguousarray(sentinel_indices, dtype=np.uint64)
        tab = np.ascontiguousarray(alphabet.io_to_dense_table, dtype=np.uint8)
        handle = C.c_void_p()
        opts = options if options is not None else build_options()
        st = lib.gdx_index_from_parts_ex2({"condensed": 0, "flat": 1}[table_kind], int(block_bits),
                                          _p(count, u64p), _p(blocks, u64p), int(n), _p(sa_samples, u32p), int(sa_rate),
                                          _p(bk, u64p), _p(bv, u64p), _p(si, u64p), si.size, _p(tab, u8p),
                                          alphabet.num_dense_symbols(), alphabet.num_searchable_dense_symbols(),
                                          int(lookup_depth), _WIDTHS[index_storage], int(device), C.byref(opts),
                                          C.byref(handle))
        _lib.check(st)
        return cls(handle, alphabet)

    # ---- this implementation's own knobs (include/gdx.h gdx_index_aux / gdx_query_options_t) ------
    def aux(self) -> dict:
        a = _lib.IndexAux()
        _lib.check(self._lib.gdx_index_aux(self._h, C.byref(a)))
        return {f: int(getattr(a, f)) for f, _ in a._fields_}

    def seed_info(self) -> dict:
        """The seed table of the index (gdx_index_seed_info); k == 0: none."""
        out = (C.c_uint64 * 8)()
        _lib.check(self._lib.gdx_index_seed_info(self._h, out))
        names = ("k", "buckets", "single_entries", "interval_entries", "overflowed_buckets", "max_displacement", "bytes",
                 "tag_bits")
        info = {n: int(v) for n, v in zip(names, out)}
        rec = (C.c_uint64 * 4)()  # (repeats of two to four copies with a record of their own: gdx_index_seed_records)
        _lib.check(self._lib.gdx_index_seed_records(self._h, rec))
        info["pair_records"], info["quad_records"] = int(rec[0]), int(rec[1])
        return info

    def set_query_options(self, search_kernel=None, search_lanes=None, load_policy=None, length_schedule=None,
                          locate_kernel=None, locate_jump_walk=None, search_defer_after=None, search_fast=None,
                          search_exact=None, max_hits_per_query=None, search_seed=None) -> None:
        """Kernel variant of the query calls on this handle; None = default.  Results never depend on it."""
        o = _lib.QueryOptions()
        self._lib.gdx_query_options_init(C.byref(o))
        names = {"pair": 2, "quad": 0, "lane": 1}
        if search_kernel is not None:
            o.search_kernel = names.get(search_kernel, search_kernel)
        if search_lanes is not None:
            o.search_lanes = int(search_lanes)
        if load_policy is not None:
            o.load_policy = int(load_policy)
        if length_schedule is not None:
            o.length_schedule = int(length_schedule)
        if locate_kernel is not None:
            o.locate_kernel = {"queue": 0, "lane": 1, "pair": 2}.get(locate_kernel, locate_kernel)
        if locate_jump_walk is not None:
            o.locate_jump_walk = int(bool(locate_jump_walk))
        if search_defer_after is not None:
            o.search_defer_after = int(search_defer_after)
        if search_fast is not None:
            o.search_fast = int(search_fast)  # False / True / 2 (jumps over up to 16 rows)
        if search_exact is not None:
            o.search_exact = int(bool(search_exact))
        if max_hits_per_query is not None:
            o.max_hits_per_query = int(max_hits_per_query)  # host-pointer locate calls: locate(q).take(k)
        if search_seed is not None:
            o.search_seed = int(bool(search_seed))
        _lib.check(self._lib.gdx_index_set_query_options(self._h, C.byref(o)))

    def rebuild_aux(self, **kw) -> None:
        """bench only (gdx_bench.h): rebuild pair lines / jump / top tables with other build options"""
        o = build_options(**kw)
        _lib.check(self._lib.gdx_index_rebuild_aux(self._h, C.byref(o)))
        _lib.check(self._lib.gdx_index_info(self._h, C.byref(self.info)))

    # ---- lib.rs:296-327 (own file format, see include/gdx.h) -------------------------------------
    def save_to_file(self, path) -> None:
        _lib.check(self._lib.gdx_index_save(self._h, str(path).encode()))

    @classmethod
    def load_from_file(cls, path, alphabet: Alphabet, device=0, options=None) -> "FmIndex":
        lib = _lib.load()
        handle = C.c_void_p()
        opts = options if options is not None else build_options()
        _lib.check(lib.gdx_index_load_ex(str(path).encode(), int(device), C.byref(opts), C.byref(handle)))
        ix = cls(handle, alphabet)
        if ix.info.sigma != alphabet.num_dense_symbols():
            raise ValueError("the file was written for a different alphabet")
        return ix

    # ---- lib.rs:283-294 ----------------------------------------------------------------------
    def alphabet(self) -> Alphabet:
        return self._alphabet

    def num_texts(self) -> int:
        return int(self.info.num_texts)

    def total_text_len(self) -> int:
        return int(self.info.total_text_len)

    # ---- raw (numpy) entry points -------------------------------------------------------------
    def cursors_raw(self, qbuf, qoff, strict=True):
        """-> (start u64[nq], end u64[nq], status u8[nq])"""
        nq = qoff.size - 1
        s = np.zeros(nq, dtype=np.uint64)
        e = np.zeros(nq, dtype=np.uint64)
        status = np.zeros(nq, dtype=np.uint8)
        st = self._lib.gdx_cursors_for_many_queries(self._h, _p(qbuf, u8p), _p(qoff, u64p), nq, _p(s, u64p),
                                                    _p(e, u64p), _p(status, u8p))
        _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
        return s, e, status

    def count_raw(self, qbuf, qoff, strict=True):
        nq = qoff.size - 1
        counts = np.zeros(nq, dtype=np.uint64)
        status = np.zeros(nq, dtype=np.uint8)
        st = self._lib.gdx_count_many(self._h, _p(qbuf, u8p), _p(qoff, u64p), nq, _p(counts, u64p), _p(status, u8p))
        _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
        return counts, status

    def locate_raw(self, qbuf, qoff, strict=True):
        """-> (hit_offsets u64[nq+1], text_ids u64[total], positions u64[total], status)"""
        nq = qoff.size - 1
        off = np.zeros(nq + 1, dtype=np.uint64)
        status = np.zeros(nq, dtype=np.uint8)
        total = C.c_uint64(0)
        allow = (_lib.GDX_ERR_CAPACITY,) + (() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
        st = self._lib.gdx_locate_many(self._h, _p(qbuf, u8p), _p(qoff, u64p), nq, _p(off, u64p), None, 0,
                                       C.byref(total), _p(status, u8p))
        _lib.check(st, allow=allow)
        hits = np.zeros((max(total.value, 1), 2), dtype=np.uint64)
        if total.value:
            st = self._lib.gdx_locate_many(self._h, _p(qbuf, u8p), _p(qoff, u64p), nq, _p(off, u64p),
                                           hits.ctypes.data_as(C.POINTER(_lib.HitStruct)), total.value,
                                           C.byref(total), _p(status, u8p))
            _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
        hits = hits[: total.value]
        return off, hits[:, 0].copy(), hits[:, 1].copy(), status

    def _layout(self, packed, uniform_len):
        lay = _lib.QueryLayout()
        self._lib.gdx_query_layout_init(C.byref(lay))
        lay.packed, lay.uniform_len = (1 if packed else 0), int(uniform_len)
        return lay

    def count_layout_raw(self, qbuf, qoff, nq, packed=False, uniform_len=0, strict=True):
        """gdx_count_many_layout: a packed (2-bit) and / or uniform (no offsets: qoff may be None) host batch"""
        counts = np.zeros(nq, dtype=np.uint64)
        status = np.zeros(nq, dtype=np.uint8)
        lay = self._layout(packed, uniform_len)
        st = self._lib.gdx_count_many_layout(self._h, _p(qbuf, u8p), _p(qoff, u64p) if qoff is not None else None, nq,
                                             C.byref(lay), _p(counts, u64p), _p(status, u8p))
        _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
        return counts, status

    def cursors_layout_raw(self, qbuf, qoff, nq, packed=False, uniform_len=0, strict=True):
        s = np.zeros(nq, dtype=np.uint64)
        e = np.zeros(nq, dtype=np.uint64)
        status = np.zeros(nq, dtype=np.uint8)
        lay = self._layout(packed, uniform_len)
        st = self._lib.gdx_cursors_for_many_queries_layout(self._h, _p(qbuf, u8p), _p(qoff, u64p) if qoff is not None else None,
                                                           nq, C.byref(lay), _p(s, u64p), _p(e, u64p), _p(status, u8p))
        _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
        return s, e, status

    def locate_layout_raw(self, qbuf, qoff, nq, packed=False, uniform_len=0, strict=True):
        """gdx_locate_many_alloc_layout -> (hit_offsets, text_ids, positions, status)"""
        off = np.zeros(nq + 1, dtype=np.uint64)
        status = np.zeros(nq, dtype=np.uint8)
        total = C.c_uint64(0)
        ptr = C.POINTER(_lib.HitStruct)()
        lay = self._layout(packed, uniform_len)
        st = self._lib.gdx_locate_many_alloc_layout(self._h, _p(qbuf, u8p), _p(qoff, u64p) if qoff is not None else None, nq,
                                                    C.byref(lay), _p(off, u64p), C.byref(ptr), C.byref(total), _p(status, u8p))
        try:
            _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
            n = total.value
            hits = np.ctypeslib.as_array(C.cast(ptr, u64p), shape=(max(n, 1) * 2,))[: 2 * n].reshape(n, 2).copy() \
                if n else np.zeros((0, 2), dtype=np.uint64)
        finally:
            if ptr:
                self._lib.gdx_free_hits(ptr)
        return off, hits[:, 0].copy(), hits[:, 1].copy(), status

    def locate_layout32_raw(self, qbuf, qoff, nq, packed=False, uniform_len=0, strict=True, qbuf_ptr=None):
        """gdx_locate_many_alloc_layout32 -> (hit_offsets u32, text_ids u32, positions u32, status): copies of the library's
        pinned arrays (a caller that cares for speed reads them in place and gives them back with gdx_free_hits32).
        qbuf_ptr: the address of the query buffer when it is not a numpy array (pinned memory of another owner)"""
        status = np.zeros(nq, dtype=np.uint8)
        res = _lib.Hits32()
        lay = self._layout(packed, uniform_len)
        qp = C.cast(C.c_void_p(qbuf_ptr), u8p) if qbuf_ptr is not None else _p(qbuf, u8p)
        st = self._lib.gdx_locate_many_alloc_layout32(self._h, qp, _p(qoff, u64p) if qoff is not None else None, nq,
                                                      C.byref(lay), C.byref(res), _p(status, u8p))
        try:
            _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
            n = res.total_hits
            off = np.ctypeslib.as_array(res.hit_offsets, shape=(nq + 1,)).copy()
            hits = np.ctypeslib.as_array(res.hits, shape=(max(n, 1) * 2,))[: 2 * n].reshape(n, 2).copy() \
                if n else np.zeros((0, 2), dtype=np.uint32)
        finally:
            self._lib.gdx_free_hits32(C.byref(res))
        return off, hits[:, 0].copy(), hits[:, 1].copy(), status

    def locate_alloc_raw(self, qbuf, qoff, strict=True):
        """gdx_locate_many_alloc (one pass) -> (hit_offsets, text_ids, positions, status)"""
        nq = qoff.size - 1
        off = np.zeros(nq + 1, dtype=np.uint64)
        status = np.zeros(nq, dtype=np.uint8)
        total = C.c_uint64(0)
        ptr = C.POINTER(_lib.HitStruct)()
        st = self._lib.gdx_locate_many_alloc(self._h, _p(qbuf, u8p), _p(qoff, u64p), nq, _p(off, u64p), C.byref(ptr),
                                             C.byref(total), _p(status, u8p))
        try:
            _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
            n = total.value
            hits = np.ctypeslib.as_array(C.cast(ptr, u64p), shape=(max(n, 1) * 2,))[: 2 * n].reshape(n, 2).copy() \
                if n else np.zeros((0, 2), dtype=np.uint64)
        finally:
            if ptr:
                self._lib.gdx_free_hits(ptr)
        return off, hits[:, 0].copy(), hits[:, 1].copy(), status

    def locate_intervals_raw(self, starts, ends):
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        ends = np.ascontiguousarray(ends, dtype=np.uint64)
        m = starts.size
        off = np.zeros(m + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        st = self._lib.gdx_cursor_locate_many(self._h, _p(starts, u64p), _p(ends, u64p), m, _p(off, u64p), None, 0,
                                              C.byref(total))
        _lib.check(st, allow=(_lib.GDX_ERR_CAPACITY,))
        hits = np.zeros((max(total.value, 1), 2), dtype=np.uint64)
        if total.value:
            st = self._lib.gdx_cursor_locate_many(self._h, _p(starts, u64p), _p(ends, u64p), m, _p(off, u64p),
                                                  hits.ctypes.data_as(C.POINTER(_lib.HitStruct)), total.value,
                                                  C.byref(total))
            _lib.check(st)
        hits = hits[: total.value]
        return off, hits[:, 0].copy(), hits[:, 1].copy()

    def extend_front_raw(self, starts, ends, io_symbols, strict=True):
        s = np.array(starts, dtype=np.uint64)
        e = np.array(ends, dtype=np.uint64)
        sym = np.ascontiguousarray(io_symbols, dtype=np.uint8)
        status = np.zeros(s.size, dtype=np.uint8)
        st = self._lib.gdx_cursor_extend_front_many(self._h, _p(s, u64p), _p(e, u64p), _p(sym, u8p), s.size,
                                                    _p(status, u8p))
        _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
        return s, e, status

    def extend_front_strings_raw(self, starts, ends, qbuf, qoff, status=None, strict=True):
        """gdx_cursor_extend_front_strings: cursor i is extended by the whole string i (right to left)."""
        s = np.array(starts, dtype=np.uint64)
        e = np.array(ends, dtype=np.uint64)
        qbuf = np.ascontiguousarray(qbuf, dtype=np.uint8)
        qoff = np.ascontiguousarray(qoff, dtype=np.uint64)
        st_arr = np.zeros(s.size, dtype=np.uint8) if status is None else np.array(status, dtype=np.uint8)
        st = self._lib.gdx_cursor_extend_front_strings(self._h, _p(s, u64p), _p(e, u64p), _p(qbuf, u8p),
                                                       _p(qoff, u64p), s.size, _p(st_arr, u8p))
        _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
        return s, e, st_arr

    def suffix_segments_raw(self, qbuf, qoff, max_segments, lf_only=False, strict=True):
        """gdx_suffix_segments_many -> (n_segments u32[nq], remaining u32[nq], length u32[nq * max_segments], start u64, end u64,
        status u8[nq]): per query its longest matching suffix segments, rightmost first (include/gdx.h has the definition)."""
        qbuf = np.ascontiguousarray(qbuf, dtype=np.uint8)
        qoff = np.ascontiguousarray(qoff, dtype=np.uint64)
        nq = qoff.size - 1
        slots = max(nq * int(max_segments), 1)
        n_seg = np.zeros(max(nq, 1), dtype=np.uint32)
        remaining = np.zeros(max(nq, 1), dtype=np.uint32)
        length = np.zeros(slots, dtype=np.uint32)
        start = np.zeros(slots, dtype=np.uint64)
        end = np.zeros(slots, dtype=np.uint64)
        status = np.zeros(max(nq, 1), dtype=np.uint8)
        st = self._lib.gdx_suffix_segments_many(self._h, _p(qbuf, u8p), _p(qoff, u64p), nq, int(max_segments),
                                                _lib.GDX_SEGMENTS_LF_ONLY if lf_only else 0, _p(n_seg, u32p),
                                                _p(remaining, u32p), _p(length, u32p), _p(start, u64p), _p(end, u64p),
                                                _p(status, u8p))
        _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
        k = nq * int(max_segments)
        return n_seg[:nq], remaining[:nq], length[:k], start[:k], end[:k], status[:nq]

    def suffix_segments_many(self, queries, max_segments=1):
        """Per query the list of its Segment(query_end, length, cursor), rightmost first: query[query_end - length : query_end]
        is the longest suffix of query[:query_end] that occurs, cursor its interval (count() / locate()); a zero-length
        segment stands for one symbol that occurs nowhere."""
        qbuf, qoff = pack_queries(queries)
        n_seg, _, length, start, end, _ = self.suffix_segments_raw(qbuf, qoff, max_segments)
        out = []
        for i in range(qoff.size - 1):
            e = int(qoff[i + 1] - qoff[i])
            segs = []
            for j in range(int(n_seg[i])):
                k = i * max_segments + j
                segs.append(Segment(e, int(length[k]), Cursor(self, int(start[k]), int(end[k]))))
                e -= max(int(length[k]), 1)
            out.append(segs)
        return out

    def longest_suffix_match(self, query):
        """(length, Cursor) of the longest suffix of `query` that occurs: length 0 with a cursor of count 0 when its last
        symbol occurs nowhere, length 0 with cursor_empty() for the empty query"""
        segs = self.suffix_segments_many([query], 1)[0]
        return (segs[0].length, segs[0].cursor) if segs else (0, self.cursor_empty())

    def smems_raw(self, reversed_index, qbuf, qoff, max_smems, min_length=1, strict=True):
        """gdx_smems_many -> (n_smems u32[nq], remaining u32[nq], begin u32[nq * max_smems], length u32, start u64, end u64,
        status u8[nq]): per query its super-maximal exact matches, rightmost first (include/gdx.h has the definition).
        reversed_index: an FmIndex of the same texts, each reversed (genedex_amd.reversed_texts)."""
        qbuf = np.ascontiguousarray(qbuf, dtype=np.uint8)
        qoff = np.ascontiguousarray(qoff, dtype=np.uint64)
        nq = qoff.size - 1
        slots = max(nq * int(max_smems), 1)
        n_smems = np.zeros(max(nq, 1), dtype=np.uint32)
        remaining = np.zeros(max(nq, 1), dtype=np.uint32)
        begin = np.zeros(slots, dtype=np.uint32)
        length = np.zeros(slots, dtype=np.uint32)
        start = np.zeros(slots, dtype=np.uint64)
        end = np.zeros(slots, dtype=np.uint64)
        status = np.zeros(max(nq, 1), dtype=np.uint8)
        st = self._lib.gdx_smems_many(self._h, reversed_index._h, _p(qbuf, u8p), _p(qoff, u64p), nq, int(max_smems),
                                      int(min_length), _p(n_smems, u32p), _p(remaining, u32p), _p(begin, u32p),
                                      _p(length, u32p), _p(start, u64p), _p(end, u64p), _p(status, u8p))
        _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
        k = nq * int(max_smems)
        return n_smems[:nq], remaining[:nq], begin[:k], length[:k], start[:k], end[:k], status[:nq]

    def smems_many(self, queries, reversed_index, max_smems, min_length=1):
        """Per query the list of its Smem(query_begin, query_end, cursor), by descending end: the matches of the query that no
        other match contains, at most max_smems of them, those shorter than min_length left out; cursor is the interval of
        query[query_begin:query_end] in this index (count() / locate())."""
        qbuf, qoff = pack_queries(queries)
        n_smems, _, begin, length, start, end, _ = self.smems_raw(reversed_index, qbuf, qoff, max_smems, min_length)
        out = []
        for i in range(qoff.size - 1):
            ks = range(i * max_smems, i * max_smems + int(n_smems[i]))
            out.append([Smem(int(begin[k]), int(begin[k]) + int(length[k]), Cursor(self, int(start[k]), int(end[k]))) for k in ks])
        return out

    # ---- seed-hit candidates (gdx_experimental.h "seed-hit candidates") -------------------------------------
    def seed_candidates_raw(self, n_seeds, begin, length, start, end, max_seeds, max_occ, band, max_candidates, strict=True):
        """gdx_seed_candidates_many -> (n_candidates, n_groups, n_skipped: u32[nq]; cand_query, cand_begin: u32[nq *
        max_candidates]; text_ids, positions: u64[..]; cand_weight: u32[..]; status u8[nq]): the seed slots of nq = len(n_seeds)
        queries (the arrays of smems_raw, max_seeds = its max_smems) as ranked, de-duplicated verification candidates; unused
        slots hold cand_query GDX_CAND_NONE and zeros.  strict=False: a query with bad seed slots is reported in status only."""
        n_seeds = np.ascontiguousarray(n_seeds, dtype=np.uint32)
        nq, ms, mc = n_seeds.size, int(max_seeds), int(max_candidates)
        begin, length = (np.ascontiguousarray(x, dtype=np.uint32) for x in (begin, length))
        start, end = (np.ascontiguousarray(x, dtype=np.uint64) for x in (start, end))
        for x in (begin, length, start, end):
            if x.size != nq * ms:
                raise ValueError("seed arrays hold nq * max_seeds slots")
        outs = max(nq * min(max(mc, 0), 1024), 1)
        n_cand, n_groups, n_skipped = (np.zeros(max(nq, 1), dtype=np.uint32) for _ in range(3))
        cq, cb, cw = (np.zeros(outs, dtype=np.uint32) for _ in range(3))
        hits = np.zeros((outs, 2), dtype=np.uint64)
        status = np.zeros(max(nq, 1), dtype=np.uint8)
        st = self._lib.gdx_seed_candidates_many(self._h, nq, ms, _p(n_seeds, u32p), _p(begin, u32p), _p(length, u32p),
                                                _p(start, u64p), _p(end, u64p), int(max_occ), int(band), mc, _p(n_cand, u32p),
                                                _p(n_groups, u32p), _p(n_skipped, u32p), _p(cq, u32p), _p(cb, u32p),
                                                hits.ctypes.data_as(C.POINTER(_lib.HitStruct)), _p(cw, u32p), _p(status, u8p))
        _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
        k = nq * mc
        return n_cand[:nq], n_groups[:nq], n_skipped[:nq], cq[:k], cb[:k], hits[:k, 0], hits[:k, 1], cw[:k], status[:nq]

    def seed_candidates_many(self, smems, max_occ, band, max_candidates):
        """Per query the list of its SeedCandidate(begin, text_id, position, weight), best first: `smems` is what smems_many
        returns (per query its Smem list).  Seeds on more than max_occ rows are left out; hits of one text within `band`
        diagonals of a group's first are one candidate, whose weight is the number of query symbols its seeds cover."""
        nq = len(smems)
        ms = max([len(s) for s in smems] + [1])
        n_seeds = np.array([len(s) for s in smems], dtype=np.uint32)
        begin, length = np.zeros(nq * ms, dtype=np.uint32), np.zeros(nq * ms, dtype=np.uint32)
        start, end = np.zeros(nq * ms, dtype=np.uint64), np.zeros(nq * ms, dtype=np.uint64)
        for i, seeds in enumerate(smems):
            for j, s in enumerate(seeds):
                k = i * ms + j
                begin[k], length[k], start[k], end[k] = s.query_begin, s.query_end - s.query_begin, s.cursor.start, s.cursor.end
        n_cand, _, _, _, cb, t, p, cw, _ = self.seed_candidates_raw(n_seeds, begin, length, start, end, ms, max_occ, band,
                                                                    max_candidates)
        mc = int(max_candidates)
        return [[SeedCandidate(int(cb[k]), int(t[k]), int(p[k]), int(cw[k])) for k in range(i * mc, i * mc + int(n_cand[i]))]
                for i in range(nq)]

    @staticmethod
    def _slot_arrays(cand_query, cand_begin, text_ids, positions, dist, end, m, what):
        """the inputs of best_hits_raw / pair_hits_raw as contiguous arrays of m (`what`) slots: u32, end or None, hits u64[m, 2]"""
        cq, cb, dist = (np.ascontiguousarray(x, dtype=np.uint32) for x in (cand_query, cand_begin, dist))
        end = None if end is None else np.ascontiguousarray(end, dtype=np.uint32)
        hits = np.ascontiguousarray(np.stack([np.asarray(text_ids, dtype=np.uint64), np.asarray(positions, dtype=np.uint64)], axis=1))
        if any(x is not None and x.size != m for x in (cq, cb, dist, end, hits[:, 0])):
            raise ValueError(f"slot arrays hold {what} slots")
        return cq, cb, dist, end, hits

    # ---- best hit per read (gdx_experimental.h "best hit per read") ------------------------------------------
    def best_hits_raw(self, cand_query, cand_begin, text_ids, positions, dist, end, n_groups, group_slots, max_dist):
        """gdx_best_hits_many -> (best_slot, best_dist, sub_dist, n_live, n_best, mapq, win_query, win_begin: u32[n_groups];
        win_text_ids, win_positions: u64[n_groups]): every group of group_slots consecutive candidate slots (the arrays of
        seed_candidates_raw) with the distances a verify call gave them reduced to its best hit; `end` = the ends of the
        edit-distance call, or None (the Hamming case: the diagonal tells loci apart).  A group without a live slot has
        best_slot GDX_BEST_NONE, mapq GDX_BEST_MAPQ_NONE and the none pattern as its winner."""
        ng, gs = int(n_groups), int(group_slots)
        cq, cb, dist, end, hits = self._slot_arrays(cand_query, cand_begin, text_ids, positions, dist, end, ng * gs,
                                                    "n_groups * group_slots")
        outs = [np.zeros(max(ng, 1), dtype=np.uint32) for _ in range(8)]
        win = np.zeros((max(ng, 1), 2), dtype=np.uint64)
        _lib.check(self._lib.gdx_best_hits_many(self._h, ng, gs, _p(cq, u32p), _p(cb, u32p),
                                                hits.ctypes.data_as(C.POINTER(_lib.HitStruct)), _p(dist, u32p),
                                                _p(end, u32p) if end is not None else None, int(max_dist),
                                                *(_p(o, u32p) for o in outs), win.ctypes.data_as(C.POINTER(_lib.HitStruct))))
        return tuple(o[:ng] for o in outs) + (win[:ng, 0], win[:ng, 1])

    # ---- paired-end pairing (gdx_experimental.h "paired-end pairing") -----------------------------------------
    def pair_hits_raw(self, cand_query, cand_begin, text_ids, positions, dist, end, n_pairs, mate_slots, max_dist, min_insert,
                      max_insert):
        """gdx_pair_hits_many -> (n_proper, n_best, pair_dist, sub_dist, mapq, pair_span: u32[n_pairs]; mate_slot, mate_dist,
        win_query, win_begin: u32[2 n_pairs]; win_text_ids, win_positions: u64[2 n_pairs]): the slots are 2 * n_pairs mates of
        mate_slots consecutive candidate slots (mates 2p and 2p + 1 make pair p) with the distances a verify call gave them;
        per pair the best combination of one slot of each mate that lies on one text, on opposite strands and min_insert ..
        max_insert apart, per mate the winner (its single-end best without such a combination).  `end` as in best_hits_raw."""
        n, ms = int(n_pairs), int(mate_slots)
        cq, cb, dist, end, hits = self._slot_arrays(cand_query, cand_begin, text_ids, positions, dist, end, 2 * n * ms,
                                                    "2 * n_pairs * mate_slots")
        pairs = [np.zeros(max(n, 1), dtype=np.uint32) for _ in range(6)]
        mates = [np.zeros(max(2 * n, 1), dtype=np.uint32) for _ in range(4)]
        win = np.zeros((max(2 * n, 1), 2), dtype=np.uint64)
        _lib.check(self._lib.gdx_pair_hits_many(self._h, n, ms, _p(cq, u32p), _p(cb, u32p),
                                                hits.ctypes.data_as(C.POINTER(_lib.HitStruct)), _p(dist, u32p),
                                                _p(end, u32p) if end is not None else None, int(max_dist), int(min_insert),
                                                int(max_insert), *(_p(o, u32p) for o in pairs + mates),
                                                win.ctypes.data_as(C.POINTER(_lib.HitStruct))))
        return tuple(o[:n] for o in pairs) + tuple(o[:2 * n] for o in mates) + (win[:2 * n, 0], win[:2 * n, 1])

    # ---- mate rescue (gdx_experimental.h "mate rescue") -------------------------------------------------------
    def mate_rescue_raw(self, qbuf, qoff, end, n_proper, mate_slot, mate_dist, win_query, win_begin, win_text_ids, win_positions,
                        n_pairs, mate_slots, max_edits, min_insert, max_insert):
        """gdx_mate_rescue_many -> (resc_dist, resc_end: u32[2 n_pairs]; resc_mate, resc_pair_dist, resc_span: u32[n_pairs];
        win_query, win_begin: u32[2 n_pairs]; win_text_ids, win_positions: u64[2 n_pairs]).  qbuf / qoff: the 4 * n_pairs queries
        (both strands of both mates of every pair); end: the ends of the edit-distance call over all 2 * n_pairs * mate_slots
        slots; the other inputs as pair_hits_raw returned them.  For a pair without a proper combination every placed mate is
        the anchor from which the other mate's opposite strand is searched where min_insert <= span <= max_insert puts it."""
        n, ms = int(n_pairs), int(mate_slots)
        qbuf = np.ascontiguousarray(qbuf, dtype=np.uint8)
        qoff = np.ascontiguousarray(qoff, dtype=np.uint64)
        u32 = lambda x, size, what: self._sized(np.ascontiguousarray(np.asarray(x).astype(np.uint32)), size, what)  # noqa: E731
        end = u32(end, 2 * n * ms, "end")
        n_proper = u32(n_proper, n, "n_proper")
        per_mate = [u32(x, 2 * n, "a per-mate input") for x in (mate_slot, mate_dist, win_query, win_begin)]
        hits = np.ascontiguousarray(np.stack([np.asarray(win_text_ids).astype(np.uint64), np.asarray(win_positions).astype(np.uint64)],
                                             axis=1))
        self._sized(hits, 4 * n, "win_hits")
        mates = [np.zeros(max(2 * n, 1), dtype=np.uint32) for _ in range(4)]       # resc_dist, resc_end, win_query, win_begin
        pairs = [np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3)]
        win = np.zeros((max(2 * n, 1), 2), dtype=np.uint64)
        _lib.check(self._lib.gdx_mate_rescue_many(
            self._h, _p(qbuf, u8p), _p(qoff, u64p), qoff.size - 1, n, ms, _p(end, u32p), _p(n_proper, u32p),
            *(_p(x, u32p) for x in per_mate), hits.ctypes.data_as(C.POINTER(_lib.HitStruct)), int(max_edits), int(min_insert),
            int(max_insert), _p(mates[0], u32p), _p(mates[1], u32p), *(_p(o, u32p) for o in pairs), _p(mates[2], u32p),
            _p(mates[3], u32p), win.ctypes.data_as(C.POINTER(_lib.HitStruct))))
        return (mates[0][:2 * n], mates[1][:2 * n]) + tuple(o[:n] for o in pairs) + (mates[2][:2 * n], mates[3][:2 * n],
                                                                                    win[:2 * n, 0], win[:2 * n, 1])

    @staticmethod
    def _sized(x, size, what):
        if x.size < size:
            raise ValueError(f"{what} holds {x.size} entries, {size} are needed")
        return x

    def rank_many(self, symbols, idx):
        """TextWithRankSupport::rank (text_with_rank_support/mod.rs:106-110), batched."""
        sym = np.ascontiguousarray(symbols, dtype=np.uint8)
        ii = np.ascontiguousarray(idx, dtype=np.uint64)
        out = np.zeros(sym.size, dtype=np.uint64)
        _lib.check(self._lib.gdx_rank_many(self._h, _p(sym, u8p), _p(ii, u64p), sym.size, _p(out, u64p)))
        return out

    def symbol_at_many(self, idx):
        ii = np.ascontiguousarray(idx, dtype=np.uint64)
        out = np.zeros(ii.size, dtype=np.uint8)
        _lib.check(self._lib.gdx_symbol_at_many(self._h, _p(ii, u64p), ii.size, _p(out, u8p)))
        return out

    # ---- lib.rs:147-246 -----------------------------------------------------------------------
    def count(self, query) -> int:
        return int(self.count_many([query])[0])

    def count_many(self, queries):
        qbuf, qoff = pack_queries(queries)
        return self.count_raw(qbuf, qoff)[0]

    def locate(self, query):
        return self.locate_many([query])[0]

    def locate_many(self, queries):
        qbuf, qoff = pack_queries(queries)
        off, t, p, _ = self.locate_raw(qbuf, qoff)
        t, p = t.tolist(), p.tolist()
        return [[Hit(t[h], p[h]) for h in range(int(off[q]), int(off[q + 1]))] for q in range(qoff.size - 1)]

    # ---- both strands (gdx.h "both strands") ------------------------------------------------------
    def count_strands_raw(self, qbuf, qoff, complement=None, strict=True):
        """gdx_count_many_strands -> (counts u64[2 nq], status u8[2 nq]); row 2i = read i, row 2i + 1 = its reverse complement"""
        nq = qoff.size - 1
        counts = np.zeros(2 * nq, dtype=np.uint64)
        status = np.zeros(2 * nq, dtype=np.uint8)
        comp = None if complement is None else _p(_complement_table(complement), u8p)
        st = self._lib.gdx_count_many_strands(self._h, _p(qbuf, u8p), _p(qoff, u64p), nq, comp, _p(counts, u64p), _p(status, u8p))
        _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
        return counts, status

    def locate_strands_raw(self, qbuf, qoff, complement=None, strict=True):
        """gdx_locate_many_alloc_strands -> (hit_offsets u64[2 nq + 1], text_ids u64[total], positions u64[total], status u8[2 nq])"""
        nq = qoff.size - 1
        off = np.zeros(2 * nq + 1, dtype=np.uint64)
        status = np.zeros(2 * nq, dtype=np.uint8)
        total = C.c_uint64(0)
        hits = C.POINTER(_lib.HitStruct)()
        comp = None if complement is None else _p(_complement_table(complement), u8p)
        st = self._lib.gdx_locate_many_alloc_strands(self._h, _p(qbuf, u8p), _p(qoff, u64p), nq, comp, _p(off, u64p),
                                                     C.byref(hits), C.byref(total), _p(status, u8p))
        try:
            _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
            n = total.value
            flat = np.ctypeslib.as_array(C.cast(hits, u64p), shape=(2 * n,)).reshape(n, 2).copy() if n else np.zeros((0, 2), np.uint64)
        finally:
            if hits:
                self._lib.gdx_free_hits(hits)
        return off, flat[:, 0].copy(), flat[:, 1].copy(), status

    def count_many_strands(self, queries, complement=None):
        """(nq, 2) array: occurrences of every read as given and of its reverse complement"""
        qbuf, qoff = pack_queries(queries)
        return self.count_strands_raw(qbuf, qoff, complement)[0].reshape(-1, 2)

    def locate_many_strands(self, queries, complement=None):
        """per read a pair of hit lists: (hits of the read as given, hits of its reverse complement -- the read maps to the
        reverse strand there, position = the leftmost text coordinate of the alignment)"""
        qbuf, qoff = pack_queries(queries)
        off, t, p, _ = self.locate_strands_raw(qbuf, qoff, complement)
        t, p = t.tolist(), p.tolist()
        rows = [[Hit(t[h], p[h]) for h in range(int(off[r]), int(off[r + 1]))] for r in range(2 * (qoff.size - 1))]
        return [(rows[2 * i], rows[2 * i + 1]) for i in range(qoff.size - 1)]

    # ---- Hamming verification of located seeds (gdx.h "Hamming verification") ---------------------------
    @staticmethod
    def _verify_arrays(qbuf, qoff, cand_query, cand_begin, text_ids, positions):
        """the batch and the candidates of a verify call as the C ABI takes them -> (qbuf, qoff, cand_query, cand_begin,
        hits u64[max(m, 1), 2], m)"""
        qbuf = np.ascontiguousarray(qbuf, dtype=np.uint8)
        qoff = np.ascontiguousarray(qoff, dtype=np.uint64)
        cq = np.ascontiguousarray(cand_query, dtype=np.uint32)
        cb = np.ascontiguousarray(cand_begin, dtype=np.uint32)
        m = cq.size
        hits = np.zeros((max(m, 1), 2), dtype=np.uint64)
        hits[:m, 0] = text_ids
        hits[:m, 1] = positions
        if cb.size != m:
            raise ValueError("cand_query and cand_begin differ in length")
        return qbuf, qoff, cq, cb, hits, m

    def hamming_raw(self, qbuf, qoff, cand_query, cand_begin, text_ids, positions, max_mismatches):
        """gdx_hamming_many -> u32[m]: per candidate (query, where its seed begins in the query, the (text_id, position) the
        seed was located at) the mismatches of the whole query against its text on that diagonal, capped at
        max_mismatches + 1 (include/gdx.h has the definition)."""
        qbuf, qoff, cq, cb, hits, m = self._verify_arrays(qbuf, qoff, cand_query, cand_begin, text_ids, positions)
        out = np.zeros(max(m, 1), dtype=np.uint32)
        _lib.check(self._lib.gdx_hamming_many(self._h, _p(qbuf, u8p), _p(qoff, u64p), qoff.size - 1, _p(cq, u32p), _p(cb, u32p),
                                              hits.ctypes.data_as(C.POINTER(_lib.HitStruct)), m, int(max_mismatches), _p(out, u32p)))
        return out[:m]

    def hamming_many(self, queries, cand_query, cand_begin, hits, max_mismatches):
        """uint32 array, one entry per candidate: candidate c says that the seed of queries[cand_query[c]] that begins at
        symbol cand_begin[c] was located at hits[c] (a Hit, or any (text_id, position) pair -- what Cursor.locate() gives for
        an Smem's or a Segment's cursor); the entry is the number of mismatches of the WHOLE query against that text on the
        seed's diagonal, min(dist, max_mismatches + 1).  Symbols that hang over an end of the text, N and bytes outside the
        alphabet count as mismatches."""
        qbuf, qoff = pack_queries(queries)
        h = np.asarray([tuple(x) for x in hits], dtype=np.uint64).reshape(-1, 2)
        return self.hamming_raw(qbuf, qoff, cand_query, cand_begin, h[:, 0], h[:, 1], max_mismatches)

    # ---- edit-distance verification of located seeds (gdx.h "edit-distance verification") ----------------
    def edit_distance_raw(self, qbuf, qoff, cand_query, cand_begin, text_ids, positions, max_edits, want_end=True):
        """gdx_edit_distance_many -> (dist u32[m], end u32[m] or None): per candidate of hamming_raw the infix edit distance of
        the whole query against its text within max_edits of the seed's diagonal, capped at max_edits + 1, and the exclusive end
        of the leftmost best alignment in that text (include/gdx.h has the definition)."""
        qbuf, qoff, cq, cb, hits, m = self._verify_arrays(qbuf, qoff, cand_query, cand_begin, text_ids, positions)
        dist = np.zeros(max(m, 1), dtype=np.uint32)
        end = np.zeros(max(m, 1), dtype=np.uint32) if want_end else None
        _lib.check(self._lib.gdx_edit_distance_many(self._h, _p(qbuf, u8p), _p(qoff, u64p), qoff.size - 1, _p(cq, u32p), _p(cb, u32p),
                                                    hits.ctypes.data_as(C.POINTER(_lib.HitStruct)), m, int(max_edits), _p(dist, u32p),
                                                    _p(end, u32p) if want_end else None))
        return dist[:m], (end[:m] if want_end else None)

    def edit_distance_many(self, queries, cand_query, cand_begin, hits, max_edits):
        """(dist, end), two uint32 arrays with one entry per candidate of hamming_many: dist is the least number of
        substitutions, insertions and deletions that turn the WHOLE query (at most 256 symbols) into a piece of its text that
        lies within max_edits of the seed's diagonal, min(dist, max_edits + 1); end is where the leftmost best such piece ends
        (exclusive, a position in the text), GDX_EDIT_NO_END when dist > max_edits.  A query that hangs over an end of its text
        pays one edit per overhanging symbol; N and bytes outside the alphabet never match."""
        qbuf, qoff = pack_queries(queries)
        h = np.asarray([tuple(x) for x in hits], dtype=np.uint64).reshape(-1, 2)
        return self.edit_distance_raw(qbuf, qoff, cand_query, cand_begin, h[:, 0], h[:, 1], max_edits)

    # ---- alignment traceback of verified seed hits (gdx.h "alignment traceback") --------------------------
    def align_raw(self, qbuf, qoff, cand_query, cand_begin, text_ids, positions, max_edits):
        """gdx_align_many -> (dist, begin, end, n_cigar, cigar[m, 2 max_edits + 1]), uint32 arrays: per candidate of
        edit_distance_raw the distance and end it gives, where the canonical best alignment begins and its runs
        (run_length << 4 | GDX_CIGAR_*; the words of a row from n_cigar on are zero).  include/gdx.h has the definition."""
        qbuf, qoff, cq, cb, hits, m = self._verify_arrays(qbuf, qoff, cand_query, cand_begin, text_ids, positions)
        dist, begin, end, n_cigar = (np.zeros(max(m, 1), dtype=np.uint32) for _ in range(4))
        # (a limit over GDX_EDIT_MAX_QUERY_LEN is refused by the call before it writes anything)
        cigar = np.zeros((max(m, 1), 2 * min(int(max_edits), _lib.GDX_EDIT_MAX_QUERY_LEN) + 1), dtype=np.uint32)
        _lib.check(self._lib.gdx_align_many(self._h, _p(qbuf, u8p), _p(qoff, u64p), qoff.size - 1, _p(cq, u32p), _p(cb, u32p),
                                            hits.ctypes.data_as(C.POINTER(_lib.HitStruct)), m, int(max_edits), _p(dist, u32p),
                                            _p(begin, u32p), _p(end, u32p), _p(n_cigar, u32p), _p(cigar, u32p)))
        return dist[:m], begin[:m], end[:m], n_cigar[:m], cigar[:m]

    def align_many(self, queries, cand_query, cand_begin, hits, max_edits):
        """One Alignment(dist, begin, end, cigar) per candidate of edit_distance_many: dist as there; the canonical best
        alignment of the WHOLE query is against text[begin : end] of the candidate's text, cigar its SAM string of = X I D runs
        ("" for an empty query).  begin, end and cigar are None when dist > max_edits or the query has more than 256 symbols."""
        qbuf, qoff = pack_queries(queries)
        h = np.asarray([tuple(x) for x in hits], dtype=np.uint64).reshape(-1, 2)
        dist, begin, end, n_cigar, cigar = self.align_raw(qbuf, qoff, cand_query, cand_begin, h[:, 0], h[:, 1], max_edits)
        return [Alignment(int(d), None, None, None) if e == _lib.GDX_EDIT_NO_END
                else Alignment(int(d), int(b), int(e), cigar_string(row[:n]))
                for d, b, e, n, row in zip(dist, begin, end, n_cigar, cigar)]

    # ---- soft clipping (gdx_experimental.h "soft clipping") -------------------------------------------------
    def soft_clip_raw(self, dist, begin, end, n_cigar, cigar, max_edits, match, mismatch, gap_open, gap_extend, min_score=0):
        """gdx_soft_clip_many -> (score: int32[m]; dist, begin, end, clip_left, clip_right, n_cigar: uint32[m]; cigar: uint32[m,
        2 max_edits + 1]; status: uint8[m]): per candidate of align_raw the best-scoring contiguous part of its runs under the
        scoring, S runs (op GDX_CIGAR_SOFT_CLIP) in place of what lies outside, begin and end moved inwards, dist the edits that
        stay.  A candidate without an alignment passes through with score GDX_CLIP_NO_SCORE; one whose best score is below
        max(1, min_score) is clipped away (end GDX_EDIT_NO_END, n_cigar 0, dist max_edits + 1, score the best score); one whose
        runs fail the check gets status GDX_CLIP_BAD_CIGAR.  The words of a cigar row from n_cigar on are zero."""
        dist, begin, end, n_cigar = (np.ascontiguousarray(x, dtype=np.uint32) for x in (dist, begin, end, n_cigar))
        m = int(dist.size)
        # (a limit over GDX_EDIT_MAX_QUERY_LEN is refused by the call before it reads or writes anything)
        stride = 2 * min(int(max_edits), _lib.GDX_EDIT_MAX_QUERY_LEN) + 1
        cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
        if any(x.size != m for x in (begin, end, n_cigar)) or (int(max_edits) <= _lib.GDX_EDIT_MAX_QUERY_LEN and cigar.size != m * stride):
            raise ValueError("dist, begin, end and n_cigar hold m entries, cigar m rows of 2 max_edits + 1 words")
        if cigar.size == 0:
            cigar = np.zeros(1, dtype=np.uint32)  # (never a null pointer)
        score = np.zeros(max(m, 1), dtype=np.int32)
        outs = [np.zeros(max(m, 1), dtype=np.uint32) for _ in range(6)]
        out_cigar = np.zeros((max(m, 1), stride), dtype=np.uint32)
        status = np.zeros(max(m, 1), dtype=np.uint8)
        pad = lambda x: x if x.size else np.zeros(1, dtype=np.uint32)  # noqa: E731
        _lib.check(self._lib.gdx_soft_clip_many(self._h, m, int(max_edits), int(match), int(mismatch), int(gap_open), int(gap_extend),
                                                int(min_score), _p(pad(dist), u32p), _p(pad(begin), u32p), _p(pad(end), u32p),
                                                _p(pad(n_cigar), u32p), _p(cigar, u32p), score.ctypes.data_as(C.POINTER(C.c_int32)),
                                                *(_p(o, u32p) for o in outs), _p(out_cigar, u32p), _p(status, _lib.u8p)))
        return (score[:m],) + tuple(o[:m] for o in outs) + (out_cigar[:m], status[:m])

    # ---- SAM records (gdx_experimental.h "SAM records") ----------------------------------------------------
    def sam_records_raw(self, qbuf, qoff, win_query, win_text_ids, dist, begin, end, n_cigar, cigar, mapq, *, strands=1,
                        mode=_lib.GDX_SAM_SINGLE, max_edits, proper=None, names=None, name_off=None, text_names=None,
                        text_name_off=None, dense_to_io=None, out_capacity=None, want_status=True):
        """gdx_sam_records_many -> (out: uint8 array of the records that fit, rec_off: uint64[n_reads + 1], status: uint8[n_reads]).
        One SAM record per read from the winners (win_query, GDX_CAND_NONE = none; win_text_ids) and what align_raw returned for
        them; cigar has 2 max_edits + 1 words a read.  out_capacity None: a sizing call first, then everything; a number: the
        records that fit whole below it; 0 with `out` empty is the sizing call alone.  names / text_names: bytes with their
        uint64 offsets, or None for numbers.  dense_to_io: 16 bytes, the byte printed in MD for a text symbol of that dense code
        (0: a symbol outside 1..4), or None for the alphabet's own."""
        n = int(np.asarray(win_query).size)
        qbuf = np.ascontiguousarray(qbuf, dtype=np.uint8)
        qoff = np.ascontiguousarray(qoff, dtype=np.uint64)
        u32 = lambda x: np.ascontiguousarray(np.asarray(x).astype(np.uint32))  # noqa: E731
        per_read = [self._sized(u32(x), n, "a per-read input") for x in (win_query, dist, begin, end, n_cigar, mapq)]
        hits = np.ascontiguousarray(np.stack([np.asarray(win_text_ids).astype(np.uint64), np.zeros(n, dtype=np.uint64)], axis=1))
        cigar = u32(cigar)
        keep = [qbuf, qoff, hits, cigar] + per_read
        a = _lib.SamInputs()
        a.qbuf, a.qoff, a.nq, a.layout = qbuf.ctypes.data, qoff.ctypes.data, max(qoff.size - 1, 0), None
        a.n_reads, a.strands, a.mode, a.max_edits = n, int(strands), int(mode), int(max_edits)
        a.win_query, a.dist, a.begin, a.end, a.n_cigar, a.mapq = (x.ctypes.data for x in per_read)
        a.win_hits, a.cigar = hits.ctypes.data, cigar.ctypes.data
        for field, x, dtype in (("proper", proper, np.uint32), ("names", names, np.uint8), ("name_off", name_off, np.uint64),
                                ("text_names", text_names, np.uint8), ("text_name_off", text_name_off, np.uint64),
                                ("dense_to_io", dense_to_io, np.uint8)):
            if x is not None:
                x = np.ascontiguousarray(np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=dtype)
                x = np.concatenate([x, np.zeros(1, dtype=dtype)]) if x.size == 0 else x  # (an empty array still has an address)
                keep.append(x)
                setattr(a, field, x.ctypes.data)
        rec_off = np.full(n + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        status = np.full(max(n, 1), 0xA5, dtype=np.uint8)
        a.rec_off, a.status = rec_off.ctypes.data, (status.ctypes.data if want_status else None)
        if out_capacity is None:
            a.out, a.out_capacity = None, 0
            _lib.check(self._lib.gdx_sam_records_many(self._h, C.byref(a)))
            out_capacity = int(rec_off[n])
        out = np.full(max(int(out_capacity), 1), 0xA5, dtype=np.uint8)
        a.out, a.out_capacity = (out.ctypes.data if out_capacity else None), int(out_capacity)
        _lib.check(self._lib.gdx_sam_records_many(self._h, C.byref(a)))
        del keep
        return out[:int(out_capacity)], rec_off, status[:n]

    def cursor_empty(self) -> "Cursor":
        s = C.c_uint64(0)
        e = C.c_uint64(0)
        _lib.check(self._lib.gdx_cursor_empty(self._h, C.byref(s), C.byref(e)))
        return Cursor(self, s.value, e.value)

    def cursor_for_query(self, query) -> "Cursor":
        return self.cursors_for_many_queries([query])[0]

    def cursors_for_many_queries(self, queries):
        qbuf, qoff = pack_queries(queries)
        s, e, _ = self.cursors_raw(qbuf, qoff)
        return [Cursor(self, int(a), int(b)) for a, b in zip(s, e)]

    # ---- exports -------------------------------------------------------------------------------
    def export_count(self):
        out = np.zeros(self.info.sigma + 1, dtype=np.uint64)
        _lib.check(self._lib.gdx_index_export_count(self._h, _p(out, u64p)))
        return out

    def export_bwt(self):
        out = np.zeros(max(self.total_text_len(), 1), dtype=np.uint8)
        _lib.check(self._lib.gdx_index_export_bwt(self._h, _p(out, u8p)))
        return out[: self.total_text_len()]

    def export_sa_samples(self):
        m = -(-self.total_text_len() // int(self.info.sa_rate))
        out = np.zeros(max(m, 1), dtype=np.uint32)
        _lib.check(self._lib.gdx_index_export_sa_samples(self._h, _p(out, u32p)))
        return out[:m]

    def export_borders(self):
        k = np.zeros(self.num_texts(), dtype=np.uint64)
        v = np.zeros(self.num_texts(), dtype=np.uint64)
        _lib.check(self._lib.gdx_index_export_borders(self._h, _p(k, u64p), _p(v, u64p)))
        return k, v

    def export_sentinel_indices(self):
        out = np.zeros(self.num_texts(), dtype=np.uint64)
        _lib.check(self._lib.gdx_index_export_sentinel_indices(self._h, _p(out, u64p)))
        return out

    def export_lookup_table(self, depth):
        entries = int(self.info.n_searchable) ** depth
        out = np.zeros((entries, 2), dtype=np.uint32)
        _lib.check(self._lib.gdx_index_export_lookup_table(self._h, depth, _p(out, u32p)))
        return out

    def export_condensed_table(self):
        n1 = self.total_text_len() + 1
        sigma = int(self.info.sigma)
        nbits = max(1, (sigma - 1).bit_length())
        blocks = np.zeros(-(-n1 // 64) * nbits, dtype=np.uint64)
        bo = np.zeros(-(-n1 // 64) * sigma, dtype=np.uint16)
        sbo = np.zeros(-(-n1 // 65536) * sigma, dtype=np.uint32)
        _lib.check(self._lib.gdx_index_export_condensed_table(self._h, _p(blocks, u64p), _p(bo, u16p), _p(sbo, u32p)))
        return blocks, bo, sbo

    def export_reference_table(self):
        """(interleaved blocks u64, superblock offsets u32) of an index built with reference_table_layout"""
        nw, ns = C.c_uint64(0), C.c_uint64(0)
        _lib.check(self._lib.gdx_index_export_reference_table(self._h, None, 0, C.byref(nw), None, 0, C.byref(ns)))
        blocks = np.zeros(max(nw.value, 1), dtype=np.uint64)
        sbo = np.zeros(max(ns.value, 1), dtype=np.uint32)
        _lib.check(self._lib.gdx_index_export_reference_table(self._h, _p(blocks, u64p), blocks.size, C.byref(nw), _p(sbo, u32p),
                                                              sbo.size, C.byref(ns)))
        return blocks[: nw.value], sbo[: ns.value]

    def build_stats(self):
        st = _lib.BuildStats()
        _lib.check(self._lib.gdx_index_build_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}


class Cursor:
    """src/cursor.rs:16-73: the currently searched query as a half-open suffix-array interval."""

    def __init__(self, index: FmIndex, start: int, end: int):
        self.index = index
        self.start = start
        self.end = end

    def extend_query_front(self, symbol) -> None:
        """cursor.rs:34-38; raises where the reference panics (symbol not in the alphabet)."""
        sym = symbol if isinstance(symbol, int) else bytes(symbol)[0]
        s, e, _ = self.index.extend_front_raw([self.start], [self.end], [sym])
        self.start, self.end = int(s[0]), int(e[0])

    def extend_query_front_by(self, symbols) -> None:
        """extend_query_front for every symbol of `symbols`, last symbol first, in one launch"""
        qbuf, qoff = pack_queries([bytes(symbols)])
        s, e, _ = self.index.extend_front_strings_raw([self.start], [self.end], qbuf, qoff)
        self.start, self.end = int(s[0]), int(e[0])

    def count(self) -> int:
        return self.end - self.start  # cursor.rs:61-63

    def interval(self):
        return self.start, self.end

    def locate(self):
        off, t, p = self.index.locate_intervals_raw([self.start], [self.end])
        return [Hit(int(a), int(b)) for a, b in zip(t, p)]

    def __copy__(self):
        return Cursor(self.index, self.start, self.end)  # cursor.rs:22-28 Cursor is Copy


class PartitionedFmIndex:
    """gdx_parts_* (include/gdx.h): a collection of texts beyond 2^32 - 1 symbols -- the reference's `IndexStorage = i64`
    case (construction/mod.rs:225-252) -- as several 32-bit indexes cut at text borders.  count / locate only: counts
    and hit sets are the reference's; there is no single suffix-array interval of the whole collection, and a query's
    hits come part after part."""

    def __init__(self, handle, alphabet: Alphabet):
        self._h = handle
        self._lib = _lib.load()
        self._alphabet = alphabet
        out = (C.c_uint64 * 4)()
        _lib.check(self._lib.gdx_parts_info(self._h, out))
        self.num_parts, self._total_len, self._num_texts, self.device_bytes = (int(x) for x in out)

    def __del__(self):
        try:
            if self._h:
                self._lib.gdx_parts_free(self._h)
                self._h = None
        except Exception:
            pass

    @classmethod
    def construct(cls, texts, alphabet: Alphabet, sa_rate=4, lookup_depth=0, device=0, max_part_symbols=0, options=None):
        texts = [bytes(t) for t in texts]
        tbuf, toff = pack_queries(texts)
        return cls._build(tbuf.ctypes.data_as(C.c_void_p), 0, toff, len(texts), alphabet, sa_rate, lookup_depth, device,
                          max_part_symbols, options)

    @classmethod
    def _build(cls, texts_ptr, on_device, toff, n_texts, alphabet, sa_rate, lookup_depth, device, max_part_symbols, options):
        lib = _lib.load()
        handle = C.c_void_p()
        tab = np.ascontiguousarray(alphabet.io_to_dense_table, dtype=np.uint8)
        opts = options if options is not None else build_options()
        toff = np.ascontiguousarray(toff, dtype=np.uint64)
        _lib.check(lib.gdx_parts_build(texts_ptr, int(on_device), _p(toff, u64p), int(n_texts), _p(tab, u8p),
                                       alphabet.num_dense_symbols(), alphabet.num_searchable_dense_symbols(), int(sa_rate),
                                       int(lookup_depth), int(device), int(max_part_symbols), C.byref(opts), C.byref(handle)))
        return cls(handle, alphabet)

    def num_texts(self) -> int:
        return self._num_texts

    def total_text_len(self) -> int:
        return self._total_len

    def set_query_options(self, **kw) -> None:
        o = _lib.QueryOptions()
        self._lib.gdx_query_options_init(C.byref(o))
        known = {name for name, _ in _lib.QueryOptions._fields_} - {"struct_size"}
        for k, v in kw.items():
            if k not in known:  # (setattr on a ctypes struct would take any name and change nothing)
                raise TypeError(f"unknown query option {k!r}; gdx_query_options_t has {sorted(known)}")
            setattr(o, k, int(v))
        _lib.check(self._lib.gdx_parts_set_query_options(self._h, C.byref(o)))

    def count_raw(self, qbuf, qoff, strict=True):
        nq = qoff.size - 1
        counts = np.zeros(nq, dtype=np.uint64)
        status = np.zeros(nq, dtype=np.uint8)
        st = self._lib.gdx_parts_count_many(self._h, _p(qbuf, u8p), _p(qoff, u64p), nq, _p(counts, u64p), _p(status, u8p))
        _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
        return counts, status

    def locate_raw(self, qbuf, qoff, strict=True):
        """-> (hit_offsets u64[nq+1], text_ids u64[total], positions u64[total], status)"""
        nq = qoff.size - 1
        off = np.zeros(nq + 1, dtype=np.uint64)
        status = np.zeros(nq, dtype=np.uint8)
        total = C.c_uint64(0)
        ptr = C.POINTER(_lib.HitStruct)()
        st = self._lib.gdx_parts_locate_many_alloc(self._h, _p(qbuf, u8p), _p(qoff, u64p), nq, _p(off, u64p), C.byref(ptr),
                                                   C.byref(total), _p(status, u8p))
        try:
            _lib.check(st, allow=() if strict else (_lib.GDX_ERR_QUERY_STATUS,))
            n = total.value
            hits = np.ctypeslib.as_array(C.cast(ptr, u64p), shape=(max(n, 1) * 2,))[: 2 * n].reshape(n, 2).copy() \
                if n else np.zeros((0, 2), dtype=np.uint64)
        finally:
            if ptr:
                self._lib.gdx_free_hits(ptr)
        return off, hits[:, 0].copy(), hits[:, 1].copy(), status

    def count_many(self, queries):
        return self.count_raw(*pack_queries(queries))[0]

    def count(self, query) -> int:
        return int(self.count_many([query])[0])

    def locate_many(self, queries):
        qbuf, qoff = pack_queries(queries)
        off, t, p, _ = self.locate_raw(qbuf, qoff)
        t, p = t.tolist(), p.tolist()
        return [[Hit(t[h], p[h]) for h in range(int(off[q]), int(off[q + 1]))] for q in range(qoff.size - 1)]

    def locate(self, query):
        return self.locate_many([query])[0]
