//! Rust binding of libgdx.so (include/gdx.h) with safe wrappers named like genedex's API.
//!
//! NOT compiled in this repository's image (no rustc/cargo); kept as the reference-side stub a
//! genedex maintainer would add, e.g. as `src/gpu.rs` behind a `gpu` cargo feature, linking with
//! `cargo:rustc-link-lib=dylib=gdx`.  It is a parallel type (`GpuFmIndex`), not `FmIndex<I, R>` itself:
//! the reference's `FmIndex` is generic over a sealed operator trait whose methods are called one
//! rank at a time (text_with_rank_support/mod.rs:88-133); a GPU cannot be driven at that granularity,
//! so the drop-in point is the batched public API (`count_many`, `locate_many`,
//! `cursors_for_many_queries`, lib.rs:155-246), whose signatures are mirrored here: any
//! `IntoIterator<Item: AsRef<[u8]>>` in, lazy iterators out (the results are computed by one call and
//! then handed out lazily).
#![allow(non_camel_case_types)]

use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct gdx_fastx_t {
    _private: [u8; 0],
}
#[repr(C)]
pub struct gdx_index_t {
    _private: [u8; 0],
}
#[repr(C)]
pub struct gdx_multi_t {
    _private: [u8; 0],
}
#[repr(C)]
pub struct gdx_parts_t {
    _private: [u8; 0],
}

/// lib.rs:331-335
#[repr(C)]
#[derive(Debug, Clone, Copy, PartialEq, Eq, PartialOrd, Ord, Hash)]
pub struct Hit {
    pub text_id: u64,
    pub position: u64,
}

/// gdx_hit32_t: a hit as two u32 (what the device writes; Hit widened on demand)
#[repr(C)]
#[derive(Debug, Clone, Copy, PartialEq, Eq, PartialOrd, Ord, Hash)]
pub struct Hit32 {
    pub text_id: u32,
    pub position: u32,
}

/// gdx_hits32_t: narrow results in pinned memory of the library's (gdx_locate_many_alloc_layout32)
#[repr(C)]
pub struct Hits32Raw {
    pub hit_offsets: *mut u32,
    pub hits: *mut Hit32,
    pub total_hits: u64,
    pub nq: u64,
    pub reserved: [u64; 2],
}

/// gdx_build_options_t: which derived acceleration structures an index carries (include/gdx.h).
/// `BuildOptions::default()` -- every field at its default -- builds the library's DEFAULT SHAPE (round 6): seed table + text
/// units + full and inverse suffix array + pair lines + top table, no jump table (104 GB at hg38 scale), the one index that
/// serves count / locate, exact intervals, cursors and reads from repeats at their best measured speeds; setting any of
/// jump_entry_bytes / full_suffix_array / text_units / seed_symbols / inverse_suffix_array makes the fields mean what they say.
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct BuildOptions {
    pub struct_size: u32,
    pub pair_lines: i32,       // -1 default, 0 off, 1 on
    pub jump_entry_bytes: i32, // -1 default (none in the default shape, else 32), 0, 8, 16, 32
    pub top_table_depth: i32,  // -1 default, 0 none, 1..=16
    pub aux_budget_bytes: u64, // 0 = default
    pub full_suffix_array: i32, // -1 / 0 off, 1: SA[row] of every row as its own array
    pub text_units: i32,        // -1 / 0 off, 1: the text at 4 bits per symbol (count / locate compare with it)
    pub seed_symbols: i32,      // -1 / 0 off, 1: seed table with k from the text length, 8..=24: that k
    pub seed_load_percent: i32, // 0 = default (60 in the default shape, else 70)
    pub inverse_suffix_array: i32, // -1 / 0 off, 1: ISA as its own array (exact intervals through the seed table)
    pub reference_table_layout: i32, // -1 / 0 this library's table, 1..=4: Condensed64 / Condensed512 / Flat64 / Flat512 as genedex builds them
}
impl Default for BuildOptions {
    fn default() -> Self {
        let mut o = std::mem::MaybeUninit::<BuildOptions>::uninit();
        unsafe {
            gdx_build_options_init(o.as_mut_ptr());
            o.assume_init()
        }
    }
}

/// gdx_query_options_t: kernel variants of the query calls on a handle (results never depend on them).
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct QueryOptions {
    pub struct_size: u32,
    pub search_kernel: i32,
    pub search_lanes: i32,
    pub load_policy: i32,
    pub length_schedule: i32,
    pub locate_kernel: i32,
    pub locate_jump_walk: i32,
    pub search_defer_after: i32,
    pub search_fast: i32,
    pub search_exact: i32,
    /// host-pointer locate calls return at most this many hits per query, the first ones in suffix-array order:
    /// `locate(q).take(k)` on the reference's lazy iterator (lib.rs:187-197); 0 = all
    pub max_hits_per_query: u32,
    pub search_seed: i32, // -1 default (on when the index has a seed table), 0 off
}

/// gdx_device_shard_t / gdx_gathered_t: gdx_multi_locate_many_gather_dev (device-resident shards, results gathered on the
/// root replica's GPU with ncclSend / ncclRecv)
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct DeviceShard {
    pub d_qbuf: *const c_void,
    pub d_qoff: *const c_void,
    pub nq: u64,
}
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct Gathered {
    pub d_counts: *mut c_void,
    pub d_hit_offsets: *mut c_void,
    pub d_hits: *mut c_void,
    pub d_status: *mut c_void,
    pub nq: u64,
    pub total_hits: u64,
    pub device_id: i32,
    pub used_rccl: i32,
}

pub const GDX_OK: c_int = 0;
pub const GDX_ERR_CAPACITY: c_int = 5;
pub const GDX_ERR_QUERY_STATUS: c_int = 6;
pub const GDX_SEGMENTS_LF_ONLY: u32 = 1;
pub const GDX_HAMMING_INVALID: u32 = 0xFFFF_FFFF;
pub const GDX_EDIT_MAX_QUERY_LEN: u32 = 256;
pub const GDX_EDIT_INVALID: u32 = 0xFFFF_FFFF;
pub const GDX_EDIT_TOO_LONG: u32 = 0xFFFF_FFFE;
pub const GDX_EDIT_NO_END: u32 = 0xFFFF_FFFF;
pub const GDX_CIGAR_INS: u32 = 1;
pub const GDX_CIGAR_DEL: u32 = 2;
pub const GDX_CIGAR_EQ: u32 = 7;
pub const GDX_CIGAR_DIFF: u32 = 8;
pub const GDX_CAND_NONE: u32 = 0xFFFF_FFFF;
pub const GDX_CAND_BAD_SEEDS: u8 = 1;
pub const GDX_CAND_MAX_ANCHORS: u32 = 1024;
pub const GDX_BEST_NONE: u32 = 0xFFFF_FFFF;
pub const GDX_BEST_MAPQ_NONE: u32 = 255;
pub const GDX_BEST_MAX_GROUP_SLOTS: u32 = 64;
pub const GDX_PAIR_NONE: u32 = 0xFFFF_FFFF;
pub const GDX_PAIR_MAPQ_NONE: u32 = 255;
pub const GDX_PAIR_MAX_MATE_SLOTS: u32 = 32;
pub const GDX_RESCUE_NONE: u32 = 0xFFFF_FFFF;
pub const GDX_RESCUE_NOT_TRIED: u32 = 0xFFFF_FFFD;
pub const GDX_RESCUE_MAX_SPREAD: u32 = 4096;
pub const GDX_SAM_SINGLE: u32 = 0;
pub const GDX_SAM_PAIRED: u32 = 1;
pub const GDX_SAM_BAD_RECORD: u8 = 1;
pub const GDX_SAM_MAX_RUN_SUM: u32 = 1 << 24;
pub const GDX_CIGAR_SOFT_CLIP: u32 = 4;
pub const GDX_CLIP_NO_SCORE: u32 = 0x8000_0000;
pub const GDX_CLIP_BAD_CIGAR: u8 = 1;
pub const GDX_CLIP_MAX_RUN_SUM: u32 = 65536;
pub const GDX_CLIP_MAX_SCORE_PARAM: u32 = 1024;

/// gdx_query_layout_t
#[repr(C)]
pub struct QueryLayout {
    pub struct_size: u32,
    pub packed: i32,      // 0: IO symbols, 1: 2-bit codes (A C G T of the DNA alphabets)
    pub uniform_len: u64, // 0: offsets array; L: every read has L symbols, no offsets
}

/// gdx_sam_inputs_t: the argument block of gdx_sam_records_many[_dev] (include/gdx_experimental.h "SAM records").  Unused
/// pointers are null; `dense_to_io` is a host pointer in both forms, every other pointer a device pointer in the device form.
#[repr(C)]
pub struct SamInputs {
    pub qbuf: *const c_void,
    pub qoff: *const c_void,
    pub nq: u64,
    pub layout: *const QueryLayout,
    pub n_reads: u64,
    pub strands: u32,
    pub mode: u32,
    pub max_edits: u32,
    pub reserved: u32,
    pub win_query: *const c_void,
    pub win_hits: *const c_void,
    pub dist: *const c_void,
    pub begin: *const c_void,
    pub end: *const c_void,
    pub n_cigar: *const c_void,
    pub cigar: *const c_void,
    pub mapq: *const c_void,
    pub proper: *const c_void,
    pub names: *const c_void,
    pub name_off: *const c_void,
    pub text_names: *const c_void,
    pub text_name_off: *const c_void,
    pub dense_to_io: *const u8,
    pub workspace: *mut c_void,
    pub workspace_bytes: u64,
    pub rec_off: *mut c_void,
    pub out: *mut c_void,
    pub out_capacity: u64,
    pub status: *mut c_void,
}

extern "C" {
    pub fn gdx_last_error() -> *const c_char;
    pub fn gdx_build_options_init(opts: *mut BuildOptions);
    pub fn gdx_query_options_init(opts: *mut QueryOptions);
    pub fn gdx_index_build_ex(
        texts_buf: *const u8, text_offsets: *const u64, n_texts: u64, io_to_dense: *const u8,
        sigma: c_int, n_searchable: c_int, sa_rate: u64, lookup_depth: c_int, index_width: c_int,
        device_id: c_int, opts: *const BuildOptions, out: *mut *mut gdx_index_t,
    ) -> c_int;
    /// table_kind 0 = condensed, 1 = flat; block_bits 64 | 512 (FmIndexCondensed64/512, FmIndexFlat64/512)
    pub fn gdx_index_from_parts_ex2(
        table_kind: c_int, block_bits: c_int, count: *const u64, interleaved_blocks: *const u64, n: u64,
        sa_samples: *const u32, sa_rate: u64, border_keys: *const u64, border_vals: *const u64,
        sentinel_indices: *const u64, n_texts: u64, io_to_dense: *const u8, sigma: c_int, n_searchable: c_int,
        lookup_depth: c_int, index_width: c_int, device_id: c_int, opts: *const BuildOptions,
        out: *mut *mut gdx_index_t,
    ) -> c_int;
    pub fn gdx_index_save(ix: *const gdx_index_t, path: *const c_char) -> c_int;
    pub fn gdx_index_load_ex(
        path: *const c_char, device_id: c_int, opts: *const BuildOptions, out: *mut *mut gdx_index_t,
    ) -> c_int;
    pub fn gdx_index_free(ix: *mut gdx_index_t);
    pub fn gdx_index_set_query_options(ix: *mut gdx_index_t, opts: *const QueryOptions) -> c_int;
    pub fn gdx_count_many(
        ix: *const gdx_index_t, qbuf: *const u8, qoff: *const u64, nq: u64, out_counts: *mut u64,
        out_status: *mut u8,
    ) -> c_int;
    pub fn gdx_cursors_for_many_queries(
        ix: *const gdx_index_t, qbuf: *const u8, qoff: *const u64, nq: u64, out_start: *mut u64,
        out_end: *mut u64, out_status: *mut u8,
    ) -> c_int;
    /// one pass, library-allocated hit array (release with gdx_free_hits)
    pub fn gdx_locate_many_alloc(
        ix: *const gdx_index_t, qbuf: *const u8, qoff: *const u64, nq: u64, out_hit_offsets: *mut u64,
        out_hits: *mut *mut Hit, out_total: *mut u64, out_status: *mut u8,
    ) -> c_int;
    pub fn gdx_free_hits(hits: *mut Hit);
    /// query layouts (include/gdx.h): packed = 2-bit codes, uniform_len = L: read i is symbols [i L, (i + 1) L), qoff may be null
    pub fn gdx_query_layout_init(layout: *mut QueryLayout);
    pub fn gdx_packed_bytes(n_symbols: u64) -> u64;
    pub fn gdx_pack_queries(
        ix: *const gdx_index_t, qbuf: *const u8, qoff: *const u64, nq: u64, out_packed: *mut u8,
        out_exceptions: *mut u64, exceptions_capacity: u64, out_n_exceptions: *mut u64,
    ) -> c_int;
    pub fn gdx_count_many_layout(
        ix: *const gdx_index_t, qbuf: *const u8, qoff: *const u64, nq: u64, layout: *const QueryLayout,
        out_counts: *mut u64, out_status: *mut u8,
    ) -> c_int;
    pub fn gdx_locate_many_alloc_layout(
        ix: *const gdx_index_t, qbuf: *const u8, qoff: *const u64, nq: u64, layout: *const QueryLayout,
        out_hit_offsets: *mut u64, out_hits: *mut *mut Hit, out_total: *mut u64, out_status: *mut u8,
    ) -> c_int;
    /// narrow results (u32 offsets, 8-byte hits) in pinned memory the library owns; release with gdx_free_hits32
    pub fn gdx_locate_many_alloc_layout32(
        ix: *const gdx_index_t, qbuf: *const u8, qoff: *const u64, nq: u64, layout: *const QueryLayout,
        out_results: *mut Hits32Raw, out_status: *mut u8,
    ) -> c_int;
    pub fn gdx_free_hits32(results: *mut Hits32Raw);
    pub fn gdx_release_cached_hits();
    pub fn gdx_cursor_empty(ix: *const gdx_index_t, start: *mut u64, end: *mut u64) -> c_int;
    pub fn gdx_cursor_extend_front_many(
        ix: *const gdx_index_t, start: *mut u64, end: *mut u64, io_symbols: *const u8, m: u64,
        out_status: *mut u8,
    ) -> c_int;
    /// every cursor extended by a whole string (right to left) in one launch
    pub fn gdx_cursor_extend_front_strings(
        ix: *const gdx_index_t, start: *mut u64, end: *mut u64, qbuf: *const u8, qoff: *const u64, m: u64,
        status: *mut u8,
    ) -> c_int;
    pub fn gdx_cursor_locate_many(
        ix: *const gdx_index_t, start: *const u64, end: *const u64, m: u64, out_hit_offsets: *mut u64,
        hits: *mut Hit, hits_capacity: u64, out_total: *mut u64,
    ) -> c_int;
    /// per query its longest matching suffix segments, rightmost first (include/gdx.h "greedy suffix segments");
    /// flags: 0 or GDX_SEGMENTS_LF_ONLY
    pub fn gdx_suffix_segments_many(
        ix: *const gdx_index_t, qbuf: *const u8, qoff: *const u64, nq: u64, max_segments: u32, flags: u32,
        out_n_segments: *mut u32, out_remaining: *mut u32, out_length: *mut u32, out_start: *mut u64, out_end: *mut u64,
        out_status: *mut u8,
    ) -> c_int;
    pub fn gdx_suffix_segments_many_dev(
        ix: *const gdx_index_t, d_qbuf: *const c_void, d_qoff: *const c_void, nq: u64, max_segments: u32, flags: u32,
        d_n_segments: *mut c_void, d_remaining: *mut c_void, d_length: *mut c_void, d_start: *mut c_void,
        d_end: *mut c_void, d_status: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    /// per query its super-maximal exact matches, rightmost first (include/gdx.h "super-maximal exact matches");
    /// ix_reversed: an index of the same texts, each reversed
    pub fn gdx_smems_many(
        ix: *const gdx_index_t, ix_reversed: *const gdx_index_t, qbuf: *const u8, qoff: *const u64, nq: u64, max_smems: u32,
        min_length: u32, out_n_smems: *mut u32, out_remaining: *mut u32, out_begin: *mut u32, out_length: *mut u32,
        out_start: *mut u64, out_end: *mut u64, out_status: *mut u8,
    ) -> c_int;
    pub fn gdx_smems_many_dev(
        ix: *const gdx_index_t, ix_reversed: *const gdx_index_t, d_qbuf: *const c_void, d_qoff: *const c_void, nq: u64,
        max_smems: u32, min_length: u32, d_n_smems: *mut c_void, d_remaining: *mut c_void, d_begin: *mut c_void,
        d_length: *mut c_void, d_start: *mut c_void, d_end: *mut c_void, d_status: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    /// both strands (include/gdx.h "both strands"): the stock complement table, the bytes of an expanded batch, the expand
    /// of a device-resident batch, and count / locate of every read as given (row 2i) and reverse-complemented (row 2i + 1)
    pub fn gdx_dna_complement_table(out: *mut u8);
    pub fn gdx_strands_out_bytes(total_symbols: u64, packed: c_int, mode: u32) -> u64;
    pub fn gdx_strands_expand_dev(
        ix: *const gdx_index_t, d_qbuf: *const c_void, d_qoff: *const c_void, nq: u64, layout: *const QueryLayout,
        total_symbols: u64, complement: *const u8, mode: u32, d_out_qbuf: *mut c_void, d_out_qoff: *mut c_void,
        stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_count_many_strands(
        ix: *const gdx_index_t, qbuf: *const u8, qoff: *const u64, nq: u64, complement: *const u8, out_counts: *mut u64,
        out_status: *mut u8,
    ) -> c_int;
    pub fn gdx_locate_many_alloc_strands(
        ix: *const gdx_index_t, qbuf: *const u8, qoff: *const u64, nq: u64, complement: *const u8, out_hit_offsets: *mut u64,
        out_hits: *mut *mut Hit, out_total: *mut u64, out_status: *mut u8,
    ) -> c_int;
    /// Hamming verification of located seeds (include/gdx.h "Hamming verification"): per candidate (query, seed begin,
    /// located hit) the mismatches of the whole read against its text on the seed's diagonal, capped at max_mismatches + 1
    pub fn gdx_hamming_many_dev(
        ix: *const gdx_index_t, d_qbuf: *const c_void, d_qoff: *const c_void, nq: u64, layout: *const QueryLayout,
        d_cand_query: *const c_void, d_cand_begin: *const c_void, d_cand_hits: *const c_void, m: u64, max_mismatches: u32,
        d_out: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_hamming_many(
        ix: *const gdx_index_t, qbuf: *const u8, qoff: *const u64, nq: u64, cand_query: *const u32, cand_begin: *const u32,
        cand_hits: *const Hit, m: u64, max_mismatches: u32, out: *mut u32,
    ) -> c_int;
    /// Edit-distance verification of located seeds (include/gdx.h "edit-distance verification"): per candidate the infix
    /// edit distance of the whole read against its text within max_edits of the seed's diagonal, capped at max_edits + 1, and
    /// the exclusive end of the leftmost best alignment (d_out_end / out_end may be null)
    pub fn gdx_edit_distance_many_dev(
        ix: *const gdx_index_t, d_qbuf: *const c_void, d_qoff: *const c_void, nq: u64, layout: *const QueryLayout,
        d_cand_query: *const c_void, d_cand_begin: *const c_void, d_cand_hits: *const c_void, m: u64, max_edits: u32,
        d_out_dist: *mut c_void, d_out_end: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_edit_distance_many(
        ix: *const gdx_index_t, qbuf: *const u8, qoff: *const u64, nq: u64, cand_query: *const u32, cand_begin: *const u32,
        cand_hits: *const Hit, m: u64, max_edits: u32, out_dist: *mut u32, out_end: *mut u32,
    ) -> c_int;
    /// Alignment traceback of verified seed hits (include/gdx.h "alignment traceback"): per candidate of
    /// gdx_edit_distance_many its distance and end, where the canonical best alignment begins and its run-length CIGAR
    /// (2 max_edits + 1 words per candidate, run_length << 4 | GDX_CIGAR_*).  d_workspace null: the size query, which
    /// writes out_workspace_bytes[0..2] (least, best) and launches nothing
    pub fn gdx_align_many_dev(
        ix: *const gdx_index_t, d_qbuf: *const c_void, d_qoff: *const c_void, nq: u64, layout: *const QueryLayout,
        d_cand_query: *const c_void, d_cand_begin: *const c_void, d_cand_hits: *const c_void, m: u64, max_edits: u32,
        d_out_dist: *mut c_void, d_out_begin: *mut c_void, d_out_end: *mut c_void, d_out_n_cigar: *mut c_void,
        d_out_cigar: *mut c_void, d_workspace: *mut c_void, workspace_bytes: u64, out_workspace_bytes: *mut u64,
        stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_align_many(
        ix: *const gdx_index_t, qbuf: *const u8, qoff: *const u64, nq: u64, cand_query: *const u32, cand_begin: *const u32,
        cand_hits: *const Hit, m: u64, max_edits: u32, out_dist: *mut u32, out_begin: *mut u32, out_end: *mut u32,
        out_n_cigar: *mut u32, out_cigar: *mut u32,
    ) -> c_int;
    /// Seed-hit candidates (include/gdx_experimental.h "seed-hit candidates"): the seed slots of nq queries, in the layout
    /// gdx_smems_many[_dev] writes, as ranked, de-duplicated candidates in slots of stride max_candidates that go straight
    /// into the verify calls; unused slots hold cand_query GDX_CAND_NONE and zeros
    pub fn gdx_seed_candidates_many_dev(
        ix: *const gdx_index_t, nq: u64, max_seeds: u32, d_n_seeds: *const c_void, d_begin: *const c_void, d_length: *const c_void,
        d_start: *const c_void, d_end: *const c_void, max_occ: u32, band: u32, max_candidates: u32, d_n_candidates: *mut c_void,
        d_n_groups: *mut c_void, d_n_skipped: *mut c_void, d_cand_query: *mut c_void, d_cand_begin: *mut c_void,
        d_cand_hits: *mut c_void, d_cand_weight: *mut c_void, d_status: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_seed_candidates_many(
        ix: *const gdx_index_t, nq: u64, max_seeds: u32, n_seeds: *const u32, begin: *const u32, length: *const u32,
        start: *const u64, end: *const u64, max_occ: u32, band: u32, max_candidates: u32, out_n_candidates: *mut u32,
        out_n_groups: *mut u32, out_n_skipped: *mut u32, out_cand_query: *mut u32, out_cand_begin: *mut u32,
        out_cand_hits: *mut Hit, out_cand_weight: *mut u32, out_status: *mut u8,
    ) -> c_int;
    /// Best hit per read (include/gdx_experimental.h "best hit per read"): every group of group_slots consecutive candidate
    /// slots with the distances of a verify call -> the best slot, its distance, the runner-up's, the counts, a mapping quality
    /// and the winner as a one-slot candidate; a group without a live slot gets GDX_BEST_NONE, GDX_BEST_MAPQ_NONE and the none
    /// pattern.  d_end / end may be null
    pub fn gdx_best_hits_many_dev(
        ix: *const gdx_index_t, n_groups: u64, group_slots: u32, d_cand_query: *const c_void, d_cand_begin: *const c_void,
        d_cand_hits: *const c_void, d_dist: *const c_void, d_end: *const c_void, max_dist: u32, d_best_slot: *mut c_void,
        d_best_dist: *mut c_void, d_sub_dist: *mut c_void, d_n_live: *mut c_void, d_n_best: *mut c_void, d_mapq: *mut c_void,
        d_win_query: *mut c_void, d_win_begin: *mut c_void, d_win_hits: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_best_hits_many(
        ix: *const gdx_index_t, n_groups: u64, group_slots: u32, cand_query: *const u32, cand_begin: *const u32,
        cand_hits: *const Hit, dist: *const u32, end: *const u32, max_dist: u32, out_best_slot: *mut u32, out_best_dist: *mut u32,
        out_sub_dist: *mut u32, out_n_live: *mut u32, out_n_best: *mut u32, out_mapq: *mut u32, out_win_query: *mut u32,
        out_win_begin: *mut u32, out_win_hits: *mut Hit,
    ) -> c_int;
    /// Paired-end pairing (include/gdx_experimental.h "paired-end pairing"): 2 * n_pairs mates of mate_slots consecutive
    /// candidate slots with the distances of a verify call -> per pair the best proper combination (one text, opposite strands,
    /// min_insert <= span <= max_insert), its counts and mapping quality; per mate the winner as a one-slot candidate, the
    /// single-end best when the pair has no proper combination.  d_end / end may be null
    pub fn gdx_pair_hits_many_dev(
        ix: *const gdx_index_t, n_pairs: u64, mate_slots: u32, d_cand_query: *const c_void, d_cand_begin: *const c_void,
        d_cand_hits: *const c_void, d_dist: *const c_void, d_end: *const c_void, max_dist: u32, min_insert: u32, max_insert: u32,
        d_n_proper: *mut c_void, d_n_best: *mut c_void, d_pair_dist: *mut c_void, d_sub_dist: *mut c_void, d_mapq: *mut c_void,
        d_pair_span: *mut c_void, d_mate_slot: *mut c_void, d_mate_dist: *mut c_void, d_win_query: *mut c_void,
        d_win_begin: *mut c_void, d_win_hits: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_pair_hits_many(
        ix: *const gdx_index_t, n_pairs: u64, mate_slots: u32, cand_query: *const u32, cand_begin: *const u32,
        cand_hits: *const Hit, dist: *const u32, end: *const u32, max_dist: u32, min_insert: u32, max_insert: u32,
        out_n_proper: *mut u32, out_n_best: *mut u32, out_pair_dist: *mut u32, out_sub_dist: *mut u32, out_mapq: *mut u32,
        out_pair_span: *mut u32, out_mate_slot: *mut u32, out_mate_dist: *mut u32, out_win_query: *mut u32,
        out_win_begin: *mut u32, out_win_hits: *mut Hit,
    ) -> c_int;
    /// Mate rescue (include/gdx_experimental.h "mate rescue"): for every pair without a proper combination, each placed mate is
    /// the anchor from which the other mate's opposite strand is searched in the insert window of the anchor's text (queries
    /// 4p .. 4p + 3 are both strands of both mates of pair p); per mate the attempt's distance and end, per pair the better
    /// successful attempt, and the merged winners for gdx_align_many in place of those of gdx_pair_hits_many
    pub fn gdx_mate_rescue_many_dev(
        ix: *const gdx_index_t, d_qbuf: *const c_void, d_qoff: *const c_void, nq: u64, layout: *const QueryLayout, n_pairs: u64,
        mate_slots: u32, d_end: *const c_void, d_n_proper: *const c_void, d_mate_slot: *const c_void, d_mate_dist: *const c_void,
        d_win_query: *const c_void, d_win_begin: *const c_void, d_win_hits: *const c_void, max_edits: u32, min_insert: u32,
        max_insert: u32, d_resc_dist: *mut c_void, d_resc_end: *mut c_void, d_resc_mate: *mut c_void, d_resc_pair_dist: *mut c_void,
        d_resc_span: *mut c_void, d_out_win_query: *mut c_void, d_out_win_begin: *mut c_void, d_out_win_hits: *mut c_void,
        stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_mate_rescue_many(
        ix: *const gdx_index_t, qbuf: *const u8, qoff: *const u64, nq: u64, n_pairs: u64, mate_slots: u32, end: *const u32,
        n_proper: *const u32, mate_slot: *const u32, mate_dist: *const u32, win_query: *const u32, win_begin: *const u32,
        win_hits: *const Hit, max_edits: u32, min_insert: u32, max_insert: u32, out_resc_dist: *mut u32, out_resc_end: *mut u32,
        out_resc_mate: *mut u32, out_resc_pair_dist: *mut u32, out_resc_span: *mut u32, out_win_query: *mut u32,
        out_win_begin: *mut u32, out_win_hits: *mut Hit,
    ) -> c_int;
    /// SAM records (include/gdx_experimental.h "SAM records"): one record per read from the winners and the outputs of
    /// gdx_align_many for them, written into `out` at the offsets `rec_off`; `out` null is the sizing call
    pub fn gdx_sam_workspace_bytes(n_reads: u64) -> u64;
    pub fn gdx_sam_record_bound(max_read_len: u64, max_name_len: u64, max_text_name_len: u64, max_edits: u32) -> u64;
    pub fn gdx_sam_records_many_dev(ix: *const gdx_index_t, input: *const SamInputs, stream: *mut c_void) -> c_int;
    pub fn gdx_sam_records_many(ix: *const gdx_index_t, input: *const SamInputs) -> c_int;
    /// Soft clipping (include/gdx_experimental.h "soft clipping"): per candidate of gdx_align_many the best-scoring contiguous
    /// part of its runs under match / mismatch / gap_open / gap_extend, S runs (op 4) around it, begin and end moved inwards,
    /// the edits that stay and the score (i32; 0x80000000 for a candidate without an alignment); `out_status` may be null
    pub fn gdx_soft_clip_many_dev(
        ix: *const gdx_index_t, m: u64, max_edits: u32, r#match: u32, mismatch: u32, gap_open: u32, gap_extend: u32, min_score: u32,
        d_dist: *const c_void, d_begin: *const c_void, d_end: *const c_void, d_n_cigar: *const c_void, d_cigar: *const c_void,
        d_out_score: *mut c_void, d_out_dist: *mut c_void, d_out_begin: *mut c_void, d_out_end: *mut c_void,
        d_out_clip_left: *mut c_void, d_out_clip_right: *mut c_void, d_out_n_cigar: *mut c_void, d_out_cigar: *mut c_void,
        d_out_status: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_soft_clip_many(
        ix: *const gdx_index_t, m: u64, max_edits: u32, r#match: u32, mismatch: u32, gap_open: u32, gap_extend: u32, min_score: u32,
        dist: *const u32, begin: *const u32, end: *const u32, n_cigar: *const u32, cigar: *const u32, out_score: *mut i32,
        out_dist: *mut u32, out_begin: *mut u32, out_end: *mut u32, out_clip_left: *mut u32, out_clip_right: *mut u32,
        out_n_cigar: *mut u32, out_cigar: *mut u32, out_status: *mut u8,
    ) -> c_int;
    pub fn gdx_rank_many(
        ix: *const gdx_index_t, symbols: *const u8, idx: *const u64, m: u64, out: *mut u64,
    ) -> c_int;
    // device-resident variants take *const c_void device pointers and a hipStream_t.  The step calls that follow are declared in
    // include/gdx_experimental.h since round 6 (the core call is gdx_locate_many_step_compact_layout_dev: the whole count + locate
    // step in one call); they stay exported.  The fused count + locate in steps:
    pub fn gdx_locate_many_search_dev(
        ix: *const gdx_index_t, d_qbuf: *const c_void, d_qoff: *const c_void, nq: u64, d_records: *mut c_void,
        stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_locate_many_offsets_dev(
        ix: *const gdx_index_t, d_records: *const c_void, nq: u64, d_hit_offsets: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_locate_workspace_bytes(total_hits: u64) -> u64;
    pub fn gdx_locate_many_hits_dev(
        ix: *const gdx_index_t, d_records: *const c_void, nq: u64, d_hit_offsets: *const c_void, total_hits: u64,
        d_hits: *mut c_void, d_workspace: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    // the same with compact results beside the records (u32 per query: position of the only hit, !0 = none, !1 = see the
    // record): on an index with a seed table scan and locate stream 4 bytes per query instead of 16
    pub fn gdx_locate_many_search_compact_dev(
        ix: *const gdx_index_t, d_qbuf: *const c_void, d_qoff: *const c_void, nq: u64, d_records: *mut c_void,
        d_compact: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_locate_many_offsets_compact_dev(
        ix: *const gdx_index_t, d_records: *const c_void, d_compact: *const c_void, nq: u64, max_hits: u32,
        d_hit_offsets: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_locate_many_hits_compact_dev(
        ix: *const gdx_index_t, d_records: *const c_void, d_compact: *const c_void, nq: u64, d_hit_offsets: *const c_void,
        total_hits: u64, d_hits: *mut c_void, d_workspace: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    // offsets and hits around the one host round trip: totals (u64[2] on the device: all hit slots, slots behind "see the
    // record") -> read back, size d_hits -> offsets + the compactly answered hits in one pass, then the rest
    pub fn gdx_locate_many_totals_workspace_bytes(nq: u64) -> u64;
    pub fn gdx_locate_many_totals_compact_dev(
        ix: *const gdx_index_t, d_records: *const c_void, d_compact: *const c_void, nq: u64, max_hits: u32,
        d_scan_workspace: *mut c_void, d_totals: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_locate_many_offsets_hits_compact_dev(
        ix: *const gdx_index_t, d_records: *const c_void, d_compact: *const c_void, nq: u64, max_hits: u32,
        d_scan_workspace: *const c_void, d_hit_offsets: *mut c_void, total_hits: u64, rest_hits: u64, d_hits: *mut c_void,
        d_workspace: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    /// the whole count + locate step of a device-resident batch in one call, no host round trip (gdx.h)
    pub fn gdx_locate_many_step_compact_layout_dev(
        ix: *const gdx_index_t, d_qbuf: *const c_void, d_qoff: *const c_void, nq: u64, layout: *const QueryLayout,
        max_hits: u32, d_records: *mut c_void, d_compact: *mut c_void, d_scan_workspace: *mut c_void, d_totals: *mut c_void,
        d_hit_offsets: *mut c_void, offsets_width: u32, d_hits: *mut c_void, hits_capacity: u64, d_workspace: *mut c_void,
        event_after_search: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    /// a located shard on its way to another device: a bit per read + the found reads' positions + the exceptions (gdx.h)
    pub fn gdx_wire_bitmap_bytes(nq: u64) -> u64;
    pub fn gdx_wire_pack_workspace_bytes(nq: u64) -> u64;
    pub fn gdx_wire_pack_dev(
        ix: *const gdx_index_t, d_compact: *const c_void, d_hit_offsets: *const c_void, offsets_width: u32,
        d_hits: *const c_void, nq: u64, d_bitmap: *mut c_void, d_tile_found: *mut c_void, d_found_pos: *mut c_void,
        found_capacity: u64, d_exc_queries: *mut c_void, d_exc_counts: *mut c_void, exc_capacity: u64,
        d_exc_text_ids: *mut c_void, d_exc_positions: *mut c_void, exc_hits_capacity: u64, d_meta: *mut c_void,
        d_workspace: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_wire_split_dev(
        ix: *const gdx_index_t, d_bitmap: *const c_void, d_tile_found: *const c_void, d_found_pos: *const c_void,
        found_capacity: u64, nq: u64, d_exc_queries: *const c_void, d_meta: *const c_void, exc_capacity: u64,
        d_out_text_ids: *mut c_void, d_out_positions: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    pub fn gdx_index_seed_info(ix: *const gdx_index_t, out: *mut u64) -> c_int;
    /// out[4]: records of two-copy repeats, of three- and four-copy repeats, their bytes, 0
    pub fn gdx_index_seed_records(ix: *const gdx_index_t, out: *mut u64) -> c_int;
    /// an index built with `reference_table_layout`: genedex's own interleaved blocks and superblock offsets as they sit in HBM
    pub fn gdx_index_export_reference_table(
        ix: *const gdx_index_t, interleaved_blocks: *mut u64, capacity_words: u64, out_n_words: *mut u64,
        interleaved_superblock_offsets: *mut u32, capacity_offsets: u64, out_n_offsets: *mut u64,
    ) -> c_int;
    pub fn gdx_locate_many_unpack_compact_dev(
        ix: *const gdx_index_t, d_records: *const c_void, d_compact: *const c_void, nq: u64, d_out_counts: *mut c_void,
        d_out_status: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    /// compact results as text id bytes + positions in the text (-1 none, -2 see the record): the multi-GPU gather's form
    pub fn gdx_compact_split_hits_dev(
        ix: *const gdx_index_t, d_compact: *const c_void, nq: u64, d_out_text_ids: *mut c_void, d_out_positions: *mut c_void,
        stream: *mut c_void,
    ) -> c_int;
    /// the queries whose compact result says "see the record" (unordered, up to `capacity`); *d_out_n (u64) = all of them
    pub fn gdx_compact_exceptions_dev(
        ix: *const gdx_index_t, d_compact: *const c_void, nq: u64, d_out_queries: *mut c_void, capacity: u64,
        d_out_n: *mut c_void, stream: *mut c_void,
    ) -> c_int;
    // several GPUs of one node behind one handle
    pub fn gdx_multi_build(
        texts_buf: *const u8, text_offsets: *const u64, n_texts: u64, io_to_dense: *const u8, sigma: c_int,
        n_searchable: c_int, sa_rate: u64, lookup_depth: c_int, index_width: c_int, device_ids: *const c_int,
        n_devices: c_int, opts: *const BuildOptions, out: *mut *mut gdx_multi_t,
    ) -> c_int;
    pub fn gdx_multi_free(m: *mut gdx_multi_t);
    // collections beyond 2^32 - 1 symbols as several 32-bit indexes cut at text borders (count / locate); a single text
    // beyond that, or cursors over the whole collection: build with index_width 64 (the 64-bit engine) instead
    pub fn gdx_parts_build(
        texts_buf: *const c_void, texts_on_device: c_int, text_offsets: *const u64, n_texts: u64, io_to_dense: *const u8,
        sigma: c_int, n_searchable: c_int, sa_rate: u64, lookup_depth: c_int, device_id: c_int, max_part_symbols: u64,
        opts: *const BuildOptions, out: *mut *mut gdx_parts_t,
    ) -> c_int;
    pub fn gdx_parts_free(p: *mut gdx_parts_t);
    pub fn gdx_parts_info(p: *const gdx_parts_t, out: *mut u64) -> c_int;
    pub fn gdx_parts_set_query_options(p: *mut gdx_parts_t, opts: *const QueryOptions) -> c_int;
    pub fn gdx_parts_count_many(
        p: *const gdx_parts_t, qbuf: *const u8, qoff: *const u64, nq: u64, out_counts: *mut u64, out_status: *mut u8,
    ) -> c_int;
    pub fn gdx_parts_locate_many_alloc(
        p: *const gdx_parts_t, qbuf: *const u8, qoff: *const u64, nq: u64, out_hit_offsets: *mut u64,
        out_hits: *mut *mut Hit, out_total: *mut u64, out_status: *mut u8,
    ) -> c_int;
    pub fn gdx_multi_set_query_options(m: *mut gdx_multi_t, opts: *const QueryOptions) -> c_int;
    pub fn gdx_multi_locate_many_gather_dev(
        m: *mut gdx_multi_t, shards: *const DeviceShard, n_shards: c_int, root: c_int, out: *mut Gathered,
    ) -> c_int;
    pub fn gdx_multi_count_many(
        m: *const gdx_multi_t, qbuf: *const u8, qoff: *const u64, nq: u64, out_counts: *mut u64, out_status: *mut u8,
    ) -> c_int;
    pub fn gdx_multi_locate_many_alloc(
        m: *const gdx_multi_t, qbuf: *const u8, qoff: *const u64, nq: u64, out_hit_offsets: *mut u64,
        out_hits: *mut *mut Hit, out_total: *mut u64, out_status: *mut u8,
    ) -> c_int;
    // FASTA / FASTQ ingestion into (qbuf, qoff) batches (host only)
    pub fn gdx_fastx_open(path: *const c_char, out: *mut *mut gdx_fastx_t) -> c_int;
    pub fn gdx_fastx_next_batch(
        reader: *mut gdx_fastx_t, qbuf: *mut u8, qbuf_capacity: u64, qoff: *mut u64, max_records: u64, n_out: *mut u64,
    ) -> c_int;
    /// the same; *out_uniform_len = the batch's common read length (0 when they differ): gdx_query_layout_t.uniform_len
    pub fn gdx_fastx_next_batch_ex(
        reader: *mut gdx_fastx_t, qbuf: *mut u8, qbuf_capacity: u64, qoff: *mut u64, max_records: u64, n_out: *mut u64,
        out_uniform_len: *mut u64,
    ) -> c_int;
    pub fn gdx_fastx_close(reader: *mut gdx_fastx_t);
}

fn check(rc: c_int) {
    if rc != GDX_OK {
        let msg = unsafe { CStr::from_ptr(gdx_last_error()) }.to_string_lossy().into_owned();
        panic!("gdx: {msg}"); // the reference panics in the same situations
    }
}

fn pack<Q: AsRef<[u8]>>(queries: impl IntoIterator<Item = Q>) -> (Vec<u8>, Vec<u64>) {
    let (mut buf, mut off) = (Vec::new(), vec![0u64]);
    for q in queries {
        buf.extend_from_slice(q.as_ref());
        off.push(buf.len() as u64);
    }
    (buf, off)
}

/// One candidate's alignment (`GpuFmIndex::align_many`): `dist` edits; the query against text[span.0 .. span.1) with the
/// runs `cigar`, each (length, GDX_CIGAR_*), first run of the query first.  `span` is None (and `cigar` empty) when dist is
/// over the limit or a GDX_EDIT_* marker.
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct Alignment {
    pub dist: u32,
    pub span: Option<(u32, u32)>,
    pub cigar: Vec<(u32, u32)>,
}

/// One group's best hit (`GpuFmIndex::best_hits_many`): `slot` is None for a group without a live slot (then best_dist =
/// sub_dist = max_dist + 1, mapq = GDX_BEST_MAPQ_NONE and `winner` is (GDX_CAND_NONE, 0, {0, 0})).  `winner` = (cand_query,
/// cand_begin, hit) of the best slot, a candidate of `align_many`.
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct BestHit {
    pub slot: Option<u32>,
    pub best_dist: u32,
    pub sub_dist: u32,
    pub n_live: u32,
    pub n_best: u32,
    pub mapq: u32,
    pub winner: (u32, u32, Hit),
}

/// One mate of a `PairHit`: `slot` is None for a mate without a live slot (then dist = max_dist + 1 and `winner` is
/// (GDX_CAND_NONE, 0, {0, 0})).  `winner` = (cand_query, cand_begin, hit) of the slot, a candidate of `align_many`.
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct MateHit {
    pub slot: Option<u32>,
    pub dist: u32,
    pub winner: (u32, u32, Hit),
}

/// One pair's result (`GpuFmIndex::pair_hits_many`): without a proper combination n_proper = n_best = 0, pair_dist = sub_dist =
/// 2 max_dist + 2, pair_span = 0, mapq = GDX_PAIR_MAPQ_NONE and `mates` are the single-end bests.
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct PairHit {
    pub n_proper: u32,
    pub n_best: u32,
    pub pair_dist: u32,
    pub sub_dist: u32,
    pub mapq: u32,
    pub pair_span: u32,
    pub mates: [MateHit; 2],
}

/// One pair after `GpuFmIndex::mate_rescue_many`.  `attempts[o]` = (resc_dist, resc_end) of mate o: dist GDX_RESCUE_NOT_TRIED where
/// no attempt exists, max_edits + 1 (and end GDX_EDIT_NO_END) where it found nothing.  `rescued` = Some(o) when mate o was placed
/// from the other mate; then pair_dist is the anchor's distance plus the attempt's and span the fragment's length, otherwise
/// 2 max_edits + 2 and 0.  `winners` = (cand_query, cand_begin, hit) per mate, candidates of `align_many`.
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct RescuedPair {
    pub attempts: [(u32, u32); 2],
    pub rescued: Option<u32>,
    pub pair_dist: u32,
    pub span: u32,
    pub winners: [(u32, u32, Hit); 2],
}

/// Hits of one call, owned by the library's allocation; handed out per query without copying.
pub struct Hits {
    ptr: *mut Hit,
    total: usize,
    offsets: Vec<u64>,
}
impl Drop for Hits {
    fn drop(&mut self) {
        unsafe { gdx_free_hits(self.ptr) }
    }
}
impl Hits {
    /// hits of query i, in suffix-array order (lib.rs:187-197)
    pub fn of(&self, i: usize) -> &[Hit] {
        let (a, b) = (self.offsets[i] as usize, self.offsets[i + 1] as usize);
        if self.total == 0 { &[] } else { unsafe { std::slice::from_raw_parts(self.ptr.add(a), b - a) } }
    }
    /// the shape of `FmIndex::locate_many`: an iterator over queries of iterators over hits
    pub fn iter(&self) -> impl Iterator<Item = impl Iterator<Item = Hit> + '_> + '_ {
        (0..self.offsets.len() - 1).map(move |i| self.of(i).iter().copied())
    }
}

/// The result of `GpuFmIndex::locate_many_packed`: u32 offsets and 8-byte hits where the device wrote them (pinned memory of
/// the library's; given back on drop).  Same shape of access as `Hits`.
pub struct Hits32 {
    raw: Hits32Raw,
}
impl Drop for Hits32 {
    fn drop(&mut self) {
        unsafe { gdx_free_hits32(&mut self.raw) }
    }
}
impl Hits32 {
    pub fn of(&self, i: usize) -> &[Hit32] {
        let off = unsafe { std::slice::from_raw_parts(self.raw.hit_offsets, self.raw.nq as usize + 1) };
        let (a, b) = (off[i] as usize, off[i + 1] as usize);
        if self.raw.total_hits == 0 { &[] } else { unsafe { std::slice::from_raw_parts(self.raw.hits.add(a), b - a) } }
    }
    pub fn iter(&self) -> impl Iterator<Item = impl Iterator<Item = Hit> + '_> + '_ {
        (0..self.raw.nq as usize).map(move |i| {
            self.of(i).iter().map(|h| Hit { text_id: h.text_id as u64, position: h.position as u64 })
        })
    }
}

/// Owns an index replica in HBM.  Send + Sync like `FmIndex` (handles are immutable).
pub struct GpuFmIndex {
    raw: *mut gdx_index_t,
}
unsafe impl Send for GpuFmIndex {}
unsafe impl Sync for GpuFmIndex {}

impl Drop for GpuFmIndex {
    fn drop(&mut self) {
        unsafe { gdx_index_free(self.raw) }
    }
}

#[derive(Clone, Copy)]
pub struct GpuCursor<'a> {
    index: &'a GpuFmIndex,
    start: u64,
    end: u64,
}

impl GpuFmIndex {
    /// `FmIndexConfig::<I>::construct_index` (config.rs:63-69); `io_to_dense` is
    /// `Alphabet::io_to_dense_representation_table` (alphabet.rs:25).
    pub fn construct<T: AsRef<[u8]>>(
        texts: impl IntoIterator<Item = T>, io_to_dense: &[u8; 256], sigma: usize, n_searchable: usize,
        sa_rate: usize, lookup_depth: usize, index_width: i32, device: i32, options: &BuildOptions,
    ) -> Self {
        let (buf, off) = pack(texts);
        let mut raw = std::ptr::null_mut();
        check(unsafe {
            gdx_index_build_ex(buf.as_ptr(), off.as_ptr(), off.len() as u64 - 1, io_to_dense.as_ptr(), sigma as c_int,
                               n_searchable as c_int, sa_rate as u64, lookup_depth as c_int, index_width, device,
                               options, &mut raw)
        });
        Self { raw }
    }

    /// lib.rs:155-161
    pub fn count_many<Q: AsRef<[u8]>>(&self, queries: impl IntoIterator<Item = Q>) -> impl Iterator<Item = usize> {
        let (buf, off) = pack(queries);
        let nq = off.len() - 1;
        let mut counts = vec![0u64; nq];
        check(unsafe { gdx_count_many(self.raw, buf.as_ptr(), off.as_ptr(), nq as u64, counts.as_mut_ptr(), std::ptr::null_mut()) });
        counts.into_iter().map(|c| c as usize)
    }

    /// lib.rs:147-149
    pub fn count(&self, query: &[u8]) -> usize {
        self.count_many([query]).next().unwrap()
    }

    /// count_many for a batch of sequencer reads of one length, as a FASTQ reader holds them: `reads` = the reads back to
    /// back (ASCII).  They cross PCIe as 2-bit codes without offsets (gdx_query_layout_t { packed, uniform_len }); reads
    /// with a symbol outside A C G T (the packed form's exceptions) are counted through the plain call.  Same counts as
    /// count_many (lib.rs:155-161).
    pub fn count_reads(&self, reads: &[u8], read_len: usize) -> Vec<usize> {
        assert!(read_len > 0 && reads.len() % read_len == 0);
        let nq = reads.len() / read_len;
        let off: Vec<u64> = (0..=nq).map(|i| (i * read_len) as u64).collect();
        let mut packed = vec![0u8; unsafe { gdx_packed_bytes(reads.len() as u64) } as usize];
        let mut exceptions = vec![0u64; nq.max(1)];
        let mut n_exc = 0u64;
        check(unsafe {
            gdx_pack_queries(self.raw, reads.as_ptr(), off.as_ptr(), nq as u64, packed.as_mut_ptr(), exceptions.as_mut_ptr(),
                             nq as u64, &mut n_exc)
        });
        let mut layout = QueryLayout { struct_size: 0, packed: 0, uniform_len: 0 };
        unsafe { gdx_query_layout_init(&mut layout) };
        layout.packed = 1;
        layout.uniform_len = read_len as u64;
        let mut counts = vec![0u64; nq];
        check(unsafe {
            gdx_count_many_layout(self.raw, packed.as_ptr(), std::ptr::null(), nq as u64, &layout, counts.as_mut_ptr(),
                                  std::ptr::null_mut())
        });
        let mut out: Vec<usize> = counts.into_iter().map(|c| c as usize).collect();
        for &q in &exceptions[..n_exc as usize] {
            let q = q as usize;
            out[q] = self.count(&reads[q * read_len..(q + 1) * read_len]);
        }
        out
    }

    /// lib.rs:179-185, one pass (search, scan, locate pipelined over chunks of the batch)
    pub fn locate_many<Q: AsRef<[u8]>>(&self, queries: impl IntoIterator<Item = Q>) -> Hits {
        let (buf, off) = pack(queries);
        let nq = off.len() - 1;
        let mut offsets = vec![0u64; nq + 1];
        let (mut total, mut ptr) = (0u64, std::ptr::null_mut());
        check(unsafe {
            gdx_locate_many_alloc(self.raw, buf.as_ptr(), off.as_ptr(), nq as u64, offsets.as_mut_ptr(), &mut ptr,
                                  &mut total, std::ptr::null_mut())
        });
        Hits { ptr, total: total as usize, offsets }
    }

    /// count_many on both strands: per read (occurrences as given, occurrences of its reverse complement under the stock
    /// IUPAC complement table).  The reads cross PCIe once; the reverse complements are made on the device.
    pub fn count_many_both_strands<Q: AsRef<[u8]>>(&self, queries: impl IntoIterator<Item = Q>) -> Vec<(usize, usize)> {
        let (buf, off) = pack(queries);
        let nq = off.len() - 1;
        let mut counts = vec![0u64; 2 * nq];
        check(unsafe {
            gdx_count_many_strands(self.raw, buf.as_ptr(), off.as_ptr(), nq as u64, std::ptr::null(), counts.as_mut_ptr(),
                                   std::ptr::null_mut())
        });
        counts.chunks(2).map(|c| (c[0] as usize, c[1] as usize)).collect()
    }

    /// locate_many on both strands: `of(2 * i)` are the hits of read i as given, `of(2 * i + 1)` those of its reverse
    /// complement (the read maps to the reverse strand there; position = the leftmost text coordinate of the alignment)
    pub fn locate_many_both_strands<Q: AsRef<[u8]>>(&self, queries: impl IntoIterator<Item = Q>) -> Hits {
        let (buf, off) = pack(queries);
        let nq = off.len() - 1;
        let mut offsets = vec![0u64; 2 * nq + 1];
        let (mut total, mut ptr) = (0u64, std::ptr::null_mut());
        check(unsafe {
            gdx_locate_many_alloc_strands(self.raw, buf.as_ptr(), off.as_ptr(), nq as u64, std::ptr::null(), offsets.as_mut_ptr(),
                                          &mut ptr, &mut total, std::ptr::null_mut())
        });
        Hits { ptr, total: total as usize, offsets }
    }

    /// lib.rs:179-185 for reads of one length handed over as 2-bit codes (gdx_pack_queries): 12.5 bytes per len-50 read go in,
    /// 12 bytes per result come out, and no host thread copies a result
    pub fn locate_many_packed(&self, packed: &[u8], n_reads: usize, read_len: usize) -> Hits32 {
        let mut lay = QueryLayout { struct_size: std::mem::size_of::<QueryLayout>() as u32, packed: 1, uniform_len: read_len as u64 };
        let mut raw = Hits32Raw { hit_offsets: std::ptr::null_mut(), hits: std::ptr::null_mut(), total_hits: 0, nq: 0, reserved: [0; 2] };
        check(unsafe {
            gdx_locate_many_alloc_layout32(self.raw, packed.as_ptr(), std::ptr::null(), n_reads as u64, &mut lay, &mut raw,
                                           std::ptr::null_mut())
        });
        Hits32 { raw }
    }

    /// lib.rs:169-177
    pub fn locate(&self, query: &[u8]) -> impl Iterator<Item = Hit> {
        self.locate_many([query]).of(0).to_vec().into_iter()
    }

    /// lib.rs:241-246
    pub fn cursors_for_many_queries<'a, Q: AsRef<[u8]>>(
        &'a self, queries: impl IntoIterator<Item = Q>,
    ) -> impl Iterator<Item = GpuCursor<'a>> {
        let (buf, off) = pack(queries);
        let nq = off.len() - 1;
        let (mut s, mut e) = (vec![0u64; nq], vec![0u64; nq]);
        check(unsafe {
            gdx_cursors_for_many_queries(self.raw, buf.as_ptr(), off.as_ptr(), nq as u64, s.as_mut_ptr(), e.as_mut_ptr(),
                                         std::ptr::null_mut())
        });
        s.into_iter().zip(e).map(move |(start, end)| GpuCursor { index: self, start, end })
    }

    /// lib.rs:217-235
    pub fn cursor_for_query(&self, query: &[u8]) -> GpuCursor<'_> {
        self.cursors_for_many_queries([query]).next().unwrap()
    }

    /// lib.rs:202-210
    pub fn cursor_empty(&self) -> GpuCursor<'_> {
        let (mut start, mut end) = (0u64, 0u64);
        check(unsafe { gdx_cursor_empty(self.raw, &mut start, &mut end) });
        GpuCursor { index: self, start, end }
    }

    /// Batched form of the cursor API (ROADMAP.md:33): every cursor extended by its own string, last symbol first,
    /// in ONE launch (up to 32 LF steps per memory fetch), instead of one launch per symbol.
    pub fn extend_cursors_front<'a, Q: AsRef<[u8]>>(
        &'a self, cursors: &mut [GpuCursor<'a>], strings: impl IntoIterator<Item = Q>,
    ) {
        let (buf, off) = pack(strings);
        assert_eq!(off.len() - 1, cursors.len());
        let mut s: Vec<u64> = cursors.iter().map(|c| c.start).collect();
        let mut e: Vec<u64> = cursors.iter().map(|c| c.end).collect();
        check(unsafe {
            gdx_cursor_extend_front_strings(self.raw, s.as_mut_ptr(), e.as_mut_ptr(), buf.as_ptr(), off.as_ptr(),
                                            cursors.len() as u64, std::ptr::null_mut())
        });
        for (c, (start, end)) in cursors.iter_mut().zip(s.into_iter().zip(e)) {
            c.start = start;
            c.end = end;
        }
    }

    /// Per query its longest matching suffix segments, rightmost first, as (query_end, length, cursor):
    /// query[query_end - length .. query_end] is the longest suffix of query[..query_end] that occurs; a segment of
    /// length 0 stands for one symbol that occurs nowhere (its cursor is empty).  At most `max_segments` per query.
    pub fn suffix_segments_many<'a, Q: AsRef<[u8]>>(
        &'a self, queries: impl IntoIterator<Item = Q>, max_segments: u32,
    ) -> Vec<Vec<(usize, usize, GpuCursor<'a>)>> {
        let (buf, off) = pack(queries);
        let nq = off.len() - 1;
        let slots = nq * max_segments as usize;
        let (mut n_seg, mut remaining, mut length) = (vec![0u32; nq], vec![0u32; nq], vec![0u32; slots]);
        let (mut s, mut e) = (vec![0u64; slots], vec![0u64; slots]);
        check(unsafe {
            gdx_suffix_segments_many(self.raw, buf.as_ptr(), off.as_ptr(), nq as u64, max_segments, 0, n_seg.as_mut_ptr(),
                                     remaining.as_mut_ptr(), length.as_mut_ptr(), s.as_mut_ptr(), e.as_mut_ptr(),
                                     std::ptr::null_mut())
        });
        (0..nq)
            .map(|i| {
                let mut end_at = (off[i + 1] - off[i]) as usize;
                (0..n_seg[i] as usize)
                    .map(|j| {
                        let k = i * max_segments as usize + j;
                        let seg = (end_at, length[k] as usize, GpuCursor { index: self, start: s[k], end: e[k] });
                        end_at -= std::cmp::max(length[k] as usize, 1);
                        seg
                    })
                    .collect()
            })
            .collect()
    }

    /// Per query its super-maximal exact matches as (query_begin, query_end, cursor), by descending end: the matches
    /// query[query_begin .. query_end] that no other match of the query contains, those shorter than `min_length` left
    /// out, at most `max_smems` per query.  `reversed` is an index of the same texts, each reversed; the cursors are
    /// intervals of `self`.
    pub fn smems_many<'a, Q: AsRef<[u8]>>(
        &'a self, reversed: &GpuFmIndex, queries: impl IntoIterator<Item = Q>, max_smems: u32, min_length: u32,
    ) -> Vec<Vec<(usize, usize, GpuCursor<'a>)>> {
        let (buf, off) = pack(queries);
        let nq = off.len() - 1;
        let slots = nq * max_smems as usize;
        let (mut n_smems, mut remaining) = (vec![0u32; nq], vec![0u32; nq]);
        let (mut begin, mut length) = (vec![0u32; slots], vec![0u32; slots]);
        let (mut s, mut e) = (vec![0u64; slots], vec![0u64; slots]);
        check(unsafe {
            gdx_smems_many(self.raw, reversed.raw, buf.as_ptr(), off.as_ptr(), nq as u64, max_smems, min_length,
                           n_smems.as_mut_ptr(), remaining.as_mut_ptr(), begin.as_mut_ptr(), length.as_mut_ptr(),
                           s.as_mut_ptr(), e.as_mut_ptr(), std::ptr::null_mut())
        });
        (0..nq)
            .map(|i| {
                (0..n_smems[i] as usize)
                    .map(|j| {
                        let k = i * max_smems as usize + j;
                        let b = begin[k] as usize;
                        (b, b + length[k] as usize, GpuCursor { index: self, start: s[k], end: e[k] })
                    })
                    .collect()
            })
            .collect()
    }

    /// The link between `smems_many` and the verify calls: per query its verification candidates (seed begin, hit, weight),
    /// best first, at most `max_candidates` each.  `seeds[i]` is what `smems_many` returned for query i.  Seeds on more than
    /// `max_occ` rows are left out; hits of one text within `band` diagonals of a group's first are ONE candidate, whose
    /// weight is the number of query symbols its seeds cover.  Element (b, hit, w) of query i goes into `hamming_many` /
    /// `edit_distance_many` / `align_many` as cand_query = i, cand_begin = b, cand_hits = hit.  Panics when the most seeds of
    /// a query times `max_occ` exceeds GDX_CAND_MAX_ANCHORS and on an index without SA[row] in one fetch.
    pub fn seed_candidates_many(
        &self, seeds: &[Vec<(usize, usize, GpuCursor<'_>)>], max_occ: u32, band: u32, max_candidates: u32,
    ) -> Vec<Vec<(u32, Hit, u32)>> {
        let nq = seeds.len();
        let ms = seeds.iter().map(|s| s.len()).max().unwrap_or(0).max(1);
        let n_seeds: Vec<u32> = seeds.iter().map(|s| s.len() as u32).collect();
        let (mut begin, mut length) = (vec![0u32; nq * ms], vec![0u32; nq * ms]);
        let (mut s, mut e) = (vec![0u64; nq * ms], vec![0u64; nq * ms]);
        for (i, list) in seeds.iter().enumerate() {
            for (j, (b, end, cursor)) in list.iter().enumerate() {
                let k = i * ms + j;
                begin[k] = *b as u32;
                length[k] = (*end - *b) as u32;
                s[k] = cursor.start;
                e[k] = cursor.end;
            }
        }
        let slots = nq * max_candidates as usize;
        let (mut n_cand, mut n_groups, mut n_skipped) = (vec![0u32; nq], vec![0u32; nq], vec![0u32; nq]);
        let (mut cq, mut cb, mut cw) = (vec![0u32; slots], vec![0u32; slots], vec![0u32; slots]);
        let mut hits = vec![Hit { text_id: 0, position: 0 }; slots];
        check(unsafe {
            gdx_seed_candidates_many(self.raw, nq as u64, ms as u32, n_seeds.as_ptr(), begin.as_ptr(), length.as_ptr(), s.as_ptr(),
                                     e.as_ptr(), max_occ, band, max_candidates, n_cand.as_mut_ptr(), n_groups.as_mut_ptr(),
                                     n_skipped.as_mut_ptr(), cq.as_mut_ptr(), cb.as_mut_ptr(), hits.as_mut_ptr(), cw.as_mut_ptr(),
                                     std::ptr::null_mut())
        });
        (0..nq)
            .map(|i| {
                (0..n_cand[i] as usize)
                    .map(|c| {
                        let k = i * max_candidates as usize + c;
                        (cb[k], hits[k], cw[k])
                    })
                    .collect()
            })
            .collect()
    }

    /// The reduction behind the verify calls: the slots are groups of `group_slots` consecutive candidates (`group_slots` =
    /// the candidates call's max_candidates makes a group a query), `dist` what `hamming_many` / `edit_distance_many` gave for
    /// them and `end` the ends of the latter, or None.  Per group the slot with the least (dist, slot) among those within
    /// `max_dist`, duplicates of one locus counted once, with the runner-up's distance, the counts and a mapping quality.
    /// Panics when `group_slots` is 0 or above GDX_BEST_MAX_GROUP_SLOTS, `max_dist` above 2^31, or the slices do not hold a
    /// whole number of groups.
    pub fn best_hits_many(
        &self, group_slots: u32, cand_query: &[u32], cand_begin: &[u32], cand_hits: &[Hit], dist: &[u32], end: Option<&[u32]>,
        max_dist: u32,
    ) -> Vec<BestHit> {
        let m = cand_query.len();
        assert!(group_slots != 0 && m % group_slots as usize == 0);
        assert!(cand_begin.len() == m && cand_hits.len() == m && dist.len() == m && end.map_or(true, |e| e.len() == m));
        let ng = m / group_slots as usize;
        let mut out: Vec<Vec<u32>> = (0..8).map(|_| vec![0u32; ng]).collect();
        let mut win = vec![Hit { text_id: 0, position: 0 }; ng];
        let p: Vec<*mut u32> = out.iter_mut().map(|v| v.as_mut_ptr()).collect();
        check(unsafe {
            gdx_best_hits_many(self.raw, ng as u64, group_slots, cand_query.as_ptr(), cand_begin.as_ptr(), cand_hits.as_ptr(),
                               dist.as_ptr(), end.map_or(std::ptr::null(), |e| e.as_ptr()), max_dist, p[0], p[1], p[2], p[3], p[4],
                               p[5], p[6], p[7], win.as_mut_ptr())
        });
        (0..ng)
            .map(|g| BestHit {
                slot: if out[0][g] == GDX_BEST_NONE { None } else { Some(out[0][g]) },
                best_dist: out[1][g],
                sub_dist: out[2][g],
                n_live: out[3][g],
                n_best: out[4][g],
                mapq: out[5][g],
                winner: (out[6][g], out[7][g], win[g]),
            })
            .collect()
    }

    /// Paired-end pairing: the slots are mates of `mate_slots` consecutive candidates, mates 2p and 2p + 1 making pair p;
    /// `dist` / `end` as in `best_hits_many`.  Per pair the best combination of one live slot of each mate that lies on one
    /// text, on opposite strands and with min_insert <= span <= max_insert, whether it is unique, and per mate the winner.
    /// Panics when `mate_slots` is 0 or above GDX_PAIR_MAX_MATE_SLOTS, `max_dist` above 2^30, the insert bounds are not
    /// min_insert <= max_insert <= 2^31 - 1, or the slices do not hold a whole number of pairs.
    pub fn pair_hits_many(
        &self, mate_slots: u32, cand_query: &[u32], cand_begin: &[u32], cand_hits: &[Hit], dist: &[u32], end: Option<&[u32]>,
        max_dist: u32, min_insert: u32, max_insert: u32,
    ) -> Vec<PairHit> {
        let m = cand_query.len();
        assert!(mate_slots != 0 && m % (2 * mate_slots as usize) == 0);
        assert!(cand_begin.len() == m && cand_hits.len() == m && dist.len() == m && end.map_or(true, |e| e.len() == m));
        let np = m / (2 * mate_slots as usize);
        let mut pairs: Vec<Vec<u32>> = (0..6).map(|_| vec![0u32; np]).collect();
        let mut mates: Vec<Vec<u32>> = (0..4).map(|_| vec![0u32; 2 * np]).collect();
        let mut win = vec![Hit { text_id: 0, position: 0 }; 2 * np];
        let p: Vec<*mut u32> = pairs.iter_mut().map(|v| v.as_mut_ptr()).collect();
        let q: Vec<*mut u32> = mates.iter_mut().map(|v| v.as_mut_ptr()).collect();
        check(unsafe {
            gdx_pair_hits_many(self.raw, np as u64, mate_slots, cand_query.as_ptr(), cand_begin.as_ptr(), cand_hits.as_ptr(),
                               dist.as_ptr(), end.map_or(std::ptr::null(), |e| e.as_ptr()), max_dist, min_insert, max_insert,
                               p[0], p[1], p[2], p[3], p[4], p[5], q[0], q[1], q[2], q[3], win.as_mut_ptr())
        });
        let mate = |x: usize| MateHit {
            slot: if mates[0][x] == GDX_PAIR_NONE { None } else { Some(mates[0][x]) },
            dist: mates[1][x],
            winner: (mates[2][x], mates[3][x], win[x]),
        };
        (0..np)
            .map(|g| PairHit {
                n_proper: pairs[0][g],
                n_best: pairs[1][g],
                pair_dist: pairs[2][g],
                sub_dist: pairs[3][g],
                mapq: pairs[4][g],
                pair_span: pairs[5][g],
                mates: [mate(2 * g), mate(2 * g + 1)],
            })
            .collect()
    }

    /// Mate rescue behind `pair_hits_many`: `queries` are the four strands of every pair (mate 0, its reverse complement, mate 1,
    /// its reverse complement), `end` the ends `edit_distance_many` gave for all 2 * pairs * mate_slots slots and `pairs` what
    /// `pair_hits_many` returned for them.  For a pair without a proper combination every placed mate serves as the anchor from
    /// which the other mate is searched, on the opposite strand, where min_insert <= span <= max_insert puts it, with at most
    /// `max_edits` (at most 256) edits.  Panics when the slices do not fit `pairs`, on insert bounds that are not min_insert <=
    /// max_insert <= 2^31 - 1 or lie more than GDX_RESCUE_MAX_SPREAD apart, and on an index without text units.
    pub fn mate_rescue_many<Q: AsRef<[u8]>>(
        &self, queries: impl IntoIterator<Item = Q>, mate_slots: u32, end: &[u32], pairs: &[PairHit], max_edits: u32, min_insert: u32,
        max_insert: u32,
    ) -> Vec<RescuedPair> {
        let np = pairs.len();
        let (buf, off) = pack(queries);
        assert!(off.len() - 1 == 4 * np && end.len() == 2 * np * mate_slots as usize);
        let mates = || pairs.iter().flat_map(|p| p.mates.iter());
        let n_proper: Vec<u32> = pairs.iter().map(|p| p.n_proper).collect();
        let mate_slot: Vec<u32> = mates().map(|m| m.slot.unwrap_or(GDX_PAIR_NONE)).collect();
        let mate_dist: Vec<u32> = mates().map(|m| m.dist).collect();
        let win_query: Vec<u32> = mates().map(|m| m.winner.0).collect();
        let win_begin: Vec<u32> = mates().map(|m| m.winner.1).collect();
        let win_hits: Vec<Hit> = mates().map(|m| m.winner.2).collect();
        let mut per_mate: Vec<Vec<u32>> = (0..4).map(|_| vec![0u32; 2 * np]).collect();
        let mut per_pair: Vec<Vec<u32>> = (0..3).map(|_| vec![0u32; np]).collect();
        let mut win = vec![Hit { text_id: 0, position: 0 }; 2 * np];
        let m: Vec<*mut u32> = per_mate.iter_mut().map(|v| v.as_mut_ptr()).collect();
        let p: Vec<*mut u32> = per_pair.iter_mut().map(|v| v.as_mut_ptr()).collect();
        check(unsafe {
            gdx_mate_rescue_many(self.raw, buf.as_ptr(), off.as_ptr(), (off.len() - 1) as u64, np as u64, mate_slots, end.as_ptr(),
                                 n_proper.as_ptr(), mate_slot.as_ptr(), mate_dist.as_ptr(), win_query.as_ptr(), win_begin.as_ptr(),
                                 win_hits.as_ptr(), max_edits, min_insert, max_insert, m[0], m[1], p[0], p[1], p[2], m[2], m[3],
                                 win.as_mut_ptr())
        });
        (0..np)
            .map(|g| RescuedPair {
                attempts: [(per_mate[0][2 * g], per_mate[1][2 * g]), (per_mate[0][2 * g + 1], per_mate[1][2 * g + 1])],
                rescued: if per_pair[0][g] == GDX_RESCUE_NONE { None } else { Some(per_pair[0][g]) },
                pair_dist: per_pair[1][g],
                span: per_pair[2][g],
                winners: [(per_mate[2][2 * g], per_mate[3][2 * g], win[2 * g]), (per_mate[2][2 * g + 1], per_mate[3][2 * g + 1], win[2 * g + 1])],
            })
            .collect()
    }

    /// Seed and verify: candidate c says that the seed of `queries[cand_query[c]]` that begins at symbol `cand_begin[c]` was
    /// located at `cand_hits[c]` (what `GpuCursor::locate` gives for an SMEM's cursor); entry c of the result is the number of
    /// mismatches of the WHOLE query against that text on the seed's diagonal, min(dist, max_mismatches + 1).  Symbols that
    /// hang over an end of the text, N and bytes outside the alphabet count as mismatches.  Panics on a candidate whose
    /// query or text id is out of range and on an index without text units.
    pub fn hamming_many<Q: AsRef<[u8]>>(
        &self, queries: impl IntoIterator<Item = Q>, cand_query: &[u32], cand_begin: &[u32], cand_hits: &[Hit], max_mismatches: u32,
    ) -> Vec<u32> {
        assert!(cand_query.len() == cand_begin.len() && cand_query.len() == cand_hits.len());
        let (buf, off) = pack(queries);
        let mut out = vec![0u32; cand_query.len()];
        check(unsafe {
            gdx_hamming_many(self.raw, buf.as_ptr(), off.as_ptr(), (off.len() - 1) as u64, cand_query.as_ptr(), cand_begin.as_ptr(),
                             cand_hits.as_ptr(), cand_query.len() as u64, max_mismatches, out.as_mut_ptr())
        });
        out
    }

    /// Seed and verify with indels: for the candidates of `hamming_many`, (dist, end) per candidate.  dist is the least number
    /// of substitutions, insertions and deletions that turn the WHOLE query (at most 256 symbols; longer ones get
    /// GDX_EDIT_TOO_LONG) into a piece of its text within `max_edits` (at most 256) of the seed's diagonal,
    /// min(dist, max_edits + 1); end is where the leftmost best such piece ends (exclusive), GDX_EDIT_NO_END when
    /// dist > max_edits.  Panics like `hamming_many`.
    pub fn edit_distance_many<Q: AsRef<[u8]>>(
        &self, queries: impl IntoIterator<Item = Q>, cand_query: &[u32], cand_begin: &[u32], cand_hits: &[Hit], max_edits: u32,
    ) -> (Vec<u32>, Vec<u32>) {
        assert!(cand_query.len() == cand_begin.len() && cand_query.len() == cand_hits.len());
        let (buf, off) = pack(queries);
        let mut dist = vec![0u32; cand_query.len()];
        let mut end = vec![0u32; cand_query.len()];
        check(unsafe {
            gdx_edit_distance_many(self.raw, buf.as_ptr(), off.as_ptr(), (off.len() - 1) as u64, cand_query.as_ptr(),
                                   cand_begin.as_ptr(), cand_hits.as_ptr(), cand_query.len() as u64, max_edits, dist.as_mut_ptr(),
                                   end.as_mut_ptr())
        });
        (dist, end)
    }

    /// The last stage of seed and verify: for the candidates of `edit_distance_many`, one `Alignment` per candidate.  dist is
    /// what `edit_distance_many` gives; when it is at most `max_edits` (at most 256), `span` is (begin, end) of the canonical
    /// best alignment in the candidate's text and `cigar` its runs, first run of the query first, each (length, op) with op
    /// one of GDX_CIGAR_INS / _DEL / _EQ / _DIFF; otherwise `span` is None and `cigar` empty.  Panics like `hamming_many`.
    pub fn align_many<Q: AsRef<[u8]>>(
        &self, queries: impl IntoIterator<Item = Q>, cand_query: &[u32], cand_begin: &[u32], cand_hits: &[Hit], max_edits: u32,
    ) -> Vec<Alignment> {
        assert!(cand_query.len() == cand_begin.len() && cand_query.len() == cand_hits.len());
        assert!(max_edits <= GDX_EDIT_MAX_QUERY_LEN);
        let (buf, off) = pack(queries);
        let m = cand_query.len();
        let stride = 2 * max_edits as usize + 1;
        let (mut dist, mut begin, mut end, mut n_cigar) = (vec![0u32; m], vec![0u32; m], vec![0u32; m], vec![0u32; m]);
        let mut cigar = vec![0u32; m * stride];
        check(unsafe {
            gdx_align_many(self.raw, buf.as_ptr(), off.as_ptr(), (off.len() - 1) as u64, cand_query.as_ptr(), cand_begin.as_ptr(),
                           cand_hits.as_ptr(), m as u64, max_edits, dist.as_mut_ptr(), begin.as_mut_ptr(), end.as_mut_ptr(),
                           n_cigar.as_mut_ptr(), cigar.as_mut_ptr())
        });
        (0..m)
            .map(|c| Alignment {
                dist: dist[c],
                span: if end[c] == GDX_EDIT_NO_END { None } else { Some((begin[c], end[c])) },
                cigar: cigar[c * stride..c * stride + n_cigar[c] as usize].iter().map(|w| (w >> 4, w & 15)).collect(),
            })
            .collect()
    }
}

impl<'a> GpuCursor<'a> {
    /// cursor.rs:34-38
    pub fn extend_query_front(&mut self, symbol: u8) {
        check(unsafe {
            gdx_cursor_extend_front_many(self.index.raw, &mut self.start, &mut self.end, &symbol, 1, std::ptr::null_mut())
        });
    }
    /// cursor.rs:61-63
    pub fn count(&self) -> usize {
        (self.end - self.start) as usize
    }
    /// cursor.rs:71-73
    pub fn locate(&self) -> impl Iterator<Item = Hit> {
        let mut offsets = [0u64; 2];
        let mut total = 0u64;
        let mut hits = vec![Hit { text_id: 0, position: 0 }; self.count()];
        check(unsafe {
            gdx_cursor_locate_many(self.index.raw, &self.start, &self.end, 1, offsets.as_mut_ptr(), hits.as_mut_ptr(),
                                   hits.len() as u64, &mut total)
        });
        hits.into_iter()
    }
}

/// Index replicas on several GPUs of one node behind one handle: the batch is cut into contiguous shards, one
/// pipeline thread per device; results equal the one-GPU results bit for bit.
pub struct MultiGpuFmIndex {
    raw: *mut gdx_multi_t,
}
unsafe impl Send for MultiGpuFmIndex {}
unsafe impl Sync for MultiGpuFmIndex {}
impl Drop for MultiGpuFmIndex {
    fn drop(&mut self) {
        unsafe { gdx_multi_free(self.raw) }
    }
}
impl MultiGpuFmIndex {
    pub fn construct<T: AsRef<[u8]>>(
        texts: impl IntoIterator<Item = T>, io_to_dense: &[u8; 256], sigma: usize, n_searchable: usize,
        sa_rate: usize, lookup_depth: usize, index_width: i32, devices: &[i32], options: &BuildOptions,
    ) -> Self {
        let (buf, off) = pack(texts);
        let mut raw = std::ptr::null_mut();
        check(unsafe {
            gdx_multi_build(buf.as_ptr(), off.as_ptr(), off.len() as u64 - 1, io_to_dense.as_ptr(), sigma as c_int,
                            n_searchable as c_int, sa_rate as u64, lookup_depth as c_int, index_width,
                            devices.as_ptr(), devices.len() as c_int, options, &mut raw)
        });
        Self { raw }
    }
    pub fn count_many<Q: AsRef<[u8]>>(&self, queries: impl IntoIterator<Item = Q>) -> impl Iterator<Item = usize> {
        let (buf, off) = pack(queries);
        let nq = off.len() - 1;
        let mut counts = vec![0u64; nq];
        check(unsafe { gdx_multi_count_many(self.raw, buf.as_ptr(), off.as_ptr(), nq as u64, counts.as_mut_ptr(), std::ptr::null_mut()) });
        counts.into_iter().map(|c| c as usize)
    }
    pub fn locate_many<Q: AsRef<[u8]>>(&self, queries: impl IntoIterator<Item = Q>) -> Hits {
        let (buf, off) = pack(queries);
        let nq = off.len() - 1;
        let mut offsets = vec![0u64; nq + 1];
        let (mut total, mut ptr) = (0u64, std::ptr::null_mut());
        check(unsafe {
            gdx_multi_locate_many_alloc(self.raw, buf.as_ptr(), off.as_ptr(), nq as u64, offsets.as_mut_ptr(), &mut ptr,
                                        &mut total, std::ptr::null_mut())
        });
        Hits { ptr, total: total as usize, offsets }
    }
}
