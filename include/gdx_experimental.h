/* gdx_experimental.h -- entry points of libgdx.so beside the core ABI of gdx.h: the steps of rounds 1-5 that the core calls have
 * superseded (separate search / offsets / hits calls around host round trips, the `_packed` calls that gdx_query_layout_t
 * replaced, hint arrays, compact-result plumbing of the multi-GPU gather) and building blocks the tests and bench.py still
 * drive one by one.  Exported and tested like the core (tests/test_abi.py, tests/test_gpu_*.py), but not what a binding of the
 * reference's API needs (INTEGRATION.md binds gdx.h only), and free to change.  Every call returns the results of the core call
 * it is a part of: lib.rs:155-246 of the reference.  The last four sections, "seed-hit candidates", "best hit per read",
 * "paired-end pairing" and "mate rescue", are calls of the seed-and-verify chain that the reference has no counterpart of; they
 * are declared here because the core header keeps to its budget of names (tests/test_abi.py). */
#ifndef GDX_EXPERIMENTAL_H
#define GDX_EXPERIMENTAL_H

#include "gdx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The same import for the reference's other table variants (lib.rs:102-113): table_kind 0 =
 * CondensedTextWithRankSupport (condensed.rs:24-30), 1 = FlatTextWithRankSupport (flat.rs:27-33: one
 * indicator block per symbol, 16-bit block offset in the low bits of each block); block_bits 64 = Block64,
 * 512 = Block512 (block.rs).  interleaved_blocks is passed as u64 words (a Block512 is 8 words). */
int gdx_index_from_parts_ex(int table_kind, int block_bits, const uint64_t *count,
                            const uint64_t *interleaved_blocks, uint64_t n, const uint32_t *sa_samples,
                            uint64_t sa_rate, const uint64_t *border_keys, const uint64_t *border_vals,
                            const uint64_t *sentinel_indices, uint64_t n_texts, const uint8_t *io_to_dense,
                            int sigma, int n_searchable, int lookup_depth, int index_width, int device_id,
                            gdx_index_t **out);

int gdx_cursors_for_many_queries_dev(const gdx_index_t *ix, const void *d_qbuf, const void *d_qoff /*u64*/,
                                     uint64_t nq, void *d_out_start /*u32*/, void *d_out_end /*u32*/,
                                     void *d_out_status /*u8 or NULL*/, void *stream);

int gdx_count_many_dev(const gdx_index_t *ix, const void *d_qbuf, const void *d_qoff, uint64_t nq,
                       void *d_out_counts /*u32*/, void *d_out_status, void *stream);

/* exclusive scan of (end-start) into d_hit_offsets (u64[m+1]); needs no workspace sizing */
int gdx_hit_offsets_dev(const gdx_index_t *ix, const void *d_start, const void *d_end, uint64_t m,
                        void *d_hit_offsets, void *stream);

int gdx_locate_intervals_dev(const gdx_index_t *ix, const void *d_start, const void *d_end, uint64_t m,
                             const void *d_hit_offsets, uint64_t total_hits, void *d_hits /*gdx_hit32_t*/,
                             void *d_workspace, void *stream);

/* The same two calls with a locate hint carried from the search to the locate of the SAME intervals (the device
 * form of the fused gdx_locate_many): d_hint is an opaque device array of 8 bytes per query (8-byte aligned),
 * written by gdx_cursors_for_many_queries_hint_dev and read by gdx_locate_intervals_hint_dev.  For a query whose
 * interval is one row wide it may name a sampled suffix-array row the search passed through and its distance
 * to the hit, which saves the walk of sampled_suffix_array.rs:118-131; results are identical with or without it.
 * The hint is only valid together with the d_start / d_end arrays of the call that produced it. */
int gdx_cursors_for_many_queries_hint_dev(const gdx_index_t *ix, const void *d_qbuf, const void *d_qoff, uint64_t nq,
                                          void *d_out_start, void *d_out_end, void *d_out_status, void *d_hint,
                                          void *stream);

int gdx_locate_intervals_hint_dev(const gdx_index_t *ix, const void *d_start, const void *d_end, uint64_t m,
                                  const void *d_hit_offsets, uint64_t total_hits, void *d_hits, void *d_workspace,
                                  const void *d_hint, void *stream);

/* ---- fused count + locate on the device (the device form of FmIndex::locate_many, lib.rs:179-185) -----------------
 * The search writes one opaque 16-byte record per query (d_records: 16-byte aligned, 16 * nq bytes) that carries the
 * query's number of occurrences, its status and what locate needs.  Because only the hits matter here -- not the
 * suffix-array interval itself -- the search may finish a query from a jump-table entry it already holds instead of
 * fetching one more line ("lazy tail"); counts and hits are the reference's, bit for bit and in
 * the same order.
 *   1. gdx_locate_many_search_dev     qbuf, qoff -> records
 *   2. gdx_locate_many_offsets_dev    records -> d_hit_offsets (u64[nq+1], exclusive scan of the counts);
 *                                     d_hit_offsets[nq] is the number of hits (read it back to size d_hits)
 *   3. gdx_locate_many_hits_dev       records + offsets -> d_hits (gdx_hit32_t[total]), hits of query i at
 *                                     [off[i], off[i+1]) in suffix-array order (lib.rs:187-197);
 *                                     d_workspace: gdx_locate_workspace_bytes(total) bytes
 * gdx_locate_many_unpack_dev extracts counts (u32) and / or status bytes from the records (either may be NULL). */
int gdx_locate_many_search_dev(const gdx_index_t *ix, const void *d_qbuf, const void *d_qoff /*u64*/, uint64_t nq,
                               void *d_records, void *stream);

int gdx_locate_many_offsets_dev(const gdx_index_t *ix, const void *d_records, uint64_t nq, void *d_hit_offsets,
                                void *stream);

/* the same scan with a per-query limit: a query with more than max_hits occurrences gets no hit slots (it is still
 * counted -- gdx_locate_many_unpack_dev reports its count -- but not located: what read mappers do with reads that
 * fall into repeats); max_hits = 0 means no limit */
int gdx_locate_many_offsets_capped_dev(const gdx_index_t *ix, const void *d_records, uint64_t nq, uint32_t max_hits,
                                       void *d_hit_offsets, void *stream);

int gdx_locate_many_hits_dev(const gdx_index_t *ix, const void *d_records, uint64_t nq, const void *d_hit_offsets,
                             uint64_t total_hits, void *d_hits, void *d_workspace, void *stream);

int gdx_locate_many_unpack_dev(const gdx_index_t *ix, const void *d_records, uint64_t nq, void *d_out_counts,
                               void *d_out_status, void *stream);

/* COMPACT results beside the records: d_compact (u32[nq], device) holds per query the text position of its ONLY hit
 * (concatenated texts incl. sentinels, as the resolved records), 0xffffffff = no occurrence, or 0xfffffffe = "see
 * d_records[q]" (several hits, a row that still has to be located, a status).  On an index with a seed table
 * (gdx_build_options_t.seed_symbols) the search answers nearly every read of a text without repeats this way and leaves
 * their 16-byte records untouched; offsets and hits then stream 4 bytes per query instead of 16.  On any other index every
 * entry says "see the record" (same results, no gain).  The four calls mirror gdx_locate_many_search_dev /
 * _offsets_capped_dev / _hits_dev / _unpack_dev; results are identical to theirs (lib.rs:155-185). */
int gdx_locate_many_search_compact_dev(const gdx_index_t *ix, const void *d_qbuf, const void *d_qoff, uint64_t nq,
                                       void *d_records, void *d_compact, void *stream);

int gdx_locate_many_offsets_compact_dev(const gdx_index_t *ix, const void *d_records, const void *d_compact, uint64_t nq,
                                        uint32_t max_hits, void *d_hit_offsets, void *stream);

int gdx_locate_many_hits_compact_dev(const gdx_index_t *ix, const void *d_records, const void *d_compact, uint64_t nq,
                                     const void *d_hit_offsets, uint64_t total_hits, void *d_hits, void *d_workspace, void *stream);

int gdx_locate_many_unpack_compact_dev(const gdx_index_t *ix, const void *d_records, const void *d_compact, uint64_t nq,
                                       void *d_out_counts, void *d_out_status, void *stream);

/* Compact results in the form they travel in between devices (the multi-GPU gather): per query one
 * text id byte and one int32 -- the position in that text of the query's only hit (lib.rs:155-185 Hit { text_id, position }),
 * -1 = no occurrence, -2 = "see the record" (the sender ships those queries' counts and hits beside).  5 bytes per query on
 * the receiving side from 4 on the wire.  Collections of at most 256 texts (else GDX_ERR_UNSUPPORTED); d_compact and
 * d_out_positions 16-byte aligned, d_out_text_ids 4-byte aligned. */
int gdx_compact_split_hits_dev(const gdx_index_t *ix, const void *d_compact, uint64_t nq, void *d_out_text_ids,
                               void *d_out_positions, void *stream);

/* The queries whose compact result says "see the record": their numbers (u32) into d_out_queries in NO particular order, as
 * many as `capacity` holds; *d_out_n (u64, device) = how many there are in all.  One streaming pass over d_compact (16-byte
 * aligned).  The sender of the multi-GPU gather lists its exceptions with this (on a text without repeats a few in a
 * million queries) and sorts them. */
int gdx_compact_exceptions_dev(const gdx_index_t *ix, const void *d_compact, uint64_t nq, void *d_out_queries,
                               uint64_t capacity, void *d_out_n, void *stream);

/* Offsets and hits in two calls around the ONE host round trip of a count + locate step (instead of offsets, round trip,
 * hits): gdx_locate_many_totals_compact_dev sums the counts -- d_totals (u64[2], device) = {all hit slots, the slots of the
 * queries whose compact result says "see the record"} -- and leaves the bases of its tiles in d_scan_workspace
 * (gdx_locate_many_totals_workspace_bytes(nq) bytes); the caller reads d_totals back, sizes d_hits (total_hits entries of
 * gdx_hit32_t) and d_workspace (gdx_locate_workspace_bytes(total_hits), only needed when rest_hits != 0) and calls
 * gdx_locate_many_offsets_hits_compact_dev, which writes d_hit_offsets (u64[nq + 1]) and in the SAME pass over the compact
 * results stores the hit of every query they answer, then locates the remaining rest_hits slots from the records.
 * d_compact may be NULL (records only: the second call is then the plain offsets + hits).  Same results as the other
 * record calls. */
uint64_t gdx_locate_many_totals_workspace_bytes(uint64_t nq);

int gdx_locate_many_totals_compact_dev(const gdx_index_t *ix, const void *d_records, const void *d_compact, uint64_t nq,
                                       uint32_t max_hits, void *d_scan_workspace, void *d_totals, void *stream);

int gdx_locate_many_offsets_hits_compact_dev(const gdx_index_t *ix, const void *d_records, const void *d_compact, uint64_t nq,
                                             uint32_t max_hits, const void *d_scan_workspace, void *d_hit_offsets,
                                             uint64_t total_hits, uint64_t rest_hits, void *d_hits, void *d_workspace, void *stream);

/* the same with NARROW hit offsets: d_hit_offsets32 is u32[nq + 1] (total_hits < 2^32, else GDX_ERR_INVALID_ARGUMENT): 4
 * bytes per query less to write -- a fifth of this pass's traffic on a batch of reads with one hit each */
int gdx_locate_many_offsets32_hits_compact_dev(const gdx_index_t *ix, const void *d_records, const void *d_compact, uint64_t nq,
                                               uint32_t max_hits, const void *d_scan_workspace, void *d_hit_offsets32,
                                               uint64_t total_hits, uint64_t rest_hits, void *d_hits, void *d_workspace,
                                               void *stream);

/* gdx_count_many / gdx_cursors_for_many_queries on packed host buffers (the same chunked pipeline) */
int gdx_count_many_packed(const gdx_index_t *ix, const uint8_t *packed, const uint64_t *qoff, uint64_t nq,
                          uint64_t *out_counts, uint8_t *out_status);

int gdx_cursors_for_many_queries_packed(const gdx_index_t *ix, const uint8_t *packed, const uint64_t *qoff,
                                        uint64_t nq, uint64_t *out_start, uint64_t *out_end, uint8_t *out_status);

/* the device-resident search calls on packed buffers; the rest of a locate (gdx_locate_many_offsets_dev,
 * gdx_locate_many_hits_dev) is unchanged */
int gdx_cursors_for_many_queries_packed_dev(const gdx_index_t *ix, const void *d_packed, const void *d_qoff,
                                            uint64_t nq, void *d_out_start, void *d_out_end, void *d_out_status,
                                            void *stream);

int gdx_count_many_packed_dev(const gdx_index_t *ix, const void *d_packed, const void *d_qoff, uint64_t nq,
                              void *d_out_counts, void *d_out_status, void *stream);

int gdx_locate_many_search_packed_dev(const gdx_index_t *ix, const void *d_packed, const void *d_qoff, uint64_t nq,
                                      void *d_records, void *stream);

/* gdx_locate_many_search_compact_dev / gdx_locate_many_search_dev / gdx_count_many_dev / gdx_cursors_for_many_queries_dev
 * on a batch in the given layout (FmIndex::locate_many / count_many / cursors_for_many_queries, lib.rs:155-246); the rest
 * of a locate (gdx_locate_many_totals_compact_dev, ..._offsets_hits_compact_dev, ..._hits_dev) never looks at the queries */
int gdx_locate_many_search_compact_layout_dev(const gdx_index_t *ix, const void *d_qbuf, const void *d_qoff, uint64_t nq,
                                              const gdx_query_layout_t *layout, void *d_records, void *d_compact, void *stream);

int gdx_locate_many_search_layout_dev(const gdx_index_t *ix, const void *d_qbuf, const void *d_qoff, uint64_t nq,
                                      const gdx_query_layout_t *layout, void *d_records, void *stream);

/* gdx_locate_many_search_compact_layout_dev and gdx_locate_many_totals_compact_dev in one call: d_scan_workspace
 * (gdx_locate_many_totals_workspace_bytes(nq)) and d_totals (u64[2]: all hit slots, those the compact results leave open)
 * are what gdx_locate_many_offsets_hits_compact_dev takes next.  On an index whose count / locate search is the seed
 * table's lane kernel the search counts its hits per scan tile while it stores them, and the separate pass over the compact
 * results (4 bytes per query) is gone; on any other index the call is the two calls one after the other. */
int gdx_locate_many_search_totals_compact_layout_dev(const gdx_index_t *ix, const void *d_qbuf, const void *d_qoff, uint64_t nq,
                                                     const gdx_query_layout_t *layout, uint32_t max_hits, void *d_records,
                                                     void *d_compact, void *d_scan_workspace, void *d_totals, void *stream);

int gdx_multi_from_indexes(gdx_index_t **replicas, int n_replicas, gdx_multi_t **out);

/* ---- seed-hit candidates (the link between gdx_smems_many and the verify calls of gdx.h) ---------------------------------
 * gdx_smems_many[_dev] ends at suffix-array intervals in fixed-stride slots; gdx_hamming_many, gdx_edit_distance_many and
 * gdx_align_many start at one (text_id, position) per candidate.  gdx_seed_candidates_many turns the seed slots of a batch into
 * ranked, de-duplicated candidates on the device: three seeds of one read on one diagonal are ONE candidate.
 * Inputs: nq queries, each with at most max_seeds seeds in the slot layout gdx_smems_many[_dev] writes: n_seeds[i], and seed j of
 * query i in slot i * max_seeds + j of begin, length, start, end; [start, end) are rows of ix.  The out arrays of
 * gdx_smems_many_dev are valid input unchanged, and so are arrays made from gdx_suffix_segments_many.  The query bytes are
 * not needed.
 * Knobs: max_occ >= 1: a seed on more rows than this is skipped, as mappers do with repeats.  band, any u32: diagonals this
 * close together are one candidate.  max_candidates, 1..1024: the slots per query in the output.  max_seeds * max_occ must
 * not exceed GDX_CAND_MAX_ANCHORS.
 * Per query i:
 *  1. Check.  The status is GDX_CAND_BAD_SEEDS when n_seeds[i] > max_seeds; when for some seed j < n_seeds[i] length == 0,
 *     start > end or end > n (this guards the suffix-array reads and comes before any of them); or when the seeds are not in
 *     strictly descending order of both begin and begin + length, compared in 64 bits (the order in which both seed calls
 *     report them).  Such a query gets 0 candidates, 0 groups, 0 skipped and the none pattern in all its slots.  Otherwise the
 *     status is 0.
 *  2. Anchors.  A seed with end - start > max_occ adds 1 to n_skipped[i] and gives no anchor.  Every other seed gives one anchor
 *     per row r in [start, end): (t, pos) is the hit gdx_cursor_locate_many returns for row r (SA[r] through the text-id
 *     lower bound), and d = (int64) pos - (int64) begin_j is the anchor's diagonal.  It may be negative.
 *  3. Order.  The anchors are sorted by (t, d, begin) ascending: a total order, since two anchors with the same triple would
 *     be the same text position.
 *  4. Groups.  Scanning in that order, an anchor opens a new group when it is the first, when its t differs from the group's,
 *     or when d - d_first > band, d_first being the diagonal of the group's FIRST anchor.  A group therefore never spans more
 *     than band diagonals, however long a tandem repeat's run is.  n_groups[i] is the number of groups.
 *  5. Per group.  weight = the number of query symbols covered by at least one of the group's anchors: a seed that occurs
 *     twice in the group counts once, overlapping seeds count their union (2^32 - 1 if it were more).  representative = the
 *     anchor of the greatest seed length, among equals the first in the order of step 3.
 *  6. Output.  The groups by descending weight, among equals by ascending (t, d_first); only the first max_candidates of
 *     them.  n_candidates[i] = min(n_groups[i], max_candidates).  Slot i * max_candidates + c holds cand_query = i,
 *     cand_begin = the representative's seed begin, cand_hits = {t, pos} of the representative, and cand_weight.  Unused slots
 *     hold the NONE PATTERN: cand_query = GDX_CAND_NONE, cand_begin = 0, cand_hits = {0, 0}, cand_weight = 0.
 * The slots go straight into the verify calls: an unused slot carries a query number >= nq, for which the device forms of
 * gdx_hamming_many, gdx_edit_distance_many and gdx_align_many already write their *_INVALID marker and return GDX_OK.  The
 * caller passes d_cand_query, d_cand_begin, d_cand_hits as they are with m = nq * max_candidates: no compaction, no offsets
 * pass, no synchronisation and no glue in between.  A compacted form is out of scope.
 * Device form: ONE launch, no synchronisation, no allocation, no copy from pageable memory; returns GDX_OK.  d_status may be
 * NULL.  Host form: the same arguments without the stream; start / end are u64 as gdx_smems_many writes them (a value of 2^32
 * or more: GDX_ERR_INVALID_ARGUMENT), cand_hits is gdx_hit_t, out_status may be NULL.  It stages the whole batch (copy in, one
 * launch, copy out) and returns GDX_ERR_QUERY_STATUS, after writing all outputs, when any query has a status != 0, like
 * gdx_smems_many.
 * GDX_ERR_INVALID_ARGUMENT: max_seeds, max_occ or max_candidates is 0; max_candidates > 1024; max_seeds * max_occ >
 * GDX_CAND_MAX_ANCHORS (computed in 64 bits); nq >= 2^32 - 1 (a query number must differ from GDX_CAND_NONE); a null required
 * pointer.  GDX_ERR_UNSUPPORTED: a handle of the 64-bit engine; an index on which SA[row] is not one fetch, i.e. one with
 * neither full_suffix_array nor 32-byte jump entries (the default shape has the full suffix array; the kernel does not walk).
 * nq == 0 is GDX_OK and writes nothing.  A refused call writes nothing.  gdx_parts_t and gdx_multi_t have no such call. */
#define GDX_CAND_NONE        0xFFFFFFFFu   /* cand_query of an unused slot                                */
#define GDX_CAND_BAD_SEEDS   1             /* status: the query's seed slots fail the check of step 1     */
#define GDX_CAND_MAX_ANCHORS 1024u         /* the most anchors of one query: max_seeds * max_occ at most  */
int gdx_seed_candidates_many_dev(const gdx_index_t *ix, uint64_t nq, uint32_t max_seeds, const void *d_n_seeds /*u32[nq]*/,
                                 const void *d_begin /*u32[nq * max_seeds]*/, const void *d_length /*u32[..]*/,
                                 const void *d_start /*u32[..]*/, const void *d_end /*u32[..]*/, uint32_t max_occ, uint32_t band,
                                 uint32_t max_candidates, void *d_n_candidates /*u32[nq]*/, void *d_n_groups /*u32[nq]*/,
                                 void *d_n_skipped /*u32[nq]*/, void *d_cand_query /*u32[nq * max_candidates]*/,
                                 void *d_cand_begin /*u32[..]*/, void *d_cand_hits /*gdx_hit32_t[..]*/,
                                 void *d_cand_weight /*u32[..]*/, void *d_status /*u8[nq] or NULL*/, void *stream);
int gdx_seed_candidates_many(const gdx_index_t *ix, uint64_t nq, uint32_t max_seeds, const uint32_t *n_seeds,
                             const uint32_t *begin, const uint32_t *length, const uint64_t *start, const uint64_t *end,
                             uint32_t max_occ, uint32_t band, uint32_t max_candidates, uint32_t *out_n_candidates,
                             uint32_t *out_n_groups, uint32_t *out_n_skipped, uint32_t *out_cand_query, uint32_t *out_cand_begin,
                             gdx_hit_t *out_cand_hits, uint32_t *out_cand_weight, uint8_t *out_status /*or NULL*/);

/* ---- best hit per read (the reduction between the verify calls of gdx.h and gdx_align_many) ------------------------------
 * gdx_hamming_many and gdx_edit_distance_many give one distance per candidate slot; a mapper wants one alignment per read, to
 * know whether it is unique, and a traceback of that one alone.  gdx_best_hits_many reduces every GROUP of group_slots
 * consecutive slots to one record and writes the group's winner as a one-slot candidate list.
 * Inputs: m = n_groups * group_slots slots, slot j of group g being g * group_slots + j: cand_query, cand_begin, cand_hits as
 * gdx_seed_candidates_many[_dev] writes them (group_slots = its max_candidates: a group is a query), dist as a verify call wrote
 * it for these slots, and end (gdx_edit_distance_many's out_end) or NULL.  After gdx_strands_expand_dev with GDX_STRANDS_BOTH
 * queries 2i and 2i + 1 are the two strands of read i and their 2 * max_candidates slots are adjacent: group_slots =
 * 2 * max_candidates makes a group a read.  The call never looks at the queries or at the index's arrays.
 * Per group g, with k = max_dist:
 *  1. Live.  Slot j is live when cand_query[j] != GDX_CAND_NONE and dist[j] <= k.  GDX_EDIT_INVALID, GDX_EDIT_TOO_LONG,
 *     GDX_HAMMING_INVALID and the capped value k + 1 are all > k: a dead slot needs no special case.
 *  2. Same locus.  The key of a live slot is (cand_query, text_id, e): e = end[j] when end is given, otherwise the diagonal
 *     position - cand_begin in wrapping 32-bit arithmetic (the Hamming case).  Of the live slots with one key only the one with
 *     the least (dist, j) stays live; the others are duplicates: two diagonal bands that reach the same alignment must not make
 *     a read look ambiguous.
 *  3. Results, over the slots still live.  n_live = their number.  The best slot is the one with the least (dist, j): best_slot
 *     = j, best_dist = its distance.  n_best = the live slots with dist == best_dist.  sub_dist = the least distance among the
 *     live slots other than the best one: best_dist when n_best >= 2, k + 1 when there is no other live slot.
 *     mapq = min(60, 60 * (sub_dist - best_dist) / (k + 1)), in 64 bits with integer division: 0 for a tie, 60 for a lone hit
 *     at distance 0.  A group without a live slot gets best_slot = GDX_BEST_NONE, best_dist = sub_dist = k + 1, n_live = n_best
 *     = 0 and mapq = GDX_BEST_MAPQ_NONE.  The raw fields are returned so that a caller with another quality model can apply it.
 *  4. Winner.  win_query[g], win_begin[g], win_hits[g] are cand_query, cand_begin, cand_hits of the best slot; for a group
 *     without one they hold the none pattern of the candidates call: GDX_CAND_NONE, 0, {0, 0}.
 * The three winner arrays go straight into gdx_align_many_dev, gdx_edit_distance_many_dev and gdx_hamming_many_dev with m =
 * n_groups: an unmapped read gets their *_INVALID marker there, as an unused candidate slot does.  With GDX_STRANDS_BOTH in
 * front and group_slots = 2 * max_candidates, win_query >> 1 is the read and win_query & 1 its strand.
 * Device form: ONE launch, no synchronisation, no allocation, no copy from pageable memory; returns GDX_OK.  All nine outputs
 * are u32[n_groups] (d_win_hits: gdx_hit32_t[n_groups]) and must not overlap the inputs.  Host form: the same arguments without
 * the stream; cand_hits and win_hits are gdx_hit_t (a text id or a position of 2^32 or more: GDX_ERR_INVALID_ARGUMENT).  It
 * stages the whole batch (copy in, one launch, copy out) like gdx_seed_candidates_many.
 * GDX_ERR_INVALID_ARGUMENT: group_slots == 0 or > GDX_BEST_MAX_GROUP_SLOTS; max_dist > 2^31; n_groups * group_slots does not fit
 * 64 bits; a null required pointer (only d_end / end may be null).  GDX_ERR_UNSUPPORTED: a handle of the 64-bit engine.
 * n_groups == 0 is GDX_OK and writes nothing.  A refused call writes nothing.  gdx_parts_t and gdx_multi_t have no such call.
 * Out of scope: secondary alignments beyond the counts, a compacted list of the mapped reads only.  Paired-end pairing is
 * gdx_pair_hits_many below. */
#define GDX_BEST_NONE            0xFFFFFFFFu  /* best_slot of a group without a live slot       */
#define GDX_BEST_MAPQ_NONE       255u         /* mapq of such a group (SAM: not available)      */
#define GDX_BEST_MAX_GROUP_SLOTS 64u          /* the most slots of one group                    */
int gdx_best_hits_many_dev(const gdx_index_t *ix, uint64_t n_groups, uint32_t group_slots, const void *d_cand_query /*u32[m]*/,
                           const void *d_cand_begin /*u32[m]*/, const void *d_cand_hits /*gdx_hit32_t[m]*/,
                           const void *d_dist /*u32[m]*/, const void *d_end /*u32[m] or NULL*/, uint32_t max_dist,
                           void *d_best_slot, void *d_best_dist, void *d_sub_dist, void *d_n_live, void *d_n_best,
                           void *d_mapq /*u32[n_groups] each*/, void *d_win_query /*u32[n_groups]*/,
                           void *d_win_begin /*u32[n_groups]*/, void *d_win_hits /*gdx_hit32_t[n_groups]*/, void *stream);
int gdx_best_hits_many(const gdx_index_t *ix, uint64_t n_groups, uint32_t group_slots, const uint32_t *cand_query,
                       const uint32_t *cand_begin, const gdx_hit_t *cand_hits, const uint32_t *dist, const uint32_t *end /*or NULL*/,
                       uint32_t max_dist, uint32_t *out_best_slot, uint32_t *out_best_dist, uint32_t *out_sub_dist,
                       uint32_t *out_n_live, uint32_t *out_n_best, uint32_t *out_mapq, uint32_t *out_win_query,
                       uint32_t *out_win_begin, gdx_hit_t *out_win_hits);

/* ---- paired-end pairing (the reduction beside gdx_best_hits_many for reads that come in pairs) ---------------------------
 * gdx_best_hits_many treats every read as single-end.  gdx_pair_hits_many picks, per read PAIR, the best properly oriented,
 * properly spaced combination of one verified slot of each mate, says whether that combination is unique, and writes the two
 * winners as a candidate list for the traceback: the mate decides a read that falls into a repeat.
 * Inputs: m = 2 * n_pairs * mate_slots slots, slot j of mate s (0 or 1) of pair p being (2p + s) * mate_slots + j, with
 * cand_query, cand_begin, cand_hits, dist and end (or NULL) per slot exactly as gdx_best_hits_many takes them.  The intended
 * producer is a batch with the mates interleaved (reads 2p and 2p + 1 are the mates of pair p) behind gdx_strands_expand_dev with
 * GDX_STRANDS_BOTH: queries 4p .. 4p + 3 are mate 0 forward, mate 0 reverse complement, mate 1 forward, mate 1 reverse
 * complement, and mate_slots = 2 * max_candidates.  The call never looks at the queries or at the index's arrays.
 * Knobs: max_dist = k; min_insert <= max_insert <= 2^31 - 1.
 * Per slot: strand = cand_query & 1 (the GDX_STRANDS_BOTH numbering); diag = (int64) position - (int64) cand_begin, not wrapped,
 * possibly negative; right = end[slot] when end is given, otherwise diag.
 * Per pair p:
 *  1. Live.  Step 1 of gdx_best_hits_many: cand_query != GDX_CAND_NONE and dist <= k.
 *  2. Same locus, per mate.  Step 2 of gdx_best_hits_many over the mate_slots slots of each mate separately: the key is
 *     (cand_query, text_id, e), e = end or the wrapping 32-bit diagonal when end is NULL; only the least (dist, j) of a key stays.
 *  3. Proper combinations.  A combination is (i, j), i a live slot of mate 0 and j a live slot of mate 1.  It is proper when the
 *     text_id of both is equal, their strands differ and, with f the strand-0 slot of the two and r the strand-1 slot, span =
 *     right_r - diag_f (signed 64 bits) has min_insert <= span <= max_insert: the forward/reverse library orientation.  Its score
 *     is dist_i + dist_j.  With end NULL the span is the distance between the two diagonals: the caller widens the bounds by the
 *     read length.
 *  4. Pair results, over the proper combinations.  n_proper = their number.  The best one is the least (score, i, j): pair_dist =
 *     its score, pair_span = its span as u32.  n_best = the combinations with score == pair_dist.  sub_dist = the least score of
 *     the other combinations: pair_dist when n_best >= 2, 2k + 2 when there is no other.  mapq = min(60, 60 * (sub_dist -
 *     pair_dist) / (2k + 2)), in 64 bits with integer division.  A pair without a proper combination gets n_proper = n_best = 0,
 *     pair_dist = sub_dist = 2k + 2, pair_span = 0 and mapq = GDX_PAIR_MAPQ_NONE.
 *  5. Winners, per mate, at index 2p + s of arrays of 2 * n_pairs entries.  With n_proper > 0 slot i is the winner of mate 0 and
 *     slot j that of mate 1.  Otherwise each mate's winner is its single-end best, the least (dist, j) of its slots live after
 *     step 2: what gdx_best_hits_many gives with n_groups = 2 * n_pairs and group_slots = mate_slots.  mate_slot = the winner's
 *     slot (GDX_PAIR_NONE without a live slot), mate_dist = its distance (k + 1 without one), win_query, win_begin, win_hits = its
 *     candidate (GDX_CAND_NONE, 0, {0, 0} without one).  The three winner arrays go straight into gdx_align_many_dev with m =
 *     2 * n_pairs.
 * Device form: ONE launch, no synchronisation, no allocation, no copy from pageable memory; returns GDX_OK.  Six outputs are
 * u32[n_pairs], four u32[2 n_pairs], d_win_hits gdx_hit32_t[2 n_pairs]; none may overlap an input.  Host form: the same arguments
 * without the stream; cand_hits and win_hits are gdx_hit_t (a text id or a position of 2^32 or more: GDX_ERR_INVALID_ARGUMENT);
 * staged like gdx_best_hits_many.
 * GDX_ERR_INVALID_ARGUMENT: mate_slots == 0 or > GDX_PAIR_MAX_MATE_SLOTS; max_dist > 2^30 (2k + 2 fits u32); min_insert >
 * max_insert or max_insert > 2^31 - 1; 2 * n_pairs * mate_slots does not fit 64 bits; a null required pointer (only d_end / end
 * may be null).  GDX_ERR_UNSUPPORTED: a handle of the 64-bit engine.  n_pairs == 0 is GDX_OK and writes nothing.  A refused call
 * writes nothing.  gdx_parts_t and gdx_multi_t have no such call.
 * Out of scope: other library orientations, an insert-size model beyond the two bounds, preferring among equal scores by span.
 * Mate rescue (aligning the missing mate in the window the found one implies) is gdx_mate_rescue_many below. */
#define GDX_PAIR_NONE           0xFFFFFFFFu  /* mate_slot of a mate without a live slot        */
#define GDX_PAIR_MAPQ_NONE      255u         /* mapq of a pair without a proper combination    */
#define GDX_PAIR_MAX_MATE_SLOTS 32u          /* the most slots of one mate                     */
int gdx_pair_hits_many_dev(const gdx_index_t *ix, uint64_t n_pairs, uint32_t mate_slots, const void *d_cand_query /*u32[m]*/,
                           const void *d_cand_begin /*u32[m]*/, const void *d_cand_hits /*gdx_hit32_t[m]*/,
                           const void *d_dist /*u32[m]*/, const void *d_end /*u32[m] or NULL*/, uint32_t max_dist,
                           uint32_t min_insert, uint32_t max_insert, void *d_n_proper, void *d_n_best, void *d_pair_dist,
                           void *d_sub_dist, void *d_mapq, void *d_pair_span /*u32[n_pairs] each*/, void *d_mate_slot,
                           void *d_mate_dist, void *d_win_query, void *d_win_begin /*u32[2 n_pairs] each*/,
                           void *d_win_hits /*gdx_hit32_t[2 n_pairs]*/, void *stream);
int gdx_pair_hits_many(const gdx_index_t *ix, uint64_t n_pairs, uint32_t mate_slots, const uint32_t *cand_query,
                       const uint32_t *cand_begin, const gdx_hit_t *cand_hits, const uint32_t *dist, const uint32_t *end /*or NULL*/,
                       uint32_t max_dist, uint32_t min_insert, uint32_t max_insert, uint32_t *out_n_proper, uint32_t *out_n_best,
                       uint32_t *out_pair_dist, uint32_t *out_sub_dist, uint32_t *out_mapq, uint32_t *out_pair_span,
                       uint32_t *out_mate_slot, uint32_t *out_mate_dist, uint32_t *out_win_query, uint32_t *out_win_begin,
                       gdx_hit_t *out_win_hits);

/* ---- mate rescue (the step behind gdx_pair_hits_many for pairs without a proper combination) ------------------------------
 * gdx_pair_hits_many can only combine slots the seed stage produced for both mates: a pair one of whose mates got no usable seed
 * has no proper combination.  gdx_mate_rescue_many takes the placed mate of such a pair as an ANCHOR and searches the other mate,
 * on the opposite strand, in the window of the anchor's text that the insert bounds imply, and merges what it finds into the
 * winners that go to the traceback.
 * Inputs: the query batch exactly as gdx_edit_distance_many_dev takes it (d_qbuf, d_qoff, nq, layout; all four layouts), being
 * the one gdx_strands_expand_dev with GDX_STRANDS_BOTH makes of interleaved mates: queries 4p .. 4p + 3 are mate 0 forward, mate 0
 * reverse complement, mate 1 forward, mate 1 reverse complement of pair p, so nq == 4 * n_pairs.  n_pairs and mate_slots as in
 * gdx_pair_hits_many.  end: u32[2 * n_pairs * mate_slots], the out_end of the edit-distance call over the slots; required here,
 * because the reverse anchor's right end comes from it.  Six outputs of gdx_pair_hits_many[_dev], unchanged: n_proper (u32[n_pairs]),
 * mate_slot, mate_dist, win_query, win_begin (u32[2 n_pairs]) and win_hits (2 n_pairs hits).
 * Knobs: max_edits = k <= 256; min_insert <= max_insert <= 2^31 - 1 with max_insert - min_insert <= GDX_RESCUE_MAX_SPREAD, which
 * bounds every search at GDX_RESCUE_MAX_SPREAD + 256 + 256 columns of the text.
 * Attempts.  For pair p and a mate o (0 or 1) to be rescued, a = 1 - o is the anchor.  Attempt (p, o) exists when n_proper[p] == 0
 * and mate_slot[2p + a] != GDX_PAIR_NONE; whether mate o has a single-end hit of its own does not matter.  A pair has 0, 1 or 2
 * attempts.  Of the anchor: strand_a = win_query[2p + a] & 1; T = win_hits[2p + a].text_id; diag_a = (int64) position - (int64)
 * win_begin[2p + a]; right_a = end[(2p + a) * mate_slots + mate_slot[2p + a]].  The searched query is rq = 4p + 2o + (1 - strand_a),
 * the opposite strand of the other mate, and L its length: the batch holds it, no reverse complement is made here.
 * Admissible ends, in signed 64-bit arithmetic.  strand_a == 0: the rescued mate is the reverse one and y is its right end; ylo =
 * diag_a + min_insert, yhi = diag_a + max_insert.  strand_a == 1: the rescued mate is the forward one and its diagonal is defined
 * as y - L; ylo = right_a - max_insert + L, yhi = right_a - min_insert + L.  Either way the rescued pair is proper by the rule of
 * gdx_pair_hits_many step 3 by construction, with span = y - diag_a, respectively right_a - (y - L).
 * Window and distance.  x0 = clamp(ylo - L - k, 0, |T|), x1 = clamp(yhi, 0, |T|); nothing is lost on the left, since an alignment
 * with at most k edits that ends at y >= ylo begins at or after ylo - L - k.  The table D over the read's rows and the columns
 * x0 .. x1, the MATCH rule (equal dense codes in 1..4) and the clipping to the text's own bounds are those of gdx_align_many:
 * D[0][y] = 0, D[i][x0] = i.  dist = the minimum of D[L][y] over max(ylo, x0) <= y <= min(yhi, x1), end = the smallest such y;
 * dist = k + 1 when that range is empty.
 * Outputs per mate, at index 2p + o of arrays of 2 * n_pairs entries.  For an attempt: resc_dist = min(dist, k + 1); resc_end = end
 * when dist <= k, otherwise GDX_EDIT_NO_END; resc_dist = GDX_EDIT_TOO_LONG when L > 256 and GDX_EDIT_INVALID when the anchor's
 * text_id is not one of the index's texts or its mate_slot is not below mate_slots (both with resc_end = GDX_EDIT_NO_END).  Where
 * no attempt exists: resc_dist = GDX_RESCUE_NOT_TRIED, resc_end = GDX_EDIT_NO_END.
 * Merge, per pair.  An attempt succeeds when resc_dist <= k; its score is mate_dist[2p + a] + resc_dist.  The pair takes the
 * successful attempt with the least (score, o): resc_mate[p] = that o (GDX_RESCUE_NONE without one), resc_pair_dist[p] = its score
 * (2k + 2 without one), resc_span[p] = its span (0 without one).
 * Winners: out_win_query, out_win_begin, out_win_hits, 2 * n_pairs entries each.  For a rescued pair index 2p + a copies the
 * anchor's input winner and index 2p + o is the rescue candidate: out_win_query = rq, out_win_begin = max(0, L - end), out_win_hits
 * = {T, max(0, end - L)}, whose diagonal is end - L exactly.  Every other pair copies both input winners.  The three arrays go
 * into gdx_align_many_dev with m = 2 * n_pairs in place of those of gdx_pair_hits_many.  For a rescue candidate the window of
 * gdx_align_many, [end - L - k, end + k), contains the rescue's alignment, so the distance gdx_align_many reports is at most
 * resc_dist.  Equality of the distance and of the end is NOT promised: that window is not the rescue window (it reaches k columns
 * beyond end, and it is not cut at ylo and yhi).
 * Device form: ONE launch, no synchronisation, no allocation, no copy from pageable memory; returns GDX_OK.  No output may overlap
 * an input.  Host form: plain queries only (qbuf, qoff: the caller supplies all 4 * n_pairs); win_hits and out_win_hits are
 * gdx_hit_t, narrowed and widened as in gdx_pair_hits_many (a text id or a position of 2^32 or more:
 * GDX_ERR_INVALID_ARGUMENT); staged with one launch.
 * GDX_ERR_INVALID_ARGUMENT: mate_slots == 0 or > GDX_PAIR_MAX_MATE_SLOTS; max_edits > 256; min_insert > max_insert or max_insert >
 * 2^31 - 1; max_insert - min_insert > GDX_RESCUE_MAX_SPREAD; nq != 4 * n_pairs; nq >= 2^32 - 1 (a query number must differ from
 * GDX_CAND_NONE); an unknown layout; a null pointer.  GDX_ERR_UNSUPPORTED: as for gdx_edit_distance_many -- an index without text
 * units, a handle of the 64-bit engine, the packed form on an index that does not take packed queries.  n_pairs == 0 (with nq ==
 * 0) is GDX_OK and writes nothing.  A refused call writes nothing.  gdx_parts_t and gdx_multi_t have no such call.
 * Out of scope: a mapping quality for rescued pairs, counting runner-up ends in the window, other library orientations, reads
 * longer than 256 symbols, rescue for pairs that already have a proper combination. */
#define GDX_RESCUE_NONE       0xFFFFFFFFu  /* resc_mate of a pair without a successful attempt */
#define GDX_RESCUE_NOT_TRIED  0xFFFFFFFDu  /* resc_dist of a mate without an attempt            */
#define GDX_RESCUE_MAX_SPREAD 4096u        /* max_insert - min_insert at most                   */
int gdx_mate_rescue_many_dev(const gdx_index_t *ix, const void *d_qbuf, const void *d_qoff, uint64_t nq,
                             const gdx_query_layout_t *layout, uint64_t n_pairs, uint32_t mate_slots,
                             const void *d_end /*u32[2 n_pairs mate_slots]*/, const void *d_n_proper /*u32[n_pairs]*/,
                             const void *d_mate_slot, const void *d_mate_dist, const void *d_win_query,
                             const void *d_win_begin /*u32[2 n_pairs] each*/, const void *d_win_hits /*gdx_hit32_t[2 n_pairs]*/,
                             uint32_t max_edits, uint32_t min_insert, uint32_t max_insert, void *d_resc_dist,
                             void *d_resc_end /*u32[2 n_pairs] each*/, void *d_resc_mate, void *d_resc_pair_dist,
                             void *d_resc_span /*u32[n_pairs] each*/, void *d_out_win_query, void *d_out_win_begin /*u32[2 n_pairs]*/,
                             void *d_out_win_hits /*gdx_hit32_t[2 n_pairs]*/, void *stream);
int gdx_mate_rescue_many(const gdx_index_t *ix, const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq, uint64_t n_pairs,
                         uint32_t mate_slots, const uint32_t *end, const uint32_t *n_proper, const uint32_t *mate_slot,
                         const uint32_t *mate_dist, const uint32_t *win_query, const uint32_t *win_begin, const gdx_hit_t *win_hits,
                         uint32_t max_edits, uint32_t min_insert, uint32_t max_insert, uint32_t *out_resc_dist,
                         uint32_t *out_resc_end, uint32_t *out_resc_mate, uint32_t *out_resc_pair_dist, uint32_t *out_resc_span,
                         uint32_t *out_win_query, uint32_t *out_win_begin, gdx_hit_t *out_win_hits);

/* ---- SAM records (the text output behind gdx_align_many: one record per read, made on the device) -------------------------
 * The chain ends in per-read tensors; a distance and an end do not make a SAM record.  gdx_sam_records_many writes the records of
 * n_reads reads, record r being read r, into one byte buffer, from the winners, the outputs of gdx_align_many for them, and the
 * index's text units (for MD).  All arrays travel in one argument block, gdx_sam_inputs_t; set unused pointers to NULL.
 * Inputs.  The batch: qbuf, qoff, nq, layout -- plain forms only (offsets or uniform); strands is 1 or 2 and nq == n_reads *
 * strands; with 2, query 2r is read r as given and 2r + 1 its reverse complement (gdx_strands_expand_dev, GDX_STRANDS_BOTH).  Per
 * read: win_query (u32, GDX_CAND_NONE = no winner), win_hits (only text_id is used), the five outputs of gdx_align_many_dev for
 * candidate r -- dist, begin, end, n_cigar, cigar with stride 2 * max_edits + 1 -- and mapq (u32).  mode: GDX_SAM_SINGLE or
 * GDX_SAM_PAIRED; paired needs an even n_reads, reads 2p and 2p + 1 are the mates of pair p, and proper (u32[n_reads / 2], may be
 * NULL = all 0) says which pairs are proper.  names + name_off (u64[n_reads + 1]): one QNAME per read, or NULL.  text_names +
 * text_name_off (u64[num_texts + 1]): RNAME per text, or NULL.  dense_to_io: u8[16], a HOST pointer in both forms, or NULL (below).
 * Mapped.  Read r is mapped when win_query[r] != GDX_CAND_NONE, end[r] != GDX_EDIT_NO_END, win_query[r] lies in [r * strands,
 * (r + 1) * strands), text_id < num_texts, n_cigar <= 2 * max_edits + 1 and the run lengths of its n_cigar words sum to at most
 * GDX_SAM_MAX_RUN_SUM.  A read with a winner that fails one of the last four is written as unmapped and its status is
 * GDX_SAM_BAD_RECORD; every other status is 0.  strand(r) = win_query[r] - r * strands.
 * The record: eleven tab-separated fields, for a mapped read two more, NM:i:<dist> and MD:Z:<md>, then '\n'.  Numbers are decimal
 * without padding.  With m = r ^ 1 the mate (paired mode; in single mode the mate counts as unmapped):
 *   QNAME  the read's name; with names NULL the decimal read number (single) or pair number (paired)
 *   FLAG   single: 0x4 if unmapped, 0x10 if mapped on strand 1.  Paired: 0x1; 0x40 for even r, 0x80 for odd r; 0x2 if both are
 *          mapped and proper[r / 2] != 0; 0x4 if r is unmapped; 0x8 if m is unmapped; 0x10 if r is mapped on strand 1; 0x20 if m is
 *   RNAME  the text's name (with text_names NULL the decimal text id), or * if unmapped
 *   POS    begin + 1, or 0          MAPQ  min(mapq, 255), or 0
 *   CIGAR  per word the run length, then "MIDNSHP=X"[op] (? for an op above 8); * if unmapped or n_cigar == 0
 *   RNEXT  * if m is unmapped; = if both are mapped on one text; otherwise m's text name
 *   PNEXT  m's begin + 1, or 0
 *   TLEN   0 unless both are mapped on one text; then span = max(end_r, end_m) - min(begin_r, begin_m), printed as span for the mate
 *          with the smaller begin (on equal begins the even one) and as -span for the other
 *   SEQ    the bytes of query win_query[r] if mapped, of query r * strands if not, as they are; * for an empty read
 *   QUAL   *
 *   MD     y = begin, n = 0; per run of length l > 0 (a run of length 0 is skipped): '=' n += l, y += l; 'X' per symbol: n, the text
 *          symbol at y, then n = 0, y += 1; 'D' n, '^', the l text symbols from y, then n = 0, y += l; any other op nothing; at the
 *          end n.  So 2=1D1X2= over ..AC.. gives 2^A0C2.
 * Text symbols.  The text unit of position y of text text_id holds the dense code 1..4 of the symbol, or that it is none of them
 * without saying which (N, IUPAC codes): such a symbol has code 0 here.  The byte printed is dense_to_io[code]; entries 5..15 are
 * reserved.  With dense_to_io NULL: entry c >= 1 is the smallest byte the alphabet maps to c, entry 0 the smallest byte of the
 * alphabet's dense code above 4 when there is exactly one such code (N of ascii_dna_with_n), and ? otherwise.  A y at or beyond
 * the text's length prints ?; nothing outside the text's own units is read.  The CIGAR is not checked against text or read.
 * Outputs.  rec_off: u64[n_reads + 1], rec_off[0] = 0, record r is bytes [rec_off[r], rec_off[r + 1]) of out.  out with
 * out_capacity: a record is written only if it fits whole below out_capacity (rec_off[r + 1] <= out_capacity); no byte at or beyond
 * rec_off[n_reads], and no byte of a record that does not fit, is touched.  out == NULL: the sizing call, only rec_off (and status)
 * are written and rec_off[n_reads] is the total.  status: u8[n_reads] or NULL.
 * gdx_sam_record_bound(max_read_len, max_name_len, max_text_name_len, max_edits): a pure host function, an upper bound of one
 * record's bytes for a caller who must not synchronise, valid for records whose read has at most max_read_len symbols, whose
 * CIGAR is what gdx_align_many writes for such a read within max_edits (at most 2 max_edits + 1 runs and max_edits 'X' and 'D'
 * symbols together, no run and no match counter above max_read_len + max_edits) and whose given names are at most that long:
 *   with d = decimal digits of (max_read_len + max_edits), k = max_edits:
 *   max(max_name_len, 10) + 4 + 2 * max(max_text_name_len, 10) + 10 + 3 + (2k + 1)(d + 1) + 10 + 11 + max(max_read_len, 1) + 1
 *   + (5 + 10) + (5 + (k + 1) d + 2k) + 12 tabs + 1
 * Device form: three small launches (lengths, scan of the workgroup sums, offsets) and, with out != NULL and out_capacity != 0,
 * the fill; no synchronisation, no allocation.  workspace / workspace_bytes: at least gdx_sam_workspace_bytes(n_reads) (a pure
 * host function), 8-byte aligned; a smaller one returns GDX_ERR_INVALID_ARGUMENT and writes nothing.  All pointers but
 * dense_to_io are device pointers; win_hits is gdx_hit32_t[n_reads].  rec_off: 8-byte aligned.  No output may overlap an input.
 * Host form: host pointers, queries with offsets only (layout must be NULL: a packed one is GDX_ERR_UNSUPPORTED as in the device
 * form, any other GDX_ERR_INVALID_ARGUMENT), win_hits is gdx_hit_t[n_reads] (a text id or position
 * of 2^32 or more: GDX_ERR_INVALID_ARGUMENT), workspace is ignored; staged like gdx_align_many (copy in, the launches, copy out).
 * GDX_ERR_INVALID_ARGUMENT: strands not 1 or 2; nq != n_reads * strands; nq >= 2^32 - 1; an odd n_reads in paired mode; an unknown
 * mode or layout; max_edits > 256; a null required pointer (rec_off, and with n_reads != 0 qbuf, the nine per-read arrays and qoff
 * unless uniform); names without their offsets or the reverse.  GDX_ERR_UNSUPPORTED: a packed layout, an index without text units,
 * a handle of the 64-bit engine.  A refused call writes nothing.  n_reads == 0 is GDX_OK and writes rec_off[0] = 0.
 * Out of scope: base qualities, BAM, secondary and supplementary records, placing an unmapped mate at its partner's position,
 * gdx_parts_t and gdx_multi_t.  Soft clipping is a stage of its own before this one, gdx_soft_clip_many below. */
#define GDX_SAM_SINGLE      0u
#define GDX_SAM_PAIRED      1u
#define GDX_SAM_BAD_RECORD  1            /* status: a winner that cannot be a record; written as unmapped        */
#define GDX_SAM_MAX_RUN_SUM 16777216u    /* the run lengths of one CIGAR sum to at most this (2^24)               */
typedef struct gdx_sam_inputs_t {
    const void *qbuf, *qoff;             /* the batch, as the verify calls take it                                */
    uint64_t nq;
    const gdx_query_layout_t *layout;    /* NULL = offsets                                                        */
    uint64_t n_reads;
    uint32_t strands, mode, max_edits, reserved;
    const void *win_query, *win_hits, *dist, *begin, *end, *n_cigar, *cigar, *mapq;
    const void *proper;                  /* u32[n_reads / 2] or NULL                                              */
    const void *names, *name_off, *text_names, *text_name_off; /* or NULL                                         */
    const uint8_t *dense_to_io;          /* HOST u8[16] or NULL                                                   */
    void *workspace;                     /* device form only                                                      */
    uint64_t workspace_bytes;
    void *rec_off;                       /* u64[n_reads + 1]                                                      */
    void *out;                           /* u8[out_capacity] or NULL (sizing)                                     */
    uint64_t out_capacity;
    void *status;                        /* u8[n_reads] or NULL                                                   */
} gdx_sam_inputs_t;
uint64_t gdx_sam_workspace_bytes(uint64_t n_reads);
uint64_t gdx_sam_record_bound(uint64_t max_read_len, uint64_t max_name_len, uint64_t max_text_name_len, uint32_t max_edits);
int gdx_sam_records_many_dev(const gdx_index_t *ix, const gdx_sam_inputs_t *in, void *stream);
int gdx_sam_records_many(const gdx_index_t *ix, const gdx_sam_inputs_t *in);

/* ---- soft clipping (the scored post-pass between gdx_align_many and gdx_sam_records_many) ----------------------------------
 * The alignments of gdx_align_many are end-to-end in the read: a read with a few bad cycles or an adapter tail, or one that hangs
 * over the end of a text, comes out with a string of X and I operations over symbols that align to nothing.  gdx_soft_clip_many
 * finds, per candidate, the best-scoring contiguous part of the traced alignment under a match / mismatch / gap-open / gap-extend
 * scoring, replaces what lies outside it by S runs, moves begin and end inwards, recomputes the edit count (NM) and returns the
 * score (AS).  The clipped dist, begin, end, n_cigar and cigar go into gdx_sam_records_many in place of the traceback's: it prints
 * op 4 as S, formats SEQ whole and skips S in MD.  The call never looks at the queries or at the index's arrays.
 * A read still has to pass the verify limit to reach the traceback at all: a caller who expects junk tails raises max_edits.  The
 * bit-parallel verify does not get slower with it, and the traceback's workspace grows as gdx_align_many's formula says.
 * Inputs: the five outputs of gdx_align_many[_dev] for m candidates as they are -- dist, begin, end, n_cigar (u32[m]) and cigar
 * (u32[m * stride], stride = 2 k + 1, k = max_edits <= 256), candidate c having the runs w_1 .. w_n, n = n_cigar[c], each word
 * len << 4 | op.  Scoring: match, mismatch, gap_extend in 1 .. GDX_CLIP_MAX_SCORE_PARAM, gap_open in 0 .. GDX_CLIP_MAX_SCORE_PARAM,
 * min_score <= 2^30.
 * Per candidate c:
 *  1. Pass through.  end[c] == GDX_EDIT_NO_END: the candidate gets the NONE PATTERN -- out_begin = out_end = GDX_EDIT_NO_END,
 *     out_n_cigar = 0, out_clip_left = out_clip_right = 0 -- with out_score = GDX_CLIP_NO_SCORE and out_dist = dist[c] as it came
 *     (GDX_EDIT_INVALID, GDX_EDIT_TOO_LONG and k + 1 survive); status 0.
 *  2. Check.  The candidate is bad unless n <= stride, every op is one of I (1), D (2), = (7), X (8), every len >= 1, the lens
 *     sum to at most GDX_CLIP_MAX_RUN_SUM, begin <= end and end - begin equals the sum of the lens of the =, X and D runs.  A bad
 *     candidate gets status GDX_CLIP_BAD_CIGAR and the none pattern with out_dist = k + 1 and out_score = GDX_CLIP_NO_SCORE (the
 *     device form cannot report an argument error without synchronising).  No word at or beyond n, or beyond the stride, is read.
 *  3. Score.  The value of a run: = is +match * len, X is -mismatch * len, I or D is -(gap_open + gap_extend * len).  Among all
 *     run intervals [i, j], 1 <= i <= j <= n, the one with the greatest sum of values is taken; among equals the smallest i, then
 *     the greatest j.  best = that sum; best = 0 for n == 0.  The parameter bounds make every run but = strictly negative, so a
 *     positive optimum begins and ends with an = run, and cutting inside a run never helps: the definition works on runs.
 *  4. Keep or drop.  The candidate is kept when best >= max(1, min_score).  Otherwise it is clipped away: the none pattern with
 *     out_dist = k + 1 and out_score = best, which is informative and may be negative.  An empty read (n == 0 with a valid end)
 *     has best = 0 and is therefore clipped away.
 *  5. Kept.  out_score = best; out_begin = begin + the text symbols (=, X, D) of the runs before i; out_end = end - the text
 *     symbols of the runs after j; out_clip_left / out_clip_right = the read symbols (=, X, I) of the runs before i / after j;
 *     out_dist = the sum of the lens of the runs other than = in [i, j].  The output row holds clip_left << 4 | 4 if clip_left > 0,
 *     then w_i .. w_j verbatim, then clip_right << 4 | 4 if clip_right > 0, and out_n_cigar is the number of those words; the
 *     words of the row from there on are NOT written.  A removed side holds at least one run and adds at most one S, so
 *     out_n_cigar <= n and the stride stays 2 k + 1; a removed side that holds only D runs adds no S.
 * Scores fit i32: at most GDX_CLIP_MAX_RUN_SUM * 2 * GDX_CLIP_MAX_SCORE_PARAM in magnitude.  out_score is i32[m], the six other
 * per-candidate outputs u32[m], out_cigar u32[m * stride], status u8[m] or NULL.  No output may overlap an input.
 * Device form: ONE launch, no synchronisation, no allocation; returns GDX_OK.  Host form: the same arguments as host pointers
 * without the stream, staged like gdx_best_hits_many (copy in, one launch, copy out).
 * GDX_ERR_INVALID_ARGUMENT, nothing written: max_edits > 256; match, mismatch or gap_extend outside 1 .. 1024; gap_open > 1024;
 * min_score > 2^30; a null required pointer (only the status may be null).  GDX_ERR_UNSUPPORTED: a handle of the 64-bit engine.
 * m == 0 is GDX_OK and writes nothing.  gdx_parts_t and gdx_multi_t have no such call.
 * Out of scope: re-aligning with affine gaps (the alignment stays the unit-cost one of gdx_align_many; only its ends are judged
 * by the scoring), choosing the best hit by score, an AS tag in the SAM records (gdx_sam_inputs_t has no field for it), hard clips,
 * supplementary records for the clipped part. */
#define GDX_CIGAR_SOFT_CLIP      4u           /* 'S': read symbols outside the kept part                              */
#define GDX_CLIP_NO_SCORE        0x80000000u  /* score of a candidate that had no alignment to clip                   */
#define GDX_CLIP_BAD_CIGAR       1            /* status: the candidate fails the check of step 2                      */
#define GDX_CLIP_MAX_RUN_SUM     65536u       /* the run lengths of one candidate sum to at most this                 */
#define GDX_CLIP_MAX_SCORE_PARAM 1024u        /* match, mismatch, gap_open, gap_extend at most                        */
int gdx_soft_clip_many_dev(const gdx_index_t *ix, uint64_t m, uint32_t max_edits, uint32_t match, uint32_t mismatch,
                           uint32_t gap_open, uint32_t gap_extend, uint32_t min_score, const void *d_dist, const void *d_begin,
                           const void *d_end, const void *d_n_cigar /*u32[m] each*/,
                           const void *d_cigar /*u32[m * (2 max_edits + 1)]*/, void *d_out_score /*i32[m]*/, void *d_out_dist,
                           void *d_out_begin, void *d_out_end, void *d_out_clip_left, void *d_out_clip_right,
                           void *d_out_n_cigar /*u32[m] each*/, void *d_out_cigar /*u32[m * (2 max_edits + 1)]*/,
                           void *d_out_status /*u8[m] or NULL*/, void *stream);
int gdx_soft_clip_many(const gdx_index_t *ix, uint64_t m, uint32_t max_edits, uint32_t match, uint32_t mismatch, uint32_t gap_open,
                       uint32_t gap_extend, uint32_t min_score, const uint32_t *dist, const uint32_t *begin, const uint32_t *end,
                       const uint32_t *n_cigar, const uint32_t *cigar, int32_t *out_score, uint32_t *out_dist, uint32_t *out_begin,
                       uint32_t *out_end, uint32_t *out_clip_left, uint32_t *out_clip_right, uint32_t *out_n_cigar,
                       uint32_t *out_cigar, uint8_t *out_status /*or NULL*/);

#ifdef __cplusplus
}
#endif
#endif
