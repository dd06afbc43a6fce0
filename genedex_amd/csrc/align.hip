// align.hip -- the last stage of seed and verify: distance, begin, end and run-length CIGAR of one canonically chosen
// optimal alignment per candidate (gdx_align_many[_dev]).  Inputs, window, MATCH rule and markers are those of
// edit_distance.hip (the shared parts live in verify.hpp); include/gdx.h "alignment traceback" has the table D and the four
// rules of the walk.
//
//   align_kernel<kXlate, kUniform, W>
//                       ONE lane per candidate, grid-stride, the instantiation scheme of edit_kernel.  The forward pass is
//                       edit_lane's column loop (Myers / Hyyro block step), written out here a second time: shared through a
//                       per-block hook it measured slower in one setting (profiles/r15/verify_refactor.md).  A change to the
//                       window rule, the MATCH rule or a text-unit edge goes into both.  Per block and column it additionally
//                       stores ONE 16-byte element {diag, pick} into the lane's workspace slot: the walk's decision at every
//                       cell of the column, which is a function of three planes the block step has anyway,
//                           Eq  (before the carry is folded in)         row matches                       -> rule 1
//                           D0 = Xh | Mv                                D[i][y] == D[i-1][y-1]            -> rule 2 when clear
//                           Pv' (the column's new vertical plus plane)  D[i][y] == D[i-1][y] + 1          -> rule 3
//                           diag = Eq | ~D0                 the step is diagonal ('=' or 'X')
//                           pick = Eq | (~diag & Pv')       diag ? ('=' : 'X') : ('I' : 'D')
//                       so the walk reads one element per step and touches neither the text nor the read's planes again
//                       (no register array is indexed by a runtime block number: no scratch).
//   workspace           lane-interleaved 16-byte elements: element e of lane t sits at ws[e * n_lanes + t], so a wavefront's
//                       store of one plane pair is one contiguous 1024-byte run.  A slot holds (Lmax + 2 k) * Wmax history
//                       elements (cell (i, y): element (y - x0 - 1) * nb + (i - 1) / 64, bit (i - 1) % 64) and behind them
//                       ceil((2 k + 1) / 4) elements in which the walk stacks its runs, last run first.  Lmax / Wmax: the
//                       uniform length and its block count, else 256 and 4.  The grid is as many blocks as the workspace
//                       holds, at most kMaxBlocks and at most kMaxBytes worth (align_workspace_bytes).
//   the walk            only when best <= k, from (L, end): one element load per step, runs built in two registers, stacked in
//                       the slot and copied out reversed, so out_cigar gets exactly words 0 .. n_cigar.  It reads columns
//                       begin + 1 .. end of the candidate it belongs to and nothing else: a lane's earlier candidate cannot
//                       show through.  At y == x0 the rest of the read is one run of insertions (D[i][x0] = i).
#include "verify.hpp"

namespace gdx {

namespace {

constexpr int kBlock = 256;
// resident lanes: 4 waves per SIMD on 256 CUs of 4 SIMDs (1024 blocks of 256 lanes), and no more blocks than 4 GiB hold
constexpr uint64_t kMaxBlocks = 1024;
constexpr uint64_t kMaxBytes = 4ull << 30;

struct AlignArgs : VerifyArgs {
    uint32_t max_edits;  // <= 256
    uint32_t *out_dist, *out_begin, *out_end, *out_n_cigar, *out_cigar;
    ulonglong2 *ws;       // lane-interleaved slots, gridDim.x * kBlock lanes
    uint32_t hist_elems;  // history elements of a slot; the run stack lies behind them
};

// the outputs of a candidate without an alignment: dist is a marker or max_edits + 1
__device__ __forceinline__ void store_no_alignment(const AlignArgs &a, uint64_t c, uint32_t dist)
{
    a.out_dist[c] = dist;
    a.out_begin[c] = GDX_EDIT_NO_END;
    a.out_end[c] = GDX_EDIT_NO_END;
    a.out_n_cigar[c] = 0;
}

// candidate c, start to finish; `lane` of `n_lanes` owns slot `lane` of the workspace
template <int kXlate, bool kUniform, int W>
__device__ __forceinline__ void align_lane(const AlignArgs &a, const uint8_t *s_dense, uint64_t c, uint64_t lane, uint64_t n_lanes)
{
    Candidate cand;
    const uint32_t marker = resolve_candidate<kUniform, true>(a, c, cand);
    if (marker != 0u) return store_no_alignment(a, c, marker);
    resolve_text(a, cand);
    const uint64_t begin = cand.begin;
    const uint32_t L = cand.L;
    const int64_t t0 = cand.t0, t_len = cand.t_len, s = cand.s;
    const int64_t k = a.max_edits;
    const int64_t x0 = clamp64(s - k, 0, t_len), x1 = clamp64(s + static_cast<int64_t>(L) + k, 0, t_len);
    const uint32_t nb = kUniform ? static_cast<uint32_t>(W) : (L + 63u) >> 6;  // blocks of this read (W when uniform: L > 64 (W - 1))
    ulonglong2 *slot = a.ws + lane;  // element e: slot[e * n_lanes]

    // read side: the bit planes of block w, rows 64 w .. 64 w + 63
    uint64_t lo[W], hi[W], valid[W], Pv[W], Mv[W];
#pragma unroll
    for (int w = 0; w < W; w++) {
        lo[w] = hi[w] = valid[w] = 0;
        Pv[w] = ~0ull;
        Mv[w] = 0;
#pragma unroll
        for (uint32_t half = 0; half < 2; half++) {
            const uint32_t j0 = 64u * w + 32u * half;
            if (j0 < L) {
                const uint32_t n_c = L - j0 < 32u ? L - j0 : 32u;
                uint64_t qc;
                uint32_t inv;
                read_chunk<kXlate>(a, s_dense, begin + j0, n_c, qc, inv);
                const uint32_t c_lo = static_cast<uint32_t>(qc), c_hi = static_cast<uint32_t>(qc >> 32);
                const uint64_t p_lo = even_bits(c_lo) | (even_bits(c_hi) << 16);
                const uint64_t p_hi = even_bits(c_lo >> 1) | (even_bits(c_hi >> 1) << 16);
                const uint64_t ok = ~inv & low_bits(n_c);
                lo[w] |= p_lo << (32u * half);
                hi[w] |= p_hi << (32u * half);
                valid[w] |= ok << (32u * half);
            }
        }
    }

    // forward pass: edit_lane's, plus the history.  Columns x1 - x0 <= L + 2 k and nb blocks each: within hist_elems
    uint32_t score = L, best = L;
    uint32_t best_end = static_cast<uint32_t>(x0);
    if (L != 0u && x0 < x1) {
        const uint32_t top_last = (L - 1u) & 63u;
        // text side.  Every column is a symbol of the text itself, so its unit exists (kTextPadUnits in front)
        uint64_t g = static_cast<uint64_t>(t0 + x0 + 32 * static_cast<int64_t>(kTextPadUnits));
        u32x4 u = a.text_units[g >> 5];
        uint64_t codes = (static_cast<uint64_t>(u.x) | (static_cast<uint64_t>(u.y) << 32)) >> (2u * (g & 31u));
        uint32_t mask = u.z >> (g & 31u);
        ulonglong2 *col = slot;  // the column's first element
        for (int64_t y = x0; y < x1; y++) {
            const uint64_t clo = 0ull - (codes & 1u), chi = 0ull - ((codes >> 1) & 1u);
            const uint64_t keep = static_cast<uint64_t>(mask & 1u) - 1ull;  // 0 when the text symbol is not one of 1..4
            int hin = 0;
#pragma unroll
            for (int w = 0; w < W; w++) {
                if (static_cast<uint32_t>(w) < nb) {
                    const bool last = static_cast<uint32_t>(w) == nb - 1u;
                    const uint32_t top = last ? top_last : 63u;
                    const uint64_t match = keep & valid[w] & ~(lo[w] ^ clo) & ~(hi[w] ^ chi);
                    uint64_t Eq = match;
                    const uint64_t Xv = Eq | Mv[w];
                    if (hin < 0) Eq |= 1u;
                    const uint64_t Xh = (((Eq & Pv[w]) + Pv[w]) ^ Pv[w]) | Eq;
                    const uint64_t diag = match | ~(Xh | Mv[w]);
                    uint64_t Ph = Mv[w] | ~(Xh | Pv[w]);
                    uint64_t Mh = Pv[w] & Xh;
                    const int hout = static_cast<int>((Ph >> top) & 1u) - static_cast<int>((Mh >> top) & 1u);
                    Ph <<= 1;
                    Mh <<= 1;
                    if (hin < 0) Mh |= 1u;
                    else if (hin > 0) Ph |= 1u;
                    Pv[w] = Mh | ~(Xv | Ph);
                    Mv[w] = Ph & Xv;
                    hin = hout;
                    if (last) score += static_cast<uint32_t>(hout);
                    col[static_cast<uint64_t>(w) * n_lanes] = make_ulonglong2(diag, match | (~diag & Pv[w]));
                }
            }
            col += static_cast<uint64_t>(nb) * n_lanes;
            if (score < best) {  // strict: the leftmost end wins
                best = score;
                best_end = static_cast<uint32_t>(y + 1);
            }
            g++;
            if ((g & 31u) != 0u) {
                codes >>= 2;
                mask >>= 1;
            } else if (y + 1 < x1) {
                u = a.text_units[g >> 5];
                codes = static_cast<uint64_t>(u.x) | (static_cast<uint64_t>(u.y) << 32);
                mask = u.z;
            }
        }
    }
    if (best > a.max_edits) return store_no_alignment(a, c, a.max_edits + 1u);

    // the walk: rules 1 to 4 from (L, end) to row 0
    const uint32_t stride = 2u * a.max_edits + 1u;
    uint32_t *stack = reinterpret_cast<uint32_t *>(slot + static_cast<uint64_t>(a.hist_elems) * n_lanes);  // word r: element r / 4
    const uint64_t stack_step = 4u * n_lanes;  // in words, from one element of the slot to the next
    uint32_t i = L, y = best_end, n = 0, run_op = 0, run_len = 0;
    const uint32_t y0 = static_cast<uint32_t>(x0);
    while (i != 0u) {
        uint32_t op, len = 1u;
        if (y == y0) {  // D[i][x0] = i: the rest of the read has no partner in the text
            op = GDX_CIGAR_INS;
            len = i;
            i = 0;
        } else {
            const ulonglong2 e = slot[(static_cast<uint64_t>(y - y0 - 1u) * nb + ((i - 1u) >> 6)) * n_lanes];
            const uint32_t bit = (i - 1u) & 63u;
            const bool diag = ((e.x >> bit) & 1u) != 0u, pick = ((e.y >> bit) & 1u) != 0u;
            op = diag ? (pick ? GDX_CIGAR_EQ : GDX_CIGAR_DIFF) : (pick ? GDX_CIGAR_INS : GDX_CIGAR_DEL);
            if (diag || pick) i--;
            if (diag || !pick) y--;
        }
        if (op == run_op) {
            run_len += len;
        } else {
            if (run_len != 0u) {
                if (n < stride) stack[(n >> 2) * stack_step + (n & 3u)] = (run_len << 4) | run_op;
                n++;
            }
            run_op = op;
            run_len = len;
        }
    }
    uint32_t *cigar = a.out_cigar + c * stride;
    if (run_len != 0u) {  // the read's first run
        cigar[0] = (run_len << 4) | run_op;
        n++;
    }
    if (n > stride) n = stride;  // (cannot happen: an alignment of dist <= k edits has at most 2 dist + 1 runs)
    for (uint32_t r = run_len != 0u ? 1u : 0u; r < n; r++) {
        const uint32_t from = n - 1u - r;
        cigar[r] = stack[(from >> 2) * stack_step + (from & 3u)];
    }
    a.out_dist[c] = best;
    a.out_begin[c] = y;
    a.out_end[c] = best_end;
    a.out_n_cigar[c] = n;
}

template <int kXlate, bool kUniform, int W>
__global__ __launch_bounds__(kBlock) void align_kernel(const AlignArgs a)
{
    __shared__ uint8_t s_dense[256];
    load_dense_table<kXlate, kBlock>(s_dense, a.io_to_dense);
    const uint64_t lane = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x, n_lanes = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t c = lane; c < a.m; c += n_lanes) align_lane<kXlate, kUniform, W>(a, s_dense, c, lane, n_lanes);
}

template <int kXlate>
void launch_xlate(const AlignArgs &a, unsigned blocks, hipStream_t stream)
{
    const dim3 grid(blocks), block(kBlock);
    dispatch_blocks(a.uniform_len, [&](auto uniform, auto w) {
        hipLaunchKernelGGL((align_kernel<kXlate, decltype(uniform)::value, decltype(w)::value>), grid, block, 0, stream, a);
    });
}

// history elements of one lane's slot: the longest window times the blocks of the longest read
uint32_t hist_elems_of(uint32_t uniform_len, uint32_t max_edits)
{
    const uint32_t l_max = uniform_len != 0u && uniform_len <= GDX_EDIT_MAX_QUERY_LEN ? uniform_len : GDX_EDIT_MAX_QUERY_LEN;
    return (l_max + 2u * max_edits) * ((l_max + 63u) >> 6);
}

uint64_t block_bytes_of(uint32_t uniform_len, uint32_t max_edits)
{
    const uint64_t stack_elems = (2u * max_edits + 1u + 3u) >> 2;
    return (hist_elems_of(uniform_len, max_edits) + stack_elems) * sizeof(ulonglong2) * kBlock;
}

uint64_t max_blocks_of(uint32_t uniform_len, uint64_t m, uint32_t max_edits)
{
    uint64_t blocks = div_ceil(m ? m : 1, static_cast<uint64_t>(kBlock));
    const uint64_t fit = kMaxBytes / block_bytes_of(uniform_len, max_edits);  // >= 1: a block's slots are at most 13 MB
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    return blocks < fit ? blocks : fit;
}

}  // namespace

void align_workspace_bytes(uint32_t uniform_len, uint64_t m, uint32_t max_edits, uint64_t out[2])
{
    out[0] = block_bytes_of(uniform_len, max_edits);
    out[1] = out[0] * max_blocks_of(uniform_len, m, max_edits);
}

void launch_align(const IndexView &ix, const uint8_t *d_qbuf, const uint64_t *d_qoff, uint64_t nq, bool packed, uint32_t uniform_len,
                  const uint32_t *d_cand_query, const uint32_t *d_cand_begin, const gdx_hit32_t *d_cand_hits, uint64_t m,
                  uint32_t max_edits, uint32_t *d_out_dist, uint32_t *d_out_begin, uint32_t *d_out_end, uint32_t *d_out_n_cigar,
                  uint32_t *d_out_cigar, void *d_workspace, uint64_t workspace_bytes, hipStream_t stream)
{
    if (m == 0) return;
    uint64_t blocks = workspace_bytes / block_bytes_of(uniform_len, max_edits);
    const uint64_t most = max_blocks_of(uniform_len, m, max_edits);
    if (blocks > most) blocks = most;
    if (blocks == 0) fail(GDX_ERR_INVALID_ARGUMENT, "the workspace holds no block of lanes");
    AlignArgs a;
    fill_verify_args(a, ix, d_qbuf, d_qoff, nq, uniform_len, d_cand_query, d_cand_begin, d_cand_hits, m);
    a.max_edits = max_edits;
    a.out_dist = d_out_dist;
    a.out_begin = d_out_begin;
    a.out_end = d_out_end;
    a.out_n_cigar = d_out_n_cigar;
    a.out_cigar = d_out_cigar;
    a.ws = static_cast<ulonglong2 *>(d_workspace);
    a.hist_elems = hist_elems_of(uniform_len, max_edits);
    if (packed) launch_xlate<2>(a, static_cast<unsigned>(blocks), stream);
    else if (ix.perm_ok) launch_xlate<1>(a, static_cast<unsigned>(blocks), stream);
    else launch_xlate<0>(a, static_cast<unsigned>(blocks), stream);
}

}  // namespace gdx
