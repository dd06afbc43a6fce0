// align.hip -- the last stage of seed and verify: distance, begin, end and run-length CIGAR of one canonically chosen
// optimal alignment per candidate (gdx_align_many[_dev]).  Inputs, window, MATCH rule and markers are those of
// edit_distance.hip; include/gdx.h "alignment traceback" has the table D and the four rules of the walk.
//
//   align_kernel<kXlate, kUniform, W>
//                       ONE lane per candidate, grid-stride, the instantiation scheme of edit_kernel.  The forward pass is
//                       edit_lane's column loop (Myers / Hyyro block step, the block step duplicated here so that
//                       edit_distance.hip stays as it is).  Per block and column it additionally stores ONE 16-byte
//                       element {diag, pick} into the lane's workspace slot: the walk's decision at every cell of the column,
//                       which is a function of three planes the block step has anyway,
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
#include "common.hpp"
#include "kernels.hpp"
#include "read_codes.hpp"

namespace gdx {

namespace {

constexpr int kBlock = 256;
// resident lanes: 4 waves per SIMD on 256 CUs of 4 SIMDs (1024 blocks of 256 lanes), and no more blocks than 4 GiB hold
constexpr uint64_t kMaxBlocks = 1024;
constexpr uint64_t kMaxBytes = 4ull << 30;

struct AlignArgs {
    const u32x4 *text_units;
    const uint32_t *sentinels;
    const uint8_t *io_to_dense;
    uint32_t perm_code_lo, perm_code_hi, perm_exp_lo, perm_exp_hi, perm_mask;
    uint32_t n_texts;
    const uint8_t *qbuf;
    const uint64_t *qoff;  // null for a uniform batch
    uint64_t nq;
    uint32_t uniform_len;
    const uint32_t *cand_query, *cand_begin;
    const gdx_hit32_t *cand_hits;
    uint64_t m;
    uint32_t max_edits;  // <= 256
    uint32_t *out_dist, *out_begin, *out_end, *out_n_cigar, *out_cigar;
    ulonglong2 *ws;       // lane-interleaved slots, gridDim.x * kBlock lanes
    uint32_t hist_elems;  // history elements of a slot; the run stack lies behind them
};

// (edit_distance.hip's read_chunk) symbols [at, at + n_c) of the batch, n_c in 1..32 -> qc: symbol i in bits 2 i + 1 : 2 i
// (garbage from n_c on); inv: bit i set when symbol i is not one of 1..4
template <int kXlate>
__device__ __forceinline__ void read_chunk(const AlignArgs &a, const uint8_t *s_dense, uint64_t at, uint32_t n_c, uint64_t &qc,
                                           uint32_t &inv)
{
    inv = 0;
    const uint32_t n_need = (static_cast<uint32_t>(at & 7u) + n_c + 7u) >> 3;
    if (kXlate == 2) {
        const uint16_t *up = reinterpret_cast<const uint16_t *>(a.qbuf) + (at >> 3);
        const uint32_t sh = static_cast<uint32_t>(at & 7u) * 2u;
        uint64_t lo64 = up[0];
        uint32_t hi16 = 0;
        if (n_need > 1u) lo64 |= static_cast<uint64_t>(up[1]) << 16;
        if (n_need > 2u) lo64 |= static_cast<uint64_t>(up[2]) << 32;
        if (n_need > 3u) lo64 |= static_cast<uint64_t>(up[3]) << 48;
        if (n_need > 4u) hi16 = up[4];
        qc = sh != 0u ? (lo64 >> sh) | (static_cast<uint64_t>(hi16) << (64u - sh)) : lo64;
    } else {
        const uint64_t *wp = reinterpret_cast<const uint64_t *>(a.qbuf) + (at >> 3);
        const uint32_t sh = static_cast<uint32_t>(at & 7u) * 8u;
        uint64_t w0 = wp[0], w1 = 0, w2 = 0, w3 = 0, w4 = 0;
        if (n_need > 1u) w1 = wp[1];
        if (n_need > 2u) w2 = wp[2];
        if (n_need > 3u) w3 = wp[3];
        if (n_need > 4u) w4 = wp[4];
        if (sh != 0u) {
            w0 = (w0 >> sh) | (w1 << (64u - sh));
            w1 = (w1 >> sh) | (w2 << (64u - sh));
            w2 = (w2 >> sh) | (w3 << (64u - sh));
            w3 = (w3 >> sh) | (w4 << (64u - sh));
        }
        const uint32_t wd[8] = {static_cast<uint32_t>(w0), static_cast<uint32_t>(w0 >> 32), static_cast<uint32_t>(w1),
                                static_cast<uint32_t>(w1 >> 32), static_cast<uint32_t>(w2), static_cast<uint32_t>(w2 >> 32),
                                static_cast<uint32_t>(w3), static_cast<uint32_t>(w3 >> 32)};
        qc = 0;
#pragma unroll
        for (uint32_t g = 0; g < 8; g++) {
            uint32_t bad;
            const uint32_t code = kXlate == 1 ? pack4_perm(a, wd[g], bad) : pack4_lds(s_dense, wd[g], bad);
            qc |= static_cast<uint64_t>(code) << (8u * g);
            inv |= bad << (4u * g);
        }
    }
}

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// candidate c, start to finish; `lane` of `n_lanes` owns slot `lane` of the workspace
template <int kXlate, bool kUniform, int W>
__device__ __forceinline__ void align_lane(const AlignArgs &a, const uint8_t *s_dense, uint64_t c, uint64_t lane, uint64_t n_lanes)
{
    const uint32_t q = a.cand_query[c], b = a.cand_begin[c];
    const gdx_hit32_t hit = a.cand_hits[c];
    uint32_t dist;
    uint64_t begin = 0;
    uint32_t L = 0;
    if (q >= a.nq || hit.text_id >= a.n_texts) {
        dist = GDX_EDIT_INVALID;
    } else {
        if (kUniform) {
            begin = static_cast<uint64_t>(q) * a.uniform_len;
            L = a.uniform_len;
        } else {
            begin = a.qoff[q];
            const uint64_t len = a.qoff[q + 1] - begin;
            L = len > GDX_EDIT_MAX_QUERY_LEN ? GDX_EDIT_MAX_QUERY_LEN + 1u : static_cast<uint32_t>(len);
        }
        dist = L > GDX_EDIT_MAX_QUERY_LEN ? GDX_EDIT_TOO_LONG : 0u;
    }
    if (dist != 0u) {
        a.out_dist[c] = dist;
        a.out_begin[c] = GDX_EDIT_NO_END;
        a.out_end[c] = GDX_EDIT_NO_END;
        a.out_n_cigar[c] = 0;
        return;
    }
    // the text's own symbols are [t0, t0 + t_len) of the concatenation: between the sentinel in front and its own
    const int64_t t0 = hit.text_id == 0u ? 0 : static_cast<int64_t>(a.sentinels[hit.text_id - 1u]) + 1;
    const int64_t t_len = static_cast<int64_t>(a.sentinels[hit.text_id]) - t0;
    const int64_t s = static_cast<int64_t>(hit.position) - static_cast<int64_t>(b);
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
    if (best > a.max_edits) {
        a.out_dist[c] = a.max_edits + 1u;
        a.out_begin[c] = GDX_EDIT_NO_END;
        a.out_end[c] = GDX_EDIT_NO_END;
        a.out_n_cigar[c] = 0;
        return;
    }

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
    if (kXlate == 0) {
        for (int i = threadIdx.x; i < 256; i += kBlock) s_dense[i] = a.io_to_dense[i];
        __syncthreads();
    }
    const uint64_t lane = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x, n_lanes = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t c = lane; c < a.m; c += n_lanes) align_lane<kXlate, kUniform, W>(a, s_dense, c, lane, n_lanes);
}

template <int kXlate>
void launch_xlate(const AlignArgs &a, unsigned blocks, hipStream_t stream)
{
    const dim3 grid(blocks), block(kBlock);
    if (a.uniform_len == 0u) {
        hipLaunchKernelGGL((align_kernel<kXlate, false, 4>), grid, block, 0, stream, a);
        return;
    }
    // (a uniform batch over the limit: every lane leaves with GDX_EDIT_TOO_LONG before it looks at a block)
    switch (a.uniform_len > GDX_EDIT_MAX_QUERY_LEN ? 4u : (a.uniform_len + 63u) >> 6) {
    case 1: hipLaunchKernelGGL((align_kernel<kXlate, true, 1>), grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL((align_kernel<kXlate, true, 2>), grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((align_kernel<kXlate, true, 3>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((align_kernel<kXlate, true, 4>), grid, block, 0, stream, a); break;
    }
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
    a.text_units = ix.text_units;
    a.sentinels = ix.sentinels;
    a.io_to_dense = ix.io_to_dense;
    a.perm_code_lo = ix.perm_code_lo;
    a.perm_code_hi = ix.perm_code_hi;
    a.perm_exp_lo = ix.perm_exp_lo;
    a.perm_exp_hi = ix.perm_exp_hi;
    a.perm_mask = ix.perm_mask;
    a.n_texts = ix.n_texts;
    a.qbuf = d_qbuf;
    a.qoff = uniform_len ? nullptr : d_qoff;
    a.nq = nq;
    a.uniform_len = uniform_len;
    a.cand_query = d_cand_query;
    a.cand_begin = d_cand_begin;
    a.cand_hits = d_cand_hits;
    a.m = m;
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
