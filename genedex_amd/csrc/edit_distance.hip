// edit_distance.hip -- seed-and-verify with indels: the infix edit distance of whole reads against the text around the
// diagonals of located seeds (gdx_edit_distance_many[_dev]).  Like hamming.hip it gathers text units and read bytes and
// never touches the index proper.
//
//   the definition      candidate c = (query q of L <= 256 symbols, seed begin b, hit (text T, position p)); s = p - b,
//                       k = max_edits; window T[x0, x1), x0 = clamp(s - k, 0, |T|), x1 = clamp(s + L + k, 0, |T|);
//                       dist = min over x0 <= x <= y <= x1 of the unit-cost edit distance of q and T[x, y), a pair of
//                       symbols matching under the Hamming rule (equal dense codes in 1..4); out_dist[c] = min(dist, k + 1),
//                       out_end[c] = the smallest such y when dist <= k, else GDX_EDIT_NO_END
//   edit_kernel<kXlate, kUniform, W>
//                       Myers' bit-vector algorithm in its block form (Hyyro's formulation), ONE lane per candidate, the
//                       read in W 64-row blocks held in registers.  The lane turns the read into bit planes once (lo / hi:
//                       the two bits of code - 1; valid: the symbol is one of 1..4; kXlate as in hamming_kernel), then walks
//                       the window's columns: one text unit per 32 columns, per column Eq = the rows whose symbol equals
//                       the text's (none when the text symbol is masked), and one block step per block with the horizontal
//                       delta of the block below as carry.  The top row is free (carry 0 into block 0), so an alignment
//                       may begin at any column; score = D[L][y] follows from the last block's delta, and the first column
//                       with the least score is the end.  Every loop is bounded by the clipped window: at most
//                       L + 2 k <= 768 columns of at most 4 blocks.  A uniform batch runs the instance with
//                       W = ceil(uniform_len / 64) blocks, an offsets batch W = 4 with the lane's own block count.
//                       The argument block, the read loader read_chunk, clamp64, the LDS table load and the instance
//                       dispatch are verify.hpp's, shared with hamming.hip and align.hip.  The lane itself is kept as it
//                       was, candidate resolution included: routed through the shared resolution or a shared forward pass
//                       it compiled to other code and measured slower at 50 symbols (profiles/r15/verify_refactor.md).
//                       align_lane carries the same forward pass with its history stores: a change to the window rule, the
//                       MATCH rule or a text-unit edge goes into both.
#include "verify.hpp"

namespace gdx {

namespace {

constexpr int kBlock = 256;

struct EditArgs : VerifyArgs {
    uint32_t max_edits;  // <= 256
    uint32_t *out_dist, *out_end;  // out_end may be null
};

// candidate c, start to finish
template <int kXlate, bool kUniform, int W>
__device__ __forceinline__ void edit_lane(const EditArgs &a, const uint8_t *s_dense, uint64_t c)
{
    const uint32_t q = a.cand_query[c], b = a.cand_begin[c];
    const gdx_hit32_t hit = a.cand_hits[c];
    uint32_t dist, end = GDX_EDIT_NO_END;
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
        if (a.out_end) a.out_end[c] = end;
        return;
    }
    // the text's own symbols are [t0, t0 + t_len) of the concatenation: between the sentinel in front and its own
    const int64_t t0 = hit.text_id == 0u ? 0 : static_cast<int64_t>(a.sentinels[hit.text_id - 1u]) + 1;
    const int64_t t_len = static_cast<int64_t>(a.sentinels[hit.text_id]) - t0;
    const int64_t s = static_cast<int64_t>(hit.position) - static_cast<int64_t>(b);
    const int64_t k = a.max_edits;
    const int64_t x0 = clamp64(s - k, 0, t_len), x1 = clamp64(s + static_cast<int64_t>(L) + k, 0, t_len);
    const uint32_t nb = kUniform ? static_cast<uint32_t>(W) : (L + 63u) >> 6;  // blocks of this read (W when uniform: L > 64 (W - 1))

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

    uint32_t score = L, best = L;
    uint32_t best_end = static_cast<uint32_t>(x0);
    if (L != 0u && x0 < x1) {
        const uint32_t top_last = (L - 1u) & 63u;
        // text side.  Every column is a symbol of the text itself, so its unit exists (kTextPadUnits in front)
        uint64_t g = static_cast<uint64_t>(t0 + x0 + 32 * static_cast<int64_t>(kTextPadUnits));
        u32x4 u = a.text_units[g >> 5];
        uint64_t codes = (static_cast<uint64_t>(u.x) | (static_cast<uint64_t>(u.y) << 32)) >> (2u * (g & 31u));
        uint32_t mask = u.z >> (g & 31u);
        for (int64_t y = x0; y < x1; y++) {
            const uint64_t clo = 0ull - (codes & 1u), chi = 0ull - ((codes >> 1) & 1u);
            const uint64_t keep = static_cast<uint64_t>(mask & 1u) - 1ull;  // 0 when the text symbol is not one of 1..4
            int hin = 0;
#pragma unroll
            for (int w = 0; w < W; w++) {
                if (static_cast<uint32_t>(w) < nb) {
                    const bool last = static_cast<uint32_t>(w) == nb - 1u;
                    const uint32_t top = last ? top_last : 63u;
                    uint64_t Eq = keep & valid[w] & ~(lo[w] ^ clo) & ~(hi[w] ^ chi);
                    const uint64_t Xv = Eq | Mv[w];
                    if (hin < 0) Eq |= 1u;
                    const uint64_t Xh = (((Eq & Pv[w]) + Pv[w]) ^ Pv[w]) | Eq;
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
                }
            }
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
    const bool within = best <= a.max_edits;
    a.out_dist[c] = within ? best : a.max_edits + 1u;
    if (a.out_end) a.out_end[c] = within ? best_end : GDX_EDIT_NO_END;
}

template <int kXlate, bool kUniform, int W>
__global__ __launch_bounds__(kBlock) void edit_kernel(const EditArgs a)
{
    __shared__ uint8_t s_dense[256];
    load_dense_table<kXlate, kBlock>(s_dense, a.io_to_dense);
    for (uint64_t c = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; c < a.m; c += static_cast<uint64_t>(gridDim.x) * kBlock)
        edit_lane<kXlate, kUniform, W>(a, s_dense, c);
}

template <int kXlate>
void launch_xlate(const EditArgs &a, hipStream_t stream)
{
    const dim3 grid(grid_for(a.m, kBlock, 256u * 32u)), block(kBlock);
    dispatch_blocks(a.uniform_len, [&](auto uniform, auto w) {
        hipLaunchKernelGGL((edit_kernel<kXlate, decltype(uniform)::value, decltype(w)::value>), grid, block, 0, stream, a);
    });
}

}  // namespace

void launch_edit_distance(const IndexView &ix, const uint8_t *d_qbuf, const uint64_t *d_qoff, uint64_t nq, bool packed,
                          uint32_t uniform_len, const uint32_t *d_cand_query, const uint32_t *d_cand_begin,
                          const gdx_hit32_t *d_cand_hits, uint64_t m, uint32_t max_edits, uint32_t *d_out_dist,
                          uint32_t *d_out_end, hipStream_t stream)
{
    if (m == 0) return;
    EditArgs a;
    fill_verify_args(a, ix, d_qbuf, d_qoff, nq, uniform_len, d_cand_query, d_cand_begin, d_cand_hits, m);
    a.max_edits = max_edits;
    a.out_dist = d_out_dist;
    a.out_end = d_out_end;
    if (packed) launch_xlate<2>(a, stream);
    else if (ix.perm_ok) launch_xlate<1>(a, stream);
    else launch_xlate<0>(a, stream);
}

}  // namespace gdx
