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
#include "common.hpp"
#include "kernels.hpp"
#include "read_codes.hpp"

namespace gdx {

namespace {

constexpr int kBlock = 256;

struct EditArgs {
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
    uint32_t *out_dist, *out_end;  // out_end may be null
};

// symbols [at, at + n_c) of the batch, n_c in 1..32 -> qc: symbol i in bits 2 i + 1 : 2 i (garbage from n_c on); inv: bit i
// set when symbol i is not one of 1..4.  The loads are those of hamming_kernel: only units / 8-byte words that hold one of
// the chunk's symbols.
template <int kXlate>
__device__ __forceinline__ void read_chunk(const EditArgs &a, const uint8_t *s_dense, uint64_t at, uint32_t n_c, uint64_t &qc,
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
    if (kXlate == 0) {
        for (int i = threadIdx.x; i < 256; i += kBlock) s_dense[i] = a.io_to_dense[i];
        __syncthreads();
    }
    for (uint64_t c = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; c < a.m; c += static_cast<uint64_t>(gridDim.x) * kBlock)
        edit_lane<kXlate, kUniform, W>(a, s_dense, c);
}

template <int kXlate>
void launch_xlate(const EditArgs &a, hipStream_t stream)
{
    const dim3 grid(grid_for(a.m, kBlock, 256u * 32u)), block(kBlock);
    if (a.uniform_len == 0u) {
        hipLaunchKernelGGL((edit_kernel<kXlate, false, 4>), grid, block, 0, stream, a);
        return;
    }
    // (a uniform batch over the limit: every lane leaves with GDX_EDIT_TOO_LONG before it looks at a block)
    switch (a.uniform_len > GDX_EDIT_MAX_QUERY_LEN ? 4u : (a.uniform_len + 63u) >> 6) {
    case 1: hipLaunchKernelGGL((edit_kernel<kXlate, true, 1>), grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL((edit_kernel<kXlate, true, 2>), grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((edit_kernel<kXlate, true, 3>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((edit_kernel<kXlate, true, 4>), grid, block, 0, stream, a); break;
    }
}

}  // namespace

void launch_edit_distance(const IndexView &ix, const uint8_t *d_qbuf, const uint64_t *d_qoff, uint64_t nq, bool packed,
                          uint32_t uniform_len, const uint32_t *d_cand_query, const uint32_t *d_cand_begin,
                          const gdx_hit32_t *d_cand_hits, uint64_t m, uint32_t max_edits, uint32_t *d_out_dist,
                          uint32_t *d_out_end, hipStream_t stream)
{
    if (m == 0) return;
    EditArgs a;
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
    a.out_end = d_out_end;
    if (packed) launch_xlate<2>(a, stream);
    else if (ix.perm_ok) launch_xlate<1>(a, stream);
    else launch_xlate<0>(a, stream);
}

}  // namespace gdx
