// hamming.hip -- seed-and-verify: the Hamming distance of whole reads against the text on the diagonals of located seeds
// (gdx_hamming_many[_dev]).  Nothing here touches the index proper: the kernel gathers text units and read bytes.
//
//   the definition      candidate c = (query q of L symbols, seed begin b, hit (text T, position p)); s = p - b; symbol j of
//                       the read matches when 0 <= s + j < |T|, dense(q[j]) is one of 1..4 and equals dense(T[s + j]);
//                       out[c] = min(#mismatches, max_mismatches + 1), GDX_HAMMING_INVALID for q >= nq or T >= n_texts
//   hamming_kernel<kXlate, kUniform>
//                       four lanes per candidate; a round covers 128 read symbols, lane `sub` the 32 from 32 sub on.  The
//                       lane funnel-shifts the two text units that hold its window into 64 bits of codes + a 32-bit "not
//                       1..4" mask, builds the same from the read (kXlate 1: v_perm_b32 tables of IndexView::perm_*; 0: the
//                       alphabet table in LDS; 2: packed reads are the codes), XORs, folds the two bits of every symbol,
//                       ORs in both masks and the symbols outside [0, |T|) -- from the text's own bounds in `sentinels`,
//                       never from the pad units or the neighbouring text -- and counts.  quad_sum adds the lanes; the
//                       group leaves the loop once it is over the limit.  Lane 0 of the group stores the result.
#include "common.hpp"
#include "kernels.hpp"
#include "read_codes.hpp"

namespace gdx {

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kGroup = 4, kGroups = kBlock / kGroup;

struct HammingArgs {
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
    uint32_t limit;  // max_mismatches + 1 (<= 2^31 + 1)
    uint32_t *out;
};

template <int kXlate, bool kUniform>
__global__ __launch_bounds__(kBlock) void hamming_kernel(const HammingArgs a)
{
    __shared__ uint8_t s_dense[256];
    if (kXlate == 0) {
        for (int i = threadIdx.x; i < 256; i += kBlock) s_dense[i] = a.io_to_dense[i];
        __syncthreads();
    }
    const uint32_t sub = threadIdx.x & (kGroup - 1u);
    for (uint64_t c = static_cast<uint64_t>(blockIdx.x) * kGroups + threadIdx.x / kGroup; c < a.m;
         c += static_cast<uint64_t>(gridDim.x) * kGroups) {
        // (everything up to the round loop is the same in the four lanes of the group: control flow is uniform in it)
        const uint32_t q = a.cand_query[c], b = a.cand_begin[c];
        const gdx_hit32_t hit = a.cand_hits[c];
        if (q >= a.nq || hit.text_id >= a.n_texts) {
            if (sub == 0u) a.out[c] = GDX_HAMMING_INVALID;
            continue;
        }
        uint64_t begin;
        uint32_t L;
        if (kUniform) {
            begin = static_cast<uint64_t>(q) * a.uniform_len;
            L = a.uniform_len;
        } else {
            begin = a.qoff[q];
            L = static_cast<uint32_t>(a.qoff[q + 1] - begin);
        }
        // the text's own symbols are [t0, t0 + t_len) of the concatenation: between the sentinel in front and its own
        const int64_t t0 = hit.text_id == 0u ? 0 : static_cast<int64_t>(a.sentinels[hit.text_id - 1u]) + 1;
        const int64_t t_len = static_cast<int64_t>(a.sentinels[hit.text_id]) - t0;
        const int64_t s = static_cast<int64_t>(hit.position) - static_cast<int64_t>(b);
        uint32_t dist = 0;
        for (uint64_t done = 0; done < L && dist < a.limit; done += 32u * kGroup) {
            const uint64_t j0 = done + 32u * sub;
            uint32_t cnt = 0;
            if (j0 < L) {
                const uint32_t n_c = L - j0 < 32u ? static_cast<uint32_t>(L - j0) : 32u;
                // which of the chunk's symbols lie inside the text: i in [lo, hi)
                const int64_t w = s + static_cast<int64_t>(j0);  // the window starts at symbol w of the text
                const int64_t lo = w < 0 ? -w : 0, hi = t_len - w < n_c ? t_len - w : n_c;
                if (lo >= hi) {
                    cnt = n_c;  // wholly outside: no load
                } else {
                    const uint32_t inside = low_bits(static_cast<uint32_t>(hi)) & ~low_bits(static_cast<uint32_t>(lo));
                    // text side.  A symbol of the window is inside the text, so -32 < t0 + w < n: the two units exist
                    // (kTextPadUnits in front, two spare units behind the text)
                    const uint64_t ts = static_cast<uint64_t>(t0 + w + 32 * static_cast<int64_t>(kTextPadUnits));
                    const uint32_t tb = static_cast<uint32_t>(ts & 31u);
                    const u32x4 *tu = a.text_units + (ts >> 5);
                    const u32x4 u0 = tu[0];
                    const u32x4 u1 = tb + n_c > 32u ? tu[1] : u32x4{0u, 0u, 0u, 0u};
                    // read side
                    const uint64_t at = begin + j0;
                    uint64_t qc;       // symbol j0 + i in bits 2 i + 1 : 2 i
                    uint32_t inv = 0;  // bit i: symbol j0 + i is not one of 1..4
                    if (kXlate == 2) {
                        // the 16-bit units that hold the chunk's codes (1 .. 5); gdx_packed_bytes covers whole units
                        const uint16_t *up = reinterpret_cast<const uint16_t *>(a.qbuf) + (at >> 3);
                        const uint32_t sh = static_cast<uint32_t>(at & 7u) * 2u;
                        const uint32_t n_need = (static_cast<uint32_t>(at & 7u) + n_c + 7u) >> 3;
                        uint64_t lo64 = up[0];
                        uint32_t hi16 = 0;
                        if (n_need > 1u) lo64 |= static_cast<uint64_t>(up[1]) << 16;
                        if (n_need > 2u) lo64 |= static_cast<uint64_t>(up[2]) << 32;
                        if (n_need > 3u) lo64 |= static_cast<uint64_t>(up[3]) << 48;
                        if (n_need > 4u) hi16 = up[4];
                        qc = sh != 0u ? (lo64 >> sh) | (static_cast<uint64_t>(hi16) << (64u - sh)) : lo64;
                    } else {
                        // the aligned 8-byte words that hold one of the chunk's bytes (1 .. 5): inside the padded buffer
                        const uint64_t *wp = reinterpret_cast<const uint64_t *>(a.qbuf) + (at >> 3);
                        const uint32_t sh = static_cast<uint32_t>(at & 7u) * 8u;
                        const uint32_t n_need = (static_cast<uint32_t>(at & 7u) + n_c + 7u) >> 3;
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
                    const uint64_t c0 = static_cast<uint64_t>(u0.x) | (static_cast<uint64_t>(u0.y) << 32);
                    const uint64_t c1 = static_cast<uint64_t>(u1.x) | (static_cast<uint64_t>(u1.y) << 32);
                    const uint64_t tc = tb != 0u ? (c0 >> (2u * tb)) | (c1 << (64u - 2u * tb)) : c0;
                    const uint32_t tm = tb != 0u ? (u0.z >> tb) | (u1.z << (32u - tb)) : u0.z;
                    uint64_t x = qc ^ tc;
                    x |= x >> 1;
                    const uint32_t differ = even_bits(static_cast<uint32_t>(x)) | (even_bits(static_cast<uint32_t>(x >> 32)) << 16);
                    cnt = __popc((differ | inv | tm | ~inside) & low_bits(n_c));
                }
            }
            dist += quad_sum(cnt);
        }
        if (sub == 0u) a.out[c] = dist < a.limit ? dist : a.limit;
    }
}

template <int kXlate>
void launch_xlate(const HammingArgs &a, hipStream_t stream)
{
    const dim3 grid(grid_for(a.m * kGroup, kBlock, 256u * 32u)), block(kBlock);
    if (a.uniform_len != 0u) hipLaunchKernelGGL((hamming_kernel<kXlate, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((hamming_kernel<kXlate, false>), grid, block, 0, stream, a);
}

}  // namespace

void launch_hamming(const IndexView &ix, const uint8_t *d_qbuf, const uint64_t *d_qoff, uint64_t nq, bool packed,
                    uint32_t uniform_len, const uint32_t *d_cand_query, const uint32_t *d_cand_begin,
                    const gdx_hit32_t *d_cand_hits, uint64_t m, uint32_t max_mismatches, uint32_t *d_out, hipStream_t stream)
{
    if (m == 0) return;
    HammingArgs a;
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
    a.limit = max_mismatches + 1u;
    a.out = d_out;
    if (packed) launch_xlate<2>(a, stream);
    else if (ix.perm_ok) launch_xlate<1>(a, stream);
    else launch_xlate<0>(a, stream);
}

}  // namespace gdx
