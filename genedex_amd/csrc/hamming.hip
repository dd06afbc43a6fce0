// hamming.hip -- seed-and-verify: the Hamming distance of whole reads against the text on the diagonals of located seeds
// (gdx_hamming_many[_dev]).  Nothing here touches the index proper: the kernel gathers text units and read bytes.  The
// argument block, the read loader (read_chunk) and the resolution of a candidate are verify.hpp's, shared with
// edit_distance.hip and align.hip.
//
//   the definition      candidate c = (query q of L symbols, seed begin b, hit (text T, position p)); s = p - b; symbol j of
//                       the read matches when 0 <= s + j < |T|, dense(q[j]) is one of 1..4 and equals dense(T[s + j]);
//                       out[c] = min(#mismatches, max_mismatches + 1), GDX_HAMMING_INVALID for q >= nq or T >= n_texts
//   hamming_kernel<kXlate, kUniform>
//                       four lanes per candidate; a round covers 128 read symbols, lane `sub` the 32 from 32 sub on.  The
//                       lane funnel-shifts the two text units that hold its window into 64 bits of codes + a 32-bit "not
//                       1..4" mask, takes the same from the read (read_chunk; kXlate 1: v_perm_b32 tables of
//                       IndexView::perm_*; 0: the alphabet table in LDS; 2: packed reads are the codes), XORs, folds the two
//                       bits of every symbol, ORs in both masks and the symbols outside [0, |T|) -- from the text's own
//                       bounds in `sentinels`, never from the pad units or the neighbouring text -- and counts.  quad_sum
//                       adds the lanes; the group leaves the loop once it is over the limit.  Lane 0 of the group stores
//                       the result.
#include "verify.hpp"

namespace gdx {

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kGroup = 4, kGroups = kBlock / kGroup;

struct HammingArgs : VerifyArgs {
    uint32_t limit;  // max_mismatches + 1 (<= 2^31 + 1)
    uint32_t *out;
};

template <int kXlate, bool kUniform>
__global__ __launch_bounds__(kBlock) void hamming_kernel(const HammingArgs a)
{
    __shared__ uint8_t s_dense[256];
    load_dense_table<kXlate, kBlock>(s_dense, a.io_to_dense);
    const uint32_t sub = threadIdx.x & (kGroup - 1u);
    for (uint64_t c = static_cast<uint64_t>(blockIdx.x) * kGroups + threadIdx.x / kGroup; c < a.m;
         c += static_cast<uint64_t>(gridDim.x) * kGroups) {
        // (everything up to the round loop is the same in the four lanes of the group: control flow is uniform in it)
        Candidate k;
        if (resolve_candidate<kUniform, false>(a, c, k) != 0u) {
            if (sub == 0u) a.out[c] = GDX_HAMMING_INVALID;
            continue;
        }
        resolve_text(a, k);
        const uint64_t begin = k.begin;
        const uint32_t L = k.L;
        const int64_t t0 = k.t0, t_len = k.t_len, s = k.s;
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
                    // read side: symbol j0 + i in bits 2 i + 1 : 2 i of qc, bit i of inv when it is not one of 1..4
                    uint64_t qc;
                    uint32_t inv;
                    read_chunk<kXlate>(a, s_dense, begin + j0, n_c, qc, inv);
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
    fill_verify_args(a, ix, d_qbuf, d_qoff, nq, uniform_len, d_cand_query, d_cand_begin, d_cand_hits, m);
    a.limit = max_mismatches + 1u;
    a.out = d_out;
    if (packed) launch_xlate<2>(a, stream);
    else if (ix.perm_ok) launch_xlate<1>(a, stream);
    else launch_xlate<0>(a, stream);
}

}  // namespace gdx
