// verify.hpp -- what the three verify stages (hamming.hip, edit_distance.hip, align.hip) have in common: the argument block of
// a batch of candidates, the read loader, the resolution of a candidate into its read and its text (hamming_kernel and
// align_lane; edit_lane keeps its own) and the instance dispatch of edit_kernel and align_kernel.  A stage keeps what is its
// own: the Hamming rounds, the forward pass of Myers' algorithm (edit_lane's, and align_lane's with the history stores), the
// output rules, the alignment's workspace and walk.
// profiles/r15/verify_refactor.md has what the shapes of these helpers do to the kernels' code.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "kernels.hpp"
#include "read_codes.hpp"

namespace gdx {

// the batch and its candidates; a stage's own arguments derive from it (pack4_perm reads the perm_* fields)
struct VerifyArgs {
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
};

inline void fill_verify_args(VerifyArgs &a, const IndexView &ix, const uint8_t *d_qbuf, const uint64_t *d_qoff, uint64_t nq,
                             uint32_t uniform_len, const uint32_t *d_cand_query, const uint32_t *d_cand_begin,
                             const gdx_hit32_t *d_cand_hits, uint64_t m)
{
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
}

// the instance of an edit_kernel / align_kernel batch: f(uniform, W) with compile-time values; an offsets batch runs W = 4
// with the lane's own block count, a uniform one W = ceil(uniform_len / 64) (over the limit 4: every lane leaves with
// GDX_EDIT_TOO_LONG before it looks at a block)
template <class F>
void dispatch_blocks(uint32_t uniform_len, F &&f)
{
    if (uniform_len == 0u) return f(std::false_type{}, std::integral_constant<int, 4>{});
    switch (uniform_len > GDX_EDIT_MAX_QUERY_LEN ? 4u : (uniform_len + 63u) >> 6) {
    case 1: return f(std::true_type{}, std::integral_constant<int, 1>{});
    case 2: return f(std::true_type{}, std::integral_constant<int, 2>{});
    case 3: return f(std::true_type{}, std::integral_constant<int, 3>{});
    default: return f(std::true_type{}, std::integral_constant<int, 4>{});
    }
}

// kXlate 0: the alphabet table in LDS, for pack4_lds
template <int kXlate, int kThreads>
__device__ __forceinline__ void load_dense_table(uint8_t *s_dense, const uint8_t *io_to_dense)
{
    if (kXlate == 0) {
        for (int i = threadIdx.x; i < 256; i += kThreads) s_dense[i] = io_to_dense[i];
        __syncthreads();
    }
}

// symbols [at, at + n_c) of the batch, n_c in 1..32 -> qc: symbol i in bits 2 i + 1 : 2 i (garbage from n_c on); inv: bit i
// set when symbol i is not one of 1..4.  kXlate 1: v_perm_b32 tables of IndexView::perm_*; 0: the alphabet table in LDS;
// 2: packed reads are the codes.  Only the 16-bit units / aligned 8-byte words (1 .. 5) that hold one of the chunk's symbols
// are loaded: gdx_packed_bytes covers whole units, and the words lie inside the padded buffer.
template <int kXlate>
__device__ __forceinline__ void read_chunk(const VerifyArgs &a, const uint8_t *s_dense, uint64_t at, uint32_t n_c, uint64_t &qc,
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

// a candidate, resolved in two steps: resolve_candidate gives its read, symbols [begin, begin + L) of the batch, and
// resolve_text its text: the text's own symbols are [t0, t0 + t_len) of the concatenation (between the sentinel in front and
// its own) and s is the seed's diagonal, its position in the text minus its begin in the read
struct Candidate {
    uint32_t L;
    uint64_t begin;
    uint32_t text_id, position, seed_begin;  // as listed: the hit and where the seed begins in the read
    int64_t t0, t_len, s;
};

static_assert(GDX_HAMMING_INVALID == GDX_EDIT_INVALID, "one out-of-range marker for the three stages");

// -> 0 and the candidate's read, or the marker the stage stores instead of a distance: GDX_EDIT_INVALID (== GDX_HAMMING_INVALID)
// for a query or text id out of range and, with kEditLimit, GDX_EDIT_TOO_LONG for a read of more than GDX_EDIT_MAX_QUERY_LEN
// symbols (Hamming has no limit)
template <bool kUniform, bool kEditLimit>
__device__ __forceinline__ uint32_t resolve_candidate(const VerifyArgs &a, uint64_t c, Candidate &k)
{
    const uint32_t q = a.cand_query[c];
    k.seed_begin = a.cand_begin[c];
    const gdx_hit32_t hit = a.cand_hits[c];
    k.text_id = hit.text_id;
    k.position = hit.position;
    k.begin = 0;
    k.L = 0;
    uint32_t marker;
    if (q >= a.nq || hit.text_id >= a.n_texts) {
        marker = GDX_EDIT_INVALID;
    } else {
        if (kUniform) {
            k.begin = static_cast<uint64_t>(q) * a.uniform_len;
            k.L = a.uniform_len;
        } else {
            k.begin = a.qoff[q];
            const uint64_t len = a.qoff[q + 1] - k.begin;
            k.L = kEditLimit && len > GDX_EDIT_MAX_QUERY_LEN ? GDX_EDIT_MAX_QUERY_LEN + 1u : static_cast<uint32_t>(len);
        }
        marker = kEditLimit && k.L > GDX_EDIT_MAX_QUERY_LEN ? GDX_EDIT_TOO_LONG : 0u;
    }
    return marker;
}

// the second step, for a candidate that resolve_candidate accepted (its text id indexes the sentinels)
__device__ __forceinline__ void resolve_text(const VerifyArgs &a, Candidate &k)
{
    k.t0 = k.text_id == 0u ? 0 : static_cast<int64_t>(a.sentinels[k.text_id - 1u]) + 1;
    k.t_len = static_cast<int64_t>(a.sentinels[k.text_id]) - k.t0;
    k.s = static_cast<int64_t>(k.position) - static_cast<int64_t>(k.seed_begin);
}

}  // namespace gdx
