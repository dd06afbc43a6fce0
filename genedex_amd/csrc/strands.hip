// strands.hip -- both-strand search: a resident query batch turned into its reverse complement, or into a batch
// that holds both strands side by side (gdx_strands_expand_dev), in front of the unchanged search chains.
//
//   the definition      r[j] = comp[q[m - 1 - j]]; comp is a 256-entry table from IO symbol to IO symbol (plain form)
//                       or code ^ 3 (packed form); dna_complement_table is the stock IUPAC table, check_complement
//                       the two host-side rules of gdx.h that tie a table to an index
//   strands_expand_kernel<PACKED, UNIFORM, BOTH>
//                       one lane per OUTPUT word (8 IO symbols in 64 bits, or 16 two-bit symbols in 32 bits); the lane
//                       finds the row that owns its first symbol -- a reciprocal multiply for a uniform batch, a binary
//                       search over the offsets otherwise -- and walks the rows that share the word.  Every piece of a
//                       row inside the word is a contiguous run of the input: two aligned words funnel-shifted, then
//                       reversed (v_perm_b32 on bytes; v_bfrev_b32 + a swap of the bits of every pair on codes) and
//                       complemented (LDS table; XOR).  Every output word is written exactly once and whole, so the
//                       bits that belong to no query are zero without a fill in front and without atomics.
//   strands_offsets_kernel   the 2 nq + 1 zero-based offsets of a BOTH batch with offsets
#include "common.hpp"
#include "kernels.hpp"

namespace gdx {

void dna_complement_table(uint8_t out[256])
{
    for (int c = 0; c < 256; c++) out[c] = static_cast<uint8_t>(c);
    const char *from = "ACGTRYKMBVDHSWN";
    const char *to = "TGCAYRMKVBHDSWN";
    for (int k = 0; from[k]; k++) {
        out[static_cast<uint8_t>(from[k])] = static_cast<uint8_t>(to[k]);
        out[static_cast<uint8_t>(from[k] + 32)] = static_cast<uint8_t>(to[k] + 32);
    }
}

void check_complement(const uint8_t *io_to_dense, const uint8_t *comp, bool packed)
{
    for (int c = 0; c < 256; c++) {
        const uint8_t d = io_to_dense[c], dc = io_to_dense[comp[c]];
        if ((d == 0) != (dc == 0))
            fail(GDX_ERR_INVALID_ARGUMENT,
                 "the complement table maps byte %d to %d and exactly one of them is in the index's alphabet: the status "
                 "bytes of the two strands would mean different things",
                 c, (int)comp[c]);
        if (packed && d >= 1 && d <= 4 && dc != 5 - d)
            fail(GDX_ERR_INVALID_ARGUMENT,
                 "packed queries are complemented as code ^ 3, which needs dense(comp[c]) == 5 - dense(c) for the dense symbols "
                 "1..4; byte %d has dense symbol %d and its complement %d",
                 c, (int)d, (int)dc);
    }
}

uint64_t strands_out_bytes(uint64_t total_symbols, bool packed, uint32_t mode)
{
    const uint64_t symbols = static_cast<uint64_t>(mode) * total_symbols;
    return packed ? gdx_packed_bytes(symbols) : div_ceil(symbols, 8) * 8 + 8;
}

namespace {

constexpr int kBlock = 256;

struct ComplementTable {
    uint8_t b[256];
};

struct StrandsArgs {
    const uint8_t *qbuf;   // plain: 8-byte aligned, padded to 8; packed: 2-byte aligned, gdx_packed_bytes of its symbols
    const uint64_t *qoff;  // null for a uniform batch
    uint64_t nq;
    uint64_t n_words;      // output words: strands_out_bytes / sizeof(word)
    uint32_t uniform_len;
    double inv_uniform_len;
    void *out;
};

template <bool PACKED>
struct Form;
template <>
struct Form<false> {
    using Word = uint64_t;
    static constexpr uint32_t kSymbols = 8, kBits = 8;
    // L (1..8) symbols from symbol s of the buffer, in the low bits
    static __device__ __forceinline__ Word fetch(const uint8_t *qbuf, uint64_t s, uint32_t L)
    {
        const uint64_t *in = reinterpret_cast<const uint64_t *>(qbuf);
        const uint32_t phase = static_cast<uint32_t>(s & 7u);
        uint64_t x = in[s >> 3] >> (8u * phase);
        if (phase + L > 8u) x |= in[(s >> 3) + 1] << (64u - 8u * phase);  // (the word holds a symbol of the query: inside the buffer)
        return x & mask(L);
    }
    static __device__ __forceinline__ Word mask(uint32_t L) { return L >= 8u ? ~0ull : (1ull << (8u * L)) - 1ull; }
    static __device__ __forceinline__ Word revcomp(Word x, uint32_t L, const uint8_t *s_comp)
    {
        const uint32_t lo = __builtin_amdgcn_perm(0u, static_cast<uint32_t>(x), 0x00010203u);
        const uint32_t hi = __builtin_amdgcn_perm(0u, static_cast<uint32_t>(x >> 32), 0x00010203u);
        const uint64_t y = ((static_cast<uint64_t>(lo) << 32) | hi) >> (8u * (8u - L));
        uint64_t r = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) r |= static_cast<uint64_t>(s_comp[(y >> (8u * k)) & 0xffu]) << (8u * k);
        return r & mask(L);
    }
};
template <>
struct Form<true> {
    using Word = uint32_t;
    static constexpr uint32_t kSymbols = 16, kBits = 2;
    // L (1..16) symbols from symbol s: the 8 bytes at 16-bit unit s >> 3 hold at least 25 symbols from s on, and end
    // inside gdx_packed_bytes of the buffer's symbols
    static __device__ __forceinline__ Word fetch(const uint8_t *qbuf, uint64_t s, uint32_t L)
    {
        const uint16_t *in = reinterpret_cast<const uint16_t *>(qbuf) + (s >> 3);
        uint64_t v;
        __builtin_memcpy(&v, in, sizeof(v));
        const uint32_t x = __builtin_amdgcn_alignbit(static_cast<uint32_t>(v >> 32), static_cast<uint32_t>(v),
                                                     2u * static_cast<uint32_t>(s & 7u));
        return x & mask(L);
    }
    static __device__ __forceinline__ Word mask(uint32_t L) { return L >= 16u ? ~0u : (1u << (2u * L)) - 1u; }
    static __device__ __forceinline__ Word revcomp(Word x, uint32_t L, const uint8_t *)
    {
        uint32_t v = __builtin_bitreverse32(x);  // symbol k -> 15 - k, the two bits of every symbol swapped
        v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
        return (v >> (2u * (16u - L))) ^ mask(L);
    }
};

// the row that owns output symbol p: how many offsets keys are <= p (0: p lies in front of the first query)
template <bool BOTH>
__device__ __forceinline__ uint64_t keys_at_or_below(const uint64_t *__restrict__ qoff, uint64_t nq, uint64_t base, uint64_t p)
{
    uint64_t lo = 0, hi = nq + 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const uint64_t key = BOTH ? 2 * (qoff[mid] - base) : qoff[mid];
        if (key <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <bool PACKED, bool UNIFORM, bool BOTH>
__global__ __launch_bounds__(kBlock) void strands_expand_kernel(const StrandsArgs a, const ComplementTable comp)
{
    using F = Form<PACKED>;
    using Word = typename F::Word;
    __shared__ uint8_t s_comp[256];
    if (!PACKED) {
        for (int i = threadIdx.x; i < 256; i += kBlock) s_comp[i] = comp.b[i];
        __syncthreads();
    }
    Word *__restrict__ out = static_cast<Word *>(a.out);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; w < a.n_words; w += stride) {
        const uint64_t first = w * F::kSymbols, wend = first + F::kSymbols;
        uint64_t cur = first;
        Word word = 0;
        if (UNIFORM) {
            const uint64_t ulen = a.uniform_len;
            const uint64_t end_all = (BOTH ? 2 : 1) * a.nq * ulen;
            // row of the word's first symbol: a reciprocal multiply and one correction step (uniform_len < 2^21)
            uint64_t row = static_cast<uint64_t>(static_cast<double>(cur) * a.inv_uniform_len);
            if (row * ulen > cur) row--;
            else if ((row + 1) * ulen <= cur) row++;
            uint64_t o = cur - row * ulen;
            while (cur < wend && cur < end_all) {
                const bool rev = BOTH ? (row & 1u) != 0 : true;
                const uint64_t i = BOTH ? row >> 1 : row;
                const uint64_t left = ulen - o, room = wend - cur;
                const uint32_t L = static_cast<uint32_t>(left < room ? left : room);
                Word x = F::fetch(a.qbuf, i * ulen + (rev ? ulen - o - L : o), L);
                if (rev) x = F::revcomp(x, L, s_comp);
                word |= x << (F::kBits * static_cast<uint32_t>(cur - first));
                cur += L;
                row++;  // (a piece that ended at the word's end leaves the loop)
                o = 0;
            }
        } else {
            const uint64_t base = a.qoff[0];
            uint64_t i = keys_at_or_below<BOTH>(a.qoff, a.nq, base, cur);
            if (i == 0) {  // in front of the first query (REVERSE of a view that starts inside its buffer): zeros
                cur = base < wend ? base : wend;
            } else {
                i--;
            }
            while (cur < wend && i < a.nq) {
                const uint64_t qb = a.qoff[i], len = a.qoff[i + 1] - qb;
                if (len == 0) {  // a run of empty queries: find the owner again instead of stepping through it
                    i = keys_at_or_below<BOTH>(a.qoff, a.nq, base, cur) - 1;
                    continue;
                }
                const uint64_t obeg = BOTH ? 2 * (qb - base) : qb;
                uint64_t o = cur - obeg;
                const bool rev = BOTH ? o >= len : true;
                if (BOTH && rev) o -= len;
                const uint64_t left = len - o, room = wend - cur;
                const uint32_t L = static_cast<uint32_t>(left < room ? left : room);
                Word x = F::fetch(a.qbuf, qb + (rev ? len - o - L : o), L);
                if (rev) x = F::revcomp(x, L, s_comp);
                word |= x << (F::kBits * static_cast<uint32_t>(cur - first));
                cur += L;
                if (o + L == len && rev) i++;
            }
        }
        out[w] = word;
    }
}

__global__ __launch_bounds__(kBlock) void strands_offsets_kernel(const uint64_t *__restrict__ qoff, uint64_t nq,
                                                                 uint64_t *__restrict__ out_qoff)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    const uint64_t base = qoff[0];
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i <= nq; i += stride) {
        const uint64_t b = 2 * (qoff[i] - base);
        out_qoff[2 * i] = b;
        if (i < nq) out_qoff[2 * i + 1] = b + (qoff[i + 1] - qoff[i]);
    }
}

template <bool PACKED, bool UNIFORM>
void launch_expand(const StrandsArgs &a, const ComplementTable &comp, bool both, hipStream_t stream)
{
    const dim3 grid(grid_for(a.n_words, kBlock, 256u * 32u)), block(kBlock);
    if (both) hipLaunchKernelGGL((strands_expand_kernel<PACKED, UNIFORM, true>), grid, block, 0, stream, a, comp);
    else hipLaunchKernelGGL((strands_expand_kernel<PACKED, UNIFORM, false>), grid, block, 0, stream, a, comp);
}

}  // namespace

void launch_strands_expand(const uint8_t *d_qbuf, const uint64_t *d_qoff, uint64_t nq, bool packed, uint32_t uniform_len,
                           uint64_t total_symbols, const uint8_t *complement, uint32_t mode, void *d_out_qbuf,
                           uint64_t *d_out_qoff, hipStream_t stream)
{
    const bool both = mode == GDX_STRANDS_BOTH;
    const uint64_t out_bytes = strands_out_bytes(total_symbols, packed, mode);
    if (nq == 0) {  // nothing to read: the (padding-only) output is zeros
        GDX_HIP(hipMemsetAsync(d_out_qbuf, 0, out_bytes, stream));
        if (both && uniform_len == 0 && d_out_qoff) GDX_HIP(hipMemsetAsync(d_out_qoff, 0, sizeof(uint64_t), stream));
        return;
    }
    StrandsArgs a;
    a.qbuf = d_qbuf;
    a.qoff = uniform_len ? nullptr : d_qoff;
    a.nq = nq;
    a.n_words = out_bytes / (packed ? 4 : 8);
    a.uniform_len = uniform_len;
    a.inv_uniform_len = uniform_len ? 1.0 / static_cast<double>(uniform_len) : 0.0;
    a.out = d_out_qbuf;
    ComplementTable comp;
    for (int c = 0; c < 256; c++) comp.b[c] = complement[c];
    if (packed) {
        if (uniform_len) launch_expand<true, true>(a, comp, both, stream);
        else launch_expand<true, false>(a, comp, both, stream);
    } else {
        if (uniform_len) launch_expand<false, true>(a, comp, both, stream);
        else launch_expand<false, false>(a, comp, both, stream);
    }
    if (both && uniform_len == 0)
        hipLaunchKernelGGL(strands_offsets_kernel, dim3(grid_for(nq + 1, kBlock)), dim3(kBlock), 0, stream, d_qoff, nq, d_out_qoff);
}

}  // namespace gdx
