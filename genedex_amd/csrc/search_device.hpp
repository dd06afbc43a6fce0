// search_device.hpp -- what more than one kernel family of search.hip, or search.hip and search_ops.hip both, use: the block
// size, the query windows (QueryWindow / PackedQueryWindow / SpanWindow / FastWindow), the top-table lookup, the length-ordered
// schedule of a block's range, the packed resume states, and on the host side grid_for_items and GDX_DISPATCH_TABLE.  A helper
// of one family only stays with that family in search.hip.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "kernels.hpp"

namespace gdx {

namespace {

constexpr int kBlock = 256;

// Reads the IO symbols of one query right-to-left through aligned 8-byte windows, so a lane
// issues one global load per 8 LF steps; the next window is requested one window ahead.
struct QueryWindow {
    const uint64_t *words;
    uint64_t cur;        // window holding byte `pos-1`
    uint64_t next;       // window below it (prefetched)
    uint64_t cur_word;   // index of `cur`
    uint64_t first_word; // lowest word that belongs to this query

    __device__ __forceinline__ void init(const uint8_t *qbuf, uint64_t begin, uint64_t pos)
    {
        words = reinterpret_cast<const uint64_t *>(qbuf);
        first_word = begin >> 3;
        const bool any = pos > begin;
        cur_word = any ? ((pos - 1) >> 3) : first_word;
        cur = any ? words[cur_word] : 0ull;
        next = (any && cur_word > first_word) ? words[cur_word - 1] : 0ull;
    }
    // byte at absolute offset `at` (at must walk downwards)
    __device__ __forceinline__ uint32_t get(uint64_t at)
    {
        const uint64_t w = at >> 3;
        if (w != cur_word) {
            cur_word = w;
            cur = next;
            next = (w > first_word) ? words[w - 1] : 0ull;
        }
        return static_cast<uint32_t>(cur >> ((at & 7u) * 8u)) & 0xffu;
    }
};

// The same over packed queries (include/gdx.h "packed queries": symbol j of the buffer in bits 2 (j & 7) of 16-bit unit
// j >> 3, offsets count symbols): one 2-byte load per 8 LF steps; get() returns the 2-bit code (dense symbol - 1).
struct PackedQueryWindow {
    const uint16_t *units;
    uint32_t cur, next;
    uint64_t cur_unit, first_unit;

    __device__ __forceinline__ void init(const uint8_t *qbuf, uint64_t begin, uint64_t pos)
    {
        units = reinterpret_cast<const uint16_t *>(qbuf);
        first_unit = begin >> 3;
        const bool any = pos > begin;
        cur_unit = any ? ((pos - 1) >> 3) : first_unit;
        cur = any ? units[cur_unit] : 0u;
        next = (any && cur_unit > first_unit) ? units[cur_unit - 1] : 0u;
    }
    __device__ __forceinline__ uint32_t get(uint64_t at)
    {
        const uint64_t u = at >> 3;
        if (u != cur_unit) {
            cur_unit = u;
            cur = next;
            next = (u > first_unit) ? units[u - 1] : 0u;
        }
        return (cur >> ((at & 7u) * 2u)) & 3u;
    }
};

// Where query q lies in the buffer: [qbeg[q], qend[q]) from the offsets arrays, or -- a UNIFORM batch, ulen != 0: every
// query has ulen symbols and query q starts at q * ulen (gdx_query_layout_t) -- computed, which saves the kernels the
// 8 bytes of offsets per query (the arrays may then be null).
__device__ __forceinline__ uint64_t query_begin(const uint64_t *__restrict__ qbeg, uint32_t ulen, uint64_t q)
{
    return ulen != 0u ? q * ulen : qbeg[q];
}
__device__ __forceinline__ uint64_t query_end(const uint64_t *__restrict__ qend, uint32_t ulen, uint64_t q)
{
    return ulen != 0u ? (q + 1u) * ulen : qend[q];
}
// the aligned word (packed, kXlate == 2: the 16-bit unit) that holds the first symbol of a query: fast_window's `wbase`
template <int kXlate>
__device__ __forceinline__ const uint64_t *query_words(const uint8_t *__restrict__ qbuf, uint64_t begin)
{
    if (kXlate == 2) return reinterpret_cast<const uint64_t *>(reinterpret_cast<const uint16_t *>(qbuf) + (begin >> 3));
    return reinterpret_cast<const uint64_t *>(qbuf) + (begin >> 3);
}

// all eight nibbles are dense codes 1..4 (searchable DNA symbols)
__device__ __forceinline__ bool all_dna(uint32_t x)
{
    const uint32_t y = x - 0x11111111u;  // per nibble c - 1 when there is no zero nibble (no borrow)
    return ((y & ~x & 0x88888888u) | (y & 0xccccccccu)) == 0u;
}

// eight nibble codes 1..4 -> eight 2-bit codes (c - 1), nibble 7 (the symbol consumed first) in bits 15:14: the form
// the jump entries store (layout.hpp).  Only meaningful when all_dna(x).
__device__ __forceinline__ uint32_t to_2bit(uint32_t x)
{
    uint32_t y = x - 0x11111111u;
    y = (y & 0x03030303u) | ((y & 0x30303030u) >> 2);
    y = (y & 0x000f000fu) | ((y & 0x0f000f00u) >> 4);
    return (y & 0xffu) | ((y >> 8) & 0xff00u);
}

// The query as the pair kernels see it: dense codes, one nibble per symbol, eight symbols per 32-bit word, read
// right-to-left.  The kGroup lanes of a query translate the query COOPERATIVELY: a span of eight 8-byte words (64
// bytes: a whole 50-mer) is loaded and translated through the alphabet table in LDS by the group at once, each lane
// its own one (8 lanes) or two (4 lanes) words, and any lane fetches any translated word of the span from its
// owner with one ds_bpermute (the LDS crossbar, no LDS memory).  Translating every word in every lane -- which is
// what a plain per-lane window does -- made the kernel VALU-bound: PMC showed 880 VALU instructions per wavefront
// and 16 queries, 85 % VALU issue utilisation, and no gain from a quarter fewer DRAM requests.
constexpr uint32_t kNoCode = 0x10000u;  // compares unequal to every 16-bit entry code

// kPacked: the query buffer holds 2-bit codes (dense symbol - 1 of the four searchable symbols, symbol j of the
// buffer in bits 2 (j & 3) of byte j >> 2; include/gdx.h "packed queries") and offsets count SYMBOLS: a span word is
// then a 16-bit unit of the buffer that needs no translation at all.
template <int kGroup, bool kPacked>
struct SpanWindow {
    static constexpr int kWordsPerLane = 8 / kGroup;
    const uint64_t *base;  // base[0] holds the first byte of the query (packed: the 16-bit unit of its first symbol)
    uint32_t off0;         // byte (packed: symbol) offset of the query inside base[0] (inside its first unit)
    uint32_t top_w;        // span word k = query word top_w - k, k = 0 .. 7 (words below 0 read as 0)
    uint32_t w0, w1;       // this lane's translated span words: k = sub * kWordsPerLane (and + 1)
    uint32_t p;            // the same words as 2-bit codes (dense - 1), 16 bits each: w0 in the low half, w1 above
    uint32_t valid8;       // bit k: all eight symbols of span word k are dense codes 1..4 (the same in the group)

    static __device__ __forceinline__ uint32_t translate(uint64_t w, const uint8_t *s_dense)
    {
        uint32_t t = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) t |= static_cast<uint32_t>(s_dense[(w >> (8u * k)) & 0xffu]) << (4u * k);
        return t;
    }
    __device__ __forceinline__ void init(const uint8_t *qbuf, uint64_t begin)
    {
        if (kPacked) base = reinterpret_cast<const uint64_t *>(reinterpret_cast<const uint16_t *>(qbuf) + (begin >> 3));
        else base = reinterpret_cast<const uint64_t *>(qbuf) + (begin >> 3);
        off0 = static_cast<uint32_t>(begin & 7u);
        top_w = 0;
        w0 = w1 = p = valid8 = 0;
    }
    // eight 2-bit codes -> eight nibble codes 1..4
    static __device__ __forceinline__ uint32_t spread(uint32_t u)
    {
        uint32_t x = u & 0xffffu;
        x = (x | (x << 8)) & 0x00ff00ffu;
        x = (x | (x << 4)) & 0x0f0f0f0fu;
        x = (x | (x << 2)) & 0x33333333u;
        return x + 0x11111111u;
    }
    // positions the span so that its first word holds symbol rem - 1 (rem >= 1); group-uniform
    __device__ __forceinline__ void load(uint32_t rem, const uint8_t *s_dense)
    {
        const uint32_t sub = threadIdx.x & (kGroup - 1u);
        top_w = (off0 + rem - 1u) >> 3;
        const int32_t first = static_cast<int32_t>(top_w) - static_cast<int32_t>(sub) * kWordsPerLane;
        if (kPacked) {  // the units ARE the 2-bit span words; every symbol is one of the four searchable ones
            const uint16_t *units = reinterpret_cast<const uint16_t *>(base);
            const uint32_t u0 = first >= 0 ? units[first] : 0u;
            const uint32_t u1 = (kWordsPerLane == 2 && first >= 1) ? units[first - 1] : 0u;
            p = u0 | (u1 << 16);
            w0 = spread(u0);
            w1 = spread(u1);
            valid8 = 0xffu;
            return;
        }
        uint64_t r0 = 0, r1 = 0;
        if (kWordsPerLane == 2) {
            if (first >= 1) {  // both words with one 16-byte load (8-byte aligned)
                const u32x4 v = *reinterpret_cast<const u32x4 *>(base + (first - 1));
                r1 = static_cast<uint64_t>(v.x) | (static_cast<uint64_t>(v.y) << 32);
                r0 = static_cast<uint64_t>(v.z) | (static_cast<uint64_t>(v.w) << 32);
            } else if (first == 0) {
                r0 = base[0];
            }
        } else if (first >= 0) {
            r0 = base[first];
        }
        finish(r0, r1, s_dense);
    }
    // the second half of load(): this lane's raw span words -> translated words, 2-bit form, validity mask
    __device__ __forceinline__ void finish(uint64_t r0, uint64_t r1, const uint8_t *s_dense)
    {
        const uint32_t sub = threadIdx.x & (kGroup - 1u);
        w0 = translate(r0, s_dense);
        if (kWordsPerLane == 2) w1 = translate(r1, s_dense);
        // 2-bit form and the group's validity mask (an OR over the group's lanes by DPP)
        p = to_2bit(w0);
        uint32_t m = all_dna(w0) ? 1u : 0u;
        if (kWordsPerLane == 2) {
            p |= to_2bit(w1) << 16;
            m |= all_dna(w1) ? 2u : 0u;
        }
        m <<= sub * kWordsPerLane;
        m |= static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(m), 0xB1, 0xF, 0xF, true));
        m |= static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(m), 0x4E, 0xF, 0xF, true));
        if (kGroup == 8) m |= static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(m), 0x141, 0xF, 0xF, true));
        valid8 = m;
    }
    // 2-bit codes of span word k (16 bits)
    __device__ __forceinline__ uint32_t word2(uint32_t k) const
    {
        const uint32_t owner = (threadIdx.x & 63u & ~(kGroup - 1u)) + k / kWordsPerLane;
        const uint32_t v = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(static_cast<int>(owner << 2), static_cast<int>(p)));
        return (kWordsPerLane == 2 && (k & 1u)) ? v >> 16 : v & 0xffffu;
    }
    // 2-bit codes of the symbols r - 1 .. r - 8 (r >= 8, covered by the span), bits 15:14 = symbol r - 1: the form the
    // jump entries store; kNoCode when a word they touch holds a symbol outside 1..4 (conservative: the caller then
    // looks at the nibbles)
    __device__ __forceinline__ uint32_t level(uint32_t r) const
    {
        const uint32_t b = off0 + r - 1u, k = top_w - (b >> 3);
        const uint32_t s = (b & 7u) + 1u;
        const uint32_t k1 = k + 1u > 7u ? 7u : k + 1u;
        const uint32_t need = (1u << k) | (s < 8u ? (1u << k1) : 0u);
        const uint32_t x = (word2(k) << 16) | word2(k1);
        return (valid8 & need) == need ? ((x >> (2u * s)) & 0xffffu) : kNoCode;
    }
    // translated span word k (0 .. 7), k uniform in the group
    __device__ __forceinline__ uint32_t word(uint32_t k) const
    {
        const uint32_t owner = (threadIdx.x & 63u & ~(kGroup - 1u)) + k / kWordsPerLane;
        const uint32_t mine = (kWordsPerLane == 2 && (k & 1u)) ? w1 : w0;
        return static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(static_cast<int>(owner << 2), static_cast<int>(mine)));
    }
    // true when the symbols r - 1 .. r - 8 (those of them that exist) lie inside the span
    __device__ __forceinline__ bool covers(uint32_t r) const
    {
        const uint32_t hi_w = (off0 + r - 1u) >> 3, lo_w = (off0 + (r >= 8u ? r - 8u : 0u)) >> 3;
        return hi_w <= top_w && top_w - lo_w <= 7u;
    }
    // codes of the 8 symbols that end with symbol r - 1 (nibble 7 = symbol r - 1); the span must cover them.
    // Nibbles of symbols before the start of the query are garbage and must not be used (callers check r).
    __device__ __forceinline__ uint32_t at(uint32_t r) const
    {
        const uint32_t b = off0 + r - 1u, k = top_w - (b >> 3);
        const uint32_t s = (b & 7u) + 1u;  // nibbles taken from span word k, the rest from word k + 1
        const uint32_t cur = word(k), next = word(k + 1u > 7u ? 7u : k + 1u);
        return s == 8u ? cur : __builtin_amdgcn_alignbit(cur, next, 4u * s);
    }
    // the same for the symbols the search consumes next (rem >= 1): moves the span down when they have left it
    __device__ __forceinline__ uint32_t code8(uint32_t rem, const uint8_t *s_dense)
    {
        if (!covers(rem)) load(rem, s_dense);
        return at(rem);
    }
};

__device__ __forceinline__ bool has_zero_nibble(uint32_t x) { return ((x - 0x11111111u) & ~x & 0x88888888u) != 0u; }

// Top table (IndexView::top): the interval after the first D = top_depth symbols of the search, i.e. the last D
// symbols of the query, when all of them are dense codes 1..4.  `a` = code8(rem), `b` = code8(rem - 8) (only its
// top D - 8 nibbles are used).  The entry of a D-mer that does not occur holds the frozen interval (start == end as
// they stood at the step that emptied it, like the reference's lookup tables, lookup_table.rs:225-258), so such a
// query is finished by the lookup.  Returns false when a symbol is outside 1..4: the caller then runs the ordinary
// steps from the start, which validate symbols as lazily as the reference does.
__device__ __forceinline__ bool top_lookup(const IndexView &ix, uint32_t a, uint32_t b, uint32_t &lo, uint32_t &hi)
{
    const uint32_t d = ix.top_depth;  // 1 .. 16: the top min(d, 8) nibbles of a and the top d - 8 of b
    const uint32_t ma = d >= 8u ? 0xffffffffu : 0xffffffffu << (4u * (8u - d));
    const uint32_t mb = d > 8u ? 0xffffffffu << (4u * (16u - d)) : 0u;
    const uint32_t va = (a & ma) | (0x11111111u & ~ma), vb = (b & mb) | (0x11111111u & ~mb);  // unused := valid
    if (!all_dna(va) || !all_dna(vb)) return false;
    const uint32_t idx = ((to_2bit(va) << 16) | to_2bit(vb)) >> (32u - 2u * d);
    const uint2 e = ix.top[idx];
    lo = e.x;
    hi = e.y;
    return true;
}

// appends the cursors of this wavefront's `alive` lanes to ca.active_out: one atomic per wavefront
__device__ __forceinline__ void compact_alive(bool alive, uint32_t q, const CursorArgs &ca)
{
    const unsigned long long mask = __ballot(alive);
    if (mask == 0ull) return;
    const uint32_t lane = __lane_id();
    const int leader = __ffsll(static_cast<long long>(mask)) - 1;
    uint32_t first = 0;
    if (static_cast<int>(lane) == leader) first = atomicAdd(ca.n_active_out, static_cast<uint32_t>(__popcll(mask)));
    first = __shfl(first, leader);
    if (alive) ca.active_out[first + __popcll(mask & ((1ull << lane) - 1ull))] = q;
}

// ---- length-ordered schedule inside a block -----------------------------------------------------------
// The lock-step kernel idles the lanes of a finished query until the longest query of its wavefront ends.  Every
// block searches a contiguous range of the batch (at most kMaxRange queries); when the lengths in that range are
// spread out it first orders the range by length (counting sort in LDS, 4 symbols per bucket, longest first) and
// its wavefronts take runs of that order, so the queries of a wavefront have nearly the same length.  Results
// are written at the original query index.  All reads and writes of a block stay inside its range, so the
// order costs no DRAM locality (an earlier batch-wide permutation did: its gathers were slower than the idle
// lanes it saved), and there is no pre-pass and no host round trip.  Ranges of (nearly) equal lengths skip it.
constexpr uint32_t kLenBuckets = 64;
constexpr uint32_t kMaxRange = 3072;  // queries per block and range: u16 permutation, 6 KB of LDS
constexpr uint32_t kMaxDefer = 512;   // stragglers a block can park per range (8 KB of LDS); more are finished in place
constexpr uint32_t kCursorRange = 1024;  // cursor extension: queries per range (their live list is 4 KB of LDS)

__device__ __forceinline__ uint32_t length_bucket(uint64_t len)
{
    const uint64_t b = len >> 2;
    return kLenBuckets - 1u - static_cast<uint32_t>(b < kLenBuckets - 1u ? b : kLenBuckets - 1u);
}

// Orders queries [base, base + cnt) of the batch by length bucket into s_perm (indices relative to base); returns
// false (s_perm untouched) when the lengths are uniform enough: max - min <= min / 4.  Block-wide, all threads.
__device__ __forceinline__ bool order_range_by_length(const uint64_t *__restrict__ qbeg,
                                                      const uint64_t *__restrict__ qend,
                                                      const uint32_t *__restrict__ active, uint64_t base, uint32_t cnt,
                                                      uint16_t *s_perm, uint32_t *s_cnt, uint32_t *s_minmax)
{
    if (threadIdx.x < kLenBuckets) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        s_minmax[0] = 0xffffffffu;
        s_minmax[1] = 0;
    }
    __syncthreads();
    uint32_t mn = 0xffffffffu, mx = 0;
    for (uint32_t i = threadIdx.x; i < cnt; i += blockDim.x) {
        const uint64_t qi = active ? active[base + i] : base + i;
        const uint64_t len = qend[qi] - qbeg[qi];
        const uint32_t l = len > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(len);
        mn = l < mn ? l : mn;
        mx = l > mx ? l : mx;
        atomicAdd(&s_cnt[length_bucket(len)], 1u);
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t omn = __shfl_xor(mn, off), omx = __shfl_xor(mx, off);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
    }
    if ((threadIdx.x & 63u) == 0) {
        atomicMin(&s_minmax[0], mn);
        atomicMax(&s_minmax[1], mx);
    }
    __syncthreads();
    mn = s_minmax[0];
    mx = s_minmax[1];
    if (mx - mn <= mn / 4u) return false;
    if (threadIdx.x < kLenBuckets) {  // exclusive scan of the histogram by the first wavefront
        const uint32_t v = s_cnt[threadIdx.x];
        uint32_t x = v;
        for (int off = 1; off < static_cast<int>(kLenBuckets); off <<= 1) {
            const uint32_t y = __shfl_up(x, off);
            if (static_cast<int>(threadIdx.x) >= off) x += y;
        }
        s_cnt[threadIdx.x] = x - v;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cnt; i += blockDim.x) {
        const uint64_t qi = active ? active[base + i] : base + i;
        const uint32_t r = atomicAdd(&s_cnt[length_bucket(qend[qi] - qbeg[qi])], 1u);
        s_perm[r] = static_cast<uint16_t>(i);
    }
    __syncthreads();
    return true;
}

// Live cursors of a block's range (cursor extension, mode 2) are appended to the global list IN THE ORDER OF THEIR
// POSITIONS in the range: s_live[p] = the cursor at position p, or kDeadCursor.  A list that starts sorted then stays
// sorted chunk by chunk, and the next call's gathers of start / end / status / string offsets by cursor number touch
// neighbouring lines; appending in the order of LDS atomics scattered them over sixteen lines per load instruction,
// which made a call over 34 M live cursors with empty strings cost 3.3 ms.
constexpr uint32_t kDeadCursor = 0xffffffffu;
__device__ __forceinline__ void flush_live_ordered(uint32_t *s_live, uint32_t cnt, uint32_t *s_part, uint32_t *s_base,
                                                   uint32_t *active_out, uint32_t *n_active_out)
{
    constexpr uint32_t kPer = kCursorRange / kBlock;
    uint32_t v[kPer], mine = 0;
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) {
        const uint32_t p = threadIdx.x * kPer + j;
        v[j] = p < cnt ? s_live[p] : kDeadCursor;
        s_live[p] = kDeadCursor;  // for the next range
        mine += v[j] != kDeadCursor ? 1u : 0u;
    }
    s_part[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {  // inclusive scan
        const uint32_t o = static_cast<int>(threadIdx.x) >= off ? s_part[threadIdx.x - off] : 0u;
        __syncthreads();
        s_part[threadIdx.x] += o;
        __syncthreads();
    }
    const uint32_t total = s_part[kBlock - 1];
    if (threadIdx.x == 0 && total != 0u) *s_base = atomicAdd(n_active_out, total);
    __syncthreads();
    uint32_t pos = *s_base + s_part[threadIdx.x] - mine;
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++)
        if (v[j] != kDeadCursor) active_out[pos++] = v[j];
    __syncthreads();
}

// resume states of the seed kernel's list in their packed form (search_seed_kernel4 -> search_fast_kernel4, state_packed):
// {lo, rows << 24 | kStatePacked | symbols left, codes hi, codes lo} carries the 32 symbols in front of the seed as 2-bit
// codes (the one to be consumed next in the top bits of `codes hi`); {lo, kStatePlain | symbols left, hi, 0} an interval
// of 256+ rows; all zero = from the beginning
constexpr uint32_t kStatePacked = 1u << 23, kStatePlain = 1u << 22;
// ... and, for search_verify_kernel4 only (state_packed == 2): {index of the k-mer's record in IndexView::seed_pairs,
// 2 << 24 | kStatePacked | kStatePair | symbols left (1..32), codes hi, codes lo} -- a k-mer on exactly two rows whose seed
// entry names such a record (kSeedPairInfo): the read is decided by that one 32-byte record.  3 << 24 / 4 << 24 in the rows' place:
// the index is that of the k-mer's 64-byte record in IndexView::seed_quads (kSeedQuadInfo)
constexpr uint32_t kStatePair = 1u << 21;
// the fields of a packed state's second word: symbols left (bits 0-20), the three flags, rows (bits 24-31, fewer than 256)
constexpr uint32_t kStateSymbolsMask = 0x1fffffu, kStateRowsShift = 24, kStateRowsMask = 0xffu << kStateRowsShift;
static_assert((kStatePacked & kStatePlain) == 0u && (kStatePacked & kStatePair) == 0u && (kStatePlain & kStatePair) == 0u,
              "state flags overlap");
static_assert(((kStatePacked | kStatePlain | kStatePair) & kStateSymbolsMask) == 0u, "a state flag overlaps the symbols left");
static_assert(((kStatePacked | kStatePlain | kStatePair) & kStateRowsMask) == 0u, "a state flag overlaps the rows");
static_assert((kStateSymbolsMask & kStateRowsMask) == 0u && kStateRowsShift + 8u == 32u, "the symbols left overlap the rows, or rows < 256 do not fill the top byte");
static_assert(kStateSymbolsMask >= 32u && (kStateSymbolsMask & (kStateSymbolsMask + 1u)) == 0u, "symbols left: a low bit field");

struct FastWindow {
    uint32_t l0, l1, l2, l3;  // level 2 t | level 2 t + 1 << 16 held by lane t of the group (level j = the 2-bit codes
                              // of the symbols rem - 1 - 8 j .. rem - 8 - 8 j, bits 15:14 = the first of them)
    uint32_t valid8;          // bit k: every symbol of span word k is one of the four searchable ones
    uint32_t s0;              // symbols of a level that lie in its first span word (1 .. 8)
};
// four query bytes -> their 2-bit codes in 8 bits (byte 0 in bits 1:0); `bad` becomes non-zero on any other byte
template <class View>
__device__ __forceinline__ uint32_t fast_pack4(const View &ix, uint32_t c, uint32_t &bad)
{
    const uint32_t sel = c & 0x07070707u;
    const uint32_t code = __builtin_amdgcn_perm(ix.perm_code_hi, ix.perm_code_lo, sel);
    const uint32_t expect = __builtin_amdgcn_perm(ix.perm_exp_hi, ix.perm_exp_lo, sel);
    bad |= (c & ix.perm_mask) ^ expect;
    uint32_t t = (code << 6) | code;
    t = (t << 12) | t;
    return (t >> 18) & 0xffu;
}
__device__ __forceinline__ uint32_t fast_pack4_lds(const uint8_t *s_dense, uint32_t c, uint32_t &bad)
{
    uint32_t out = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint32_t d = static_cast<uint32_t>(s_dense[(c >> (8u * k)) & 0xffu]) - 1u;
        bad |= d & ~3u;
        out |= (d & 3u) << (2u * k);
    }
    return out;
}
// positions the window so that level 0 starts at symbol rem - 1 (rem >= 1): each lane loads and translates two of
// the eight span words (as SpanWindow::load), then the levels are cut out of the group's 128-bit code string
// kXlate: 0 = bytes through the table in LDS, 1 = bytes through the v_perm tables, 2 = packed queries (the span words
// are 16-bit units of the buffer, wbase points at the unit of the query's first symbol and off0 counts symbols)
// the loads of fast_window: this lane's two span words, untranslated (packed queries: both units in .x)
template <int kXlate>
__device__ __forceinline__ u32x4 fast_window_load(const uint64_t *wbase, uint32_t off0, uint32_t rem, uint32_t sub)
{
    const uint32_t b = off0 + rem - 1u;
    const int32_t first = static_cast<int32_t>(b >> 3) - static_cast<int32_t>(sub) * 2;
    u32x4 raw = {0u, 0u, 0u, 0u};  // x, y = word first - 1 (span word 2 sub + 1); z, w = word first (span word 2 sub)
    if (kXlate == 2) {
        const uint16_t *units = reinterpret_cast<const uint16_t *>(wbase);
        const uint32_t u0 = first >= 0 ? units[first] : 0u;
        const uint32_t u1 = first >= 1 ? units[first - 1] : 0u;
        raw.x = u0 | (u1 << 16);
    } else if (first >= 1) {
        raw = *reinterpret_cast<const u32x4 *>(wbase + (first - 1));
    } else if (first == 0) {
        const uint64_t r0 = wbase[0];
        raw.z = static_cast<uint32_t>(r0);
        raw.w = static_cast<uint32_t>(r0 >> 32);
    }
    return raw;
}
template <int kXlate, class View>
__device__ __forceinline__ FastWindow fast_window_finish(const View &ix, const uint8_t *s_dense, u32x4 raw,
                                                         uint32_t off0, uint32_t rem, uint32_t sub)
{
    const uint32_t b = off0 + rem - 1u;
    const int32_t first = static_cast<int32_t>(b >> 3) - static_cast<int32_t>(sub) * 2;
    uint32_t bad0 = 0, bad1 = 0, p;
    if (kXlate == 2) {
        p = raw.x;
    } else {
        if (kXlate == 1) {
            p = fast_pack4(ix, raw.z, bad0) | (fast_pack4(ix, raw.w, bad0) << 8) | (fast_pack4(ix, raw.x, bad1) << 16) |
                (fast_pack4(ix, raw.y, bad1) << 24);
        } else {
            p = fast_pack4_lds(s_dense, raw.z, bad0) | (fast_pack4_lds(s_dense, raw.w, bad0) << 8) |
                (fast_pack4_lds(s_dense, raw.x, bad1) << 16) | (fast_pack4_lds(s_dense, raw.y, bad1) << 24);
        }
    }
    uint32_t m = ((bad0 == 0u && first >= 0) ? 1u : 0u) | ((bad1 == 0u && first >= 1) ? 2u : 0u);
    m <<= 2u * sub;
    m |= static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(m), 0xB1, 0xF, 0xF, true));
    m |= static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(m), 0x4E, 0xF, 0xF, true));
    FastWindow w;
    w.valid8 = m;
    w.s0 = (b & 7u) + 1u;
    // lane t: words 2 t (low half of p), 2 t + 1 (high half) and, from lane t + 1, word 2 t + 2
    const uint32_t nxt = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(p), 0xF9, 0xF, 0xF, true));  // quad_perm [1,2,3,3]
    const uint32_t even = __builtin_amdgcn_alignbit(p, p, 16);       // word 2 t << 16 | word 2 t + 1
    const uint32_t odd = (p & 0xffff0000u) | (nxt & 0xffffu);         // word 2 t + 1 << 16 | word 2 t + 2
    const uint32_t sh = 2u * w.s0;                                    // 2 .. 16
    const uint32_t lv = ((even >> sh) & 0xffffu) | ((odd >> sh) << 16);
    w.l0 = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(lv), 0x00, 0xF, 0xF, true));
    w.l1 = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(lv), 0x55, 0xF, 0xF, true));
    w.l2 = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(lv), 0xAA, 0xF, 0xF, true));
    w.l3 = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(lv), 0xFF, 0xF, 0xF, true));
    return w;
}
template <int kXlate, class View>
__device__ __forceinline__ FastWindow fast_window(const View &ix, const uint8_t *s_dense, const uint64_t *wbase,
                                                  uint32_t off0, uint32_t rem, uint32_t sub)
{
    return fast_window_finish<kXlate>(ix, s_dense, fast_window_load<kXlate>(wbase, off0, rem, sub), off0, rem, sub);
}

__device__ __forceinline__ uint32_t sel4(uint32_t i, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    uint32_t v = a;
    v = i == 1u ? b : v;
    v = i == 2u ? c : v;
    v = i == 3u ? d : v;
    return v;
}

}  // namespace

#define GDX_DISPATCH_TABLE(ix, KERNEL, grid, stream, ...)                                        \
    do {                                                                                         \
        if ((ix).layout == 0)                                                                    \
            hipLaunchKernelGGL(KERNEL<LineTable>, dim3(grid), dim3(kBlock), 0, stream, __VA_ARGS__); \
        else                                                                                     \
            hipLaunchKernelGGL(KERNEL<GenericTable>, dim3(grid), dim3(kBlock), 0, stream, __VA_ARGS__); \
    } while (0)

static unsigned grid_for_items(uint64_t items)
{
    const uint64_t blocks = (items + kBlock - 1) / kBlock;
    const uint64_t cap = 256u * 8u;  // 8 blocks of 256 threads per CU
    return static_cast<unsigned>(blocks < 1 ? 1 : (blocks < cap ? blocks : cap));
}

}  // namespace gdx
