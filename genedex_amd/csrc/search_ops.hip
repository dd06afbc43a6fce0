// search_ops.hip -- the operators that take no part in the search chain of search.hip: cursor extension by one symbol, suffix
// segments, SMEMs, rank / symbol_at / LF walk, the lookup and top table fills, query packing, top_wide; each kernel with its
// launch_* (kernels.hpp).
#include "search_device.hpp"

namespace gdx {

namespace {

// Cursor::extend_query_front for m independent cursors (cursor.rs:34-51).  kGroup lanes per cursor as in
// search_kernel; with pair lines (kPair) a symbol in 1..4 costs one 128-byte fetch and no table lookup.
template <class Table, int kGroup, bool kPair>
__global__ __launch_bounds__(kBlock) void extend_front_kernel(IndexView ix, uint32_t *__restrict__ start,
                                                              uint32_t *__restrict__ end,
                                                              const uint8_t *__restrict__ io_symbols, uint64_t m,
                                                              uint8_t *__restrict__ out_status)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * (kBlock / kGroup);
    const bool writer = (threadIdx.x % kGroup) == 0;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * (kBlock / kGroup) + threadIdx.x / kGroup; i < m; i += stride) {
        uint32_t lo = start[i], hi = end[i];
        const uint32_t c = ix.io_to_dense[io_symbols[i]];  // cursor.rs:34-38: translated before anything else
        uint32_t status = GDX_Q_OK;
        if (c == 0) {
            status = GDX_Q_INVALID_SYMBOL;
        } else if (lo != hi) {  // cursor.rs:41-48
            if (kPair && c <= 4u) {
                PairTable::lf1<1, 8>(ix, c, lo, hi, lo, hi);
            } else {
                uint32_t rlo, rhi;
                Table::rank2(ix, c, lo, hi, rlo, rhi);
                const uint32_t cc = ix.count[c];
                lo = cc + rlo;
                hi = cc + rhi;
            }
            if (writer) {
                start[i] = lo;
                end[i] = hi;
            }
        }
        if (out_status && writer) out_status[i] = static_cast<uint8_t>(status);
    }
}

// gdx_suffix_segments_many[_dev]: the greedy backward factorisation of every read into its longest matching suffix
// segments (include/gdx.h).  A segment is what Cursor::extend_query_front (cursor.rs:34-51) makes of the read's symbols
// from position e leftwards, starting from [0, n), until a step would empty the interval: the interval BEFORE that step
// and the number of steps taken.  The next segment starts in front of it, up to max_segments times, all in one launch.
// kGroup lanes per read and the table access of search_kernel / extend_front_kernel; control flow is uniform inside a
// group, its first lane writes.  Three routes, identical results:
//   LF steps    one per symbol: PairTable::lf1 (one 128-byte fetch) for symbols 1..4 on pair lines, else Table::rank2
//   top table   a segment that has top_depth symbols 1..4 to start with takes their interval from the top table; the
//               entry of an absent D-mer only says that the segment is shorter, which is then found step by step
//   text        (kText: the index holds text units, SA and ISA) once the interval is ONE row the rest of the segment
//               is read off the text in front of p = SA[row]: every lane compares eight symbols, a round covers
//               8 kGroup, and the row afterwards is ISA[p - matched].  Text symbols outside 1..4 (sentinels, N, the
//               pad in front of the text) never match; a READ symbol outside 1..4 hands the segment back to the LF
//               steps, which know what an N matches and report symbols that are not in the alphabet.
struct SegmentsOut {
    uint32_t *n_segments, *remaining, *length, *start, *end;
    uint8_t *status;
};

// The fetch chain of a read is dependent and latency-bound, so the kernel lives on reads in flight.  Waves per SIMD from
// the registers the compiler reports (-Rpass-analysis=kernel-resource-usage): pair lines + text route 83 VGPRs = 5 waves
// (asked for 6 it spills 20 bytes to scratch), the other text and one-lane instances 6 (61 .. 73 VGPRs), the rest 7
// (53 .. 71); no scratch in any instance.
template <class Table, int kGroup, bool kPair, bool kText>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu((kText && kPair) ? 5 : ((kText || kGroup == 1) ? 6 : 7)))) void suffix_segments_kernel(
    IndexView ix, const uint8_t *__restrict__ qbuf, const uint64_t *__restrict__ qoff, uint64_t nq, uint32_t max_segments,
    SegmentsOut out)
{
    __shared__ uint8_t s_dense[256];
    __shared__ uint32_t s_count[257];
    for (int i = threadIdx.x; i < 256; i += kBlock) s_dense[i] = ix.io_to_dense[i];
    for (int i = threadIdx.x; i <= ix.sigma; i += kBlock) s_count[i] = ix.count[i];
    __syncthreads();

    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * (kBlock / kGroup);
    const bool writer = (threadIdx.x % kGroup) == 0;
    const uint32_t sub = threadIdx.x % kGroup;
    const uint32_t depth = (ix.top != nullptr && ix.layout == 0) ? ix.top_depth : 0u;
    for (uint64_t q = static_cast<uint64_t>(blockIdx.x) * (kBlock / kGroup) + threadIdx.x / kGroup; q < nq; q += stride) {
        const uint64_t begin = qoff[q];
        const uint32_t m = static_cast<uint32_t>(qoff[q + 1] - begin);
        const uint64_t slot0 = q * max_segments;
        uint32_t e = m, n_seg = 0, status = GDX_Q_OK;
        while (e > 0u && n_seg < max_segments) {
            uint32_t lo = 0, hi = ix.n, len = 0;
            if (depth != 0u && e >= depth) {  // the segment's first `depth` symbols as top_lookup takes them
                uint32_t a = 0, b = 0;
                for (uint32_t s = 0; s < depth; s++) {
                    const uint32_t c = s_dense[qbuf[begin + e - 1u - s]];
                    if (s < 8u) a |= c << (4u * (7u - s));
                    else b |= c << (4u * (15u - s));
                }
                uint32_t tlo, thi;
                if (top_lookup(ix, a, b, tlo, thi) && tlo != thi) {
                    lo = tlo;
                    hi = thi;
                    len = depth;
                }
            }
            QueryWindow win;
            win.init(qbuf, begin, begin + (e - len));
            bool text_open = kText;  // false between a read symbol outside 1..4 and the LF step that takes it
            while (len < e) {
                if (kText && text_open && len != 0u && hi - lo == 1u) {
                    uint32_t p = ix.sa_full[lo];  // the suffix at p starts with the segment so far
                    bool blocked = false;
                    while (len < e) {
                        const uint32_t rem = e - len;
                        const uint64_t at = begin + rem;  // read symbol j of the round sits at at - 1 - j, text symbol at p - 1 - j
                        // (a round begins with p >= 0 and looks at most 8 kGroup <= 32 symbols back: inside the pad units)
                        const uint64_t t_hi = static_cast<uint64_t>(p) + 32u * kTextPadUnits - 1u - 8u * sub, t_lo = t_hi - 7u;
                        const u32x4 u_hi = ix.text_units[t_hi >> 5];
                        const u32x4 u_lo = (t_lo >> 5) != (t_hi >> 5) ? ix.text_units[t_lo >> 5] : u_hi;
                        uint32_t mine = 0, dirty = 0;
                        for (uint32_t k = 0; k < 8u; k++) {
                            const uint32_t j = 8u * sub + k;
                            if (j >= rem) break;
                            const uint32_t c = s_dense[qbuf[at - 1u - j]];
                            if (c - 1u >= 4u) {
                                dirty = 1u;
                                break;
                            }
                            const uint64_t t = t_hi - k;
                            const u32x4 u = (t >> 5) == (t_hi >> 5) ? u_hi : u_lo;
                            const uint32_t i = static_cast<uint32_t>(t & 31u);
                            const uint32_t code = ((i < 16u ? u.x >> (2u * i) : u.y >> (2u * (i - 16u)))) & 3u;
                            if (((u.z >> i) & 1u) != 0u || code != c - 1u) break;
                            mine++;
                        }
                        const uint32_t v = mine | (dirty << 8);
                        uint32_t total = 0, stop = 0, stop_dirty = 0;
#pragma unroll
                        for (int l = 0; l < kGroup; l++) {
                            const uint32_t vl = kGroup == 1 ? v : static_cast<uint32_t>(__shfl(static_cast<int>(v), l, kGroup));
                            if (stop == 0u) {
                                total += vl & 0xffu;
                                if ((vl & 0xffu) < 8u) {
                                    stop = 1u;
                                    stop_dirty = vl >> 8;
                                }
                            }
                        }
                        p -= total;
                        len += total;
                        if (stop != 0u) {
                            blocked = stop_dirty == 0u;  // a mismatch, a sentinel, the text's or the read's first symbol
                            break;
                        }
                    }
                    lo = ix.isa[p];
                    hi = lo + 1u;
                    if (blocked || len == e) break;
                    text_open = false;
                    win.init(qbuf, begin, begin + (e - len));
                    continue;
                }
                const uint32_t c = s_dense[win.get(begin + (e - len) - 1u)];
                if (c == 0u) {  // alphabet.rs:195-198: cursor.rs:34-38 translates before anything else
                    status = GDX_Q_INVALID_SYMBOL;
                    break;
                }
                if (lo == hi) break;  // (an index without rows: nothing occurs)
                uint32_t nlo, nhi;
                if (kPair && c <= 4u) {
                    PairTable::lf1<0, kGroup>(ix, c, lo, hi, nlo, nhi);
                } else {
                    Table::rank2(ix, c, lo, hi, nlo, nhi);
                    const uint32_t cc = s_count[c];
                    nlo += cc;
                    nhi += cc;
                }
                if (nlo == nhi) break;  // the stop rule: the interval from before the step that emptied it
                lo = nlo;
                hi = nhi;
                len++;
                text_open = kText;
            }
            if (status != GDX_Q_OK) break;
            if (writer) {
                out.length[slot0 + n_seg] = len;
                out.start[slot0 + n_seg] = len != 0u ? lo : 0u;
                out.end[slot0 + n_seg] = len != 0u ? hi : 0u;
            }
            e -= len != 0u ? len : 1u;
            n_seg++;
        }
        if (status != GDX_Q_OK) {
            n_seg = 0;
            e = m;
        }
        if (writer) {
            for (uint32_t j = n_seg; j < max_segments; j++) {
                out.length[slot0 + j] = 0u;
                out.start[slot0 + j] = 0u;
                out.end[slot0 + j] = 0u;
            }
            out.n_segments[q] = n_seg;
            out.remaining[q] = e;
            if (out.status != nullptr) out.status[q] = static_cast<uint8_t>(status);
        }
    }
}

// gdx_smems_many[_dev]: the super-maximal exact matches of every read (include/gdx.h has the definition), found by a walk
// that alternates between two one-directional indexes: fx over the texts, rx over the same texts each reversed.  From
// position p a FORWARD pass on rx consumes q[p], q[p + 1], ... (extending in front of the reversed match) and gives the
// longest e with q[p, e) occurring; a BACKWARD pass on fx from e, the pass of suffix_segments_kernel, gives the longest
// match [s, e) that ends there and its interval in fx; [s, e) is an SMEM and the walk goes on at p = s - 1.  All in one
// launch; kGroup lanes per read, control flow uniform inside a group, its first lane writes.  Both passes step as the
// segments kernel does (PairTable::lf1 for symbols 1..4 on pair lines -- kPair: BOTH views hold them -- else Table::rank2
// plus count) and enter through their own index's top table when the pass has top_depth symbols 1..4 ahead of it; the
// entry of an absent D-mer only says that the pass is shorter, which is then found step by step.  io_to_dense and count
// are the same in both indexes (the host checks it), so the block keeps one copy.
struct SmemsOut {
    uint32_t *n_smems, *remaining, *begin, *length, *start, *end;
    uint8_t *status;
};

// The query's symbols left to right through aligned 8-byte windows, the next one requested a window ahead: QueryWindow
// for the forward pass.  Bytes [pos, end) with pos < end; get() must walk upwards from pos.
struct ForwardQueryWindow {
    const uint64_t *words;
    uint64_t cur, next, cur_word, last_word;

    __device__ __forceinline__ void init(const uint8_t *qbuf, uint64_t pos, uint64_t end)
    {
        words = reinterpret_cast<const uint64_t *>(qbuf);
        last_word = (end - 1) >> 3;
        cur_word = pos >> 3;
        cur = words[cur_word];
        next = cur_word < last_word ? words[cur_word + 1] : 0ull;
    }
    __device__ __forceinline__ uint32_t get(uint64_t at)
    {
        const uint64_t w = at >> 3;
        if (w != cur_word) {
            cur_word = w;
            cur = next;
            next = w < last_word ? words[w + 1] : 0ull;
        }
        return static_cast<uint32_t>(cur >> ((at & 7u) * 8u)) & 0xffu;
    }
};

// one cursor step of either pass with dense symbol c >= 1
template <class Table, int kGroup, bool kPair>
__device__ __forceinline__ void smems_step(const IndexView &ix, const uint32_t *s_count, uint32_t c, uint32_t lo, uint32_t hi,
                                           uint32_t &nlo, uint32_t &nhi)
{
    if (kPair && c <= 4u) {
        PairTable::lf1<0, kGroup>(ix, c, lo, hi, nlo, nhi);
    } else {
        Table::rank2(ix, c, lo, hi, nlo, nhi);
        const uint32_t cc = s_count[c];
        nlo += cc;
        nhi += cc;
    }
}

// The top-table entry of a pass: its first `depth` symbols sit at first[0], first[dir], first[2 dir], ... (first consumed
// symbol in the highest bits, as top_lookup takes them).  False, lo / hi untouched: a symbol outside 1..4 or a D-mer that
// does not occur -- the pass then runs step by step from its start.
__device__ __forceinline__ bool smems_top(const IndexView &ix, uint32_t depth, const uint8_t *s_dense, const uint8_t *first, int dir,
                                          uint32_t &lo, uint32_t &hi)
{
    uint32_t a = 0, b = 0;
    for (uint32_t s = 0; s < depth; s++) {
        const uint32_t c = s_dense[first[static_cast<int64_t>(dir) * static_cast<int64_t>(s)]];
        if (s < 8u) a |= c << (4u * (7u - s));
        else b |= c << (4u * (15u - s));
    }
    uint32_t tlo, thi;
    if (!top_lookup(ix, a, b, tlo, thi) || tlo == thi) return false;
    lo = tlo;
    hi = thi;
    return true;
}

// Like the segments kernel this one lives on reads in flight (a dependent, latency-bound fetch chain per read).  Waves per
// SIMD from the registers the compiler reports (-Rpass-analysis=kernel-resource-usage, gfx950): pair lines 77 VGPRs and
// one lane per read on rank lines 75 VGPRs = 6 waves; four lanes on rank lines 57 and the generic table 61: 7 asked for,
// 8 reported; no scratch in any instance (profiles/r09/smems.md).
template <class Table, int kGroup, bool kPair>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu((kPair || std::is_same<Table, LineTable>::value) ? 6 : 7))) void smems_kernel(
    IndexView fx, IndexView rx, const uint8_t *__restrict__ qbuf, const uint64_t *__restrict__ qoff, uint64_t nq,
    uint32_t max_smems, uint32_t min_length, SmemsOut out)
{
    __shared__ uint8_t s_dense[256];
    __shared__ uint32_t s_count[257];
    for (int i = threadIdx.x; i < 256; i += kBlock) s_dense[i] = fx.io_to_dense[i];
    for (int i = threadIdx.x; i <= fx.sigma; i += kBlock) s_count[i] = fx.count[i];
    __syncthreads();

    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * (kBlock / kGroup);
    const bool writer = (threadIdx.x % kGroup) == 0;
    const uint32_t fdepth = (fx.top != nullptr && fx.layout == 0) ? fx.top_depth : 0u;
    const uint32_t rdepth = (rx.top != nullptr && rx.layout == 0) ? rx.top_depth : 0u;
    for (uint64_t q = static_cast<uint64_t>(blockIdx.x) * (kBlock / kGroup) + threadIdx.x / kGroup; q < nq; q += stride) {
        const uint64_t begin = qoff[q];
        const uint32_t m = static_cast<uint32_t>(qoff[q + 1] - begin);
        const uint64_t slot0 = q * max_smems;
        uint32_t pe = m, n_smems = 0, status = GDX_Q_OK;  // pe = p + 1: the walk stands at p, 0 = it is through
        while (pe > 0u && n_smems < max_smems) {
            const uint32_t p = pe - 1u;
            // forward pass on rx: the longest e with q[p, e) occurring
            uint32_t lo = 0, hi = rx.n, e = p;
            if (rdepth != 0u && m - p >= rdepth && smems_top(rx, rdepth, s_dense, qbuf + begin + p, 1, lo, hi)) e = p + rdepth;
            if (e < m) {
                ForwardQueryWindow win;
                win.init(qbuf, begin + e, begin + m);
                while (e < m) {
                    const uint32_t c = s_dense[win.get(begin + e)];
                    if (c == 0u) {  // also as the symbol that blocks: translation comes before anything else
                        status = GDX_Q_INVALID_SYMBOL;
                        break;
                    }
                    if (lo == hi) break;  // (an index without rows: nothing occurs)
                    uint32_t nlo, nhi;
                    smems_step<Table, kGroup, kPair>(rx, s_count, c, lo, hi, nlo, nhi);
                    if (nlo == nhi) break;
                    lo = nlo;
                    hi = nhi;
                    e++;
                }
            }
            if (status != GDX_Q_OK) break;
            if (e == p) {  // q[p] occurs nowhere: no SMEM covers p
                pe = p;
                continue;
            }
            // backward pass on fx: the longest match that ends at e, with the interval from before the step that emptied it
            uint32_t len = 0;
            lo = 0;
            hi = fx.n;
            if (fdepth != 0u && e >= fdepth && smems_top(fx, fdepth, s_dense, qbuf + begin + e - 1u, -1, lo, hi)) len = fdepth;
            QueryWindow win;
            win.init(qbuf, begin, begin + (e - len));
            while (len < e) {
                const uint32_t c = s_dense[win.get(begin + (e - len) - 1u)];
                if (c == 0u) {
                    status = GDX_Q_INVALID_SYMBOL;
                    break;
                }
                if (lo == hi) break;
                uint32_t nlo, nhi;
                smems_step<Table, kGroup, kPair>(fx, s_count, c, lo, hi, nlo, nhi);
                if (nlo == nhi) break;
                lo = nlo;
                hi = nhi;
                len++;
            }
            if (status != GDX_Q_OK) break;
            const uint32_t s = e - len;
            if (len >= min_length) {
                if (writer) {
                    out.begin[slot0 + n_smems] = s;
                    out.length[slot0 + n_smems] = len;
                    out.start[slot0 + n_smems] = lo;
                    out.end[slot0 + n_smems] = hi;
                }
                n_smems++;
            }
            // s <= p when rx indexes the reversed texts of fx; with a companion built from other texts (the host cannot
            // tell) the walk must still move left
            pe = s < p ? s : p;
        }
        if (status != GDX_Q_OK) {
            n_smems = 0;
            pe = m;
        }
        if (writer) {
            for (uint32_t j = n_smems; j < max_smems; j++) {
                out.begin[slot0 + j] = 0u;
                out.length[slot0 + j] = 0u;
                out.start[slot0 + j] = 0u;
                out.end[slot0 + j] = 0u;
            }
            out.n_smems[q] = n_smems;
            out.remaining[q] = pe;
            if (out.status != nullptr) out.status[q] = static_cast<uint8_t>(status);
        }
    }
}

template <class Table>
__global__ __launch_bounds__(kBlock) void rank_many_kernel(IndexView ix, const uint8_t *__restrict__ symbols,
                                                           const uint32_t *__restrict__ idx, uint64_t m,
                                                           uint32_t *__restrict__ out, uint32_t *error)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < m; i += stride) {
        const uint32_t c = symbols[i], p = idx[i];
        if (c >= static_cast<uint32_t>(ix.sigma) || p > ix.n) {  // mod.rs:107-108
            *error = 1;
            out[i] = 0;
            continue;
        }
        out[i] = Table::rank(ix, c, p);
    }
}

template <class Table>
__global__ __launch_bounds__(kBlock) void symbol_at_kernel(IndexView ix, const uint32_t *__restrict__ idx,
                                                           uint64_t m, uint8_t *__restrict__ out, uint32_t *error)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < m; i += stride) {
        const uint32_t p = idx[i];
        if (p >= ix.n) {  // condensed.rs:344
            *error = 1;
            out[i] = 0;
            continue;
        }
        out[i] = static_cast<uint8_t>(Table::symbol_at(ix, p));
    }
}

// gdx_bench_lf_walk_dev: the text read backwards through the occurrence table alone (symbol_at + rank + count, i.e.
// sampled_suffix_array.rs:118-131 without the samples)
template <class Table>
__global__ __launch_bounds__(kBlock) void lf_walk_kernel(IndexView ix, const uint32_t *__restrict__ rows, uint64_t m,
                                                         uint32_t steps, uint8_t *__restrict__ symbols,
                                                         uint32_t *__restrict__ end_rows)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < m; i += stride) {
        uint32_t row = rows[i];
        uint8_t *out = symbols + i * steps;
        uint32_t j = 0;
        for (; j < steps && row < ix.n; j++) {
            uint32_t r;
            const uint32_t c = Table::symbol_and_rank(ix, row, r);
            out[j] = static_cast<uint8_t>(c);
            if (c == 0) {
                j++;
                break;
            }
            row = ix.count[c] + r;
        }
        for (; j < steps; j++) out[j] = 0xffu;
        if (end_rows) end_rows[i] = row;
    }
}

// lookup_table.rs:163-258: table[depth][idx] = interval of the depth-mer whose j-th symbol is digit j
// of idx in base k (+1 to skip the sentinel).  Plain backward search with freeze-on-empty gives the
// same (start, end) as the reference's recursive fill through the smaller tables.
template <class Table>
__global__ __launch_bounds__(kBlock) void fill_lookup_kernel(IndexView ix, uint2 *__restrict__ lookup, int depth,
                                                             uint64_t entries)
{
    const uint32_t k = static_cast<uint32_t>(ix.n_searchable);
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    const uint64_t first = lookup_offset(k, static_cast<uint32_t>(depth));
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; e < entries; e += stride) {
        uint64_t pw = 1;
        for (int j = 1; j < depth; j++) pw *= k;  // k^(depth-1)
        uint32_t lo = 0, hi = ix.n;
        for (int j = depth - 1; j >= 0 && lo != hi; j--) {
            const uint32_t c = static_cast<uint32_t>((e / pw) % k) + 1u;
            uint32_t rlo, rhi;
            Table::rank2(ix, c, lo, hi, rlo, rhi);
            const uint32_t cc = ix.count[c];
            lo = cc + rlo;
            hi = cc + rhi;
            pw /= k;
        }
        lookup[first + e] = make_uint2(lo, hi);
    }
}

// top[idx]: idx holds the 2-bit codes (dense - 1) of the D symbols in consumption order, first consumed symbol in
// the highest bit pair (top_lookup builds the same index from the query's nibble codes).  Plain backward search
// with freeze-on-empty, exactly fill_lookup_kernel's.
__global__ __launch_bounds__(kBlock) void fill_top_kernel(IndexView ix, uint2 *__restrict__ top, uint32_t depth,
                                                          uint64_t entries)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; e < entries; e += stride) {
        uint32_t lo = 0, hi = ix.n;
        for (uint32_t s = 0; s < depth && lo != hi; s++) {
            const uint32_t c = (static_cast<uint32_t>(e >> (2u * (depth - 1u - s))) & 3u) + 1u;
            uint32_t rlo, rhi;
            LineTable::rank2(ix, c, lo, hi, rlo, rhi);
            const uint32_t cc = ix.count[c];
            lo = cc + rlo;
            hi = cc + rhi;
        }
        top[e] = make_uint2(lo, hi);  // an empty interval stays as it was when it emptied (the loop stopped there)
    }
}

}  // namespace

// ASCII -> 2-bit: packed byte b holds the codes of bytes 4 b .. 4 b + 3 of the query buffer; *bad_symbols counts the
// symbols that are not one of the dense codes 1..4 (their code is written as 0), bad_flags (optional, one byte per
// 64 symbols) marks where they are so that the caller can find the queries they belong to
__global__ __launch_bounds__(kBlock) void pack_queries_kernel(const uint8_t *__restrict__ io_to_dense,
                                                              const uint8_t *__restrict__ qbuf, uint64_t n_symbols,
                                                              uint8_t *__restrict__ packed, uint8_t *__restrict__ bad_flags,
                                                              unsigned long long *__restrict__ bad_symbols)
{
    __shared__ uint8_t s_dense[256];
    for (int i = threadIdx.x; i < 256; i += kBlock) s_dense[i] = io_to_dense[i];
    __syncthreads();
    const uint64_t n_bytes = (n_symbols + 3) / 4;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    uint32_t bad = 0;
    for (uint64_t b = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; b < n_bytes; b += stride) {
        uint32_t out = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint64_t j = 4 * b + k;
            if (j < n_symbols) {
                const uint32_t d = s_dense[qbuf[j]];
                if (d - 1u < 4u) {
                    out |= (d - 1u) << (2u * k);
                } else {
                    bad++;
                    if (bad_flags) bad_flags[j >> 6] = 1;
                }
            }
        }
        packed[b] = static_cast<uint8_t>(out);
    }
    if (bad && bad_symbols) atomicAdd(bad_symbols, static_cast<unsigned long long>(bad));
}

void launch_pack_queries(const IndexView &ix, const uint8_t *d_qbuf, uint64_t n_symbols, uint8_t *d_packed,
                         uint8_t *d_bad_flags, unsigned long long *d_bad_symbols, hipStream_t stream)
{
    if (n_symbols == 0) return;
    hipLaunchKernelGGL(pack_queries_kernel, dim3(grid_for_items((n_symbols + 3) / 4)), dim3(kBlock), 0, stream,
                       ix.io_to_dense, d_qbuf, n_symbols, d_packed, d_bad_flags, d_bad_symbols);
}

void launch_extend_front(const IndexView &ix, uint32_t *d_start, uint32_t *d_end, const uint8_t *d_io_symbols,
                         uint64_t m, uint8_t *d_out_status, hipStream_t stream)
{
    if (m == 0) return;
    if (ix.layout == 0 && ix.pair_lines != nullptr) {
        hipLaunchKernelGGL((extend_front_kernel<QuadLineTable, 8, true>), dim3(grid_for_items(m * 8)), dim3(kBlock), 0,
                           stream, ix, d_start, d_end, d_io_symbols, m, d_out_status);
    } else if (ix.layout == 0) {
        hipLaunchKernelGGL((extend_front_kernel<QuadLineTable, 4, false>), dim3(grid_for_items(m * 4)), dim3(kBlock), 0,
                           stream, ix, d_start, d_end, d_io_symbols, m, d_out_status);
    } else {
        hipLaunchKernelGGL((extend_front_kernel<GenericTable, 1, false>), dim3(grid_for_items(m)), dim3(kBlock), 0,
                           stream, ix, d_start, d_end, d_io_symbols, m, d_out_status);
    }
}

void launch_suffix_segments(const IndexView &ix, const uint8_t *d_qbuf, const uint64_t *d_qoff, uint64_t nq,
                            uint32_t max_segments, bool lf_only, uint32_t *d_n_segments, uint32_t *d_remaining,
                            uint32_t *d_length, uint32_t *d_start, uint32_t *d_end, uint8_t *d_status, hipStream_t stream,
                            const QueryOptions &qo)
{
    if (nq == 0) return;
    const int variant = qo.search_variant >= 0 ? qo.search_variant : search_variant();
    const bool text = !lf_only && ix.text_units != nullptr && ix.sa_full != nullptr && ix.isa != nullptr;
    const SegmentsOut out = {d_n_segments, d_remaining, d_length, d_start, d_end, d_status};
#define GDX_SEGMENTS_LAUNCH(TABLE, GROUP, PAIR)                                                                          \
    do {                                                                                                                 \
        if (text)                                                                                                        \
            hipLaunchKernelGGL((suffix_segments_kernel<TABLE, GROUP, PAIR, true>), dim3(grid_for_items(nq * GROUP)),     \
                               dim3(kBlock), 0, stream, ix, d_qbuf, d_qoff, nq, max_segments, out);                      \
        else                                                                                                             \
            hipLaunchKernelGGL((suffix_segments_kernel<TABLE, GROUP, PAIR, false>), dim3(grid_for_items(nq * GROUP)),    \
                               dim3(kBlock), 0, stream, ix, d_qbuf, d_qoff, nq, max_segments, out);                      \
    } while (0)
    if (ix.layout == 0 && variant == 2 && ix.pair_lines != nullptr) GDX_SEGMENTS_LAUNCH(QuadLineTable, 4, true);
    else if (ix.layout == 0 && variant != 1) GDX_SEGMENTS_LAUNCH(QuadLineTable, 4, false);
    else if (ix.layout == 0) GDX_SEGMENTS_LAUNCH(LineTable, 1, false);
    else GDX_SEGMENTS_LAUNCH(GenericTable, 1, false);
#undef GDX_SEGMENTS_LAUNCH
}

void launch_smems(const IndexView &fx, const IndexView &rx, const uint8_t *d_qbuf, const uint64_t *d_qoff, uint64_t nq,
                  uint32_t max_smems, uint32_t min_length, uint32_t *d_n_smems, uint32_t *d_remaining, uint32_t *d_begin,
                  uint32_t *d_length, uint32_t *d_start, uint32_t *d_end, uint8_t *d_status, hipStream_t stream,
                  const QueryOptions &qo)
{
    if (nq == 0) return;
    const int variant = qo.search_variant >= 0 ? qo.search_variant : search_variant();
    const SmemsOut out = {d_n_smems, d_remaining, d_begin, d_length, d_start, d_end, d_status};
#define GDX_SMEMS_LAUNCH(TABLE, GROUP, PAIR)                                                                                  \
    hipLaunchKernelGGL((smems_kernel<TABLE, GROUP, PAIR>), dim3(grid_for_items(nq * GROUP)), dim3(kBlock), 0, stream, fx, rx, \
                       d_qbuf, d_qoff, nq, max_smems, min_length, out)
    // (the callers have checked that both views have the same table layout)
    if (fx.layout == 0 && variant == 2 && fx.pair_lines != nullptr && rx.pair_lines != nullptr) GDX_SMEMS_LAUNCH(QuadLineTable, 4, true);
    else if (fx.layout == 0 && variant != 1) GDX_SMEMS_LAUNCH(QuadLineTable, 4, false);
    else if (fx.layout == 0) GDX_SMEMS_LAUNCH(LineTable, 1, false);
    else GDX_SMEMS_LAUNCH(GenericTable, 1, false);
#undef GDX_SMEMS_LAUNCH
}

void launch_rank_many(const IndexView &ix, const uint8_t *d_symbols, const uint32_t *d_idx, uint64_t m,
                      uint32_t *d_out, uint32_t *d_error, hipStream_t stream)
{
    if (m == 0) return;
    GDX_DISPATCH_TABLE(ix, rank_many_kernel, grid_for_items(m), stream, ix, d_symbols, d_idx, m, d_out, d_error);
}

void launch_symbol_at_many(const IndexView &ix, const uint32_t *d_idx, uint64_t m, uint8_t *d_out,
                           uint32_t *d_error, hipStream_t stream)
{
    if (m == 0) return;
    GDX_DISPATCH_TABLE(ix, symbol_at_kernel, grid_for_items(m), stream, ix, d_idx, m, d_out, d_error);
}

void launch_lf_walk(const IndexView &ix, const uint32_t *d_rows, uint64_t m, uint32_t steps, uint8_t *d_symbols,
                    uint32_t *d_end_rows, hipStream_t stream)
{
    if (m == 0 || steps == 0) return;
    GDX_DISPATCH_TABLE(ix, lf_walk_kernel, grid_for_items(m), stream, ix, d_rows, m, steps, d_symbols, d_end_rows);
}

void launch_fill_lookup(const IndexView &ix, uint2 *d_lookup, int depth, hipStream_t stream)
{
    uint64_t entries = 1;
    for (int j = 0; j < depth; j++) entries *= static_cast<uint64_t>(ix.n_searchable);
    GDX_DISPATCH_TABLE(ix, fill_lookup_kernel, grid_for_items(entries), stream, ix, d_lookup, depth, entries);
}

// sum of the interval widths of the top-table entries wider than `rows` rows = the number of text positions whose
// D-mer stays wider than a jump can take after the top table (a measure of how repetitive the text is)
__global__ __launch_bounds__(kBlock) void top_wide_kernel(const uint2 *__restrict__ top, uint64_t entries, uint32_t rows,
                                                          unsigned long long *__restrict__ sum)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    unsigned long long mine = 0;
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; e < entries; e += stride) {
        const uint2 v = top[e];
        const uint32_t w = v.y - v.x;
        if (w > rows) mine += w;
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(sum, mine);
}

void launch_top_wide(const uint2 *d_top, uint32_t depth, uint32_t rows, unsigned long long *d_sum, hipStream_t stream)
{
    const uint64_t entries = 1ull << (2u * depth);
    hipLaunchKernelGGL(top_wide_kernel, dim3(grid_for_items(entries)), dim3(kBlock), 0, stream, d_top, entries, rows, d_sum);
}

void launch_fill_top(const IndexView &ix, uint2 *d_top, uint32_t depth, hipStream_t stream)
{
    const uint64_t entries = 1ull << (2u * depth);
    hipLaunchKernelGGL(fill_top_kernel, dim3(grid_for_items(entries)), dim3(kBlock), 0, stream, ix, d_top, depth,
                       entries);
}

}  // namespace gdx
