// soft_clip.hip -- scored soft clipping of traced alignments: per candidate of gdx_align_many[_dev] the best-scoring contiguous
// part of its run-length CIGAR under a match / mismatch / gap-open / gap-extend scoring, what lies outside replaced by S runs,
// begin and end moved inwards, the edit count and the score (gdx_soft_clip_many[_dev]; the definition is in
// include/gdx_experimental.h "soft clipping").  A pure post-pass over the five outputs of the traceback: it never looks at the
// queries or at the index's arrays.  The constants and the instance dispatch are select.hpp's.
//
//   soft_clip_kernel<P, kLong>  P = the next power of two >= min(stride, 64), stride = 2 max_edits + 1: a candidate is P adjacent
//                        lanes, lane r holds run r, a wavefront holds 64 / P candidates of consecutive numbers, so the words a
//                        wavefront loads from `cigar` are contiguous runs of rows, not 64 rows a stride apart.  kLong (stride >
//                        64, P = 64): one candidate per wavefront, its row walked in chunks of 64 runs with a carry; the number
//                        of chunks is uniform in the wavefront.  Blocks of four wavefronts, grid-stride over tiles of 64 / P
//                        candidates with a bound that is uniform in the wavefront: every lane shuffles.
//   A. check and score   per chunk, over the words below n_cigar only: the sum of all run lengths and of the text run lengths
//                        (each length capped at GDX_CLIP_MAX_RUN_SUM + 1 and a run that is bad in itself counted as that, so
//                        neither sum wraps and a bad run fails the sum rule); an inclusive prefix sum S of the run values; a
//                        prefix minimum of (S before run i, i), which is for every j the best i; the maximum of the key
//                        (S_j - that minimum, -i, j).  Carries: the sum so far, the minimum so far, the best key so far.
//   B. sums              with the interval [i, j] known: text and read symbols before i and after j, edits inside: two
//                        butterflies of packed 20-bit fields (every field is at most GDX_CLIP_MAX_RUN_SUM once the row passed).
//   C. output            each lane of [i, j] stores its own run, shifted by the left S; lane 0 of the group stores the S words,
//                        the seven per-candidate words and the status.  Words from out_n_cigar on are not written.
// A short row (stride <= 64) is loaded once and stays in a register through A, B and C; a long one is loaded once per phase
// (513 words at the most, from the cache).  No LDS, no atomics, one launch.  Candidate numbers are 64 bits wide throughout.
// Sums of a row that fails the check may wrap (unsigned arithmetic): nothing of them is stored.
// Measured (profiles/r26/soft_clip.md): 3.0 ms for 10 M reads at max_edits 11 (P = 32), 7.0 ms at 24 (P = 64), a tenth and a
// fifth of the traceback over the same winners but 19 and 45 times a copy of the bytes: the ladders of shuffles over mostly
// idle lanes (rows have four or five runs) are what the time goes into, not the loads and stores.
#include <atomic>

#include "fm_index.hpp"
#include "select.hpp"

namespace gdx {

namespace {

using namespace select;

std::atomic<uint32_t> g_clip_grid{0};  // gdx_debug_set_clip_grid: 0 = the launcher's choice

constexpr uint32_t kRunCap = GDX_CLIP_MAX_RUN_SUM + 1u;  // what a run length counts as at the most
constexpr long long kNoMin = 0x7fffffffffffffffll;       // prefix minimum of a lane without a run, carry before the first
constexpr long long kNoKey = -0x7fffffffffffffffll - 1;  // key of a lane without a run

// the sum of v over the group of P lanes, in every lane
template <int P, class T>
__device__ __forceinline__ T butterfly_sum(T v)
{
#pragma unroll
    for (int o = P / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, P);
    return v;
}

template <int P>
__device__ __forceinline__ long long butterfly_max(long long v)
{
#pragma unroll
    for (int o = P / 2; o > 0; o >>= 1) {
        const long long w = __shfl_xor(v, o, P);
        v = w > v ? w : v;
    }
    return v;
}

__device__ __forceinline__ bool is_text_op(uint32_t op) { return op == GDX_CIGAR_EQ || op == GDX_CIGAR_DIFF || op == GDX_CIGAR_DEL; }
__device__ __forceinline__ bool is_read_op(uint32_t op) { return op == GDX_CIGAR_EQ || op == GDX_CIGAR_DIFF || op == GDX_CIGAR_INS; }

template <int P, bool kLong>
__global__ __launch_bounds__(kBlock) void soft_clip_kernel(const ClipArgs a)
{
    constexpr uint32_t kGroups = kWave / P;  // candidates of a wavefront
    const uint32_t lane = threadIdx.x & (kWave - 1), j = lane & (P - 1);
    const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave;
    const uint64_t step = static_cast<uint64_t>(gridDim.x) * (kBlock / kWave) * kGroups;
    const uint32_t k = a.max_edits, stride = 2u * k + 1u;

    for (uint64_t g0 = wave * kGroups; g0 < a.m; g0 += step) {  // (uniform in the wavefront: every lane shuffles)
        const uint64_t g = g0 + lane / P;
        const bool in_range = g < a.m;
        uint32_t d = 0, b = 0, e = GDX_EDIT_NO_END, n = 0;
        if (in_range) {
            d = a.dist[g];
            b = a.begin[g];
            e = a.end[g];
            n = a.n_cigar[g];
        }
        const bool pass = e == GDX_EDIT_NO_END;  // 1. (and the lanes of a group beyond the batch)
        bool bad = !pass && (n > stride || b > e);
        uint32_t nn = pass || bad ? 0u : n;  // the runs that are looked at: never a word at or beyond n_cigar or the stride
        if (kLong) nn = __builtin_amdgcn_readfirstlane(nn);  // (one candidate per wavefront)
        const uint32_t chunks = kLong ? (nn + P - 1) / P : 1u;
        const uint32_t *row = a.cigar + g * stride;
        uint32_t *out_row = a.out_cigar + g * stride;

        // A. check and score
        uint32_t w0 = 0;  // the word of a short row
        uint32_t carry_sum = 0;
        unsigned long long lens = 0;  // all run lengths | text run lengths << 32
        long long carry_min = kNoMin, best_key = kNoKey;
        for (uint32_t c = 0; c < chunks; c++) {
            const uint32_t r = c * P + j;
            const bool has = r < nn;
            const uint32_t w = has ? row[r] : 0u;
            if (!kLong) w0 = w;
            const uint32_t op = w & 15u, len = w >> 4;
            const bool known = op == GDX_CIGAR_INS || op == GDX_CIGAR_DEL || op == GDX_CIGAR_EQ || op == GDX_CIGAR_DIFF;
            const uint32_t lc = !has ? 0u : (!known || len == 0u || len > kRunCap) ? kRunCap : len;
            lens += butterfly_sum<P>(static_cast<unsigned long long>(lc) |
                                     (static_cast<unsigned long long>(is_text_op(op) ? lc : 0u) << 32));
            // 3. the value of the run, as a wrapping 32-bit number
            const uint32_t v = op == GDX_CIGAR_EQ ? a.match * lc : op == GDX_CIGAR_DIFF ? 0u - a.mismatch * lc
                                                                                        : 0u - (has ? a.gap_open + a.gap_extend * lc : 0u);
            uint32_t s = v;
#pragma unroll
            for (int o = 1; o < P; o <<= 1) {
                const uint32_t t = __shfl_up(s, o, P);
                if (j >= static_cast<uint32_t>(o)) s += t;
            }
            s += carry_sum;
            const int32_t before = static_cast<int32_t>(s - v);  // S before this run
            long long mk = has ? static_cast<long long>(before) * 0x100000000ll + r : kNoMin;
#pragma unroll
            for (int o = 1; o < P; o <<= 1) {
                const long long t = __shfl_up(mk, o, P);
                if (j >= static_cast<uint32_t>(o) && t < mk) mk = t;
            }
            if (carry_min < mk) mk = carry_min;
            const int32_t score = static_cast<int32_t>(s) - static_cast<int32_t>(mk >> 32);
            const uint32_t from = static_cast<uint32_t>(mk) & 1023u;
            const long long key = has ? static_cast<long long>(score) * 0x100000ll + (((1023u - from) << 10) | r) : kNoKey;
            const long long chunk_key = butterfly_max<P>(key);
            if (chunk_key > best_key) best_key = chunk_key;
            if (kLong) {
                carry_sum = __shfl(s, P - 1, P);
                carry_min = __shfl(mk, P - 1, P);
            }
        }
        // 2. (a run that is bad in itself has pushed the first sum over the bound)
        bad = bad || (!pass && (static_cast<uint32_t>(lens) > GDX_CLIP_MAX_RUN_SUM || static_cast<uint32_t>(lens >> 32) != e - b));
        const int32_t best = nn != 0u ? static_cast<int32_t>(best_key >> 20) : 0;
        const uint32_t bi = 1023u - (static_cast<uint32_t>(best_key >> 10) & 1023u), bj = static_cast<uint32_t>(best_key) & 1023u;
        const uint32_t least = a.min_score > 1u ? a.min_score : 1u;
        const bool kept = !pass && !bad && nn != 0u && best >= static_cast<int32_t>(least);  // 4.

        // B. text and read symbols before i | after j, the edits inside: 20-bit fields
        unsigned long long outside = 0, inside = 0;
        for (uint32_t c = 0; c < chunks; c++) {
            const uint32_t r = c * P + j;
            const uint32_t w = kLong ? (r < nn ? row[r] : 0u) : w0;
            const uint32_t op = w & 15u;
            const unsigned long long len = w >> 4, tl = is_text_op(op) ? len : 0ull, rl = is_read_op(op) ? len : 0ull;
            outside += butterfly_sum<P>(r < bi ? tl | (rl << 20) : r > bj ? tl << 40 : 0ull);
            inside += butterfly_sum<P>(r > bj ? rl : (r >= bi && op != GDX_CIGAR_EQ) ? len << 20 : 0ull);
        }
        const uint32_t text_before = static_cast<uint32_t>(outside) & 0xfffffu, read_before = static_cast<uint32_t>(outside >> 20) & 0xfffffu;
        const uint32_t text_after = static_cast<uint32_t>(outside >> 40) & 0xfffffu;
        const uint32_t read_after = static_cast<uint32_t>(inside) & 0xfffffu, edits = static_cast<uint32_t>(inside >> 20) & 0xfffffu;

        // C. output
        const uint32_t has_left = read_before != 0u ? 1u : 0u, has_right = read_after != 0u ? 1u : 0u;
        if (kept) {
            for (uint32_t c = 0; c < chunks; c++) {
                const uint32_t r = c * P + j;
                if (r >= bi && r <= bj) out_row[r - bi + has_left] = kLong ? row[r] : w0;
            }
        }
        if (in_range && j == 0u) {
            const uint32_t n_kept = bj - bi + 1u;
            if (kept && has_left) out_row[0] = (read_before << 4) | GDX_CIGAR_SOFT_CLIP;
            if (kept && has_right) out_row[has_left + n_kept] = (read_after << 4) | GDX_CIGAR_SOFT_CLIP;
            a.out_score[g] = pass || bad ? static_cast<int32_t>(GDX_CLIP_NO_SCORE) : best;
            a.out_dist[g] = kept ? edits : pass ? d : k + 1u;
            a.out_begin[g] = kept ? b + text_before : GDX_EDIT_NO_END;
            a.out_end[g] = kept ? e - text_after : GDX_EDIT_NO_END;
            a.out_clip_left[g] = kept ? read_before : 0u;
            a.out_clip_right[g] = kept ? read_after : 0u;
            a.out_n_cigar[g] = kept ? has_left + n_kept + has_right : 0u;
            if (a.out_status != nullptr) a.out_status[g] = bad ? GDX_CLIP_BAD_CIGAR : 0;
        }
    }
}

}  // namespace

void check_soft_clip(const ClipArgs &a)
{
    if (a.max_edits > GDX_EDIT_MAX_QUERY_LEN) fail(GDX_ERR_INVALID_ARGUMENT, "max_edits must be at most %u", GDX_EDIT_MAX_QUERY_LEN);
    const uint32_t hi = GDX_CLIP_MAX_SCORE_PARAM;
    if (a.match == 0 || a.match > hi || a.mismatch == 0 || a.mismatch > hi || a.gap_extend == 0 || a.gap_extend > hi)
        fail(GDX_ERR_INVALID_ARGUMENT, "match, mismatch and gap_extend must be 1..%u", hi);
    if (a.gap_open > hi) fail(GDX_ERR_INVALID_ARGUMENT, "gap_open must be at most %u", hi);
    if (a.min_score > 0x40000000u) fail(GDX_ERR_INVALID_ARGUMENT, "min_score must not exceed 2^30");
    if (a.m != 0 && any_null({a.dist, a.begin, a.end, a.n_cigar, a.cigar, a.out_score, a.out_dist, a.out_begin, a.out_end, a.out_clip_left,
                  a.out_clip_right, a.out_n_cigar, a.out_cigar}))
        fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
}

void set_clip_grid(uint32_t grid) { g_clip_grid.store(grid); }

void launch_soft_clip(const ClipArgs &a, hipStream_t stream)
{
    if (a.m == 0) return;
    const uint32_t stride = 2u * a.max_edits + 1u, forced = g_clip_grid.load();
    constexpr uint32_t wave = kWave;
    dispatch_slots<kWave>(stride < wave ? stride : wave, [&](auto p) {  // (max_edits <= 256: checked by the caller)
        constexpr int P = decltype(p)::value;
        unsigned grid = grid_for(a.m, kBlock / P, kMaxGrid);  // (a block takes kBlock / P candidates in one stride)
        if (forced != 0 && forced < grid) grid = forced;
        if constexpr (P == kWave) {
            if (stride > wave) {
                hipLaunchKernelGGL((soft_clip_kernel<P, true>), dim3(grid), dim3(kBlock), 0, stream, a);
                return;
            }
        }
        hipLaunchKernelGGL((soft_clip_kernel<P, false>), dim3(grid), dim3(kBlock), 0, stream, a);
    });
}

int soft_clip_host(const FmIndex &f, const ClipArgs &h)
{
    check_soft_clip(h);
    if (h.m == 0) return GDX_OK;
    const uint64_t m = h.m, stride = 2ull * h.max_edits + 1ull;
    f.make_current();
    hipStream_t stream = hipStreamPerThread;
    DeviceBuffer<uint32_t> d_in(4 * m + m * stride), d_out(7 * m + m * stride);  // dist, begin, end, n_cigar, cigar | seven words, cigar
    DeviceBuffer<uint8_t> d_status(m);
    const uint32_t *columns[4] = {h.dist, h.begin, h.end, h.n_cigar};
    for (int x = 0; x < 4; x++)
        GDX_HIP(hipMemcpyAsync(d_in.get() + x * m, columns[x], m * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    GDX_HIP(hipMemcpyAsync(d_in.get() + 4 * m, h.cigar, m * stride * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    // (the words of a row from out_n_cigar on are not written: the caller's stay as they are)
    GDX_HIP(hipMemcpyAsync(d_out.get() + 7 * m, h.out_cigar, m * stride * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    ClipArgs a = h;
    uint32_t *i = d_in.get(), *o = d_out.get();
    a.dist = i, a.begin = i + m, a.end = i + 2 * m, a.n_cigar = i + 3 * m, a.cigar = i + 4 * m;
    a.out_score = reinterpret_cast<int32_t *>(o), a.out_dist = o + m, a.out_begin = o + 2 * m, a.out_end = o + 3 * m;
    a.out_clip_left = o + 4 * m, a.out_clip_right = o + 5 * m, a.out_n_cigar = o + 6 * m, a.out_cigar = o + 7 * m;
    a.out_status = d_status.get();
    launch_soft_clip(a, stream);
    GDX_HIP(hipGetLastError());
    uint32_t *outs[7] = {reinterpret_cast<uint32_t *>(h.out_score), h.out_dist, h.out_begin, h.out_end, h.out_clip_left, h.out_clip_right,
                         h.out_n_cigar};
    for (int x = 0; x < 7; x++) GDX_HIP(hipMemcpyAsync(outs[x], o + x * m, m * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipMemcpyAsync(h.out_cigar, o + 7 * m, m * stride * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (h.out_status) GDX_HIP(hipMemcpyAsync(h.out_status, d_status.get(), m, hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipStreamSynchronize(stream));
    return GDX_OK;
}

}  // namespace gdx
