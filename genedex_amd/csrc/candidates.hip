// candidates.hip -- the link between seeds and verification: the seed slots of a batch (gdx_smems_many[_dev]'s layout) become
// ranked, de-duplicated candidates (cand_query, cand_begin, cand_hits) in fixed-stride slots that go straight into
// gdx_hamming_many_dev / gdx_edit_distance_many_dev / gdx_align_many_dev (gdx_seed_candidates_many[_dev]; the definition is in
// include/gdx_experimental.h "seed-hit candidates").
//
//   candidates_kernel   ONE wavefront (a block of 64 lanes) per query, grid-stride.  Dynamic LDS sized from max_seeds and
//                       max_seeds * max_occ (<= GDX_CAND_MAX_ANCHORS); every phase ends in a block barrier, which on a
//                       one-wave block costs next to nothing and keeps the LDS hand-overs between lanes well defined.
//   1. check            a lane per seed: length, start <= end <= n (before any suffix-array read), strictly descending begin and
//                       end in 64 bits; begin / length / anchor count of every seed go to LDS.
//   2. anchors          a wave scan of the anchor counts gives every seed its first anchor; then a lane per ANCHOR (the seed by
//                       binary search over the scan), so the SA loads of one seed's rows are consecutive.  An anchor is the key
//                       (t, (d + 2^32) << 10 | 1023 - j): seeds descend in begin, so ascending begin is descending j, and the
//                       seed number is all that has to travel with the key (pos = d + begin[j]).
//      one anchor       the common read of a non-repetitive text: one group of weight length[j], no sort.
//   3. sort             bitonic network over the next power of two of the query's anchors (uniform in the wave).
//   4. groups           a lane per anchor finds by binary search where a group that OPENS at it ends (first anchor of another
//                       text or more than `band` diagonals on); lane 0 follows these links from anchor 0 and leaves the heads.
//   5. per group        groups of one anchor: weight = the seed's length.  Others, one after the other with all lanes: the seeds
//                       of the group as a bit set in LDS, a lane per seed adds what its seed covers beyond the next seed of the
//                       set that begins in front of it (seeds descend in begin AND end, so that one alone can overlap it from the
//                       left), a wave sum; the representative by a wave maximum of (length, first in order).
//   6. output           the groups as keys (~weight, group number, representative), sorted ascending by the same network; the
//                       first max_candidates are decoded and stored, the other slots get the none pattern.
#include "../../include/gdx_experimental.h"
#include "common.hpp"
#include "kernels.hpp"
#include "layout.hpp"

namespace gdx {

namespace {

constexpr int kWave = 64;
constexpr uint32_t kMaxGrid = 256u * 16u;
constexpr uint64_t kBias = 1ull << 32;  // d + kBias > 0 for every diagonal

struct CandArgs {
    const uint32_t *sa_full, *jump32;  // SA[row], or word 6 of the 32-byte jump entry of the row
    const uint32_t *sentinels;
    uint32_t n, n_texts;
    uint64_t nq;
    uint32_t max_seeds, max_occ, band, max_candidates;
    uint32_t cap;  // anchors a slot holds: the next power of two of max_seeds * max_occ
    const uint32_t *n_seeds, *begin, *length, *start, *end;
    uint32_t *n_candidates, *n_groups, *n_skipped;
    uint32_t *cand_query, *cand_begin;
    gdx_hit32_t *cand_hits;
    uint32_t *cand_weight;
    uint8_t *status;  // or null
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

__device__ __forceinline__ uint64_t wave_max64(uint64_t v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const uint64_t w = __shfl_xor(v, o, kWave);
        v = w > v ? w : v;
    }
    return v;
}

__device__ __forceinline__ uint32_t pow2_ceil(uint32_t v)  // v >= 1
{
    return v <= 1u ? 1u : 1u << (32 - __clz(static_cast<int>(v - 1u)));
}

// ascending bitonic sort of p (a power of two) keys (hi[x], lo[x]), hi == nullptr: of lo alone.  All 64 lanes, ends in a barrier
__device__ __forceinline__ void bitonic_sort(uint32_t *hi, uint64_t *lo, uint32_t p)
{
    for (uint32_t k = 2; k <= p; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t x = threadIdx.x; x < p; x += kWave) {
                const uint32_t y = x ^ j;
                if (y > x) {
                    const uint64_t lx = lo[x], ly = lo[y];
                    const uint32_t hx = hi ? hi[x] : 0u, hy = hi ? hi[y] : 0u;
                    const bool greater = hx > hy || (hx == hy && lx > ly);
                    if (greater == ((x & k) == 0u)) {
                        lo[x] = ly;
                        lo[y] = lx;
                        if (hi) {
                            hi[x] = hy;
                            hi[y] = hx;
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kWave) void candidates_kernel(const CandArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    // the 8-byte arrays first: every base stays aligned
    uint64_t *s_k = reinterpret_cast<uint64_t *>(smem);  // [cap] anchor keys below the text id
    uint64_t *s_g = s_k + a.cap;                          // [cap] group keys
    uint32_t *s_t = reinterpret_cast<uint32_t *>(s_g + a.cap);  // [cap] anchor text ids
    uint32_t *s_next = s_t + a.cap;                       // [cap] where a group opening at x ends; then the group heads
    uint32_t *s_sb = s_next + a.cap;                      // [max_seeds] seed begin
    uint32_t *s_sl = s_sb + a.max_seeds;                  // [max_seeds] seed length
    uint32_t *s_off = s_sl + a.max_seeds;                 // [max_seeds + 1] first anchor of a seed
    uint32_t *s_mask = s_off + a.max_seeds + 1u;          // [ceil(max_seeds / 32)] the seeds of one group
    const uint32_t lane = threadIdx.x;

    for (uint64_t q = blockIdx.x; q < a.nq; q += gridDim.x) {
        const uint64_t slot0 = q * a.max_seeds, out0 = q * a.max_candidates;
        const uint32_t ns = a.n_seeds[q];

        // 1. check, and the seeds into LDS
        int bad = ns > a.max_seeds;
        uint32_t skipped = 0;
        if (!bad) {
            for (uint32_t j = lane; j < ns; j += kWave) {
                const uint32_t b = a.begin[slot0 + j], len = a.length[slot0 + j], s = a.start[slot0 + j], e = a.end[slot0 + j];
                if (len == 0u || s > e || e > a.n) bad = 1;
                if (j > 0u) {
                    const uint32_t pb = a.begin[slot0 + j - 1u], pl = a.length[slot0 + j - 1u];
                    if (b >= pb || static_cast<uint64_t>(b) + len >= static_cast<uint64_t>(pb) + pl) bad = 1;
                }
                const uint32_t occ = s <= e ? e - s : 0u;
                s_sb[j] = b;
                s_sl[j] = len;
                s_off[j] = occ <= a.max_occ ? occ : 0u;  // (the count; the scan below turns it into the first anchor)
                if (occ > a.max_occ) skipped++;
            }
        }
        bad = __any(bad);  // (one wavefront: s_off is read back by the lane that wrote it)
        uint32_t n_anchors = 0;
        if (!bad) {
            skipped = wave_sum(skipped);
            // exclusive scan of the counts, 64 seeds a round
            for (uint32_t j0 = 0; j0 < ns; j0 += kWave) {
                const uint32_t j = j0 + lane;
                const uint32_t c = j < ns ? s_off[j] : 0u;
                uint32_t incl = c;
#pragma unroll
                for (int o = 1; o < kWave; o <<= 1) {
                    const uint32_t up = __shfl_up(incl, o, kWave);
                    if (lane >= static_cast<uint32_t>(o)) incl += up;
                }
                if (j < ns) s_off[j] = n_anchors + incl - c;
                n_anchors += __shfl(incl, kWave - 1, kWave);
            }
            if (lane == 0u) s_off[ns] = n_anchors;
        }
        __syncthreads();

        uint32_t n_groups = 0;
        if (!bad && n_anchors != 0u) {  // (n_anchors <= ns * max_occ <= cap)
            // 2. anchors
            for (uint32_t x = lane; x < n_anchors; x += kWave) {
                uint32_t lo = 0, hi = ns;  // the last seed j with s_off[j] <= x (seeds without anchors share an offset)
                while (hi - lo > 1u) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (s_off[mid] <= x) lo = mid;
                    else hi = mid;
                }
                const uint32_t j = lo;
                const uint32_t row = a.start[slot0 + j] + (x - s_off[j]);  // < end <= n
                const uint32_t g = a.sa_full != nullptr ? a.sa_full[row] : a.jump32[static_cast<uint64_t>(row) * 8u + 6u];
                const uint32_t t = lower_bound_u32(a.sentinels, a.n_texts, g);
                const uint32_t pos = t == 0u ? g : g - a.sentinels[t - 1u] - 1u;
                const uint64_t d = kBias + pos - s_sb[j];
                s_t[x] = t;
                s_k[x] = (d << 10) | (1023u - j);
            }
            if (n_anchors == 1u) {  // one group of one anchor
                if (lane == 0u) {
                    const uint32_t j = 1023u - static_cast<uint32_t>(s_k[0] & 1023u);
                    s_g[0] = static_cast<uint64_t>(0xFFFFFFFFu - s_sl[j]) << 32;
                }
                n_groups = 1;
                __syncthreads();
            } else {
                // 3. sort by (t, d, begin)
                const uint32_t p = pow2_ceil(n_anchors);
                for (uint32_t x = n_anchors + lane; x < p; x += kWave) {
                    s_t[x] = 0xFFFFFFFFu;
                    s_k[x] = ~0ull;
                }
                __syncthreads();
                bitonic_sort(s_t, s_k, p);
                // 4. where a group that opens at x ends
                for (uint32_t x = lane; x < n_anchors; x += kWave) {
                    const uint32_t t = s_t[x];
                    const uint64_t d_max = (s_k[x] >> 10) + a.band;
                    uint32_t lo = x + 1u, hi = n_anchors;  // first y in (x, n_anchors] of another text or beyond d_max
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (s_t[mid] == t && (s_k[mid] >> 10) <= d_max) lo = mid + 1u;
                        else hi = mid;
                    }
                    s_next[x] = lo;
                }
                __syncthreads();
                uint32_t heads = 0;
                if (lane == 0u) {  // the heads, in place: head g sits at or behind slot g, and its link is read before slot g is written
                    uint32_t h = 0;
                    while (h < n_anchors) {
                        const uint32_t nh = s_next[h];
                        s_next[heads++] = h;
                        h = nh;
                    }
                }
                n_groups = __shfl(heads, 0, kWave);
                __syncthreads();
                // 5. weight and representative of every group
                const uint32_t n_words = (ns + 31u) >> 5;
                for (uint32_t g = 0; g < n_groups; g++) {
                    const uint32_t x0 = s_next[g], x1 = g + 1u < n_groups ? s_next[g + 1u] : n_anchors;
                    if (x1 - x0 == 1u) {
                        if (lane == 0u) {
                            const uint32_t j = 1023u - static_cast<uint32_t>(s_k[x0] & 1023u);
                            s_g[g] = (static_cast<uint64_t>(0xFFFFFFFFu - s_sl[j]) << 32) | (g << 10) | x0;
                        }
                        continue;
                    }
                    for (uint32_t w = lane; w < n_words; w += kWave) s_mask[w] = 0u;
                    __syncthreads();
                    uint64_t best = 0;  // (length, first in order) of the lane's anchors
                    for (uint32_t x = x0 + lane; x < x1; x += kWave) {
                        const uint32_t j = 1023u - static_cast<uint32_t>(s_k[x] & 1023u);
                        atomicOr(&s_mask[j >> 5], 1u << (j & 31u));
                        const uint64_t key = (static_cast<uint64_t>(s_sl[j]) << 32) | (0xFFFFFFFFu - x);
                        best = key > best ? key : best;
                    }
                    __syncthreads();
                    uint64_t covered = 0;
                    for (uint32_t j = lane; j < ns; j += kWave) {
                        if (((s_mask[j >> 5] >> (j & 31u)) & 1u) == 0u) continue;
                        const uint64_t b = s_sb[j], e = b + s_sl[j];
                        // the next seed of the set behind j: it begins and ends in front of seed j
                        uint32_t w = j >> 5;
                        uint32_t bits = (j & 31u) == 31u ? 0u : s_mask[w] & (~0u << ((j & 31u) + 1u));
                        while (bits == 0u && ++w < n_words) bits = s_mask[w];
                        uint64_t from = b;
                        if (bits != 0u) {
                            const uint32_t j2 = (w << 5) + static_cast<uint32_t>(__ffs(static_cast<int>(bits)) - 1);
                            const uint64_t e2 = static_cast<uint64_t>(s_sb[j2]) + s_sl[j2];
                            from = e2 > b ? e2 : b;
                        }
                        covered += e - from;
                    }
                    covered = wave_sum64(covered);
                    best = wave_max64(best);
                    if (lane == 0u) {
                        const uint32_t weight = covered > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(covered);
                        const uint32_t rep = 0xFFFFFFFFu - static_cast<uint32_t>(best);
                        s_g[g] = (static_cast<uint64_t>(0xFFFFFFFFu - weight) << 32) | (g << 10) | rep;
                    }
                    __syncthreads();  // (the set is cleared again by the next group of several anchors)
                }
                // 6. by descending weight, then in the order of the heads: ascending (t, d_first)
                const uint32_t pg = pow2_ceil(n_groups);
                for (uint32_t g = n_groups + lane; g < pg; g += kWave) s_g[g] = ~0ull;
                __syncthreads();
                bitonic_sort(nullptr, s_g, pg);
            }
        }

        const uint32_t n_out = n_groups < a.max_candidates ? n_groups : a.max_candidates;
        for (uint32_t c = lane; c < a.max_candidates; c += kWave) {
            uint32_t cq = GDX_CAND_NONE, cb = 0, weight = 0;
            gdx_hit32_t hit;
            hit.text_id = 0;
            hit.position = 0;
            if (c < n_out) {
                const uint64_t key = s_g[c];
                const uint32_t rep = static_cast<uint32_t>(key & 1023u);
                const uint64_t k = s_k[rep];
                const uint32_t j = 1023u - static_cast<uint32_t>(k & 1023u);
                cq = static_cast<uint32_t>(q);
                cb = s_sb[j];
                weight = 0xFFFFFFFFu - static_cast<uint32_t>(key >> 32);
                hit.text_id = s_t[rep];
                hit.position = static_cast<uint32_t>((k >> 10) - kBias + cb);
            }
            a.cand_query[out0 + c] = cq;
            a.cand_begin[out0 + c] = cb;
            a.cand_hits[out0 + c] = hit;
            a.cand_weight[out0 + c] = weight;
        }
        if (lane == 0u) {
            a.n_candidates[q] = n_out;
            a.n_groups[q] = n_groups;
            a.n_skipped[q] = bad ? 0u : skipped;
            if (a.status != nullptr) a.status[q] = bad ? GDX_CAND_BAD_SEEDS : 0u;
        }
        __syncthreads();  // the slot is the next query's
    }
}

}  // namespace

bool seed_candidates_supported(const IndexView &ix) { return ix.sa_full != nullptr || (ix.jump != nullptr && ix.jump_bytes == 32); }

void launch_seed_candidates(const IndexView &ix, uint64_t nq, uint32_t max_seeds, const uint32_t *d_n_seeds, const uint32_t *d_begin,
                            const uint32_t *d_length, const uint32_t *d_start, const uint32_t *d_end, uint32_t max_occ, uint32_t band,
                            uint32_t max_candidates, uint32_t *d_n_candidates, uint32_t *d_n_groups, uint32_t *d_n_skipped,
                            uint32_t *d_cand_query, uint32_t *d_cand_begin, gdx_hit32_t *d_cand_hits, uint32_t *d_cand_weight,
                            uint8_t *d_status, hipStream_t stream)
{
    if (nq == 0) return;
    CandArgs a;
    a.sa_full = ix.sa_full;
    a.jump32 = ix.sa_full == nullptr ? static_cast<const uint32_t *>(ix.jump) : nullptr;
    a.sentinels = ix.sentinels;
    a.n = ix.n;
    a.n_texts = ix.n_texts;
    a.nq = nq;
    a.max_seeds = max_seeds;
    a.max_occ = max_occ;
    a.band = band;
    a.max_candidates = max_candidates;
    uint32_t cap = 1;
    while (cap < max_seeds * max_occ) cap <<= 1;  // (the product is at most GDX_CAND_MAX_ANCHORS: checked by the caller)
    a.cap = cap;
    a.n_seeds = d_n_seeds;
    a.begin = d_begin;
    a.length = d_length;
    a.start = d_start;
    a.end = d_end;
    a.n_candidates = d_n_candidates;
    a.n_groups = d_n_groups;
    a.n_skipped = d_n_skipped;
    a.cand_query = d_cand_query;
    a.cand_begin = d_cand_begin;
    a.cand_hits = d_cand_hits;
    a.cand_weight = d_cand_weight;
    a.status = d_status;
    // at most 24 * 1024 + 12 * 1024 + 4 + 128 bytes: below the 64 KiB a launch may ask for without further ado
    const size_t lds = static_cast<size_t>(cap) * 24u + static_cast<size_t>(max_seeds) * 12u + 4u + ((max_seeds + 31u) / 32u) * 4u;
    const unsigned grid = static_cast<unsigned>(nq < kMaxGrid ? nq : kMaxGrid);
    hipLaunchKernelGGL(candidates_kernel, dim3(grid), dim3(kWave), lds, stream, a);
}

}  // namespace gdx
