// pair_hits.hip -- paired-end pairing of verified candidate slots: per read pair the best properly oriented, properly spaced
// combination of one slot of each mate, whether it is unique, and the two winners as a candidate list for the traceback
// (gdx_pair_hits_many[_dev]; the definition is in include/gdx_experimental.h "paired-end pairing").  Steps 1 and 2, the
// butterfly of the least key, the mapq rule, the winner store and the dispatch are select.hpp's, shared with best_hits.hip.
//
//   pair_hits_kernel<P>  P = the next power of two >= mate_slots: a pair is 2P adjacent lanes, mate 0 on the lower P and mate 1 on
//                        the upper, a wavefront holds 64 / 2P pairs of consecutive numbers, so the slots a wavefront loads from
//                        each of the five input arrays are one contiguous run (lanes j >= mate_slots of a mate idle).  Blocks of
//                        four wavefronts, grid-stride over tiles of 64 / 2P pairs with a bound that is uniform in the wavefront.
//   1. live              load_slot: a dead lane carries distance 2^32 - 1 from here on
//   2. same locus        same_locus_pass at width P, inside each mate
//   3. combinations      P rotations across the halves (__shfl of width 2P): lane i of one mate meets every lane of the other.
//                        A slot ships its distance, its text and ONE signed 64-bit word -- twice its diagonal when it is on
//                        strand 0, twice its right end when on strand 1, the strand in bit 0 -- so span = right_r - diag_f
//                        whichever side the lane is on.
//                        Each lane keeps its least score and the least partner that has it, that partner's span, how often the
//                        score occurs, its second-least score and its count of proper partners.  Both halves run the pass.
//   4. results           xor butterflies over the half: the least (score, i, j) as one 64-bit value (butterfly_min; the same
//                        value in both halves, so each mate's winning lane knows itself), the sums of the proper and tied counts
//                        in one word, and sub_dist as the least of the best lane's second-least and the other lanes' least.
//   5. winners           without a proper combination the least (dist, j) of each half, carried by the same butterfly under a flag
//                        bit.  Each mate's winning lane stores its five words, mate 0's the six words of the pair (it holds the
//                        span).
// No LDS, no atomics, no second launch.  Slot and pair numbers are 64 bits wide throughout; diagonals are signed 64-bit values.
#include "select.hpp"

namespace gdx {

namespace {

using namespace select;

template <int P>
__global__ __launch_bounds__(kBlock) void pair_hits_kernel(const PairArgs a)
{
    constexpr int W = 2 * P;                 // lanes of a pair
    constexpr uint32_t kPairs = kWave / W;   // pairs of a wavefront
    const uint32_t lane = threadIdx.x & (kWave - 1), j = lane & (P - 1), h = (lane / P) & 1u;
    const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * (kBlock / kWave) * kPairs;
    const uint32_t k = a.max_dist;
    const int64_t lo = a.min_insert, hi = a.max_insert;

    for (uint64_t g0 = wave * kPairs; g0 < a.n_pairs; g0 += stride) {  // (uniform in the wavefront: every lane shuffles)
        const uint64_t g = g0 + lane / W, mate = 2 * g + h;
        const Slot x = load_slot(a, g < a.n_pairs && j < a.mate_slots, mate, a.mate_slots, j);
        const uint32_t d = x.d, tid = x.tid, strand = x.cq & 1u;
        const int64_t diag = static_cast<int64_t>(x.pos) - static_cast<int64_t>(x.cb);
        const int64_t right = a.end != nullptr ? static_cast<int64_t>(x.e) : diag;
        const int64_t coord = (strand ? right : diag) * 2 + strand;  // (34 bits and a sign: the strand travels in bit 0)
        const bool live = same_locus_pass<P>(x, j);
        const uint32_t dl = live ? d : kDead;

        // 3. every slot of the other mate: least score and its least partner, the tie count, the second-least, the proper count
        uint32_t m1 = kDead, m2 = kDead, cnt = 0, part = 0, span32 = 0, n_prop = 0;
#pragma unroll
        for (int r = 0; r < P; r++) {
            const uint32_t pj = (j + r) & (P - 1);
            const int src = static_cast<int>((h ^ 1u) * P + pj);
            const uint32_t od = __shfl(dl, src, W), ot = __shfl(tid, src, W);
            const int64_t ow = __shfl(coord, src, W), oc = ow >> 1;
            const uint32_t os = static_cast<uint32_t>(ow) & 1u;
            const int64_t span = strand ? right - oc : oc - diag;  // (right_r - diag_f: the partner shipped the other one)
            const bool proper = live && od != kDead && ot == tid && os != strand && span >= lo && span <= hi;
            if (proper) {
                const uint32_t s = dl + od;
                n_prop++;
                if (s < m1) {
                    m2 = m1;
                    m1 = s;
                    cnt = 1;
                    part = pj;
                    span32 = static_cast<uint32_t>(span);
                } else if (s == m1) {
                    m2 = s;
                    cnt++;
                    if (pj < part) {
                        part = pj;
                        span32 = static_cast<uint32_t>(span);
                    }
                } else if (s < m2) {
                    m2 = s;
                }
            }
        }

        // 4. the pair's results, the same in both halves, and 5. the single-end best of this mate in one butterfly: a lane with a
        // proper partner offers score << 16 | i << 8 | j (a score is at most 2 * 2^30: below 2^48), a live lane without one bit 63
        // and dist << 8 | j -- above every proper key, so the least is the mate's single-end best exactly when the pair has no
        // proper combination
        const uint32_t ci = h ? part : j, cj = h ? j : part;  // the combination (slot of mate 0, slot of mate 1)
        constexpr uint64_t kAlone = 1ull << 63;
        const uint64_t best = butterfly_min<P>(m1 != kDead ? (static_cast<uint64_t>(m1) << 16) | (ci << 8) | cj
                                               : live      ? kAlone | (static_cast<uint64_t>(d) << 8) | j
                                                           : ~0ull);
        const bool any = best < kAlone, mapped = best != ~0ull;
        const uint32_t pd = any ? static_cast<uint32_t>(best >> 16) : 2u * k + 2u;
        const uint32_t mine = h || !any ? static_cast<uint32_t>(best) & 0xFFu : (static_cast<uint32_t>(best) >> 8) & 0xFFu;
        const bool winner = any && live && j == mine;
        uint32_t counts = (n_prop << 16) | (any && m1 == pd ? cnt : 0u);  // (both sums are at most 32 * 32)
        uint32_t sub = winner ? m2 : m1;
#pragma unroll
        for (int o = P / 2; o > 0; o >>= 1) {  // (butterfly_min's steps with the sum of the counts between them)
            counts += __shfl_xor(counts, o, P);
            const uint32_t w = __shfl_xor(sub, o, P);
            sub = w < sub ? w : sub;
        }
        n_prop = counts >> 16;
        const uint32_t n_best = counts & 0xFFFFu;
        if (sub == kDead) sub = 2u * k + 2u;
        const bool writer = mapped ? live && j == mine : j == 0u;

        if (g < a.n_pairs && writer) {  // (without a live slot: lane 0 of the mate writes the pattern)
            a.mate_slot[mate] = mapped ? j : GDX_PAIR_NONE;
            a.mate_dist[mate] = mapped ? d : k + 1u;
            store_winner(a, mate, mapped, x);
            if (h == 0u) {
                const uint32_t mapq = any ? mapq_of(sub, pd, 2ull * k + 2ull) : GDX_PAIR_MAPQ_NONE;
                a.n_proper[g] = n_prop;
                a.n_best[g] = n_best;
                a.pair_dist[g] = pd;
                a.sub_dist[g] = sub;
                a.mapq[g] = mapq;
                a.pair_span[g] = any ? span32 : 0u;
            }
        }
    }
}

}  // namespace

void launch_pair_hits(const PairArgs &a, hipStream_t stream)
{
    if (a.n_pairs == 0) return;
    dispatch_slots<GDX_PAIR_MAX_MATE_SLOTS>(a.mate_slots, [&](auto p) {  // (mate_slots <= 32: checked by the caller)
        constexpr int P = decltype(p)::value;
        const unsigned grid = grid_for(a.n_pairs, kBlock / (2 * P), kMaxGrid);  // (a block takes kBlock / 2P pairs in one stride)
        hipLaunchKernelGGL(pair_hits_kernel<P>, dim3(grid), dim3(kBlock), 0, stream, a);
    });
}

}  // namespace gdx
