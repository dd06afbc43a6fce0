// best_hits.hip -- the reduction behind the verify calls: of the group_slots verified candidate slots of a read, the one that is
// the alignment, whether it is unique, and the winner as a one-slot candidate list for the traceback (gdx_best_hits_many[_dev]; the
// definition is in include/gdx_experimental.h "best hit per read").  Step 1, the butterflies, the mapq rule, the winner store and
// the dispatch are select.hpp's, shared with pair_hits.hip; step 2 is select.hpp's same_locus_pass in the kernel's own text.
//
//   best_hits_kernel<P>  P = the next power of two >= group_slots: a group is P adjacent lanes, a wavefront holds 64 / P groups of
//                        consecutive numbers, so the slots a wavefront loads from each of the five input arrays are one
//                        contiguous run (lanes j >= group_slots of a group idle: at most half of them).  Blocks of four
//                        wavefronts, grid-stride over tiles of 64 / P groups with a bound that is uniform in the wavefront.
//   1. live              load_slot: a dead lane carries distance 2^32 - 1 from here on
//   2. same locus        P - 1 rotations of (cand_query, text_id, e, dist) inside the group (__shfl of width P; the source slot
//                        is the rotation itself and does not travel): a lane drops out when a live slot with its key has a
//                        smaller (dist, slot).  Unrolled: P is a compile-time instance.
//   3. results           the least (dist, slot) as one 64-bit value and the least distance of the others as a 32-bit one
//                        (butterfly_min); the two counts from the group's bits of a ballot.
//   4. output            the winner's lane stores the three winner words, lane 0 of the group the six per-group words (and the
//                        none pattern of a group without a live slot).
// No LDS, no atomics, no second launch.  Slot and group numbers are 64 bits wide throughout.
#include "select.hpp"

namespace gdx {

namespace {

using namespace select;

template <int P>
__global__ __launch_bounds__(kBlock) void best_hits_kernel(const BestArgs a)
{
    constexpr uint32_t kGroups = kWave / P;  // groups of a wavefront
    const uint32_t lane = threadIdx.x & (kWave - 1), j = lane & (P - 1), first = lane & ~static_cast<uint32_t>(P - 1);
    const uint64_t wave = static_cast<uint64_t>(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave;
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * (kBlock / kWave) * kGroups;
    const uint32_t k = a.max_dist;

    for (uint64_t g0 = wave * kGroups; g0 < a.n_groups; g0 += stride) {  // (uniform in the wavefront: every lane shuffles)
        const uint64_t g = g0 + lane / P;
        const Slot x = load_slot(a, g < a.n_groups && j < a.group_slots, g, a.group_slots, j);

        // 2. select.hpp's same_locus_pass, written out: called from here it measured slower (profiles/r19/select_refactor.md)
        bool live = x.d != kDead;
#pragma unroll
        for (int r = 1; r < P; r++) {
            const int src = static_cast<int>((j + r) & (P - 1));
            const uint32_t oq = __shfl(x.cq, src, P), ot = __shfl(x.tid, src, P), oe = __shfl(x.e, src, P), od = __shfl(x.d, src, P);
            const bool same = od != kDead && oq == x.cq && ot == x.tid && oe == x.e;
            if (same && (od < x.d || (od == x.d && static_cast<uint32_t>(src) < j))) live = false;
        }

        // 3. the best slot, the runner-up's distance, the counts
        const uint64_t best = butterfly_min<P>(live ? (static_cast<uint64_t>(x.d) << 32) | j : ~0ull);
        const bool any = best != ~0ull;
        const uint32_t bj = static_cast<uint32_t>(best), bd = any ? static_cast<uint32_t>(best >> 32) : k + 1u;
        uint32_t sub = butterfly_min<P>(live && j != bj ? x.d : kDead);
        if (sub == kDead) sub = k + 1u;
        constexpr uint64_t group_bits = ~0ull >> (kWave - P);
        const uint32_t n_live = __popcll((__ballot(live) >> first) & group_bits);
        const uint32_t n_best = __popcll((__ballot(live && x.d == bd) >> first) & group_bits);

        // 4. output
        if (g < a.n_groups) {
            if (any ? (live && j == bj) : j == 0u) store_winner(a, g, any, x);  // (without a live slot: lane 0 writes the pattern)
            if (j == 0u) {
                const uint32_t mapq = any ? mapq_of(sub, bd, static_cast<uint64_t>(k) + 1ull) : GDX_BEST_MAPQ_NONE;
                a.best_slot[g] = any ? bj : GDX_BEST_NONE;
                a.best_dist[g] = bd;
                a.sub_dist[g] = sub;
                a.n_live[g] = n_live;
                a.n_best[g] = n_best;
                a.mapq[g] = mapq;
            }
        }
    }
}

}  // namespace

void launch_best_hits(const BestArgs &a, hipStream_t stream)
{
    if (a.n_groups == 0) return;
    dispatch_slots<GDX_BEST_MAX_GROUP_SLOTS>(a.group_slots, [&](auto p) {  // (group_slots <= 64: checked by the caller)
        constexpr int P = decltype(p)::value;
        const unsigned grid = grid_for(a.n_groups, kBlock / P, kMaxGrid);  // (a block takes kBlock / P groups in one stride)
        hipLaunchKernelGGL(best_hits_kernel<P>, dim3(grid), dim3(kBlock), 0, stream, a);
    });
}

}  // namespace gdx
