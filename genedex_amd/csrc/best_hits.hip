// best_hits.hip -- the reduction behind the verify calls: of the group_slots verified candidate slots of a read, the one that is
// the alignment, whether it is unique, and the winner as a one-slot candidate list for the traceback (gdx_best_hits_many[_dev]; the
// definition is in include/gdx_experimental.h "best hit per read").
//
//   best_hits_kernel<P>  P = the next power of two >= group_slots: a group is P adjacent lanes, a wavefront holds 64 / P groups of
//                        consecutive numbers, so the slots a wavefront loads from each of the five input arrays are one
//                        contiguous run (lanes j >= group_slots of a group idle: at most half of them).  Blocks of four
//                        wavefronts, grid-stride over tiles of 64 / P groups with a bound that is uniform in the wavefront.
//   1. live              cand_query != GDX_CAND_NONE and dist <= max_dist; a dead lane carries distance 2^32 - 1 from here on
//   2. same locus        P - 1 rotations of (cand_query, text_id, e, dist) inside the group (__shfl of width P; the source slot
//                        is the rotation itself and does not travel): a lane drops out when a live slot with its key has a
//                        smaller (dist, slot).  Unrolled: P is a compile-time instance.
//   3. results           the least (dist, slot) as one 64-bit value and the least distance of the others as a 32-bit one by xor
//                        butterflies of log2 P steps; the two counts from the group's bits of a ballot.
//   4. output            the winner's lane stores the three winner words, lane 0 of the group the six per-group words (and the
//                        none pattern of a group without a live slot).
// No LDS, no atomics, no second launch.  Slot and group numbers are 64 bits wide throughout.
#include "../../include/gdx_experimental.h"
#include "common.hpp"
#include "kernels.hpp"

namespace gdx {

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr uint32_t kMaxGrid = 256u * 16u;
constexpr uint32_t kDead = 0xFFFFFFFFu;  // the distance a dead lane carries: above every max_dist (<= 2^31)

struct BestArgs {
    uint64_t n_groups;
    uint32_t group_slots, max_dist;
    const uint32_t *cand_query, *cand_begin;
    const gdx_hit32_t *cand_hits;
    const uint32_t *dist, *end;  // end: or null
    uint32_t *best_slot, *best_dist, *sub_dist, *n_live, *n_best, *mapq;
    uint32_t *win_query, *win_begin;
    gdx_hit32_t *win_hits;
};

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
        const bool in_group = g < a.n_groups && j < a.group_slots;
        uint32_t cq = GDX_CAND_NONE, cb = 0, e = 0, d = kDead;
        uint32_t tid = 0, pos = 0;
        if (in_group) {
            const uint64_t s = g * a.group_slots + j;
            cq = a.cand_query[s];
            cb = a.cand_begin[s];
            tid = a.cand_hits[s].text_id;
            pos = a.cand_hits[s].position;
            const uint32_t ds = a.dist[s];
            e = a.end != nullptr ? a.end[s] : pos - cb;
            if (cq != GDX_CAND_NONE && ds <= k) d = ds;
        }

        // 2. a live slot with this lane's key and a smaller (dist, slot) takes the lane out
        bool live = d != kDead;
#pragma unroll
        for (int r = 1; r < P; r++) {
            const int src = static_cast<int>((j + r) & (P - 1));
            const uint32_t oq = __shfl(cq, src, P), ot = __shfl(tid, src, P), oe = __shfl(e, src, P), od = __shfl(d, src, P);
            const bool same = od != kDead && oq == cq && ot == tid && oe == e;
            if (same && (od < d || (od == d && static_cast<uint32_t>(src) < j))) live = false;
        }

        // 3. the best slot, the runner-up's distance, the counts
        uint64_t best = live ? (static_cast<uint64_t>(d) << 32) | j : ~0ull;
#pragma unroll
        for (int o = P / 2; o > 0; o >>= 1) {
            const uint64_t w = __shfl_xor(best, o, P);
            best = w < best ? w : best;
        }
        const bool any = best != ~0ull;
        const uint32_t bj = static_cast<uint32_t>(best), bd = any ? static_cast<uint32_t>(best >> 32) : k + 1u;
        uint32_t sub = live && j != bj ? d : kDead;
#pragma unroll
        for (int o = P / 2; o > 0; o >>= 1) {
            const uint32_t w = __shfl_xor(sub, o, P);
            sub = w < sub ? w : sub;
        }
        if (sub == kDead) sub = k + 1u;
        constexpr uint64_t group_bits = ~0ull >> (kWave - P);
        const uint32_t n_live = __popcll((__ballot(live) >> first) & group_bits);
        const uint32_t n_best = __popcll((__ballot(live && d == bd) >> first) & group_bits);

        // 4. output
        if (g < a.n_groups) {
            if (any ? (live && j == bj) : j == 0u) {  // (without a live slot: lane 0 still holds what it loaded, so the pattern)
                a.win_query[g] = any ? cq : GDX_CAND_NONE;
                a.win_begin[g] = any ? cb : 0u;
                a.win_hits[g].text_id = any ? tid : 0u;
                a.win_hits[g].position = any ? pos : 0u;
            }
            if (j == 0u) {
                uint32_t mapq = GDX_BEST_MAPQ_NONE;
                if (any) {
                    const uint64_t q = 60ull * (sub - bd) / (static_cast<uint64_t>(k) + 1ull);
                    mapq = q < 60ull ? static_cast<uint32_t>(q) : 60u;
                }
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

template <int P>
void launch_instance(const BestArgs &a, hipStream_t stream)
{
    constexpr uint64_t per_block = static_cast<uint64_t>(kBlock) / P;  // groups a block takes in one stride
    const uint64_t blocks = (a.n_groups + per_block - 1) / per_block;
    const unsigned grid = static_cast<unsigned>(blocks < kMaxGrid ? blocks : kMaxGrid);
    hipLaunchKernelGGL(best_hits_kernel<P>, dim3(grid), dim3(kBlock), 0, stream, a);
}

}  // namespace

void launch_best_hits(uint64_t n_groups, uint32_t group_slots, const uint32_t *d_cand_query, const uint32_t *d_cand_begin,
                      const gdx_hit32_t *d_cand_hits, const uint32_t *d_dist, const uint32_t *d_end, uint32_t max_dist,
                      uint32_t *d_best_slot, uint32_t *d_best_dist, uint32_t *d_sub_dist, uint32_t *d_n_live, uint32_t *d_n_best,
                      uint32_t *d_mapq, uint32_t *d_win_query, uint32_t *d_win_begin, gdx_hit32_t *d_win_hits, hipStream_t stream)
{
    if (n_groups == 0) return;
    BestArgs a;
    a.n_groups = n_groups;
    a.group_slots = group_slots;
    a.max_dist = max_dist;
    a.cand_query = d_cand_query;
    a.cand_begin = d_cand_begin;
    a.cand_hits = d_cand_hits;
    a.dist = d_dist;
    a.end = d_end;
    a.best_slot = d_best_slot;
    a.best_dist = d_best_dist;
    a.sub_dist = d_sub_dist;
    a.n_live = d_n_live;
    a.n_best = d_n_best;
    a.mapq = d_mapq;
    a.win_query = d_win_query;
    a.win_begin = d_win_begin;
    a.win_hits = d_win_hits;
    if (group_slots <= 1u) launch_instance<1>(a, stream);
    else if (group_slots <= 2u) launch_instance<2>(a, stream);
    else if (group_slots <= 4u) launch_instance<4>(a, stream);
    else if (group_slots <= 8u) launch_instance<8>(a, stream);
    else if (group_slots <= 16u) launch_instance<16>(a, stream);
    else if (group_slots <= 32u) launch_instance<32>(a, stream);
    else launch_instance<64>(a, stream);  // (group_slots <= GDX_BEST_MAX_GROUP_SLOTS = 64: checked by the caller)
}

}  // namespace gdx
