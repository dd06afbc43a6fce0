// select.hpp -- what the two selection stages behind the verify calls (best_hits.hip, pair_hits.hip) have in common.  For the
// host: the argument blocks, which capi.hip and fm_query.hip fill and the launch functions of kernels.hpp take.  For the kernels
// (namespace select): the constants, the slot loader with the "live" rule, the same-locus rotation pass, the xor-butterfly
// minimum, the mapq rule, the winner store with its none pattern and the instance dispatch.  A stage keeps what is its own:
// best_hits.hip the ballot counts and the per-group stores, pair_hits.hip the combinations pass, its fused butterfly of counts and
// sub_dist, the kAlone flag encoding and the per-pair stores.  best_hits_kernel also keeps a copy of same_locus_pass in its own
// text: a change to the rule "same locus" goes into both.
// profiles/r19/select_refactor.md has what the shapes of these helpers do to the kernels' code, and why that copy stays.
#pragma once
#include <type_traits>

#include "../../include/gdx_experimental.h"
#include "common.hpp"
#include "kernels.hpp"

namespace gdx {

// the candidate slots and their distances from a verify call, and the winner triple; a stage's own arguments derive from it
struct SlotArgs {
    const uint32_t *cand_query, *cand_begin;
    const gdx_hit32_t *cand_hits;
    const uint32_t *dist, *end;  // end: or null
    uint32_t max_dist;
    uint32_t *win_query, *win_begin;
    gdx_hit32_t *win_hits;
};

struct BestArgs : SlotArgs {
    uint64_t n_groups;
    uint32_t group_slots;
    uint32_t *best_slot, *best_dist, *sub_dist, *n_live, *n_best, *mapq;
};

struct PairArgs : SlotArgs {
    uint64_t n_pairs;
    uint32_t mate_slots, min_insert, max_insert;
    uint32_t *n_proper, *n_best, *pair_dist, *sub_dist, *mapq, *pair_span;
    uint32_t *mate_slot, *mate_dist;
};

namespace select {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr uint32_t kMaxGrid = 256u * 16u;
constexpr uint32_t kDead = 0xFFFFFFFFu;  // the distance a dead lane and the score a missing combination carry: above 2^31

// a lane's slot: e is where its alignment ends (its diagonal without `end`), d its distance, or kDead when it is not live
struct Slot {
    uint32_t cq, cb, e, d, tid, pos;
};

// 1. slot j of unit `unit` (a group, a mate) of `slots` slots; a lane out of range gets GDX_CAND_NONE / kDead and zeros.  Live:
// cand_query != GDX_CAND_NONE and dist <= max_dist
__device__ __forceinline__ Slot load_slot(const SlotArgs &a, bool in_range, uint64_t unit, uint32_t slots, uint32_t j)
{
    Slot x = {GDX_CAND_NONE, 0, 0, kDead, 0, 0};
    if (in_range) {
        const uint64_t s = unit * slots + j;
        x.cq = a.cand_query[s];
        x.cb = a.cand_begin[s];
        x.tid = a.cand_hits[s].text_id;
        x.pos = a.cand_hits[s].position;
        const uint32_t ds = a.dist[s];
        x.e = a.end != nullptr ? a.end[s] : x.pos - x.cb;
        if (x.cq != GDX_CAND_NONE && ds <= a.max_dist) x.d = ds;
    }
    return x;
}

// 2. same locus: P - 1 rotations of (cq, tid, e, d) inside the group of P lanes (__shfl of width P; the source slot is the
// rotation itself and does not travel).  -> live: no live slot with this lane's key has a smaller (dist, slot).  Unrolled.
template <int P>
__device__ __forceinline__ bool same_locus_pass(const Slot &x, uint32_t j)
{
    bool live = x.d != kDead;
#pragma unroll
    for (int r = 1; r < P; r++) {
        const int src = static_cast<int>((j + r) & (P - 1));
        const uint32_t oq = __shfl(x.cq, src, P), ot = __shfl(x.tid, src, P), oe = __shfl(x.e, src, P), od = __shfl(x.d, src, P);
        const bool same = od != kDead && oq == x.cq && ot == x.tid && oe == x.e;
        if (same && (od < x.d || (od == x.d && static_cast<uint32_t>(src) < j))) live = false;
    }
    return live;
}

// the least v of the group of P lanes, in every lane: an xor butterfly of log2 P steps
template <int P, class T>
__device__ __forceinline__ T butterfly_min(T v)
{
#pragma unroll
    for (int o = P / 2; o > 0; o >>= 1) {
        const T w = __shfl_xor(v, o, P);
        v = w < v ? w : v;
    }
    return v;
}

// min(60, 60 (sub - best) / denom); denom is the stage's: one more than the largest distance a winner can have
__device__ __forceinline__ uint32_t mapq_of(uint32_t sub, uint32_t best, uint64_t denom)
{
    const uint64_t q = 60ull * (sub - best) / denom;
    return q < 60ull ? static_cast<uint32_t>(q) : 60u;
}

// the winner triple of entry `at`: the lane's slot, or the none pattern GDX_CAND_NONE, 0, (0, 0)
__device__ __forceinline__ void store_winner(const SlotArgs &a, uint64_t at, bool some, const Slot &x)
{
    a.win_query[at] = some ? x.cq : GDX_CAND_NONE;
    a.win_begin[at] = some ? x.cb : 0u;
    a.win_hits[at].text_id = some ? x.tid : 0u;
    a.win_hits[at].position = some ? x.pos : 0u;
}

// the instance of a batch: f(P) with P = the next power of two >= slots, at most kMax, as a compile-time value
template <int kMax, int P = 1, class F>
void dispatch_slots(uint32_t slots, F &&f)
{
    if constexpr (P < kMax) {
        if (slots > static_cast<uint32_t>(P)) return dispatch_slots<kMax, 2 * P>(slots, f);
    }
    f(std::integral_constant<int, P>{});
}

}  // namespace select

}  // namespace gdx
