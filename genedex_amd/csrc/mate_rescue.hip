// mate_rescue.hip -- mate rescue behind the paired-end pairing: for a pair without a proper combination, the placed mate is the
// anchor and the other mate's opposite strand is searched in the window of the text the insert bounds imply
// (gdx_mate_rescue_many[_dev]; the definition is in include/gdx_experimental.h "mate rescue").
//
//   the attempts        (p, o): n_proper[p] == 0 and mate 1 - o of pair p has a winner.  On a mapper's batch few mates have one (4 in
//                       a thousand on the genome-like text of profiles/r22/mate_rescue.md), so a lane per mate would run the window
//                       loop (up to 4608 columns) with one or two lanes of a wavefront.
//   rescue_kernel<kXlate, kUniform, W>
//                       ONE launch.  A workgroup of 256 lanes takes a TILE of consecutive pairs (by default its whole share of the
//                       batch) and goes through it in three steps.
//   1. sweep            256 pairs at a time, a lane per pair: the lane reads n_proper and the two mate_slot words, stores the
//                       not-tried pattern of a mate without an attempt, and appends its attempts (0, 1 or 2: the number of the mate
//                       inside the tile) to a ring in LDS -- ballot and popcount inside the wavefront, the four wavefront totals
//                       through LDS, no atomics.  The ring's order is that of the mates.
//   2. drain            whenever the ring holds 256 attempts or more, and once more at the end of the tile for what is left, a round:
//                       lane t takes the t-th oldest attempt and runs rescue_lane.  Every round but the tile's last has all its
//                       lanes at work.
//   rescue_lane         Myers' block algorithm as in edit_lane (edit_distance.hip): the read in W 64-row blocks in registers, one
//                       text unit per 32 columns.  The read number and the window come from the anchor, and a column's score
//                       competes only when its y is admissible -- the column y = x0 in front of any text symbol included.  It
//                       stores resc_dist and resc_end of its mate.
//   3. merge            after a barrier, 256 pairs at a time again, a lane per pair: it reads the two resc_dist / resc_end words its
//                       own workgroup stored (both attempts of a pair are in one tile, so no other workgroup's stores are needed),
//                       picks the successful attempt with the least (score, o) and writes the pair's three words and the two
//                       winners -- the anchor and the rescue candidate, or both input winners as they came.
// The ring never overflows: fewer than 256 attempts are left after the rounds, a sweep adds at most 512, the ring holds 1024.
// Nothing depends on the tile, the grid or the order of the ring: an attempt's result is a function of its inputs alone.
// LDS: the 4 KiB ring, 16 bytes of totals and the 256-byte alphabet table (kXlate 0): 4112 or 4368 bytes a workgroup, far from
// limiting the occupancy (profiles/r22/mate_rescue.md).  Pair, mate and slot numbers are 64 bits wide.
// edit_lane and align_lane are not touched: this file has its own copy of the forward pass (profiles/r15/verify_refactor.md).
#include <atomic>

#include "../../include/gdx_experimental.h"
#include "verify.hpp"

namespace gdx {

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr uint32_t kRing = 1024;           // attempts the ring holds: 255 left over + 512 of a sweep at the most
// (tools/exp_mate_rescue.py counts the rounds of a batch on the host from copies of the next two and of kBlock: change them together)
constexpr uint32_t kMaxGrid = 256u * 4u;   // workgroups of a launch at the most
constexpr uint64_t kMinTile = 2048;        // pairs: a tile below this would leave most lanes of its one round idle

// gdx_debug_set_rescue_tiling (gdx_bench.h): the tile and the grid of the launches to come, 0 = the defaults
std::atomic<uint64_t> g_tile_pairs{0}, g_grid{0};

// the batch (verify.hpp; the candidate fields stay empty), the call and the tile the launch has chosen
struct RescueArgs : VerifyArgs, RescueCall {
    uint64_t tile_pairs;  // a multiple of kBlock, at most 2^30
};

// the attempt of mate `mate` = 2p + o: the anchor is mate 2p + (1 - o)
template <int kXlate, bool kUniform, int W>
__device__ __forceinline__ void rescue_lane(const RescueArgs &a, const uint8_t *s_dense, uint64_t mate)
{
    const uint64_t p = mate >> 1, anchor = mate ^ 1u;
    const uint32_t o = static_cast<uint32_t>(mate & 1u);
    const uint32_t slot = a.mate_slot[anchor], wq = a.win_query[anchor], wb = a.win_begin[anchor];
    const gdx_hit32_t hit = a.win_hits[anchor];
    const uint32_t strand_a = wq & 1u;
    const uint64_t rq = 4 * p + 2u * o + (1u - strand_a);
    uint32_t dist = 0;
    uint64_t begin = 0;
    uint32_t L = 0;
    if (hit.text_id >= a.n_texts || slot >= a.mate_slots) {
        dist = GDX_EDIT_INVALID;
    } else {
        if (kUniform) {
            begin = rq * a.uniform_len;
            L = a.uniform_len;
        } else {
            begin = a.qoff[rq];
            const uint64_t len = a.qoff[rq + 1] - begin;
            L = len > GDX_EDIT_MAX_QUERY_LEN ? GDX_EDIT_MAX_QUERY_LEN + 1u : static_cast<uint32_t>(len);
        }
        if (L > GDX_EDIT_MAX_QUERY_LEN) dist = GDX_EDIT_TOO_LONG;
    }
    if (dist != 0u) {
        a.resc_dist[mate] = dist;
        a.resc_end[mate] = GDX_EDIT_NO_END;
        return;
    }
    const int64_t t0 = hit.text_id == 0u ? 0 : static_cast<int64_t>(a.sentinels[hit.text_id - 1u]) + 1;
    const int64_t t_len = static_cast<int64_t>(a.sentinels[hit.text_id]) - t0;
    const int64_t k = a.max_edits, lo = a.min_insert, hi = a.max_insert, len = L;
    int64_t ylo, yhi;
    if (strand_a == 0u) {  // the rescued mate is the reverse one: its right end is y
        const int64_t diag_a = static_cast<int64_t>(hit.position) - static_cast<int64_t>(wb);
        ylo = diag_a + lo;
        yhi = diag_a + hi;
    } else {               // the forward one: its diagonal is y - L
        const int64_t right_a = a.end[anchor * a.mate_slots + slot];
        ylo = right_a - hi + len;
        yhi = right_a - lo + len;
    }
    const int64_t x0 = clamp64(ylo - len - k, 0, t_len), x1 = clamp64(yhi, 0, t_len);
    const uint32_t nb = kUniform ? static_cast<uint32_t>(W) : (L + 63u) >> 6;

    // read side: the bit planes of block w, rows 64 w .. 64 w + 63
    uint64_t lo_p[W], hi_p[W], valid[W], Pv[W], Mv[W];
#pragma unroll
    for (int w = 0; w < W; w++) {
        lo_p[w] = hi_p[w] = valid[w] = 0;
        Pv[w] = ~0ull;
        Mv[w] = 0;
#pragma unroll
        for (uint32_t half = 0; half < 2; half++) {
            const uint32_t j0 = 64u * w + 32u * half;
            if (j0 < L) {
                const uint32_t n_c = L - j0 < 32u ? L - j0 : 32u;
                uint64_t qc;
                uint32_t inv;
                read_chunk<kXlate>(a, s_dense, begin + j0, n_c, qc, inv);
                const uint32_t c_lo = static_cast<uint32_t>(qc), c_hi = static_cast<uint32_t>(qc >> 32);
                const uint64_t p_lo = even_bits(c_lo) | (even_bits(c_hi) << 16);
                const uint64_t p_hi = even_bits(c_lo >> 1) | (even_bits(c_hi >> 1) << 16);
                const uint64_t ok = ~inv & low_bits(n_c);
                lo_p[w] |= p_lo << (32u * half);
                hi_p[w] |= p_hi << (32u * half);
                valid[w] |= ok << (32u * half);
            }
        }
    }

    // column x0, in front of any text symbol: D[L][x0] = L competes when x0 is admissible
    uint32_t score = L, best = GDX_EDIT_INVALID;
    uint32_t best_end = GDX_EDIT_NO_END;
    if (x0 >= ylo && x0 <= yhi) {
        best = L;
        best_end = static_cast<uint32_t>(x0);
    }
    if (L != 0u && x0 < x1) {  // (L == 0: every score is 0 and the least admissible y wins, below)
        const uint32_t top_last = (L - 1u) & 63u;
        // text side.  Every column is a symbol of the text itself, so its unit exists (kTextPadUnits in front)
        uint64_t g = static_cast<uint64_t>(t0 + x0 + 32 * static_cast<int64_t>(kTextPadUnits));
        u32x4 u = a.text_units[g >> 5];
        uint64_t codes = (static_cast<uint64_t>(u.x) | (static_cast<uint64_t>(u.y) << 32)) >> (2u * (g & 31u));
        uint32_t mask = u.z >> (g & 31u);
        for (int64_t y = x0; y < x1; y++) {  // (at most max_insert - min_insert + L + k columns: x1 <= yhi, x0 >= ylo - L - k)
            const uint64_t clo = 0ull - (codes & 1u), chi = 0ull - ((codes >> 1) & 1u);
            const uint64_t keep = static_cast<uint64_t>(mask & 1u) - 1ull;  // 0 when the text symbol is not one of 1..4
            int hin = 0;
#pragma unroll
            for (int w = 0; w < W; w++) {
                if (static_cast<uint32_t>(w) < nb) {
                    const bool last = static_cast<uint32_t>(w) == nb - 1u;
                    const uint32_t top = last ? top_last : 63u;
                    uint64_t Eq = keep & valid[w] & ~(lo_p[w] ^ clo) & ~(hi_p[w] ^ chi);
                    const uint64_t Xv = Eq | Mv[w];
                    if (hin < 0) Eq |= 1u;
                    const uint64_t Xh = (((Eq & Pv[w]) + Pv[w]) ^ Pv[w]) | Eq;
                    uint64_t Ph = Mv[w] | ~(Xh | Pv[w]);
                    uint64_t Mh = Pv[w] & Xh;
                    const int hout = static_cast<int>((Ph >> top) & 1u) - static_cast<int>((Mh >> top) & 1u);
                    Ph <<= 1;
                    Mh <<= 1;
                    if (hin < 0) Mh |= 1u;
                    else if (hin > 0) Ph |= 1u;
                    Pv[w] = Mh | ~(Xv | Ph);
                    Mv[w] = Ph & Xv;
                    hin = hout;
                    if (last) score += static_cast<uint32_t>(hout);
                }
            }
            if (y + 1 >= ylo && score < best) {  // strict: the leftmost end wins (y + 1 <= x1 <= yhi)
                best = score;
                best_end = static_cast<uint32_t>(y + 1);
            }
            g++;
            if ((g & 31u) != 0u) {
                codes >>= 2;
                mask >>= 1;
            } else if (y + 1 < x1) {
                u = a.text_units[g >> 5];
                codes = static_cast<uint64_t>(u.x) | (static_cast<uint64_t>(u.y) << 32);
                mask = u.z;
            }
        }
    } else if (L == 0u && best == GDX_EDIT_INVALID && ylo <= x1 && ylo > x0) {
        best = 0;  // (x0 < ylo <= x1: the admissible range begins inside the window)
        best_end = static_cast<uint32_t>(ylo);
    }
    const bool within = best <= a.max_edits;
    a.resc_dist[mate] = within ? best : a.max_edits + 1u;
    a.resc_end[mate] = within ? best_end : GDX_EDIT_NO_END;
}

// pair p after its attempts: the three words of the pair and the two winners
template <bool kUniform>
__device__ __forceinline__ void merge_pair(const RescueArgs &a, uint64_t p)
{
    const uint32_t k = a.max_edits;
    const bool open = a.n_proper[p] == 0u;
    uint32_t wq[2], wb[2], sl[2], rd[2];
    gdx_hit32_t wh[2];
#pragma unroll
    for (uint32_t s = 0; s < 2; s++) {
        wq[s] = a.win_query[2 * p + s];
        wb[s] = a.win_begin[2 * p + s];
        wh[s] = a.win_hits[2 * p + s];
        sl[s] = a.mate_slot[2 * p + s];
    }
    uint32_t pick = GDX_RESCUE_NONE, score = 2u * k + 2u;
#pragma unroll
    for (uint32_t o = 0; o < 2; o++) {  // (o ascending and a strict comparison: the least (score, o))
        rd[o] = open && sl[1u - o] != GDX_PAIR_NONE ? a.resc_dist[2 * p + o] : GDX_RESCUE_NOT_TRIED;
        if (rd[o] <= k) {
            const uint32_t s = a.mate_dist[2 * p + (1u - o)] + rd[o];
            if (pick == GDX_RESCUE_NONE || s < score) {
                pick = o;
                score = s;
            }
        }
    }
    uint32_t span = 0;
    if (pick != GDX_RESCUE_NONE) {
        // (the anchor by selects, not by wq[1 - pick]: arrays indexed by a value of the lane's go to LDS or scratch)
        const bool one = pick == 1u;  // the rescued mate is mate 1, the anchor mate 0
        const uint32_t a_wq = one ? wq[0] : wq[1], a_wb = one ? wb[0] : wb[1], a_sl = one ? sl[0] : sl[1];
        const gdx_hit32_t a_wh = one ? wh[0] : wh[1];
        const uint32_t strand_a = a_wq & 1u;
        const uint64_t rq = 4 * p + 2u * pick + (1u - strand_a);
        const int64_t L = kUniform ? static_cast<int64_t>(a.uniform_len) : static_cast<int64_t>(a.qoff[rq + 1] - a.qoff[rq]);
        const int64_t y = a.resc_end[2 * p + pick];
        if (strand_a == 0u) {
            span = static_cast<uint32_t>(y - (static_cast<int64_t>(a_wh.position) - static_cast<int64_t>(a_wb)));
        } else {
            const int64_t right_a = a.end[(2 * p + (1u - pick)) * a.mate_slots + a_sl];
            span = static_cast<uint32_t>(right_a - (y - L));
        }
        const uint32_t r_wb = y < L ? static_cast<uint32_t>(L - y) : 0u, r_pos = y > L ? static_cast<uint32_t>(y - L) : 0u;
#pragma unroll
        for (uint32_t s = 0; s < 2; s++) {
            if (s == pick) {
                wq[s] = static_cast<uint32_t>(rq);
                wb[s] = r_wb;
                wh[s].text_id = a_wh.text_id;
                wh[s].position = r_pos;
            }
        }
    }
    a.resc_mate[p] = pick;
    a.resc_pair_dist[p] = score;
    a.resc_span[p] = span;
#pragma unroll
    for (uint32_t s = 0; s < 2; s++) {
        a.out_win_query[2 * p + s] = wq[s];
        a.out_win_begin[2 * p + s] = wb[s];
        a.out_win_hits[2 * p + s] = wh[s];
    }
}

template <int kXlate, bool kUniform, int W>
__global__ __launch_bounds__(kBlock) void rescue_kernel(const RescueArgs a)
{
    __shared__ uint8_t s_dense[256];
    __shared__ uint32_t s_ring[kRing];
    __shared__ uint32_t s_total[kBlock / kWave];
    load_dense_table<kXlate, kBlock>(s_dense, a.io_to_dense);
    const uint32_t t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    const uint64_t below = (1ull << lane) - 1ull;

    for (uint64_t tile0 = static_cast<uint64_t>(blockIdx.x) * a.tile_pairs; tile0 < a.n_pairs;
         tile0 += static_cast<uint64_t>(gridDim.x) * a.tile_pairs) {  // (uniform in the workgroup: every lane meets the barriers)
        const uint64_t tile1 = a.n_pairs - tile0 < a.tile_pairs ? a.n_pairs : tile0 + a.tile_pairs;
        uint32_t head = 0, tail = 0;  // attempts taken from and put into the ring so far (uniform; a tile has fewer than 2^32)
        for (uint64_t c0 = tile0; c0 < tile1; c0 += kBlock) {
            // 1. sweep
            const uint64_t p = c0 + t;
            bool f0 = false, f1 = false;
            if (p < tile1) {
                const bool open = a.n_proper[p] == 0u;
                f0 = open && a.mate_slot[2 * p + 1] != GDX_PAIR_NONE;  // mate 0 is searched from mate 1
                f1 = open && a.mate_slot[2 * p] != GDX_PAIR_NONE;
                if (!f0) {
                    a.resc_dist[2 * p] = GDX_RESCUE_NOT_TRIED;
                    a.resc_end[2 * p] = GDX_EDIT_NO_END;
                }
                if (!f1) {
                    a.resc_dist[2 * p + 1] = GDX_RESCUE_NOT_TRIED;
                    a.resc_end[2 * p + 1] = GDX_EDIT_NO_END;
                }
            }
            const uint64_t b0 = __ballot(f0), b1 = __ballot(f1);
            if (lane == 0) s_total[wave] = __popcll(b0) + __popcll(b1);
            __syncthreads();  // (also: every lane has left the rounds of the sweep before, whose ring entries may be overwritten now)
            uint32_t at = tail + __popcll(b0 & below) + __popcll(b1 & below), all = 0;
#pragma unroll
            for (uint32_t w = 0; w < kBlock / kWave; w++) {
                const uint32_t n = s_total[w];
                if (w < wave) at += n;
                all += n;
            }
            const uint32_t local = static_cast<uint32_t>(2 * (p - tile0));  // (below 2^32: launch_mate_rescue caps the tile)
            if (f0) s_ring[at++ & (kRing - 1)] = local;
            if (f1) s_ring[at & (kRing - 1)] = local + 1u;
            tail += all;
            __syncthreads();
            // 2. drain: full rounds, and at the end of the tile what is left
            const bool last_sweep = c0 + kBlock >= tile1;
            while (tail - head >= static_cast<uint32_t>(kBlock) || (last_sweep && tail != head)) {
                if (t < tail - head) rescue_lane<kXlate, kUniform, W>(a, s_dense, 2 * tile0 + s_ring[(head + t) & (kRing - 1)]);
                head += tail - head < static_cast<uint32_t>(kBlock) ? tail - head : static_cast<uint32_t>(kBlock);
            }
        }
        // 3. merge: the stores of the rounds are the workgroup's own; the barrier orders them before these loads
        __syncthreads();
        for (uint64_t p = tile0 + t; p < tile1; p += kBlock) merge_pair<kUniform>(a, p);
    }
}

template <int kXlate>
void launch_xlate(const RescueArgs &a, unsigned grid, hipStream_t stream)
{
    dispatch_blocks(a.uniform_len, [&](auto uniform, auto w) {
        hipLaunchKernelGGL((rescue_kernel<kXlate, decltype(uniform)::value, decltype(w)::value>), dim3(grid), dim3(kBlock), 0, stream, a);
    });
}

}  // namespace

void set_rescue_tiling(uint64_t tile_pairs, uint64_t grid)
{
    g_tile_pairs.store(tile_pairs);
    g_grid.store(grid);
}

void launch_mate_rescue(const IndexView &ix, const uint8_t *d_qbuf, const uint64_t *d_qoff, bool packed, uint32_t uniform_len,
                        const RescueCall &call, hipStream_t stream)
{
    if (call.n_pairs == 0) return;
    RescueArgs a;
    static_cast<RescueCall &>(a) = call;
    fill_verify_args(a, ix, d_qbuf, d_qoff, 4 * a.n_pairs, uniform_len, nullptr, nullptr, nullptr, 0);
    // a tile is a whole number of sweeps; by default the batch is cut into as many tiles as the grid has workgroups
    constexpr uint64_t kMaxTile = 1ull << 30;  // (twice a tile's pairs number its mates in 32 bits)
    uint64_t tile = g_tile_pairs.load();
    if (tile == 0) {
        tile = (a.n_pairs + kMaxGrid - 1) / kMaxGrid;
        if (tile < kMinTile) tile = kMinTile;
    }
    tile = (tile + kBlock - 1) / kBlock * kBlock;
    if (tile > kMaxTile) tile = kMaxTile;
    const uint64_t n_tiles = (a.n_pairs + tile - 1) / tile;
    uint64_t grid = g_grid.load();
    if (grid == 0 || grid > kMaxGrid) grid = kMaxGrid;
    if (grid > n_tiles) grid = n_tiles;
    a.tile_pairs = tile;
    if (packed) launch_xlate<2>(a, static_cast<unsigned>(grid), stream);
    else if (ix.perm_ok) launch_xlate<1>(a, static_cast<unsigned>(grid), stream);
    else launch_xlate<0>(a, static_cast<unsigned>(grid), stream);
}

}  // namespace gdx
