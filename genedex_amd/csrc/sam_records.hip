// sam_records.hip -- the text output behind the mapping chain: one SAM record per read, made on the device from the winners, the
// outputs of gdx_align_many_dev and the text units (gdx_sam_records_many[_dev]; the definition of a record is in
// include/gdx_experimental.h "SAM records").
//
//   emit_record<Sink>   THE record, written once: every field goes through a sink.  CountSink counts the bytes, LdsSink writes
//                       them into the workgroup's tile, GlobalSink (a record larger than a tile) straight into `out`.  The long
//                       copies -- a given QNAME and SEQ -- are not written by the lane: a writing sink leaves room and notes a copy
//                       job (source, destination, length).  Lengths and bytes cannot disagree: they are the same code, except
//                       for MD, whose length has a closed form per run (md_count) beside the symbol loop (md_write).
//   1. sam_lengths_kernel
//                       a lane per record, workgroups of 256 consecutive records: the lane resolves its read (mapped, bad,
//                       strand) and in paired mode its mate, counts its record, stores the flags byte (workspace) and the status;
//                       the workgroup scans its 256 lengths in LDS: rec_off[r] = the bytes of the workgroup's records before r,
//                       tile_sums[workgroup] = all of them.
//   2. sam_scan_kernel  ONE workgroup scans the tile sums in place (exclusive) and stores rec_off[n_reads];
//      sam_offsets_kernel adds a workgroup's base to its 256 entries of rec_off.
//   3. sam_fill_kernel  `out` is cut into TILES of tile_bytes (a multiple of 16; 4 KiB) on 16-byte borders of its ADDRESS.  A
//                       record belongs to the tile its first byte lies in, so a tile's records are consecutive and contiguous
//                       in `out`.  A workgroup is ONE wavefront and takes a run of consecutive tiles: one binary search in
//                       rec_off for its first record, then a tile's records end where a look ahead from the tile before says
//                       (a load per 64 records).  The tile buffer in LDS holds two tiles: a record that begins in the tile
//                       and ends inside the buffer is staged, and only a record LONGER than a tile can fail that -- it is then
//                       the tile's last record and takes the slow path.  Per pass of 64 records: a lane formats its record's
//                       short fields into the buffer (ds_write_b8), then the wavefront takes the pass's copy jobs four at a
//                       time, sixteen lanes on each: 16-byte loads from the aligned part of the source, byte loads at its two ends.  Then the
//                       buffer leaves LDS: 16 bytes per lane, consecutive lanes consecutive addresses, from the first 16-byte
//                       border to the last; byte stores only in front of and behind them.
//                       Slow path: the record's lane writes the short fields byte by byte into `out`, the wavefront copies
//                       QNAME and SEQ with a byte per lane.
//                       Why one wavefront and 4 KiB: a lane's formatting is a chain of dependent loads (its fields, its offsets,
//                       its CIGAR words, its text units), so the fill's time follows the wavefronts a CU has formatting at once,
//                       not the bytes.  Measured (profiles/r23/sam_records.md): 7.0 ms for 10 M reads of 150 symbols against
//                       0.9 ms for a copy of the same bytes, 2.8 ms of it per tile and 4.2 ms per record.
// Nothing depends on tile_bytes or the grid (gdx_debug_set_sam_tiling).  A record that does not fit whole below out_capacity, and
// everything behind it, is left out by cutting the record range, not by testing bytes.  Every store is a plain C++ store.
// LDS of the fill: 8 KiB buffer + 2 KiB jobs.  The tiles are dealt out in equal runs; their number is read from rec_off on the device.
#include <atomic>
#include <cstring>
#include <functional>
#include <vector>

#include "../../include/gdx_experimental.h"
#include "common.hpp"
#include "fm_index.hpp"
#include "kernels.hpp"

namespace gdx {

namespace {

constexpr int kBlock = 256;
constexpr int kFill = 64;              // lanes of a workgroup of the fill: one wavefront
constexpr uint32_t kTileMax = 4096;    // bytes of a tile at the most; the buffer holds two
constexpr uint32_t kTileMin = 64;
constexpr uint32_t kMaxGrid = 8192;
constexpr uint32_t kFlagMapped = 1u, kFlagBad = 2u, kFlagStrand = 4u;

std::atomic<uint32_t> g_tile_bytes{0}, g_grid{0};

struct SamArgs {
    const u32x4 *text_units;
    const uint32_t *sentinels;
    uint32_t n_texts;
    uint32_t uniform_len;  // 0: qoff
    const uint8_t *qbuf;
    const uint64_t *qoff;
    uint64_t n_reads;
    uint32_t strands, paired, stride, tile_bytes;
    const uint32_t *win_query;
    const gdx_hit32_t *win_hits;
    const uint32_t *dist, *begin, *end, *n_cigar, *cigar, *mapq, *proper;
    const uint8_t *names, *text_names;
    const uint64_t *name_off, *text_name_off;
    uint4 tab;  // dense_to_io[0 .. 15], byte c of the 16
    uint64_t *tile_sums;
    uint8_t *flags;
    uint64_t *rec_off;
    uint8_t *out;
    uint64_t out_capacity;
    uint8_t *status;
};

// mapped / bad / strand of read r from the inputs alone (the rule of the header)
__device__ __forceinline__ uint32_t resolve_read(const SamArgs &a, uint64_t r)
{
    const uint32_t wq = a.win_query[r];
    if (wq == GDX_CAND_NONE) return 0u;
    const uint64_t lo = r * a.strands;
    const uint32_t nc = a.n_cigar[r];
    if (wq < lo || wq >= lo + a.strands || a.win_hits[r].text_id >= a.n_texts || nc > a.stride) return kFlagBad;
    if (a.end[r] == GDX_EDIT_NO_END) return 0u;
    uint64_t sum = 0;
    const uint32_t *cigar = a.cigar + r * a.stride;
    for (uint32_t w = 0; w < nc; w++) sum += cigar[w] >> 4;
    if (sum > GDX_SAM_MAX_RUN_SUM) return kFlagBad;
    return kFlagMapped | (wq != lo ? kFlagStrand : 0u);
}

// ---- sinks ----
struct CountSink {
    static constexpr bool kCount = true;
    uint64_t n = 0;
    __device__ __forceinline__ void put(uint32_t) { n++; }
    __device__ __forceinline__ void job(uint32_t, const uint8_t *, uint64_t len) { n += len; }
};

// the tile buffer: positions below `limit` only (the record's own end: a guard, never met when lengths and bytes agree)
struct LdsSink {
    static constexpr bool kCount = false;
    uint8_t *tile;
    uint64_t *job_src;
    uint32_t *job_dst, *job_len;  // the lane's two slots
    uint32_t pos, limit;
    __device__ __forceinline__ void put(uint32_t c)
    {
        if (pos < limit) tile[pos] = static_cast<uint8_t>(c);
        pos++;
    }
    __device__ __forceinline__ void job(uint32_t slot, const uint8_t *src, uint64_t len)
    {
        const uint32_t room = pos < limit ? limit - pos : 0u;
        job_src[slot] = reinterpret_cast<uint64_t>(src);
        job_dst[slot] = pos;
        job_len[slot] = len < room ? static_cast<uint32_t>(len) : room;
        pos += static_cast<uint32_t>(len);
    }
};

struct GlobalSink {
    static constexpr bool kCount = false;
    uint8_t *out;
    uint64_t *slow_src, *slow_dst, *slow_len;  // two slots of the workgroup
    uint64_t pos, limit;
    __device__ __forceinline__ void put(uint32_t c)
    {
        if (pos < limit) out[pos] = static_cast<uint8_t>(c);
        pos++;
    }
    __device__ __forceinline__ void job(uint32_t slot, const uint8_t *src, uint64_t len)
    {
        const uint64_t room = pos < limit ? limit - pos : 0u;
        slow_src[slot] = reinterpret_cast<uint64_t>(src);
        slow_dst[slot] = pos;
        slow_len[slot] = len < room ? len : room;
        pos += len;
    }
};

// decimal, no padding.  The powers are compile-time constants: a division each, no digit buffer (no scratch)
template <class S>
__device__ __forceinline__ void dec32(S &s, uint32_t v)
{
    bool started = false;
#pragma unroll
    for (uint32_t p = 1000000000u; p >= 10u; p /= 10u) {
        if (started || v >= p) {
            const uint32_t d = v / p;
            v -= d * p;
            s.put('0' + d);
            started = true;
        }
    }
    s.put('0' + v);
}

// v < 10^18
template <class S>
__device__ __forceinline__ void dec64(S &s, uint64_t v)
{
    if (v < 1000000000ull) return dec32(s, static_cast<uint32_t>(v));
    const uint64_t hi = v / 1000000000ull;
    uint32_t lo = static_cast<uint32_t>(v - hi * 1000000000ull);
    dec32(s, static_cast<uint32_t>(hi));
#pragma unroll
    for (uint32_t p = 100000000u; p >= 1u; p /= 10u) {
        const uint32_t d = lo / p;
        lo -= d * p;
        s.put('0' + d);
    }
}

__device__ __forceinline__ uint32_t digits32(uint32_t v)
{
    uint32_t n = 1;
#pragma unroll
    for (uint64_t p = 10u; p <= 1000000000ull; p *= 10u) n += v >= p ? 1u : 0u;
    return n;
}

template <class S>
__device__ __forceinline__ void text_name(S &s, const SamArgs &a, uint32_t text_id)
{
    if (a.text_names == nullptr) return dec32(s, text_id);
    const uint64_t b = a.text_name_off[text_id], e = a.text_name_off[text_id + 1];
    if constexpr (S::kCount) {
        s.job(0, nullptr, e - b);
    } else {
        for (uint64_t i = b; i < e; i++) s.put(a.text_names[i]);
    }
}

// MD of a mapped read: its length in closed form per run ...
__device__ __forceinline__ uint64_t md_count(const uint32_t *cigar, uint32_t nc)
{
    uint64_t bytes = 0;
    uint32_t n = 0;
    for (uint32_t w = 0; w < nc; w++) {
        const uint32_t op = cigar[w] & 15u, l = cigar[w] >> 4;
        if (l == 0u) continue;
        if (op == GDX_CIGAR_EQ) {
            n += l;
        } else if (op == GDX_CIGAR_DIFF) {
            bytes += digits32(n) + 1u + 2ull * (l - 1u);  // n and a symbol, then "0" and a symbol for each further one
            n = 0;
        } else if (op == GDX_CIGAR_DEL) {
            bytes += digits32(n) + 1u + l;
            n = 0;
        }
    }
    return bytes + digits32(n);
}

// ... and its bytes.  One text unit stays in registers while y stays inside it
template <class S>
__device__ __forceinline__ void md_write(S &s, const SamArgs &a, const uint32_t *cigar, uint32_t nc, uint32_t text_id, uint32_t begin)
{
    const uint64_t t0 = text_id == 0u ? 0u : static_cast<uint64_t>(a.sentinels[text_id - 1u]) + 1u;
    const uint64_t t_len = static_cast<uint64_t>(a.sentinels[text_id]) - t0;
    const uint64_t g0 = t0 + 32u * static_cast<uint64_t>(kTextPadUnits);
    uint64_t cur = ~0ull, y = begin;
    u32x4 u = {0u, 0u, 0u, 0u};
    auto symbol = [&](uint64_t at) -> uint32_t {
        if (at >= t_len) return '?';  // (nothing outside the text's own units is read)
        const uint64_t g = g0 + at;
        if ((g >> 5) != cur) {
            cur = g >> 5;
            u = a.text_units[cur];
        }
        const uint32_t bit = static_cast<uint32_t>(g & 31u);
        const uint64_t codes = static_cast<uint64_t>(u.x) | (static_cast<uint64_t>(u.y) << 32);
        const uint32_t code = ((u.z >> bit) & 1u) != 0u ? 0u : 1u + static_cast<uint32_t>((codes >> (2u * bit)) & 3u);
        return ((code < 4u ? a.tab.x >> (8u * code) : a.tab.y) & 0xffu);
    };
    uint32_t n = 0;
    for (uint32_t w = 0; w < nc; w++) {
        const uint32_t op = cigar[w] & 15u, l = cigar[w] >> 4;
        if (l == 0u) continue;
        if (op == GDX_CIGAR_EQ) {
            n += l;
            y += l;
        } else if (op == GDX_CIGAR_DIFF) {
            for (uint32_t i = 0; i < l; i++) {
                dec32(s, n);
                s.put(symbol(y++));
                n = 0;
            }
        } else if (op == GDX_CIGAR_DEL) {
            dec32(s, n);
            s.put('^');
            for (uint32_t i = 0; i < l; i++) s.put(symbol(y++));
            n = 0;
        }
    }
    dec32(s, n);
}

// record r through the sink; fl / fl_m: the flags bytes of r and of its mate (fl_m: 0 in single mode)
template <class S>
__device__ __forceinline__ void emit_record(S &s, const SamArgs &a, uint64_t r, uint32_t fl, uint32_t fl_m)
{
    const bool mapped = (fl & kFlagMapped) != 0u, m_mapped = a.paired != 0u && (fl_m & kFlagMapped) != 0u;
    const uint64_t m = r ^ 1u;
    uint32_t tid = 0, b = 0, e = 0, nc = 0, tid_m = 0, b_m = 0, e_m = 0;
    if (mapped) {
        tid = a.win_hits[r].text_id;
        b = a.begin[r];
        e = a.end[r];
        nc = a.n_cigar[r];
    }
    if (m_mapped) {
        tid_m = a.win_hits[m].text_id;
        b_m = a.begin[m];
        e_m = a.end[m];
    }
    const uint32_t *cigar = a.cigar + r * a.stride;
    // QNAME
    if (a.names != nullptr) {
        const uint64_t n0 = a.name_off[r];
        s.job(0, a.names + n0, a.name_off[r + 1] - n0);
    } else {
        dec32(s, static_cast<uint32_t>(a.paired != 0u ? r >> 1 : r));
        if constexpr (!S::kCount) s.job(0, nullptr, 0);
    }
    s.put('\t');
    // FLAG
    uint32_t flag = 0;
    if (a.paired != 0u) {
        flag = 0x1u | ((r & 1u) != 0u ? 0x80u : 0x40u);
        if (mapped && m_mapped && a.proper != nullptr && a.proper[r >> 1] != 0u) flag |= 0x2u;
        if (!m_mapped) flag |= 0x8u;
        if (m_mapped && (fl_m & kFlagStrand) != 0u) flag |= 0x20u;
    }
    if (!mapped) flag |= 0x4u;
    if (mapped && (fl & kFlagStrand) != 0u) flag |= 0x10u;
    dec32(s, flag);
    s.put('\t');
    // RNAME, POS, MAPQ
    if (mapped) text_name(s, a, tid);
    else s.put('*');
    s.put('\t');
    dec64(s, mapped ? static_cast<uint64_t>(b) + 1u : 0u);
    s.put('\t');
    uint32_t q = 0;
    if (mapped) {
        q = a.mapq[r];
        if (q > 255u) q = 255u;
    }
    dec32(s, q);
    s.put('\t');
    // CIGAR
    if (nc == 0u) {
        s.put('*');
    } else {
        for (uint32_t w = 0; w < nc; w++) {
            const uint32_t op = cigar[w] & 15u;
            dec32(s, cigar[w] >> 4);
            s.put(op < 8u ? static_cast<uint32_t>(0x3D5048534E44494Dull >> (8u * op)) & 0xffu : (op == 8u ? 'X' : '?'));  // "MIDNSHP=" 'X'
        }
    }
    s.put('\t');
    // RNEXT, PNEXT, TLEN
    const bool together = mapped && m_mapped && tid == tid_m;
    if (!m_mapped) s.put('*');
    else if (together) s.put('=');
    else text_name(s, a, tid_m);
    s.put('\t');
    dec64(s, m_mapped ? static_cast<uint64_t>(b_m) + 1u : 0u);
    s.put('\t');
    if (together) {
        const int64_t span = static_cast<int64_t>(e > e_m ? e : e_m) - static_cast<int64_t>(b < b_m ? b : b_m);
        const bool left = b < b_m || (b == b_m && (r & 1u) == 0u);
        int64_t v = left ? span : -span;
        if (v < 0) {
            s.put('-');
            v = -v;
        }
        dec64(s, static_cast<uint64_t>(v));
    } else {
        s.put('0');
    }
    s.put('\t');
    // SEQ
    {
        const uint64_t qn = mapped ? a.win_query[r] : r * a.strands;
        uint64_t q0, len;
        if (a.uniform_len != 0u) {
            q0 = qn * a.uniform_len;
            len = a.uniform_len;
        } else {
            q0 = a.qoff[qn];
            len = a.qoff[qn + 1] - q0;
        }
        if (len == 0u) s.put('*');
        s.job(1, a.qbuf + q0, len);
    }
    s.put('\t');
    s.put('*');  // QUAL
    if (mapped) {
        s.put('\t');
        s.put('N');
        s.put('M');
        s.put(':');
        s.put('i');
        s.put(':');
        dec32(s, a.dist[r]);
        s.put('\t');
        s.put('M');
        s.put('D');
        s.put(':');
        s.put('Z');
        s.put(':');
        if constexpr (S::kCount) s.job(0, nullptr, md_count(cigar, nc));
        else md_write(s, a, cigar, nc, tid, b);
    }
    s.put('\n');
}

// ---- 1. lengths ----
__global__ __launch_bounds__(kBlock) void sam_lengths_kernel(const SamArgs a)
{
    __shared__ uint64_t s_scan[kBlock];
    const uint32_t t = threadIdx.x;
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * kBlock + t;
    uint64_t len = 0;
    if (r < a.n_reads) {
        const uint32_t fl = resolve_read(a, r);
        const uint32_t fl_m = a.paired != 0u ? resolve_read(a, r ^ 1u) : 0u;
        a.flags[r] = static_cast<uint8_t>(fl);
        if (a.status != nullptr) a.status[r] = (fl & kFlagBad) != 0u ? GDX_SAM_BAD_RECORD : 0;
        CountSink s;
        emit_record(s, a, r, fl, fl_m);
        len = s.n;
    }
    // inclusive scan over the workgroup
    s_scan[t] = len;
    __syncthreads();
#pragma unroll
    for (uint32_t d = 1; d < kBlock; d <<= 1) {
        const uint64_t add = t >= d ? s_scan[t - d] : 0u;
        __syncthreads();
        s_scan[t] += add;
        __syncthreads();
    }
    if (r < a.n_reads) a.rec_off[r] = s_scan[t] - len;
    if (t == kBlock - 1) a.tile_sums[blockIdx.x] = s_scan[t];
}

// ---- 2. scan of the workgroup sums, in place and exclusive; rec_off[n_reads] = the total ----
__global__ __launch_bounds__(kBlock) void sam_scan_kernel(uint64_t *sums, uint64_t n_sums, uint64_t *total)
{
    __shared__ uint64_t s_scan[kBlock];
    const uint32_t t = threadIdx.x;
    uint64_t carry = 0;
    for (uint64_t c0 = 0; c0 < n_sums; c0 += kBlock) {  // (uniform)
        const uint64_t v = c0 + t < n_sums ? sums[c0 + t] : 0u;
        s_scan[t] = v;
        __syncthreads();
#pragma unroll
        for (uint32_t d = 1; d < kBlock; d <<= 1) {
            const uint64_t add = t >= d ? s_scan[t - d] : 0u;
            __syncthreads();
            s_scan[t] += add;
            __syncthreads();
        }
        if (c0 + t < n_sums) sums[c0 + t] = carry + s_scan[t] - v;
        carry += s_scan[kBlock - 1];
        __syncthreads();
    }
    if (t == 0) *total = carry;
}

__global__ __launch_bounds__(kBlock) void sam_offsets_kernel(uint64_t *rec_off, uint64_t n_reads, const uint64_t *sums)
{
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (r < n_reads) rec_off[r] += sums[blockIdx.x];
}

// ---- 3. fill ----
// the first i in [0, n] with off[i] + shift >= v (off ascending)
__device__ __forceinline__ uint64_t first_at_least(const uint64_t *off, uint64_t n, uint64_t shift, uint64_t v)
{
    uint64_t lo = 0, hi = n;  // the answer lies in [lo, hi]; hi = n when no entry below n qualifies
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] + shift >= v) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(kFill) void sam_fill_kernel(const SamArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[2 * kTileMax];
    __shared__ uint64_t s_job_src[2 * kFill];
    __shared__ uint32_t s_job_dst[2 * kFill], s_job_len[2 * kFill];
    __shared__ uint64_t s_slow_src[2], s_slow_dst[2], s_slow_len[2];
    const uint32_t t = threadIdx.x;  // (the workgroup is one wavefront: ballots count over it)
    const uint64_t T = a.tile_bytes, A = reinterpret_cast<uint64_t>(a.out) & 15u, n = a.n_reads;
    // the records that fit whole: [0, n_fit), rec_off[n_fit] <= out_capacity
    uint64_t n_fit;
    {
        uint64_t lo = 0, hi = n;  // the largest i with rec_off[i] <= capacity (rec_off[0] = 0)
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo + 1) >> 1);
            if (a.rec_off[mid] <= a.out_capacity) lo = mid;
            else hi = mid - 1;
        }
        n_fit = lo;
    }
    if (n_fit == 0) return;
    // this workgroup's run of consecutive tiles: one binary search for its first record, then every tile's records end where
    // a forward look from the tile before says (a load per 64 records instead of a search per tile)
    const uint64_t n_tiles = (a.rec_off[n_fit] + A + T - 1) / T, per = (n_tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t tile_lo = blockIdx.x * per, tile_hi = tile_lo + per < n_tiles ? tile_lo + per : n_tiles;
    if (tile_lo >= tile_hi) return;
    uint64_t next = first_at_least(a.rec_off, n_fit, A, tile_lo * T);
    for (uint64_t tile = tile_lo; tile < tile_hi; tile++) {  // (everything up to the passes is uniform)
        const uint64_t i0 = next, bound = (tile + 1) * T;
        uint64_t i1 = i0;
        for (;;) {
            const uint64_t idx = i1 + t;
            const uint32_t cnt = __popcll(__ballot(idx < n_fit && a.rec_off[idx] + A < bound));  // (ascending: the set lanes come first)
            i1 += cnt;
            if (cnt < static_cast<uint32_t>(kFill)) break;
        }
        next = i1;
        if (i0 >= i1) continue;
        // position p of the buffer is byte p - A + tile * T of out; out + that is 16-byte aligned when p is
        const uint64_t shift = tile * T - A;  // (wraps for tile 0 with A != 0: only sums with it are used)
        const uint64_t last_off = a.rec_off[i1 - 1], end_off = a.rec_off[i1];
        const bool slow = end_off - shift > 2 * T;  // the last record ends beyond the buffer: longer than a tile
        for (uint64_t c0 = i0; c0 < i1; c0 += kFill) {
            const uint64_t i = c0 + t;
            s_job_len[2 * t] = 0;
            s_job_len[2 * t + 1] = 0;
            if (i < i1) {
                const uint64_t off = a.rec_off[i], nxt = a.rec_off[i + 1];
                const uint32_t fl = a.flags[i], fl_m = a.paired != 0u ? a.flags[i ^ 1u] : 0u;
                if (slow && i == i1 - 1) {
                    GlobalSink s{a.out, s_slow_src, s_slow_dst, s_slow_len, off, nxt};
                    emit_record(s, a, i, fl, fl_m);
                } else {
                    LdsSink s{s_tile, s_job_src + 2 * t, s_job_dst + 2 * t, s_job_len + 2 * t, static_cast<uint32_t>(off - shift),
                              static_cast<uint32_t>(nxt - shift)};
                    emit_record(s, a, i, fl, fl_m);
                }
            }
            __syncthreads();
            // the copy jobs of the pass: four at a time, sixteen lanes on each (256 bytes a step: a read of 150 symbols is one step),
            // so that the loads of four jobs are in flight together
            const uint32_t n_jobs = 2u * static_cast<uint32_t>(i1 - c0 < kFill ? i1 - c0 : kFill);
            const uint32_t sub = t >> 4, l = t & 15u;
            for (uint32_t j = sub; j < n_jobs; j += kFill / 16) {
                const uint32_t len = s_job_len[j];
                if (len == 0u) continue;
                const uint8_t *src = reinterpret_cast<const uint8_t *>(s_job_src[j]);
                uint8_t *dst = s_tile + s_job_dst[j];
                uint32_t head = (16u - static_cast<uint32_t>(s_job_src[j] & 15u)) & 15u;
                if (head > len) head = len;
                const uint32_t body = (len - head) >> 4;
                if (l < head) dst[l] = src[l];
                const uint32_t at = s_job_dst[j] + head;  // (the widest LDS store the destination's alignment allows)
                for (uint32_t k = l; k < body; k += 16u) {
                    const u32x4 v = *reinterpret_cast<const u32x4 *>(src + head + 16u * k);
                    uint8_t *d = dst + head + 16u * k;
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                    if ((at & 15u) == 0u) {
                        *reinterpret_cast<u32x4 *>(d) = v;
                    } else if ((at & 3u) == 0u) {
#pragma unroll
                        for (uint32_t x = 0; x < 4; x++) reinterpret_cast<uint32_t *>(d)[x] = w[x];
                    } else {
#pragma unroll
                        for (uint32_t x = 0; x < 4; x++) {
#pragma unroll
                            for (uint32_t y = 0; y < 4; y++) d[4u * x + y] = static_cast<uint8_t>(w[x] >> (8u * y));
                        }
                    }
                }
                const uint32_t tail0 = head + 16u * body;
                if (tail0 + l < len) dst[tail0 + l] = src[tail0 + l];
            }
            __syncthreads();
        }
        // the buffer leaves LDS: [p0, p1)
        {
            const uint32_t p0 = static_cast<uint32_t>(a.rec_off[i0] - shift), p1 = static_cast<uint32_t>((slow ? last_off : end_off) - shift);
            uint8_t *g = a.out + shift;  // (g + p is inside out for every p in [p0, p1))
            uint32_t a0 = (p0 + 15u) & ~15u, a1 = p1 & ~15u;
            if (a0 >= a1) a0 = a1 = p1;  // no 16 bytes between two borders: bytes only
            for (uint32_t p = p0 + t; p < a0; p += kFill) g[p] = s_tile[p];
            for (uint32_t p = a0 + 16u * t; p < a1; p += 16u * kFill)
                *reinterpret_cast<u32x4 *>(g + p) = *reinterpret_cast<const u32x4 *>(s_tile + p);
            for (uint32_t p = a1 + t; p < p1; p += kFill) g[p] = s_tile[p];
        }
        if (slow) {  // (its jobs were noted before the pass's first barrier)
            for (uint32_t j = 0; j < 2; j++) {
                const uint8_t *src = reinterpret_cast<const uint8_t *>(s_slow_src[j]);
                uint8_t *dst = a.out + s_slow_dst[j];
                const uint64_t len = s_slow_len[j];
                for (uint64_t x = t; x < len; x += kFill) dst[x] = src[x];
            }
        }
        __syncthreads();  // the buffer and the job slots are free again
    }
}

uint64_t round_up(uint64_t v, uint64_t to) { return (v + to - 1) / to * to; }

uint64_t n_groups_of(uint64_t n_reads) { return div_ceil(n_reads ? n_reads : 1, static_cast<uint64_t>(kBlock)); }

}  // namespace

uint64_t sam_workspace_bytes(uint64_t n_reads)
{
    // the workgroup sums of the lengths pass, then a flags byte per read
    return round_up(n_groups_of(n_reads) * sizeof(uint64_t), 256) + round_up(n_reads ? n_reads : 1, 256);
}

namespace {
uint32_t digits_of(uint64_t v)
{
    uint32_t n = 1;
    while (v >= 10) {
        v /= 10;
        n++;
    }
    return n;
}
}  // namespace

uint64_t sam_record_bound(uint64_t max_read_len, uint64_t max_name_len, uint64_t max_text_name_len, uint32_t max_edits)
{
    const uint64_t qname = max_name_len > 10 ? max_name_len : 10, rname = max_text_name_len > 10 ? max_text_name_len : 10;
    const uint64_t k = max_edits, num = digits_of(max_read_len + k);  // a run length, a match counter: at most max_read_len + k
    const uint64_t cigar = (2 * k + 1) * (num + 1), md = (k + 1) * num + 2 * k;
    const uint64_t seq = max_read_len > 1 ? max_read_len : 1;
    // QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL, NM:i:<10> MD:Z:<md>, 12 tabs and the newline
    return qname + 4 + rname + 10 + 3 + cigar + rname + 10 + 11 + seq + 1 + 15 + 5 + md + 12 + 1;
}

void set_sam_tiling(uint32_t tile_bytes, uint32_t grid)
{
    g_tile_bytes.store(tile_bytes);
    g_grid.store(grid);
}

void launch_sam_records(const IndexView &ix, const SamCall &c, hipStream_t stream)
{
    SamArgs a;
    a.text_units = ix.text_units;
    a.sentinels = ix.sentinels;
    a.n_texts = ix.n_texts;
    a.uniform_len = c.uniform_len;
    a.qbuf = c.d_qbuf;
    a.qoff = c.uniform_len ? nullptr : c.d_qoff;
    a.n_reads = c.n_reads;
    a.strands = c.strands;
    a.paired = c.paired ? 1u : 0u;
    a.stride = 2u * c.max_edits + 1u;
    a.win_query = c.win_query;
    a.win_hits = c.win_hits;
    a.dist = c.dist;
    a.begin = c.begin;
    a.end = c.end;
    a.n_cigar = c.n_cigar;
    a.cigar = c.cigar;
    a.mapq = c.mapq;
    a.proper = c.proper;
    a.names = c.names;
    a.name_off = c.name_off;
    a.text_names = c.text_names;
    a.text_name_off = c.text_name_off;
    uint32_t tab[4];
    std::memcpy(tab, c.dense_to_io, 16);
    a.tab = make_uint4(tab[0], tab[1], tab[2], tab[3]);
    const uint64_t groups = n_groups_of(c.n_reads);
    a.tile_sums = static_cast<uint64_t *>(c.d_workspace);
    a.flags = static_cast<uint8_t *>(c.d_workspace) + round_up(groups * sizeof(uint64_t), 256);
    a.rec_off = c.rec_off;
    a.out = c.out;
    a.out_capacity = c.out_capacity;
    a.status = c.status;
    uint32_t tile = g_tile_bytes.load();
    if (tile == 0 || tile > kTileMax) tile = kTileMax;
    if (tile < kTileMin) tile = kTileMin;
    a.tile_bytes = tile & ~15u;
    if (groups > 0xffffffffull) fail(GDX_ERR_INVALID_ARGUMENT, "too many reads");
    hipLaunchKernelGGL(sam_lengths_kernel, dim3(static_cast<unsigned>(groups)), dim3(kBlock), 0, stream, a);
    hipLaunchKernelGGL(sam_scan_kernel, dim3(1), dim3(kBlock), 0, stream, a.tile_sums, groups, a.rec_off + c.n_reads);
    hipLaunchKernelGGL(sam_offsets_kernel, dim3(static_cast<unsigned>(groups)), dim3(kBlock), 0, stream, a.rec_off, c.n_reads, a.tile_sums);
    if (c.out == nullptr || c.out_capacity == 0) return;
    uint64_t grid = g_grid.load();
    if (grid == 0) grid = div_ceil(c.n_reads, 64);  // a few tiles a workgroup at the least
    if (grid > kMaxGrid) grid = kMaxGrid;
    if (grid == 0) grid = 1;
    hipLaunchKernelGGL(sam_fill_kernel, dim3(static_cast<unsigned>(grid)), dim3(kFill), 0, stream, a);
}

// ---- the two forms of the call: what both refuse, then the device launches or the staged host form ----
namespace {

void default_dense_to_io(const uint8_t *io_to_dense, uint8_t out[16])
{
    // code c in 1..15: the smallest byte the alphabet maps to it.  Code 0 stands for every text symbol outside 1..4 (a text unit
    // does not keep which): the smallest byte of the one dense code above 4 when the alphabet has exactly one (N of DNA)
    int first[256], others = 0, other = 0;
    for (int d = 0; d < 256; d++) first[d] = -1;
    for (int b = 255; b >= 0; b--) first[io_to_dense[b]] = b;
    for (int c = 0; c < 16; c++) out[c] = c >= 1 && first[c] >= 0 ? static_cast<uint8_t>(first[c]) : '?';
    for (int d = 5; d < 256; d++)
        if (first[d] >= 0) {
            others++;
            other = d;
        }
    if (others == 1) out[0] = static_cast<uint8_t>(first[other]);
}

struct Checked {
    SamCall call;
    bool nothing = false;  // n_reads == 0
};

// the checks of include/gdx_experimental.h in their order; fills everything of the call but the pointers
Checked check_sam(const FmIndex &f, const gdx_sam_inputs_t *in, bool packed, uint32_t uniform_len, uint8_t tab[16])
{
    if (f.view().text_units == nullptr)
        fail(GDX_ERR_UNSUPPORTED, "the index holds no text units (gdx_build_options_t.text_units): MD needs the text");
    if (packed) fail(GDX_ERR_UNSUPPORTED, "SAM records take plain queries: SEQ is a copy of the read's bytes");
    if (in->strands != 1 && in->strands != 2) fail(GDX_ERR_INVALID_ARGUMENT, "strands must be 1 or 2");
    if (in->mode != GDX_SAM_SINGLE && in->mode != GDX_SAM_PAIRED) fail(GDX_ERR_INVALID_ARGUMENT, "mode must be GDX_SAM_SINGLE or GDX_SAM_PAIRED");
    if (in->max_edits > GDX_EDIT_MAX_QUERY_LEN) fail(GDX_ERR_INVALID_ARGUMENT, "max_edits must be at most %u", GDX_EDIT_MAX_QUERY_LEN);
    if (in->nq >= 0xffffffffull) fail(GDX_ERR_INVALID_ARGUMENT, "more than 2^32 - 2 queries (win_query is 32 bits wide)");
    if (in->nq % in->strands != 0 || in->nq / in->strands != in->n_reads)
        fail(GDX_ERR_INVALID_ARGUMENT, "%llu queries for %llu reads of %u strands", (unsigned long long)in->nq,
             (unsigned long long)in->n_reads, in->strands);
    if (in->mode == GDX_SAM_PAIRED && in->n_reads % 2 != 0) fail(GDX_ERR_INVALID_ARGUMENT, "paired mode takes an even number of reads");
    if (!in->rec_off) fail(GDX_ERR_INVALID_ARGUMENT, "rec_off is null");
    if ((in->names != nullptr) != (in->name_off != nullptr) || (in->text_names != nullptr) != (in->text_name_off != nullptr))
        fail(GDX_ERR_INVALID_ARGUMENT, "names go with their offsets");
    Checked k;
    k.nothing = in->n_reads == 0;
    if (!k.nothing && any_null({in->qbuf, in->win_query, in->win_hits, in->dist, in->begin, in->end, in->n_cigar, in->cigar, in->mapq}))
        fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
    if (!k.nothing && uniform_len == 0 && !in->qoff) fail(GDX_ERR_INVALID_ARGUMENT, "qoff is null and the layout is not uniform");
    if (in->dense_to_io) std::memcpy(tab, in->dense_to_io, 16);
    else default_dense_to_io(f.config().io_to_dense, tab);
    SamCall &c = k.call;
    c.uniform_len = uniform_len;
    c.n_reads = in->n_reads;
    c.strands = in->strands;
    c.paired = in->mode == GDX_SAM_PAIRED;
    c.max_edits = in->max_edits;
    c.dense_to_io = tab;
    c.out_capacity = in->out_capacity;
    return k;
}

template <class T>
const T *as(const void *p)
{
    return static_cast<const T *>(p);
}

}  // namespace

void sam_records_dev(const FmIndex &f, const gdx_sam_inputs_t *in, bool packed, uint32_t uniform_len, hipStream_t stream,
                     const std::function<void()> &enter)
{
    uint8_t tab[16];
    Checked k = check_sam(f, in, packed, uniform_len, tab);
    if (!in->workspace || in->workspace_bytes < sam_workspace_bytes(in->n_reads))
        fail(GDX_ERR_INVALID_ARGUMENT, "workspace of %llu bytes, %llu are needed (gdx_sam_workspace_bytes)",
             (unsigned long long)in->workspace_bytes, (unsigned long long)sam_workspace_bytes(in->n_reads));
    if ((reinterpret_cast<uintptr_t>(in->workspace) & 7u) != 0 || (reinterpret_cast<uintptr_t>(in->rec_off) & 7u) != 0)
        fail(GDX_ERR_INVALID_ARGUMENT, "workspace and rec_off must be 8-byte aligned");
    SamCall &c = k.call;
    c.d_qbuf = as<uint8_t>(in->qbuf);
    c.d_qoff = as<uint64_t>(in->qoff);
    c.win_query = as<uint32_t>(in->win_query);
    c.win_hits = as<gdx_hit32_t>(in->win_hits);
    c.dist = as<uint32_t>(in->dist);
    c.begin = as<uint32_t>(in->begin);
    c.end = as<uint32_t>(in->end);
    c.n_cigar = as<uint32_t>(in->n_cigar);
    c.cigar = as<uint32_t>(in->cigar);
    c.mapq = as<uint32_t>(in->mapq);
    c.proper = as<uint32_t>(in->proper);
    c.names = as<uint8_t>(in->names);
    c.name_off = as<uint64_t>(in->name_off);
    c.text_names = as<uint8_t>(in->text_names);
    c.text_name_off = as<uint64_t>(in->text_name_off);
    c.d_workspace = in->workspace;
    c.rec_off = static_cast<uint64_t *>(in->rec_off);
    c.out = static_cast<uint8_t *>(in->out);
    c.status = static_cast<uint8_t *>(in->status);
    enter();
    if (k.nothing) {
        GDX_HIP(hipMemsetAsync(c.rec_off, 0, sizeof(uint64_t), stream));
        return;
    }
    launch_sam_records(f.view(), c, stream);
}

int sam_records_host(const FmIndex &f, const gdx_sam_inputs_t *in)
{
    uint8_t tab[16];
    if (in->layout != nullptr) {
        if (in->layout->struct_size >= 8 && in->layout->packed == 1) fail(GDX_ERR_UNSUPPORTED, "SAM records take plain queries: SEQ is a copy of the read's bytes");
        fail(GDX_ERR_INVALID_ARGUMENT, "the host form takes queries with offsets: layout must be null");
    }
    Checked k = check_sam(f, in, false, 0, tab);
    uint64_t *rec_off = static_cast<uint64_t *>(in->rec_off);
    if (k.nothing) {
        rec_off[0] = 0;
        return GDX_OK;
    }
    const uint64_t n = in->n_reads, nq = in->nq, stride = 2ull * in->max_edits + 1;
    const uint64_t *qoff = as<uint64_t>(in->qoff);
    for (uint64_t i = 0; i < nq; i++)
        if (qoff[i + 1] < qoff[i]) fail(GDX_ERR_INVALID_ARGUMENT, "qoff must be non-decreasing");
    const gdx_hit_t *hits = as<gdx_hit_t>(in->win_hits);
    std::vector<gdx_hit32_t> narrow(n);
    for (uint64_t r = 0; r < n; r++) {
        if (hits[r].text_id > 0xffffffffull || hits[r].position > 0xffffffffull)
            fail(GDX_ERR_INVALID_ARGUMENT, "read %llu: hit (%llu, %llu) does not fit 32 bits", (unsigned long long)r,
                 (unsigned long long)hits[r].text_id, (unsigned long long)hits[r].position);
        narrow[r] = {static_cast<uint32_t>(hits[r].text_id), static_cast<uint32_t>(hits[r].position)};
    }
    f.make_current();
    hipStream_t stream = hipStreamPerThread;
    // one upload per array: 8-byte aligned pieces of one allocation
    struct Piece {
        const void *src;
        uint64_t bytes;
        uint64_t at;
    };
    const uint64_t n_pairs = n / 2, n_texts = f.num_texts();
    const uint64_t name_bytes = in->names ? as<uint64_t>(in->name_off)[n] : 0;
    const uint64_t tname_bytes = in->text_names ? as<uint64_t>(in->text_name_off)[n_texts] : 0;
    Piece pieces[] = {
        {in->qbuf, qoff[nq], 0},
        {qoff, (nq + 1) * 8, 0},
        {in->win_query, n * 4, 0},
        {narrow.data(), n * 8, 0},
        {in->dist, n * 4, 0},
        {in->begin, n * 4, 0},
        {in->end, n * 4, 0},
        {in->n_cigar, n * 4, 0},
        {in->cigar, n * stride * 4, 0},
        {in->mapq, n * 4, 0},
        {k.call.paired ? in->proper : nullptr, n_pairs * 4, 0},
        {in->names, name_bytes, 0},
        {in->name_off, (n + 1) * 8, 0},
        {in->text_names, tname_bytes, 0},
        {in->text_name_off, (n_texts + 1) * 8, 0},
    };
    uint64_t total = 0;
    for (Piece &p : pieces) {
        p.at = total;
        total += round_up(p.bytes + 16, 16);  // (a null piece keeps its room: simpler than to skip it)
    }
    DeviceBuffer<uint8_t> d_in(total), d_ws(sam_workspace_bytes(n)), d_status(n);
    DeviceBuffer<uint64_t> d_off(n + 1);
    for (const Piece &p : pieces)
        if (p.src != nullptr && p.bytes != 0) GDX_HIP(hipMemcpyAsync(d_in.get() + p.at, p.src, p.bytes, hipMemcpyHostToDevice, stream));
    auto dev = [&](int i) -> const void * { return pieces[i].src != nullptr ? d_in.get() + pieces[i].at : nullptr; };
    SamCall &c = k.call;
    c.d_qbuf = as<uint8_t>(d_in.get() + pieces[0].at);  // (an empty batch of reads still has a pointer)
    c.d_qoff = as<uint64_t>(dev(1));
    c.win_query = as<uint32_t>(dev(2));
    c.win_hits = as<gdx_hit32_t>(dev(3));
    c.dist = as<uint32_t>(dev(4));
    c.begin = as<uint32_t>(dev(5));
    c.end = as<uint32_t>(dev(6));
    c.n_cigar = as<uint32_t>(dev(7));
    c.cigar = as<uint32_t>(dev(8));
    c.mapq = as<uint32_t>(dev(9));
    c.proper = as<uint32_t>(dev(10));
    c.names = in->names ? as<uint8_t>(d_in.get() + pieces[11].at) : nullptr;
    c.name_off = as<uint64_t>(dev(12));
    c.text_names = in->text_names ? as<uint8_t>(d_in.get() + pieces[13].at) : nullptr;
    c.text_name_off = as<uint64_t>(dev(14));
    c.d_workspace = d_ws.get();
    c.rec_off = d_off.get();
    c.status = d_status.get();
    // sizing first: the staged output is as large as what fits
    c.out = nullptr;
    launch_sam_records(f.view(), c, stream);
    GDX_HIP(hipGetLastError());
    GDX_HIP(hipMemcpyAsync(rec_off, d_off.get(), (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    if (in->status) GDX_HIP(hipMemcpyAsync(in->status, d_status.get(), n, hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipStreamSynchronize(stream));
    if (in->out == nullptr) return GDX_OK;
    uint64_t n_fit = 0;
    while (n_fit < n && rec_off[n_fit + 1] <= in->out_capacity) n_fit++;
    if (n_fit == 0) return GDX_OK;
    const uint64_t bytes = rec_off[n_fit];
    DeviceBuffer<uint8_t> d_out(bytes);
    c.out = d_out.get();
    c.out_capacity = bytes;
    launch_sam_records(f.view(), c, stream);
    GDX_HIP(hipGetLastError());
    GDX_HIP(hipMemcpyAsync(in->out, d_out.get(), bytes, hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipStreamSynchronize(stream));
    return GDX_OK;
}

}  // namespace gdx
