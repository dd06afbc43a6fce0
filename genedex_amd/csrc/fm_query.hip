// fm_query.hip -- the host-pointer forms of FmIndex's query and mapping calls: each uploads its batch, runs the launch
// functions of kernels.hpp, downloads and synchronises.  (The chunked pipeline behind count / locate is host_api.hip; what
// makes and persists an index is fm_index.hip.)
#include "../../include/gdx_experimental.h"
#include "fm_index.hpp"

#include <cstring>
#include <vector>

#include "kernels.hpp"
#include "select.hpp"

namespace gdx {

namespace {

constexpr int kBlock = 256;

unsigned grid_for_items(uint64_t items) { return grid_for(items, kBlock); }

__global__ __launch_bounds__(kBlock) void widen_u32_kernel(const uint32_t *in, uint64_t *out, uint64_t m)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < m; i += stride) out[i] = in[i];
}

// max_hits_per_query of the staged host calls: an interval keeps its first max_hits rows (suffix-array order)
__global__ __launch_bounds__(kBlock) void take_first_rows_kernel(const uint32_t *start, uint32_t *end, uint64_t m, uint32_t max_hits)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < m; i += stride)
        if (end[i] > start[i] && end[i] - start[i] > max_hits) end[i] = start[i] + max_hits;
}

__global__ __launch_bounds__(kBlock) void narrow_u64_kernel(const uint64_t *in, uint32_t *out, uint64_t m,
                                                            uint64_t limit, uint32_t *error)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < m; i += stride) {
        const uint64_t v = in[i];
        if (v > limit) *error = 1;
        out[i] = static_cast<uint32_t>(v);
    }
}

}  // namespace

// =============================================================================================
// host-pointer query API

namespace {

struct DeviceQueries {
    DeviceBuffer<uint8_t> qbuf;
    DeviceBuffer<uint64_t> qoff;
    DeviceQueries(const uint8_t *h_qbuf, const uint64_t *h_qoff, uint64_t nq, hipStream_t stream)
    {
        const uint64_t base = h_qoff[0];
        const uint64_t bytes = h_qoff[nq] - base;
        const uint64_t padded = div_ceil(bytes + 1, 8) * 8;  // 8-byte windows may read past the last query
        qbuf.alloc(padded);
        GDX_HIP(hipMemsetAsync(qbuf.get() + (padded - 8), 0, 8, stream));
        if (bytes) GDX_HIP(hipMemcpyAsync(qbuf.get(), h_qbuf + base, bytes, hipMemcpyHostToDevice, stream));
        qoff.alloc(nq + 1);
        if (base == 0) {
            GDX_HIP(hipMemcpyAsync(qoff.get(), h_qoff, (nq + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        } else {
            std::vector<uint64_t> rel(nq + 1);
            for (uint64_t i = 0; i <= nq; i++) rel[i] = h_qoff[i] - base;
            GDX_HIP(hipMemcpy(qoff.get(), rel.data(), (nq + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
        }
    }
};

// the calls whose kernels keep a query's length in 32 bits
void check_query_lengths(const uint64_t *qoff, uint64_t nq)
{
    for (uint64_t i = 0; i < nq; i++)
        if (qoff[i + 1] - qoff[i] > 0xffffffffull)
            fail(GDX_ERR_INVALID_ARGUMENT, "query %llu is longer than 2^32 - 1 symbols", (unsigned long long)i);
}

// m hits narrowed to 32 bits; check(i) refuses, before hit i is narrowed, what the call does not take
template <class Check>
std::vector<gdx_hit32_t> narrow_hits(const gdx_hit_t *hits, uint64_t m, Check &&check)
{
    std::vector<gdx_hit32_t> narrow(m);
    for (uint64_t i = 0; i < m; i++) {
        check(i);
        narrow[i] = {static_cast<uint32_t>(hits[i].text_id), static_cast<uint32_t>(hits[i].position)};
    }
    return narrow;
}

// the m candidates of a verify call (hamming_many, edit_distance_many, align_many) on the index's device: checked against the
// batch and the index, the hits narrowed to 32 bits, uploaded on `stream` of the current device
struct DeviceCandidates {
    DeviceBuffer<uint32_t> query, begin;
    DeviceBuffer<gdx_hit32_t> hits;
    std::vector<gdx_hit32_t> narrow;  // the source of an asynchronous copy: lives until the call has synchronised
    DeviceCandidates(uint64_t n_texts, uint64_t nq, const uint32_t *cand_query, const uint32_t *cand_begin, const gdx_hit_t *cand_hits,
                     uint64_t m, hipStream_t stream)
        : narrow(narrow_hits(cand_hits, m, [&](uint64_t c) {
              if (cand_query[c] >= nq)
                  fail(GDX_ERR_INVALID_ARGUMENT, "candidate %llu belongs to query %u of %llu", (unsigned long long)c, cand_query[c],
                       (unsigned long long)nq);
              if (cand_hits[c].text_id >= n_texts)
                  fail(GDX_ERR_INVALID_ARGUMENT, "candidate %llu lies in text %llu of %llu", (unsigned long long)c,
                       (unsigned long long)cand_hits[c].text_id, (unsigned long long)n_texts);
              if (cand_hits[c].position > 0xffffffffull)
                  fail(GDX_ERR_INVALID_ARGUMENT, "candidate %llu: position %llu does not fit 32 bits", (unsigned long long)c,
                       (unsigned long long)cand_hits[c].position);
          }))
    {
        query.alloc(m);
        begin.alloc(m);
        hits.alloc(m);
        GDX_HIP(hipMemcpyAsync(query.get(), cand_query, m * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        GDX_HIP(hipMemcpyAsync(begin.get(), cand_begin, m * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        GDX_HIP(hipMemcpyAsync(hits.get(), narrow.data(), m * sizeof(gdx_hit32_t), hipMemcpyHostToDevice, stream));
    }
};

// the m slots of best_hits_many / pair_hits_many with their verify results: both words of a hit must fit 32 bits, every cand_query
// passes (GDX_CAND_NONE marks an unused slot); then the index's device is made current and the slots are uploaded on `stream`
struct DeviceSlots {
    std::vector<gdx_hit32_t> narrow;  // (as in DeviceCandidates)
    DeviceBuffer<uint32_t> in;        // query, begin, dist, end
    DeviceBuffer<gdx_hit32_t> hits;
    const bool has_end;
    DeviceSlots(const FmIndex &ix, const uint32_t *cand_query, const uint32_t *cand_begin, const gdx_hit_t *cand_hits,
                const uint32_t *dist, const uint32_t *end, uint64_t m, hipStream_t stream)
        : narrow(narrow_hits(cand_hits, m, [&](uint64_t s) {
              if (cand_hits[s].position > 0xffffffffull || cand_hits[s].text_id > 0xffffffffull)
                  fail(GDX_ERR_INVALID_ARGUMENT, "slot %llu: hit (%llu, %llu) does not fit 32 bits", (unsigned long long)s,
                       (unsigned long long)cand_hits[s].text_id, (unsigned long long)cand_hits[s].position);
          })), has_end(end != nullptr)
    {
        ix.make_current();
        const uint32_t *columns[4] = {cand_query, cand_begin, dist, end};
        in.alloc((has_end ? 4 : 3) * m);
        hits.alloc(m);
        for (int x = 0; x < (has_end ? 4 : 3); x++)
            GDX_HIP(hipMemcpyAsync(in.get() + x * m, columns[x], m * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        GDX_HIP(hipMemcpyAsync(hits.get(), narrow.data(), m * sizeof(gdx_hit32_t), hipMemcpyHostToDevice, stream));
    }
    // the shared part of a stage's argument block: the slots, and the winner triple the caller has made room for
    SlotArgs args(uint32_t max_dist, uint32_t *win_query, uint32_t *win_begin, gdx_hit32_t *win_hits) const
    {
        const uint64_t m = narrow.size();
        return {in.get(), in.get() + m, hits.get(), in.get() + 2 * m, has_end ? in.get() + 3 * m : nullptr, max_dist, win_query, win_begin,
                win_hits};
    }
};

void check_queries(const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq)
{
    if (!qoff) fail(GDX_ERR_INVALID_ARGUMENT, "qoff is null");
    if (nq >= 0xffffffffull) fail(GDX_ERR_UNSUPPORTED, "more than 2^32-2 queries in one call");
    for (uint64_t i = 0; i < nq; i++)
        if (qoff[i + 1] < qoff[i]) fail(GDX_ERR_INVALID_ARGUMENT, "qoff must be non-decreasing");
    if (qoff[nq] > qoff[0] && !qbuf) fail(GDX_ERR_INVALID_ARGUMENT, "qbuf is null");
}

int any_status(const uint8_t *status, uint64_t n)
{
    for (uint64_t i = 0; i < n; i++)
        if (status[i]) return GDX_ERR_QUERY_STATUS;
    return GDX_OK;
}

void download_widened(const uint32_t *d_in, uint64_t *h_out, uint64_t m, hipStream_t stream)
{
    if (!h_out || m == 0) return;
    DeviceBuffer<uint64_t> wide(m);
    hipLaunchKernelGGL(widen_u32_kernel, dim3(grid_for_items(m)), dim3(kBlock), 0, stream, d_in, wide.get(), m);
    GDX_HIP(hipMemcpyAsync(h_out, wide.get(), m * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipStreamSynchronize(stream));
}

// consecutive columns of n words each, from d_in on, into the host arrays `outs` (asynchronous: the caller synchronises)
void download_columns(std::initializer_list<uint32_t *> outs, const uint32_t *d_in, uint64_t n, hipStream_t stream)
{
    for (uint32_t *out : outs) {
        GDX_HIP(hipMemcpyAsync(out, d_in, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        d_in += n;
    }
}

// n narrow hits of the device widened into `out`; the stream has run dry when it returns
void widen_hits(gdx_hit_t *out, uint64_t n, const gdx_hit32_t *d_hits, hipStream_t stream)
{
    std::vector<gdx_hit32_t> hits(n);
    GDX_HIP(hipMemcpyAsync(hits.data(), d_hits, n * sizeof(gdx_hit32_t), hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipStreamSynchronize(stream));
    for (uint64_t i = 0; i < n; i++) out[i] = {hits[i].text_id, hits[i].position};
}

}  // namespace

void FmIndex::locate_device(const uint32_t *d_start, const uint32_t *d_end, uint64_t m, uint64_t *out_hit_offsets,
                            gdx_hit_t *hits, uint64_t hits_capacity, uint64_t *out_total, int *rc,
                            const uint4 *d_rec) const
{
    hipStream_t stream = hipStreamPerThread;
    DeviceBuffer<uint64_t> d_off(m + 1);
    if (d_rec) {
        const size_t tb = hit_offsets_rec_temp_bytes(m);
        DeviceBuffer<uint8_t> temp(tb ? tb : 1);
        launch_hit_offsets_rec(d_rec, m, d_off.get(), temp.get(), tb, stream);
        GDX_HIP(hipStreamSynchronize(stream));
    } else {
        const size_t tb = hit_offsets_temp_bytes(m);
        DeviceBuffer<uint8_t> temp(tb ? tb : 1);
        launch_hit_offsets(d_start, d_end, m, d_off.get(), temp.get(), tb, stream);
        GDX_HIP(hipStreamSynchronize(stream));
    }
    uint64_t total = 0;
    GDX_HIP(hipMemcpy(&total, d_off.get() + m, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (out_total) *out_total = total;
    if (out_hit_offsets)
        GDX_HIP(hipMemcpy(out_hit_offsets, d_off.get(), (m + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (total == 0) return;
    if (!hits || hits_capacity < total) {
        *rc = GDX_ERR_CAPACITY;
        return;
    }
    DeviceBuffer<gdx_hit_t> d_hits(total);
    DeviceBuffer<uint8_t> ws(locate_workspace_bytes(total));
    LocateCall loc;
    loc.d_start = d_start;
    loc.d_end = d_end;
    loc.d_rec = d_rec;
    loc.m = m;
    loc.d_hit_offsets = d_off.get();
    loc.total_hits = total;
    loc.d_hits = d_hits.get();
    loc.wide = true;
    loc.d_workspace = ws.get();
    launch_locate(view_, loc, stream, query_options());
    GDX_HIP(hipGetLastError());
    GDX_HIP(hipMemcpyAsync(hits, d_hits.get(), total * sizeof(gdx_hit_t), hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipStreamSynchronize(stream));
}

namespace {

void upload_narrowed(const uint64_t *h_in, uint32_t *d_out, uint64_t m, uint64_t limit, const char *what,
                     hipStream_t stream)
{
    DeviceBuffer<uint64_t> wide(m);
    DeviceBuffer<uint32_t> flag(1);
    GDX_HIP(hipMemcpyAsync(wide.get(), h_in, m * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    GDX_HIP(hipMemsetAsync(flag.get(), 0, sizeof(uint32_t), stream));
    hipLaunchKernelGGL(narrow_u64_kernel, dim3(grid_for_items(m)), dim3(kBlock), 0, stream, wide.get(), d_out, m,
                       limit, flag.get());
    uint32_t f = 0;
    GDX_HIP(hipMemcpyAsync(&f, flag.get(), sizeof(f), hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipStreamSynchronize(stream));
    if (f) fail(GDX_ERR_INVALID_ARGUMENT, "%s exceeds the text length", what);
}

}  // namespace

int FmIndex::cursor_extend_front_many(uint64_t *start, uint64_t *end, const uint8_t *io_symbols, uint64_t m,
                                      uint8_t *out_status) const
{
    if (m == 0) return GDX_OK;
    if (!start || !end || !io_symbols) fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
    make_current();
    hipStream_t stream = hipStreamPerThread;
    DeviceBuffer<uint32_t> d_start(m), d_end(m);
    DeviceBuffer<uint8_t> d_sym(m), d_status(m);
    upload_narrowed(start, d_start.get(), m, n_, "cursor start", stream);
    upload_narrowed(end, d_end.get(), m, n_, "cursor end", stream);
    GDX_HIP(hipMemcpyAsync(d_sym.get(), io_symbols, m, hipMemcpyHostToDevice, stream));
    launch_extend_front(view_, d_start.get(), d_end.get(), d_sym.get(), m, d_status.get(), stream);
    GDX_HIP(hipGetLastError());
    download_widened(d_start.get(), start, m, stream);
    download_widened(d_end.get(), end, m, stream);
    std::vector<uint8_t> status(m);
    GDX_HIP(hipMemcpy(status.data(), d_status.get(), m, hipMemcpyDeviceToHost));
    if (out_status) std::memcpy(out_status, status.data(), m);
    return any_status(status.data(), m);
}

int FmIndex::cursor_extend_front_strings(uint64_t *start, uint64_t *end, const uint8_t *qbuf, const uint64_t *qoff,
                                         uint64_t m, uint8_t *status) const
{
    check_queries(qbuf, qoff, m);
    if (m == 0) return GDX_OK;
    if (!start || !end) fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
    make_current();
    hipStream_t stream = hipStreamPerThread;
    DeviceQueries dq(qbuf, qoff, m, stream);
    DeviceBuffer<uint32_t> d_start(m), d_end(m);
    DeviceBuffer<uint8_t> d_status(m);
    upload_narrowed(start, d_start.get(), m, n_, "cursor start", stream);
    upload_narrowed(end, d_end.get(), m, n_, "cursor end", stream);
    if (status) GDX_HIP(hipMemcpyAsync(d_status.get(), status, m, hipMemcpyHostToDevice, stream));
    else GDX_HIP(hipMemsetAsync(d_status.get(), 0, m, stream));
    SearchCall c;
    c.d_qbuf = dq.qbuf.get();
    c.d_qbeg = dq.qoff.get();
    c.d_qend = dq.qoff.get() + 1;
    c.nq = m;
    c.d_start = d_start.get();
    c.d_end = d_end.get();
    c.d_status = d_status.get();
    c.mode = 2;
    launch_search_call(view_, c, stream, query_options());
    GDX_HIP(hipGetLastError());
    download_widened(d_start.get(), start, m, stream);
    download_widened(d_end.get(), end, m, stream);
    std::vector<uint8_t> st(m);
    GDX_HIP(hipMemcpy(st.data(), d_status.get(), m, hipMemcpyDeviceToHost));
    if (status) std::memcpy(status, st.data(), m);
    return any_status(st.data(), m);
}

int FmIndex::cursor_locate_many(const uint64_t *start, const uint64_t *end, uint64_t m, uint64_t *out_hit_offsets,
                                gdx_hit_t *hits, uint64_t hits_capacity, uint64_t *out_total) const
{
    if (out_total) *out_total = 0;
    if (m == 0) {
        if (out_hit_offsets) out_hit_offsets[0] = 0;
        return GDX_OK;
    }
    if (!start || !end) fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
    for (uint64_t i = 0; i < m; i++)
        if (start[i] > end[i]) fail(GDX_ERR_INVALID_ARGUMENT, "cursor %llu has start > end", (unsigned long long)i);
    make_current();
    hipStream_t stream = hipStreamPerThread;
    DeviceBuffer<uint32_t> d_start(m), d_end(m);
    upload_narrowed(start, d_start.get(), m, n_, "cursor start", stream);
    upload_narrowed(end, d_end.get(), m, n_, "cursor end", stream);
    int rc = GDX_OK;
    locate_device(d_start.get(), d_end.get(), m, out_hit_offsets, hits, hits_capacity, out_total, &rc);
    return rc;
}

int FmIndex::suffix_segments_many(const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq, uint32_t max_segments,
                                  uint32_t flags, uint32_t *out_n_segments, uint32_t *out_remaining, uint32_t *out_length,
                                  uint64_t *out_start, uint64_t *out_end, uint8_t *out_status) const
{
    if (max_segments == 0) fail(GDX_ERR_INVALID_ARGUMENT, "max_segments must be at least 1");
    if ((flags & ~static_cast<uint32_t>(GDX_SEGMENTS_LF_ONLY)) != 0u) fail(GDX_ERR_INVALID_ARGUMENT, "unknown bit in flags");
    check_queries(qbuf, qoff, nq);
    if (nq == 0) return GDX_OK;
    if (!out_n_segments || !out_remaining || !out_length || !out_start || !out_end) fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
    check_query_lengths(qoff, nq);
    make_current();
    hipStream_t stream = hipStreamPerThread;
    DeviceQueries dq(qbuf, qoff, nq, stream);
    const uint64_t slots = nq * max_segments;
    DeviceBuffer<uint32_t> d_n(nq), d_rem(nq), d_len(slots), d_start(slots), d_end(slots);
    DeviceBuffer<uint8_t> d_status(nq);
    launch_suffix_segments(view_, dq.qbuf.get(), dq.qoff.get(), nq, max_segments, (flags & GDX_SEGMENTS_LF_ONLY) != 0u, d_n.get(),
                           d_rem.get(), d_len.get(), d_start.get(), d_end.get(), d_status.get(), stream, query_options());
    GDX_HIP(hipGetLastError());
    GDX_HIP(hipMemcpyAsync(out_n_segments, d_n.get(), nq * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipMemcpyAsync(out_remaining, d_rem.get(), nq * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipMemcpyAsync(out_length, d_len.get(), slots * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    download_widened(d_start.get(), out_start, slots, stream);
    download_widened(d_end.get(), out_end, slots, stream);
    std::vector<uint8_t> st(nq);
    GDX_HIP(hipMemcpy(st.data(), d_status.get(), nq, hipMemcpyDeviceToHost));
    if (out_status) std::memcpy(out_status, st.data(), nq);
    return any_status(st.data(), nq);
}

void FmIndex::check_companion(const FmIndex &r) const
{
    if (r.cfg_.device_id != cfg_.device_id) fail(GDX_ERR_INVALID_ARGUMENT, "the reversed index lives on another device");
    if (r.n_ != n_ || r.n_texts_ != n_texts_)
        fail(GDX_ERR_INVALID_ARGUMENT, "the reversed index holds %llu symbols in %llu texts, the index %llu in %llu",
             (unsigned long long)r.n_, (unsigned long long)r.n_texts_, (unsigned long long)n_, (unsigned long long)n_texts_);
    if (r.cfg_.sigma != cfg_.sigma || r.cfg_.n_searchable != cfg_.n_searchable ||
        std::memcmp(r.cfg_.io_to_dense, cfg_.io_to_dense, 256) != 0)
        fail(GDX_ERR_INVALID_ARGUMENT, "the reversed index was built with another alphabet");
    if (r.count_host_ != count_host_)
        fail(GDX_ERR_INVALID_ARGUMENT, "the reversed index counts other symbols: it was not built from the same texts, reversed");
    if (r.view_.layout != view_.layout)
        fail(GDX_ERR_UNSUPPORTED, "the reversed index has another occurrence-table layout (reference_table_layout)");
}

int FmIndex::smems_many(const FmIndex &reversed, const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq, uint32_t max_smems,
                        uint32_t min_length, uint32_t *out_n_smems, uint32_t *out_remaining, uint32_t *out_begin,
                        uint32_t *out_length, uint64_t *out_start, uint64_t *out_end, uint8_t *out_status) const
{
    if (max_smems == 0) fail(GDX_ERR_INVALID_ARGUMENT, "max_smems must be at least 1");
    if (min_length == 0) fail(GDX_ERR_INVALID_ARGUMENT, "min_length must be at least 1");
    check_companion(reversed);
    check_queries(qbuf, qoff, nq);
    if (nq == 0) return GDX_OK;
    if (!out_n_smems || !out_remaining || !out_begin || !out_length || !out_start || !out_end)
        fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
    check_query_lengths(qoff, nq);
    make_current();
    hipStream_t stream = hipStreamPerThread;
    DeviceQueries dq(qbuf, qoff, nq, stream);
    const uint64_t slots = nq * max_smems;
    DeviceBuffer<uint32_t> d_n(nq), d_rem(nq), d_begin(slots), d_len(slots), d_start(slots), d_end(slots);
    DeviceBuffer<uint8_t> d_status(nq);
    launch_smems(view_, reversed.view_, dq.qbuf.get(), dq.qoff.get(), nq, max_smems, min_length, d_n.get(), d_rem.get(),
                 d_begin.get(), d_len.get(), d_start.get(), d_end.get(), d_status.get(), stream, query_options());
    GDX_HIP(hipGetLastError());
    GDX_HIP(hipMemcpyAsync(out_n_smems, d_n.get(), nq * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipMemcpyAsync(out_remaining, d_rem.get(), nq * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipMemcpyAsync(out_begin, d_begin.get(), slots * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipMemcpyAsync(out_length, d_len.get(), slots * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    download_widened(d_start.get(), out_start, slots, stream);
    download_widened(d_end.get(), out_end, slots, stream);
    std::vector<uint8_t> st(nq);
    GDX_HIP(hipMemcpy(st.data(), d_status.get(), nq, hipMemcpyDeviceToHost));
    if (out_status) std::memcpy(out_status, st.data(), nq);
    return any_status(st.data(), nq);
}

int FmIndex::strands_many(const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq, const uint8_t *complement, uint64_t *out_counts,
                          uint64_t *out_hit_offsets, gdx_hit_t **out_hits, uint64_t *out_total, uint8_t *out_status) const
{
    const bool locate = out_hit_offsets != nullptr;
    if (locate) {
        if (!out_hits) fail(GDX_ERR_INVALID_ARGUMENT, "out_hits is null");
        *out_hits = nullptr;
        if (out_total) *out_total = 0;
        out_hit_offsets[0] = 0;
    }
    uint8_t stock[256];
    if (!complement) {
        dna_complement_table(stock);
        complement = stock;
    }
    check_complement(cfg_.io_to_dense, complement, false);
    check_queries(qbuf, qoff, nq);
    if (2 * nq >= 0xffffffffull) fail(GDX_ERR_UNSUPPORTED, "more than 2^31-1 queries in one both-strand call");
    if (nq == 0) return GDX_OK;
    if (!locate && !out_counts) fail(GDX_ERR_INVALID_ARGUMENT, "out_counts is null");
    make_current();
    hipStream_t stream = hipStreamPerThread;
    DeviceQueries dq(qbuf, qoff, nq, stream);  // the forward reads cross the link once
    const uint64_t total = qoff[nq] - qoff[0], m = 2 * nq;
    DeviceBuffer<uint8_t> d_both(strands_out_bytes(total, false, GDX_STRANDS_BOTH));
    DeviceBuffer<uint64_t> d_both_off(m + 1);
    launch_strands_expand(dq.qbuf.get(), dq.qoff.get(), nq, false, 0, total, complement, GDX_STRANDS_BOTH, d_both.get(),
                          d_both_off.get(), stream);
    DeviceBuffer<uint32_t> d_start(m), d_end(m);
    DeviceBuffer<uint8_t> d_status(m);
    SearchCall c;
    c.d_qbuf = d_both.get();
    c.d_qbeg = d_both_off.get();
    c.d_qend = d_both_off.get() + 1;
    c.nq = m;
    c.d_start = d_start.get();
    c.d_end = d_end.get();
    c.d_status = d_status.get();
    c.mode = 0;
    launch_search_call(view_, c, stream, query_options());
    GDX_HIP(hipGetLastError());
    std::vector<uint8_t> st(m);
    GDX_HIP(hipMemcpyAsync(st.data(), d_status.get(), m, hipMemcpyDeviceToHost, stream));
    if (!locate) {
        std::vector<uint64_t> s(m), e(m);
        download_widened(d_start.get(), s.data(), m, stream);
        download_widened(d_end.get(), e.data(), m, stream);
        for (uint64_t i = 0; i < m; i++) out_counts[i] = e[i] > s[i] ? e[i] - s[i] : 0;
    } else {
        const uint32_t max_hits = query_options().max_hits_per_query;
        if (max_hits != 0)
            hipLaunchKernelGGL(take_first_rows_kernel, dim3(grid_for_items(m)), dim3(kBlock), 0, stream, d_start.get(), d_end.get(),
                               m, max_hits);
        uint64_t n_hits = 0;
        int rc = GDX_OK;
        locate_device(d_start.get(), d_end.get(), m, out_hit_offsets, nullptr, 0, &n_hits, &rc);  // offsets and the total
        gdx_hit_t *hits = static_cast<gdx_hit_t *>(std::malloc((n_hits ? n_hits : 1) * sizeof(gdx_hit_t)));
        if (!hits) fail(GDX_ERR_DEVICE, "out of host memory for %llu hits", static_cast<unsigned long long>(n_hits));
        if (n_hits != 0) {
            rc = GDX_OK;
            try {
                locate_device(d_start.get(), d_end.get(), m, nullptr, hits, n_hits, nullptr, &rc);
            } catch (...) {
                std::free(hits);
                throw;
            }
        }
        *out_hits = hits;
        if (out_total) *out_total = n_hits;
    }
    GDX_HIP(hipStreamSynchronize(stream));
    if (out_status) std::memcpy(out_status, st.data(), m);
    return any_status(st.data(), m);
}

void FmIndex::check_hamming(bool packed, uint32_t max_mismatches) const
{
    if (view_.text_units == nullptr)
        fail(GDX_ERR_UNSUPPORTED, "the index holds no text units (gdx_build_options_t.text_units): there is no text to compare with");
    if (packed) check_packed_supported();
    if (max_mismatches > 0x80000000u) fail(GDX_ERR_INVALID_ARGUMENT, "max_mismatches must be at most 2^31");
}

int FmIndex::hamming_many(const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq, const uint32_t *cand_query, const uint32_t *cand_begin,
                          const gdx_hit_t *cand_hits, uint64_t m, uint32_t max_mismatches, uint32_t *out) const
{
    check_hamming(false, max_mismatches);
    check_queries(qbuf, qoff, nq);
    if (m == 0) return GDX_OK;
    if (!cand_query || !cand_begin || !cand_hits || !out) fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
    if (nq == 0) {  // every candidate is out of range
        for (uint64_t c = 0; c < m; c++) out[c] = GDX_HAMMING_INVALID;
        return GDX_OK;
    }
    check_query_lengths(qoff, nq);
    make_current();
    hipStream_t stream = hipStreamPerThread;
    DeviceCandidates dc(n_texts_, nq, cand_query, cand_begin, cand_hits, m, stream);
    DeviceQueries dq(qbuf, qoff, nq, stream);
    DeviceBuffer<uint32_t> d_out(m);
    launch_hamming(view_, dq.qbuf.get(), dq.qoff.get(), nq, false, 0, dc.query.get(), dc.begin.get(), dc.hits.get(), m, max_mismatches,
                   d_out.get(), stream);
    GDX_HIP(hipGetLastError());
    GDX_HIP(hipMemcpyAsync(out, d_out.get(), m * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipStreamSynchronize(stream));
    return GDX_OK;
}

void FmIndex::check_edit_distance(bool packed, uint32_t max_edits) const
{
    check_hamming(packed, 0);
    if (max_edits > GDX_EDIT_MAX_QUERY_LEN)
        fail(GDX_ERR_INVALID_ARGUMENT, "max_edits must be at most %u (no distance exceeds the longest query)", GDX_EDIT_MAX_QUERY_LEN);
}

int FmIndex::edit_distance_many(const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq, const uint32_t *cand_query,
                                const uint32_t *cand_begin, const gdx_hit_t *cand_hits, uint64_t m, uint32_t max_edits,
                                uint32_t *out_dist, uint32_t *out_end) const
{
    check_edit_distance(false, max_edits);
    check_queries(qbuf, qoff, nq);
    if (m == 0) return GDX_OK;
    if (!cand_query || !cand_begin || !cand_hits || !out_dist) fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
    if (nq == 0) {  // every candidate is out of range
        for (uint64_t c = 0; c < m; c++) {
            out_dist[c] = GDX_EDIT_INVALID;
            if (out_end) out_end[c] = GDX_EDIT_NO_END;
        }
        return GDX_OK;
    }
    make_current();
    hipStream_t stream = hipStreamPerThread;
    DeviceCandidates dc(n_texts_, nq, cand_query, cand_begin, cand_hits, m, stream);
    DeviceQueries dq(qbuf, qoff, nq, stream);
    DeviceBuffer<uint32_t> d_dist(m), d_end(out_end ? m : 0);
    launch_edit_distance(view_, dq.qbuf.get(), dq.qoff.get(), nq, false, 0, dc.query.get(), dc.begin.get(), dc.hits.get(), m, max_edits,
                         d_dist.get(), out_end ? d_end.get() : nullptr, stream);
    GDX_HIP(hipGetLastError());
    GDX_HIP(hipMemcpyAsync(out_dist, d_dist.get(), m * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (out_end) GDX_HIP(hipMemcpyAsync(out_end, d_end.get(), m * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipStreamSynchronize(stream));
    return GDX_OK;
}

int FmIndex::align_many(const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq, const uint32_t *cand_query, const uint32_t *cand_begin,
                        const gdx_hit_t *cand_hits, uint64_t m, uint32_t max_edits, uint32_t *out_dist, uint32_t *out_begin,
                        uint32_t *out_end, uint32_t *out_n_cigar, uint32_t *out_cigar) const
{
    check_align(false, max_edits);
    check_queries(qbuf, qoff, nq);
    if (!out_dist || !out_begin || !out_end || !out_n_cigar || !out_cigar) fail(GDX_ERR_INVALID_ARGUMENT, "null output");
    if (m == 0) return GDX_OK;
    if (!cand_query || !cand_begin || !cand_hits) fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
    if (nq == 0) {  // every candidate is out of range
        for (uint64_t c = 0; c < m; c++) {
            out_dist[c] = GDX_EDIT_INVALID;
            out_begin[c] = out_end[c] = GDX_EDIT_NO_END;
            out_n_cigar[c] = 0;
        }
        return GDX_OK;
    }
    make_current();
    hipStream_t stream = hipStreamPerThread;
    DeviceCandidates dc(n_texts_, nq, cand_query, cand_begin, cand_hits, m, stream);
    const uint64_t stride = 2ull * max_edits + 1;
    uint64_t ws_bytes[2];
    align_workspace_bytes(0, m, max_edits, ws_bytes);
    DeviceQueries dq(qbuf, qoff, nq, stream);
    DeviceBuffer<uint32_t> d_out(4 * m), d_cigar(m * stride);  // d_out: dist, begin, end, n_cigar
    DeviceBuffer<uint8_t> d_ws(ws_bytes[1]);
    launch_align(view_, dq.qbuf.get(), dq.qoff.get(), nq, false, 0, dc.query.get(), dc.begin.get(), dc.hits.get(), m, max_edits,
                 d_out.get(), d_out.get() + m, d_out.get() + 2 * m, d_out.get() + 3 * m, d_cigar.get(), d_ws.get(), ws_bytes[1], stream);
    GDX_HIP(hipGetLastError());
    download_columns({out_dist, out_begin, out_end, out_n_cigar}, d_out.get(), m, stream);
    GDX_HIP(hipStreamSynchronize(stream));
    // only the words below n_cigar are the call's: the words behind them stay as the caller left them
    std::vector<uint32_t> cigar(m * stride);
    GDX_HIP(hipMemcpy(cigar.data(), d_cigar.get(), cigar.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint64_t c = 0; c < m; c++)
        std::copy_n(cigar.data() + c * stride, out_n_cigar[c], out_cigar + c * stride);
    return GDX_OK;
}

void FmIndex::check_seed_candidates(uint32_t max_seeds, uint32_t max_occ, uint32_t max_candidates) const
{
    if (max_seeds == 0) fail(GDX_ERR_INVALID_ARGUMENT, "max_seeds must be at least 1");
    if (max_occ == 0) fail(GDX_ERR_INVALID_ARGUMENT, "max_occ must be at least 1");
    if (max_candidates == 0 || max_candidates > 1024u) fail(GDX_ERR_INVALID_ARGUMENT, "max_candidates must be 1..1024");
    if (static_cast<uint64_t>(max_seeds) * max_occ > GDX_CAND_MAX_ANCHORS)
        fail(GDX_ERR_INVALID_ARGUMENT, "max_seeds * max_occ = %llu exceeds GDX_CAND_MAX_ANCHORS (%u)",
             (unsigned long long)max_seeds * max_occ, GDX_CAND_MAX_ANCHORS);
    if (!seed_candidates_supported(view_))
        fail(GDX_ERR_UNSUPPORTED, "seed candidates need SA[row] in one fetch: an index with full_suffix_array or 32-byte jump entries");
}

int FmIndex::seed_candidates_many(uint64_t nq, uint32_t max_seeds, const uint32_t *n_seeds, const uint32_t *begin,
                                  const uint32_t *length, const uint64_t *start, const uint64_t *end, uint32_t max_occ, uint32_t band,
                                  uint32_t max_candidates, uint32_t *out_n_candidates, uint32_t *out_n_groups, uint32_t *out_n_skipped,
                                  uint32_t *out_cand_query, uint32_t *out_cand_begin, gdx_hit_t *out_cand_hits,
                                  uint32_t *out_cand_weight, uint8_t *out_status) const
{
    check_seed_candidates(max_seeds, max_occ, max_candidates);
    if (nq == 0) return GDX_OK;
    if (nq >= 0xffffffffull) fail(GDX_ERR_INVALID_ARGUMENT, "more than 2^32 - 2 queries (cand_query is 32 bits wide)");
    if (any_null({n_seeds, begin, length, start, end, out_n_candidates, out_n_groups, out_n_skipped, out_cand_query, out_cand_begin,
                  out_cand_hits, out_cand_weight}))
        fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
    const uint64_t slots = nq * max_seeds, outs = nq * max_candidates;
    std::vector<uint32_t> narrow(2 * slots);  // start, end
    for (uint64_t s = 0; s < slots; s++) {
        if (start[s] > 0xffffffffull || end[s] > 0xffffffffull)
            fail(GDX_ERR_INVALID_ARGUMENT, "seed slot %llu: interval [%llu, %llu) does not fit 32 bits", (unsigned long long)s,
                 (unsigned long long)start[s], (unsigned long long)end[s]);
        narrow[s] = static_cast<uint32_t>(start[s]);
        narrow[slots + s] = static_cast<uint32_t>(end[s]);
    }
    make_current();
    hipStream_t stream = hipStreamPerThread;
    DeviceBuffer<uint32_t> d_n(nq), d_begin(slots), d_len(slots), d_iv(2 * slots);
    DeviceBuffer<uint32_t> d_per(3 * nq), d_out(3 * outs);  // d_per: n_candidates, n_groups, n_skipped; d_out: query, begin, weight
    DeviceBuffer<gdx_hit32_t> d_hits(outs);
    DeviceBuffer<uint8_t> d_status(nq);
    GDX_HIP(hipMemcpyAsync(d_n.get(), n_seeds, nq * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    GDX_HIP(hipMemcpyAsync(d_begin.get(), begin, slots * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    GDX_HIP(hipMemcpyAsync(d_len.get(), length, slots * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    GDX_HIP(hipMemcpyAsync(d_iv.get(), narrow.data(), 2 * slots * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    launch_seed_candidates(view_, nq, max_seeds, d_n.get(), d_begin.get(), d_len.get(), d_iv.get(), d_iv.get() + slots, max_occ, band,
                           max_candidates, d_per.get(), d_per.get() + nq, d_per.get() + 2 * nq, d_out.get(), d_out.get() + outs,
                           d_hits.get(), d_out.get() + 2 * outs, d_status.get(), stream);
    GDX_HIP(hipGetLastError());
    std::vector<uint8_t> st(nq);
    download_columns({out_n_candidates, out_n_groups, out_n_skipped}, d_per.get(), nq, stream);
    download_columns({out_cand_query, out_cand_begin, out_cand_weight}, d_out.get(), outs, stream);
    GDX_HIP(hipMemcpyAsync(st.data(), d_status.get(), nq, hipMemcpyDeviceToHost, stream));
    widen_hits(out_cand_hits, outs, d_hits.get(), stream);
    if (out_status) std::memcpy(out_status, st.data(), nq);
    return any_status(st.data(), nq);
}

void FmIndex::check_best_hits(uint64_t n_groups, uint32_t group_slots, uint32_t max_dist) const
{
    if (group_slots == 0 || group_slots > GDX_BEST_MAX_GROUP_SLOTS)
        fail(GDX_ERR_INVALID_ARGUMENT, "group_slots must be 1..%u", GDX_BEST_MAX_GROUP_SLOTS);
    if (max_dist > 0x80000000u) fail(GDX_ERR_INVALID_ARGUMENT, "max_dist must not exceed 2^31");
    if (n_groups > ~0ull / group_slots)
        fail(GDX_ERR_INVALID_ARGUMENT, "%llu groups of %u slots: the number of slots does not fit 64 bits", (unsigned long long)n_groups,
             group_slots);
}

int FmIndex::best_hits_many(uint64_t n_groups, uint32_t group_slots, const uint32_t *cand_query, const uint32_t *cand_begin,
                            const gdx_hit_t *cand_hits, const uint32_t *dist, const uint32_t *end, uint32_t max_dist,
                            uint32_t *out_best_slot, uint32_t *out_best_dist, uint32_t *out_sub_dist, uint32_t *out_n_live,
                            uint32_t *out_n_best, uint32_t *out_mapq, uint32_t *out_win_query, uint32_t *out_win_begin,
                            gdx_hit_t *out_win_hits) const
{
    check_best_hits(n_groups, group_slots, max_dist);
    if (n_groups == 0) return GDX_OK;
    if (any_null({cand_query, cand_begin, cand_hits, dist, out_best_slot, out_best_dist, out_sub_dist, out_n_live, out_n_best, out_mapq,
                  out_win_query, out_win_begin, out_win_hits}))
        fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
    hipStream_t stream = hipStreamPerThread;
    DeviceSlots slots(*this, cand_query, cand_begin, cand_hits, dist, end, n_groups * group_slots, stream);
    DeviceBuffer<uint32_t> d_out(8 * n_groups);  // the six results, win_query, win_begin
    DeviceBuffer<gdx_hit32_t> d_win(n_groups);
    uint32_t *o = d_out.get();
    const BestArgs a = {slots.args(max_dist, o + 6 * n_groups, o + 7 * n_groups, d_win.get()), n_groups, group_slots, o, o + n_groups,
                        o + 2 * n_groups, o + 3 * n_groups, o + 4 * n_groups, o + 5 * n_groups};
    launch_best_hits(a, stream);
    GDX_HIP(hipGetLastError());
    download_columns({out_best_slot, out_best_dist, out_sub_dist, out_n_live, out_n_best, out_mapq, out_win_query, out_win_begin}, o,
                     n_groups, stream);
    widen_hits(out_win_hits, n_groups, d_win.get(), stream);
    return GDX_OK;
}

void FmIndex::check_pair_hits(uint64_t n_pairs, uint32_t mate_slots, uint32_t max_dist, uint32_t min_insert, uint32_t max_insert) const
{
    if (mate_slots == 0 || mate_slots > GDX_PAIR_MAX_MATE_SLOTS)
        fail(GDX_ERR_INVALID_ARGUMENT, "mate_slots must be 1..%u", GDX_PAIR_MAX_MATE_SLOTS);
    if (max_dist > 0x40000000u) fail(GDX_ERR_INVALID_ARGUMENT, "max_dist must not exceed 2^30");
    if (min_insert > max_insert || max_insert > 0x7fffffffu)
        fail(GDX_ERR_INVALID_ARGUMENT, "insert bounds [%u, %u]: min_insert <= max_insert <= 2^31 - 1", min_insert, max_insert);
    if (n_pairs > ~0ull / mate_slots / 2)
        fail(GDX_ERR_INVALID_ARGUMENT, "%llu pairs of 2 x %u slots: the number of slots does not fit 64 bits", (unsigned long long)n_pairs,
             mate_slots);
}

int FmIndex::pair_hits_many(uint64_t n_pairs, uint32_t mate_slots, const uint32_t *cand_query, const uint32_t *cand_begin,
                            const gdx_hit_t *cand_hits, const uint32_t *dist, const uint32_t *end, uint32_t max_dist,
                            uint32_t min_insert, uint32_t max_insert, uint32_t *out_n_proper, uint32_t *out_n_best,
                            uint32_t *out_pair_dist, uint32_t *out_sub_dist, uint32_t *out_mapq, uint32_t *out_pair_span,
                            uint32_t *out_mate_slot, uint32_t *out_mate_dist, uint32_t *out_win_query, uint32_t *out_win_begin,
                            gdx_hit_t *out_win_hits) const
{
    check_pair_hits(n_pairs, mate_slots, max_dist, min_insert, max_insert);
    if (n_pairs == 0) return GDX_OK;
    if (any_null({cand_query, cand_begin, cand_hits, dist, out_n_proper, out_n_best, out_pair_dist, out_sub_dist, out_mapq, out_pair_span,
                  out_mate_slot, out_mate_dist, out_win_query, out_win_begin, out_win_hits}))
        fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
    const uint64_t n_mates = 2 * n_pairs;
    hipStream_t stream = hipStreamPerThread;
    DeviceSlots slots(*this, cand_query, cand_begin, cand_hits, dist, end, n_mates * mate_slots, stream);
    DeviceBuffer<uint32_t> d_out(14 * n_pairs);  // six per pair, then four per mate
    DeviceBuffer<gdx_hit32_t> d_win(n_mates);
    uint32_t *o = d_out.get(), *w = o + 6 * n_pairs;
    const PairArgs a = {slots.args(max_dist, w + 2 * n_mates, w + 3 * n_mates, d_win.get()), n_pairs, mate_slots, min_insert, max_insert,
                        o, o + n_pairs, o + 2 * n_pairs, o + 3 * n_pairs, o + 4 * n_pairs, o + 5 * n_pairs, w, w + n_mates};
    launch_pair_hits(a, stream);
    GDX_HIP(hipGetLastError());
    download_columns({out_n_proper, out_n_best, out_pair_dist, out_sub_dist, out_mapq, out_pair_span}, o, n_pairs, stream);
    download_columns({out_mate_slot, out_mate_dist, out_win_query, out_win_begin}, w, n_mates, stream);
    widen_hits(out_win_hits, n_mates, d_win.get(), stream);
    return GDX_OK;
}

void FmIndex::check_mate_rescue(bool packed, uint64_t nq, uint64_t n_pairs, uint32_t mate_slots, uint32_t max_edits, uint32_t min_insert,
                                uint32_t max_insert) const
{
    check_edit_distance(packed, max_edits);
    if (mate_slots == 0 || mate_slots > GDX_PAIR_MAX_MATE_SLOTS)
        fail(GDX_ERR_INVALID_ARGUMENT, "mate_slots must be 1..%u", GDX_PAIR_MAX_MATE_SLOTS);
    if (min_insert > max_insert || max_insert > 0x7fffffffu)
        fail(GDX_ERR_INVALID_ARGUMENT, "insert bounds [%u, %u]: min_insert <= max_insert <= 2^31 - 1", min_insert, max_insert);
    if (max_insert - min_insert > GDX_RESCUE_MAX_SPREAD)
        fail(GDX_ERR_INVALID_ARGUMENT, "insert bounds [%u, %u] are more than GDX_RESCUE_MAX_SPREAD (%u) apart", min_insert, max_insert,
             GDX_RESCUE_MAX_SPREAD);
    if (nq >= 0xffffffffull) fail(GDX_ERR_INVALID_ARGUMENT, "more than 2^32 - 2 queries (win_query is 32 bits wide)");
    if (nq % 4 != 0 || nq / 4 != n_pairs)  // (not 4 * n_pairs, which wraps)
        fail(GDX_ERR_INVALID_ARGUMENT, "%llu queries for %llu pairs: a pair is four queries (both strands of both mates)",
             (unsigned long long)nq, (unsigned long long)n_pairs);
}

int FmIndex::mate_rescue_many(const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq, uint64_t n_pairs, uint32_t mate_slots,
                              const uint32_t *end, const uint32_t *n_proper, const uint32_t *mate_slot, const uint32_t *mate_dist,
                              const uint32_t *win_query, const uint32_t *win_begin, const gdx_hit_t *win_hits, uint32_t max_edits,
                              uint32_t min_insert, uint32_t max_insert, uint32_t *out_resc_dist, uint32_t *out_resc_end,
                              uint32_t *out_resc_mate, uint32_t *out_resc_pair_dist, uint32_t *out_resc_span, uint32_t *out_win_query,
                              uint32_t *out_win_begin, gdx_hit_t *out_win_hits) const
{
    check_mate_rescue(false, nq, n_pairs, mate_slots, max_edits, min_insert, max_insert);
    check_queries(qbuf, qoff, nq);
    if (n_pairs == 0) return GDX_OK;
    if (any_null({end, n_proper, mate_slot, mate_dist, win_query, win_begin, win_hits, out_resc_dist, out_resc_end, out_resc_mate,
                  out_resc_pair_dist, out_resc_span, out_win_query, out_win_begin, out_win_hits}))
        fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
    const uint64_t n_mates = 2 * n_pairs, n_slots = n_mates * mate_slots;
    hipStream_t stream = hipStreamPerThread;
    // the winners travel as slots do: query, begin, mate_dist in the place of dist and mate_slot in that of end
    DeviceSlots win(*this, win_query, win_begin, win_hits, mate_dist, mate_slot, n_mates, stream);
    const SlotArgs w = win.args(0, nullptr, nullptr, nullptr);
    DeviceQueries dq(qbuf, qoff, nq, stream);
    DeviceBuffer<uint32_t> d_in(n_slots + n_pairs);  // end, n_proper
    GDX_HIP(hipMemcpyAsync(d_in.get(), end, n_slots * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    GDX_HIP(hipMemcpyAsync(d_in.get() + n_slots, n_proper, n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    DeviceBuffer<uint32_t> d_out(11 * n_pairs);  // four per mate, then three per pair
    DeviceBuffer<gdx_hit32_t> d_win(n_mates);
    uint32_t *o = d_out.get(), *per_pair = o + 4 * n_mates;
    const RescueCall call = {n_pairs, mate_slots, max_edits, min_insert, max_insert, d_in.get(), d_in.get() + n_slots, w.end, w.dist,
                             w.cand_query, w.cand_begin, w.cand_hits, o, o + n_mates, per_pair, per_pair + n_pairs,
                             per_pair + 2 * n_pairs, o + 2 * n_mates, o + 3 * n_mates, d_win.get()};
    launch_mate_rescue(view_, dq.qbuf.get(), dq.qoff.get(), false, 0, call, stream);
    GDX_HIP(hipGetLastError());
    download_columns({out_resc_dist, out_resc_end, out_win_query, out_win_begin}, o, n_mates, stream);
    download_columns({out_resc_mate, out_resc_pair_dist, out_resc_span}, per_pair, n_pairs, stream);
    widen_hits(out_win_hits, n_mates, d_win.get(), stream);
    return GDX_OK;
}

int FmIndex::rank_many(const uint8_t *symbols, const uint64_t *idx, uint64_t m, uint64_t *out) const
{
    if (m == 0) return GDX_OK;
    if (!symbols || !idx || !out) fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
    make_current();
    hipStream_t stream = hipStreamPerThread;
    DeviceBuffer<uint8_t> d_sym(m);
    DeviceBuffer<uint32_t> d_idx(m), d_out(m), d_err(1);
    GDX_HIP(hipMemcpyAsync(d_sym.get(), symbols, m, hipMemcpyHostToDevice, stream));
    upload_narrowed(idx, d_idx.get(), m, n_, "rank index", stream);  // mod.rs:107-108 idx <= text_len
    GDX_HIP(hipMemsetAsync(d_err.get(), 0, sizeof(uint32_t), stream));
    launch_rank_many(view_, d_sym.get(), d_idx.get(), m, d_out.get(), d_err.get(), stream);
    GDX_HIP(hipGetLastError());
    uint32_t err = 0;
    GDX_HIP(hipMemcpyAsync(&err, d_err.get(), sizeof(err), hipMemcpyDeviceToHost, stream));
    download_widened(d_out.get(), out, m, stream);
    if (err) fail(GDX_ERR_INVALID_ARGUMENT, "rank: symbol >= alphabet size or idx > text_len (mod.rs:107-108)");
    return GDX_OK;
}

int FmIndex::symbol_at_many(const uint64_t *idx, uint64_t m, uint8_t *out) const
{
    if (m == 0) return GDX_OK;
    if (!idx || !out) fail(GDX_ERR_INVALID_ARGUMENT, "null argument");
    if (n_ == 0) fail(GDX_ERR_INVALID_ARGUMENT, "symbol_at: idx >= text_len (condensed.rs:344)");
    make_current();
    hipStream_t stream = hipStreamPerThread;
    DeviceBuffer<uint32_t> d_idx(m), d_err(1);
    DeviceBuffer<uint8_t> d_out(m);
    upload_narrowed(idx, d_idx.get(), m, n_ - 1, "symbol_at index", stream);
    GDX_HIP(hipMemsetAsync(d_err.get(), 0, sizeof(uint32_t), stream));
    launch_symbol_at_many(view_, d_idx.get(), m, d_out.get(), d_err.get(), stream);
    GDX_HIP(hipGetLastError());
    GDX_HIP(hipMemcpyAsync(out, d_out.get(), m, hipMemcpyDeviceToHost, stream));
    GDX_HIP(hipStreamSynchronize(stream));
    return GDX_OK;
}

}  // namespace gdx
