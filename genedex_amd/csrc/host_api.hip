// host_api.hip -- the host-pointer query calls (gdx_count_many, gdx_cursors_for_many_queries, gdx_locate_many[_alloc][_layout][32]):
// FmIndex::count_many / cursors_for_many_queries / locate_many of the reference (lib.rs:155-185) for callers whose
// queries and results live in host memory.
//
// A call is a pipeline over chunks of the batch, four chunks in flight (Slot), three host threads (ThreeStageRunner):
//
//     feeder thread + workers: user memory -> pinned staging  |  H2D (copy-in stream)  |  kernels (compute stream)
//     calling thread: waits for a chunk's search (locate: its number of hits), enqueues locate and the copies out
//                                                             |  D2H (copy-out stream) |  drainer thread + workers:
//                                                                                         pinned -> the user's arrays
//
// so that the PCIe transfers of chunk k + 1 / k - 1 run beside the kernels of chunk k and a call costs about
// max(H2D time, D2H time, kernel time) instead of their sum.  Results are order preserving: chunk boundaries are invisible
// to the caller.
//
// How it reads: a call site names its batch and outputs in a HostCall (fm_index.hpp); make_host_plan resolves it, with the
// index and the environment, into a HostPlan -- one of five result paths (enum Path: what crosses the link in which form is
// said there), the chunk list and the wire layout (host_plan.hpp), the sizes; fill_slots gives every slot the buffers of
// that path; the three stages (stage_in, stage_mid, stage_out) each dispatch over the path to one short function per path.
#include <malloc.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>

#include <sched.h>
#include <sys/mman.h>

#include "fm_index.hpp"
#include "host_plan.hpp"
#include "kernels.hpp"
#include "pack_host.hpp"
#include "wire_host.hpp"

namespace gdx {

namespace {
double now_seconds()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

constexpr int kSlots = 4;
std::atomic<uint64_t> g_chunk_bytes{32ull << 20};   // query bytes per chunk
std::atomic<uint64_t> g_chunk_queries{1ull << 20};  // and at most this many queries

// ---- a small persistent worker pool for the staging copies ------------------------------------------------
class WorkerPool {
public:
    explicit WorkerPool(unsigned n) : n_(n < 1 ? 1 : n)
    {
        for (unsigned i = 1; i < n_; i++) threads_.emplace_back([this, i] { loop(i); });
    }
    ~WorkerPool()
    {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
            gen_++;
        }
        cv_.notify_all();
        for (auto &t : threads_) t.join();
    }
    unsigned size() const { return n_; }
    // fn(worker, n_workers) on every worker (the caller is worker 0); returns when all are done
    void run(const std::function<void(unsigned, unsigned)> &fn)
    {
        {
            std::lock_guard<std::mutex> g(m_);
            fn_ = &fn;
            pending_ = n_ - 1;
            gen_++;
        }
        cv_.notify_all();
        fn(0, n_);
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [this] { return pending_ == 0; });
        fn_ = nullptr;
    }
    // [0, n) split into contiguous parts of whole `align` units
    template <class F>
    void parallel_range(uint64_t n, uint64_t align, F f)
    {
        if (n < (1u << 16) || n_ == 1) {
            f(0, n);
            return;
        }
        run([&](unsigned w, unsigned nw) {
            const uint64_t per = (n / nw + align) / align * align;
            const uint64_t lo = std::min<uint64_t>(n, per * w), hi = std::min<uint64_t>(n, lo + per);
            if (hi > lo) f(lo, hi);
        });
    }

private:
    void loop(unsigned idx)
    {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(unsigned, unsigned)> *fn = nullptr;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&] { return gen_ != seen; });
                seen = gen_;
                if (stop_) return;
                fn = fn_;
            }
            if (fn) (*fn)(idx, n_);
            {
                std::lock_guard<std::mutex> g(m_);
                if (--pending_ == 0) done_.notify_one();
            }
        }
    }
    unsigned n_;
    std::vector<std::thread> threads_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(unsigned, unsigned)> *fn_ = nullptr;
    unsigned pending_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

// CPUs this process may use: the affinity mask cut by the cgroup quota (a container on a 256-thread host may own 16)
unsigned usable_cpus()
{
    static const unsigned n = [] {
        unsigned cpus = std::thread::hardware_concurrency();
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) cpus = static_cast<unsigned>(CPU_COUNT(&set));
        if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota> <period>" or "max <period>"
            char quota[32] = {0};
            unsigned long period = 0;
            if (std::fscanf(f, "%31s %lu", quota, &period) == 2 && period != 0 && std::strcmp(quota, "max") != 0)
                cpus = std::min<unsigned>(cpus, std::max(1ul, std::strtoul(quota, nullptr, 10) / period));
            std::fclose(f);
        } else if (FILE *g = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {  // cgroup v1 (period 100 ms default)
            long q = -1;
            if (std::fscanf(g, "%ld", &q) == 1 && q > 0) cpus = std::min<unsigned>(cpus, std::max(1l, q / 100000));
            std::fclose(g);
        }
        return std::max(1u, cpus);
    }();
    return n;
}

// workers of ONE pool; a call runs two pools (staging in, draining out) beside its three pipeline threads
unsigned host_threads()
{
    static const unsigned n = [] {
        if (const char *e = getenv("GDX_HOST_THREADS")) return static_cast<unsigned>(std::max(1, atoi(e)));
        const unsigned cpus = usable_cpus();
        return std::min(16u, std::max(2u, cpus > 6u ? (cpus - 2u) / 2u : 2u));
    }();
    return n;
}

// ---- grow-only pinned host memory and device memory per (thread, device, slot) -----------------------------
struct Buf {
    void *ptr = nullptr;
    size_t bytes = 0;
};
struct BufCache {
    std::vector<std::pair<uint64_t, Buf>> pinned, device;  // key = device << 8 | id
    ~BufCache()
    {
        for (auto &kv : pinned)
            if (kv.second.ptr) (void)hipHostFree(kv.second.ptr);
        for (auto &kv : device)
            if (kv.second.ptr) (void)hipFree(kv.second.ptr);
    }
};
BufCache &cache()
{
    thread_local BufCache c;
    return c;
}
void *cached(std::vector<std::pair<uint64_t, Buf>> &v, uint64_t key, size_t bytes, bool pinned)
{
    Buf *b = nullptr;
    for (auto &kv : v)
        if (kv.first == key) b = &kv.second;
    if (!b) {
        v.emplace_back(key, Buf{});
        b = &v.back().second;
    }
    if (b->bytes < bytes) {
        if (b->ptr) {
            GDX_HIP(hipDeviceSynchronize());
            if (pinned) GDX_HIP(hipHostFree(b->ptr));
            else GDX_HIP(hipFree(b->ptr));
            b->ptr = nullptr;
            b->bytes = 0;
        }
        const size_t want = bytes + bytes / 4 + 4096;
        if (pinned) GDX_HIP(hipHostMalloc(&b->ptr, want, hipHostMallocDefault));
        else GDX_HIP(hipMalloc(&b->ptr, want));
        b->bytes = want;
    }
    return b->ptr;
}
template <class T>
T *pinned_buf(int device, int id, size_t count)
{
    return static_cast<T *>(cached(cache().pinned, (static_cast<uint64_t>(device) << 8) | id, count * sizeof(T) + 16, true));
}
template <class T>
T *device_buf(int device, int id, size_t count)
{
    return static_cast<T *>(cached(cache().device, (static_cast<uint64_t>(device) << 8) | id, count * sizeof(T) + 16, false));
}

struct Streams {
    hipStream_t in = nullptr, k = nullptr, out = nullptr;
    hipEvent_t ev_in[kSlots] = {}, ev_k[kSlots] = {}, ev_out[kSlots] = {}, ev_total[kSlots] = {};
    Streams()
    {
        GDX_HIP(hipStreamCreateWithFlags(&in, hipStreamNonBlocking));
        GDX_HIP(hipStreamCreateWithFlags(&k, hipStreamNonBlocking));
        GDX_HIP(hipStreamCreateWithFlags(&out, hipStreamNonBlocking));
        for (int s = 0; s < kSlots; s++) {
            GDX_HIP(hipEventCreateWithFlags(&ev_in[s], hipEventDisableTiming));
            GDX_HIP(hipEventCreateWithFlags(&ev_k[s], hipEventDisableTiming));
            GDX_HIP(hipEventCreateWithFlags(&ev_out[s], hipEventDisableTiming));
            GDX_HIP(hipEventCreateWithFlags(&ev_total[s], hipEventDisableTiming));
        }
    }
    ~Streams()
    {
        for (int s = 0; s < kSlots; s++) {
            if (ev_in[s]) (void)hipEventDestroy(ev_in[s]);
            if (ev_k[s]) (void)hipEventDestroy(ev_k[s]);
            if (ev_out[s]) (void)hipEventDestroy(ev_out[s]);
            if (ev_total[s]) (void)hipEventDestroy(ev_total[s]);
        }
        if (in) (void)hipStreamDestroy(in);
        if (k) (void)hipStreamDestroy(k);
        if (out) (void)hipStreamDestroy(out);
    }
};

__global__ __launch_bounds__(256) void unpack_status_kernel(const uint4 *__restrict__ rec, uint64_t nq,
                                                            uint8_t *__restrict__ status)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t q = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; q < nq; q += stride)
        status[q] = static_cast<uint8_t>(rec[q].w >> 24);
}

// *flag |= 1 when a status byte is not 0 (then, and only then, a chunk's status bytes cross the link)
__global__ __launch_bounds__(256) void any_status_kernel(const uint8_t *__restrict__ status, uint64_t nq, unsigned long long *__restrict__ flag)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u, quads = nq / 16u;
    uint32_t any = 0;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < quads; i += stride) {
        const uint4 v = reinterpret_cast<const uint4 *>(status)[i];
        any |= v.x | v.y | v.z | v.w;
    }
    if (blockIdx.x == 0 && threadIdx.x < (nq & 15u)) any |= status[quads * 16u + threadIdx.x];
    if (any != 0u) atomicOr(flag, 1ull);
}

void check_queries(const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq, WorkerPool &pool, uint64_t uniform_len)
{
    if (nq >= 0xffffffffull) fail(GDX_ERR_UNSUPPORTED, "more than 2^32-2 queries in one call");
    if (uniform_len != 0) {  // a uniform batch: query i = symbols [i * uniform_len, (i + 1) * uniform_len), no offsets
        if (uniform_len >= (1ull << 21)) fail(GDX_ERR_INVALID_ARGUMENT, "uniform_len must be below 2^21");
        if (nq != 0 && !qbuf) fail(GDX_ERR_INVALID_ARGUMENT, "qbuf is null");
        return;
    }
    if (!qoff) fail(GDX_ERR_INVALID_ARGUMENT, "qoff is null");
    std::atomic<bool> bad{false};
    pool.parallel_range(nq, 1, [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; i++)
            if (qoff[i + 1] < qoff[i]) bad.store(true);
    });
    if (bad.load()) fail(GDX_ERR_INVALID_ARGUMENT, "qoff must be non-decreasing");
    if (qoff[nq] > qoff[0] && !qbuf) fail(GDX_ERR_INVALID_ARGUMENT, "qbuf is null");
}

// every slot's u32 offsets (entries 1 .. n of a chunk) shifted by the hits of the chunks before it
__global__ __launch_bounds__(256) void add_hit_base_kernel(uint32_t *__restrict__ off, uint64_t n, uint32_t base)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n; i += stride) off[i] += base;
}

// true: `p` is host memory the device can copy from directly (hipHostMalloc / hipHostRegister): no staging copy
bool is_pinned_host(const void *p)
{
    if (p == nullptr) return false;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();  // (ordinary pageable memory: not an error of the call)
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

// A chunk of the wide locate calls whose hits do not fit the fused step's 32-bit offsets: the call is run again on the plain
// path (u64 offsets throughout), which has no such limit (FmIndex::locate_wide)
struct RetryWithWideOffsets {};
// (tests: GDX_TEST_CHUNK_HIT_LIMIT lowers the number of hits a chunk of the fused step may hold; read per call)
uint64_t chunk_hit_limit()
{
    const char *e = getenv("GDX_TEST_CHUNK_HIT_LIMIT");
    const uint64_t v = e ? std::strtoull(e, nullptr, 10) : 0;
    return v != 0 ? v : 0xffffffffull;
}
// GDX_HOST_TIMING=1 (debug): where the three threads spend the call, in seconds
bool host_timing()
{
    static const bool timing = getenv("GDX_HOST_TIMING") != nullptr;
    return timing;
}

using Kind = HostCall::Kind;

// ---- the plan of a call: its result path, chunks and sizes, resolved once ----------------------------------------------------
// How a chunk's results cross the link and reach the caller's arrays:
//   kIntervals, kCounts  search; u32 borders / counts by D2H copy, widened by the drainer; the status bytes stay on the device
//                        unless one of the chunk's is set
//   kPlainLocate         search | the chunk's total to the host | locate; u64 offsets and 8-byte hits (GDX_HOST_WIDE_HITS=1: 16-byte
//                        hits, the drainer then only copies) by D2H copy, shifted and widened by the drainer.  The wide calls when
//                        the wire is off, their sizing call (no hit buffer: the locate launch is skipped) and their second run
//   kStepDma             every chunk is ONE fused step (launch_locate_step: search, totals, u32 offsets, 8-byte hits, no host round
//                        trip); offsets and hits go by D2H copy straight into the pinned arrays of the sink (narrow call only)
//   kStepWire            the fused step, then the "found bitmap" wire the multi-GPU gather uses (launch_wire_pack: a bit per read,
//                        position + text id byte per found read, the exceptions with their hits -- 3.7-4.6 bytes per read instead of
//                        12.2 narrow / 16.2 wide), expanded into the caller's arrays by the drainer's workers (wire_host.hpp): the
//                        link's two directions share its rate (65 GB/s together on the test box against 57 alone), so bytes saved
//                        going out are time saved.  The default of the narrow and the wide locate calls.  GDX_HOST_RESULTS=dma: the
//                        device-written forms (hosts with few cores to spare).  Collections of more than 256 texts take those too
//                        (text ids travel as bytes).
enum class Path { kIntervals, kCounts, kPlainLocate, kStepDma, kStepWire };

struct HostPlan {
    Path path = Path::kCounts;
    bool flagged = false;       // kIntervals, kCounts
    bool stepped = false;       // kStepDma, kStepWire
    bool sizing_only = false;   // gdx_locate_many without a hit buffer: search, totals and offsets only
    bool host_pack = false;     // ASCII chunks are packed by the feeder's workers and cross the link as 2-bit codes
    bool pinned_input = false;  // the caller's query buffer is pinned: no staging copy
    bool wide_hits = false;     // kPlainLocate: 16-byte hits from the device (GDX_HOST_WIDE_HITS=1)
    size_t hit_bytes = 0;       // kPlainLocate: of a hit on the link
    PackPlan pack_plan;
    uint64_t hit_limit = 0;     // hits a chunk of the fused step may hold (wide calls)
    unsigned in_threads = 1;    // workers of the feeder
    std::vector<HostChunk> chunks;
    uint64_t max_nq = 0, qbuf_cap = 0;  // the largest chunk's queries, and the bytes a slot's query buffer holds
    uint64_t n32_cap = 0;               // stepped: hit slots a chunk's device buffers hold
    WireLayout wl;
};

// (call, index, environment) -> plan; the batch is checked on the way (check_queries).  nq == 0: no chunks.
HostPlan make_host_plan(const HostCall &call, const FmIndex &ix, WorkerPool &pool)
{
    static const int narrow_mode = [] {
        const char *e = getenv("GDX_HOST_RESULTS");
        if (e && std::strcmp(e, "dma") == 0) return 0;
        if (e && std::strcmp(e, "wire") == 0) return 1;
        return host_threads() >= 4 ? 1 : 0;
    }();
    const IndexView &view = ix.view();
    const Kind kind = call.kind;
    const bool locate = kind == Kind::kLocate || kind == Kind::kLocate32;
    HostPlan p;
    // A sizing call of gdx_locate_many: nothing is located, packed or copied out that the call would throw away
    p.sizing_only = kind == Kind::kLocate && call.grow_hits == nullptr && (call.hits == nullptr || call.hits_capacity == 0);
    const bool wire = locate && narrow_mode == 1 && ix.num_texts() <= 256 && !p.sizing_only && !(kind == Kind::kLocate && call.plain_locate_only);
    p.flagged = !locate;
    p.stepped = kind == Kind::kLocate32 || wire;
    p.path = kind == Kind::kIntervals ? Path::kIntervals
             : kind == Kind::kCounts  ? Path::kCounts
             : !p.stepped             ? Path::kPlainLocate
                                      : (wire ? Path::kStepWire : Path::kStepDma);
    p.pinned_input = is_pinned_host(call.qbuf);
    check_queries(call.qbuf, call.qoff, call.nq, pool, call.uniform_len);
    // ASCII batches of the count / locate calls are packed ON THE HOST, chunk by chunk in the feeder's worker pool (pack_host.hpp:
    // 32 symbols per step when the alphabet's table has a nucleotide alphabet's shape), and cross the link as 2-bit codes -- 12.5
    // bytes per len-50 read (+ 8 of offsets) instead of 58: the link, not the kernels, bounds these calls.  A chunk that holds a
    // symbol 2 bits cannot name (N, an invalid byte) goes as it is, ASCII, and gives the reference's result for it.  Exact
    // intervals stay ASCII (their kernels read bytes).  GDX_HOST_PACK=0: never.
    const bool env_host_pack = [] { const char *e = getenv("GDX_HOST_PACK"); return !(e && atoi(e) == 0); }();  // (read per call: tests)
    p.pack_plan = make_pack_plan(ix.config().io_to_dense);
    p.host_pack = !call.packed && env_host_pack && kind != Kind::kIntervals && view.layout == 0 && view.n_searchable >= 4 &&
                  p.pack_plan.fast && pack_have_avx2();
    if (call.nq == 0) return p;
    if (kind == Kind::kLocate32 && call.narrow == nullptr) fail(GDX_ERR_INVALID_ARGUMENT, "internal: the narrow locate needs its sink");
    // hits leave the device NARROW (gdx_hit32_t, 8 bytes) and are widened into the ABI's 16-byte gdx_hit_t by the drainer's
    // workers: with reads handed over as 2-bit codes the D2H link is the longer leg of a locate call (23 bytes per read out
    // against 12.5 in), and the drainer reads half as much from the staging buffer
    static const bool wide_hits = [] { const char *e = getenv("GDX_HOST_WIDE_HITS"); return e && atoi(e) != 0; }();
    p.wide_hits = wide_hits;
    p.hit_bytes = wide_hits ? sizeof(gdx_hit_t) : sizeof(gdx_hit32_t);
    p.hit_limit = chunk_hit_limit();
    // (a feeder that packs is the call's bound: it gets half as many workers again as the drainer -- 10 of a 16-CPU container's:
    // count 1.0 -> 2.1, wide locate 0.9 -> 1.8 G reads/s on one box; both pools at 10 or 14 were slower than both at 7.
    // GDX_HOST_IN_THREADS: experiments)
    p.in_threads = [&] {
        if (const char *e = getenv("GDX_HOST_IN_THREADS")) return static_cast<unsigned>(std::max(1, atoi(e)));
        if (!p.host_pack || getenv("GDX_HOST_THREADS")) return host_threads();
        const unsigned cpus = usable_cpus();
        return std::max(host_threads(), std::min(host_threads() * 3u / 2u, cpus > 4u ? cpus - 4u : 1u));
    }();
    // (a chunk's limit counts the bytes that cross the link: four symbols per byte of a packed batch; the fused step is a dozen
    // launches per chunk and takes up to four times the queries)
    p.chunks = plan_host_chunks(call.qoff, call.nq, call.uniform_len, g_chunk_bytes.load() * ((call.packed || p.host_pack) ? 4 : 1),
                                g_chunk_queries.load() * (p.stepped ? 4 : 1));
    uint64_t max_bytes = 0;
    for (const HostChunk &c : p.chunks) {
        p.max_nq = std::max(p.max_nq, c.nq);
        max_bytes = std::max(max_bytes, c.bytes);
    }
    // (packed: max_bytes counts symbols, four per byte, and a chunk starts up to seven symbols before its first query)
    p.qbuf_cap = div_ceil((call.packed ? div_ceil(max_bytes + 8, 4) : max_bytes) + 1, 8) * 8 + 24;
    if (p.stepped) p.n32_cap = p.max_nq + p.max_nq / 4 + 4096;
    p.wl = make_wire_layout(p.max_nq, ix.num_texts());
    return p;
}

// ---- a slot: the buffers of one chunk in flight ------------------------------------------------------------------------------
// Buffer ids of the grow-only cache (slot * 16 + id).  The numbers are kept from when they were literals: calls of different
// kinds on one thread then share the blocks they always shared (pinned 7 and 8 and device 5, 7, 8, 9 serve two paths each).
enum PinnedId { kPinIn = 0, kPinQoff = 1, kPinA = 2, kPinB = 3, kPinStatus = 4, kPinTotal = 5, kPinHits = 6, kPinWire = 7, kPinExc = 8, kPinOff = 10 };
enum DeviceId {
    kDevQbuf = 0, kDevQoff = 1, kDevA = 2, kDevB = 3, kDevStatus = 4, kDevRec = 5, kDevOff = 6, kDevScan = 7, kDevHits = 8, kDevWs = 9,
    kDevWireWs = 10, kDevCmp = 11, kDevOff32 = 12, kDevTotals = 13, kDevWire = 14, kDevExc = 15
};

struct Slot {
    int dev = 0, s = 0;
    // every path: the chunk's queries, pinned and on the device; narrow results a / b (counts, or interval borders), status bytes
    uint8_t *h_in = nullptr, *d_qbuf = nullptr, *h_status = nullptr, *d_status = nullptr;
    uint64_t *h_qoff = nullptr, *d_qoff = nullptr;
    uint32_t *h_a = nullptr, *h_b = nullptr, *d_a = nullptr, *d_b = nullptr;
    uint64_t *h_total = nullptr;          // [0..2] totals / the any-status flag, [4..5] the wire's meta
    unsigned long long *d_tot = nullptr;  // flagged: the any-status flag; stepped: the step's totals
    // the locate paths
    uint4 *d_rec = nullptr;
    void *d_scan = nullptr, *d_hits = nullptr, *h_hits = nullptr, *d_ws = nullptr;
    uint64_t *d_off = nullptr, *h_off = nullptr;  // plain: the chunk's hit offsets (h_off[i] = hits of its queries before query i)
    uint32_t *d_cmp = nullptr, *d_off32 = nullptr;  // stepped
    // the wire: sections at HostPlan::wl's offsets on both sides; the exceptions {reads | counts | hits} (pinned: packed tight)
    uint8_t *d_wire = nullptr, *h_wire = nullptr, *d_exc = nullptr, *h_exc = nullptr, *d_wws = nullptr;
    uint64_t exc_hits_cap = 0;
    uint64_t w_found = 0, w_exc = 0, w_exc_hits = 0;  // of the chunk in the slot: found reads, exceptions, their hits
    bool w_status = false;                            // and: its status bytes crossed the link (one of them is set)

    // INVARIANT: every call of these two runs on the calling thread of the pipeline (fill_slots, the middle stage).  The cache
    // behind them is thread_local and grow-only; the feeder and the drainer live for one call, so a block they asked for would
    // be allocated anew in every call and freed when the thread ends, under the copies still on their way.
    template <class T>
    T *pinned(PinnedId id, size_t count) const { return pinned_buf<T>(dev, s * 16 + id, count); }
    template <class T>
    T *device(DeviceId id, size_t count) const { return device_buf<T>(dev, s * 16 + id, count); }
};

// one call's state, shared by the stages
struct HostRun {
    const HostCall &call;
    const HostPlan plan;
    std::vector<HostChunk> chunks;  // the plan's, with the totals filled in as the call runs
    const IndexView &view;
    const uint8_t *io_to_dense;
    const QueryOptions qo;
    WorkerPool &pool;  // the drainer's workers
    Streams st;
    Slot slots[kSlots];
    size_t scan_bytes = 0;  // kPlainLocate: of the offsets scan's workspace
    gdx_hit_t *hits = nullptr;  // wide locate: the caller's (or grow_hits') array as it stands
    uint64_t hits_capacity = 0;
    std::atomic<bool> any_status{false};
    uint64_t hit_base = 0;      // hits of the chunks drained so far
    uint64_t mid_hit_base = 0;  // stepped: hits of the chunks whose copies out are enqueued
    bool capacity_ok = true;    // wide locate: the caller's buffer holds everything so far
    double t_out_sync = 0;      // (timing) the drainer's wait for the copies out

    HostRun(const HostCall &c, HostPlan &&p, const FmIndex &ix, WorkerPool &drain_pool)
        : call(c), plan(std::move(p)), chunks(plan.chunks), view(ix.view()), io_to_dense(ix.config().io_to_dense), qo(ix.query_options()),
          pool(drain_pool), hits(c.hits), hits_capacity(c.hits_capacity)
    {
    }
};

// Which path needs which buffer.  Sizes: for the largest chunk; hits of the plain path and a chunk of the fused step with
// more hits than n32_cap grow theirs in the middle stage.
void fill_slots(HostRun &r, int dev)
{
    const HostPlan &p = r.plan;
    const uint64_t max_nq = p.max_nq;
    if (p.path == Path::kPlainLocate) r.scan_bytes = hit_offsets_rec_temp_bytes(max_nq);
    const size_t tws = p.stepped ? scan_totals_workspace_bytes(max_nq) : 0;
    for (int s = 0; s < kSlots; s++) {
        Slot &sl = r.slots[s];
        sl.dev = dev, sl.s = s;
        // (all of these for every path, a / d_a of a locate call too: the cache holds the same blocks whichever call came first)
        sl.h_in = sl.pinned<uint8_t>(kPinIn, p.qbuf_cap);
        sl.h_qoff = sl.pinned<uint64_t>(kPinQoff, max_nq + 1);
        sl.h_a = sl.pinned<uint32_t>(kPinA, max_nq);
        sl.h_status = sl.pinned<uint8_t>(kPinStatus, max_nq);
        sl.h_total = sl.pinned<uint64_t>(kPinTotal, p.path == Path::kPlainLocate ? 1 : 8);
        sl.d_qbuf = sl.device<uint8_t>(kDevQbuf, p.qbuf_cap);
        sl.d_qoff = sl.device<uint64_t>(kDevQoff, max_nq + 1);
        sl.d_a = sl.device<uint32_t>(kDevA, max_nq);
        sl.d_status = sl.device<uint8_t>(kDevStatus, max_nq);
        switch (p.path) {
        case Path::kIntervals:
            sl.h_b = sl.pinned<uint32_t>(kPinB, max_nq);
            sl.d_b = sl.device<uint32_t>(kDevB, max_nq);
            [[fallthrough]];
        case Path::kCounts:
            sl.d_tot = sl.device<unsigned long long>(kDevTotals, 4);
            break;
        case Path::kPlainLocate:
            sl.d_rec = sl.device<uint4>(kDevRec, max_nq);
            sl.d_off = sl.device<uint64_t>(kDevOff, max_nq + 1);
            sl.d_scan = sl.device<uint8_t>(kDevScan, r.scan_bytes ? r.scan_bytes : 1);
            sl.h_off = sl.pinned<uint64_t>(kPinOff, max_nq + 1);
            break;  // (d_hits, h_hits, d_ws: sized for the chunk's total in the middle stage)
        case Path::kStepWire:
            sl.d_wire = sl.device<uint8_t>(kDevWire, p.wl.bytes);
            sl.h_wire = sl.pinned<uint8_t>(kPinWire, p.wl.bytes);
            sl.exc_hits_cap = p.n32_cap;
            sl.d_exc = sl.device<uint8_t>(kDevExc, p.wl.exc_hits + sl.exc_hits_cap * sizeof(gdx_hit32_t));
            sl.d_wws = sl.device<uint8_t>(kDevWireWs, wire_pack_workspace_bytes(max_nq));
            [[fallthrough]];  // (h_exc: sized for the chunk's exceptions in the middle stage)
        case Path::kStepDma:
            sl.d_rec = sl.device<uint4>(kDevRec, max_nq);
            sl.d_cmp = sl.device<uint32_t>(kDevCmp, max_nq);
            sl.d_off32 = sl.device<uint32_t>(kDevOff32, max_nq + 1);
            sl.d_tot = sl.device<unsigned long long>(kDevTotals, 4);
            sl.d_scan = sl.device<uint8_t>(kDevScan, tws ? tws : 1);
            sl.d_hits = sl.device<uint8_t>(kDevHits, p.n32_cap * sizeof(gdx_hit32_t));
            sl.d_ws = sl.device<uint8_t>(kDevWs, locate_workspace_bytes(p.n32_cap));
            break;
        }
    }
}

// ---- the three-thread loop ---------------------------------------------------------------------------------------------------
// Software pipeline with three host threads: the feeder stages chunks in (its own worker pool) as soon as a slot is free;
// the calling thread waits for the search of chunk k (locate: for its number of hits), enqueues locate and the copies out;
// the drainer widens chunk k - 1 into the caller's arrays (its own pool).  Copy-in, kernels, copy-out and both host-side
// copies of different chunks overlap; with the middle and the drain stage on one thread the locate call took 1.6-1.8 x the
// PCIe time of its input, the thread being busy widening hits while a finished search waited for its locate launch.
// A stage that throws stops all three; the first exception is thrown again when both side threads are joined and the device
// is idle.
class ThreeStageRunner {
public:
    using Stage = std::function<void(size_t)>;
    // out_sync: seconds of stage_out's work that were a wait for the copies out (the timing line names them)
    void run(size_t n_chunks, int dev, const Stage &stage_in, const Stage &stage_mid, const Stage &stage_out, const double &out_sync)
    {
        Times t_in, t_mid, t_out;
        std::thread feeder([&] { loop(n_chunks, dev, stage_in, staged_, [&](size_t k) { return k < drained_ + kSlots; }, t_in); });
        std::thread drainer([&] { loop(n_chunks, dev, stage_out, drained_, [&](size_t k) { return launched_ > k; }, t_out); });
        loop(n_chunks, -1, stage_mid, launched_, [&](size_t k) { return staged_ > k; }, t_mid);
        feeder.join();
        drainer.join();
        if (host_timing())
            fprintf(stderr, "gdx host pipeline: %zu chunks; feeder wait %.3f work %.3f; launcher wait %.3f work %.3f; drainer wait %.3f work %.3f (of it %.3f waiting for the copies out)\n",
                    n_chunks, t_in.wait, t_in.work, t_mid.wait, t_mid.work, t_out.wait, t_out.work, out_sync);
        if (error_) {
            (void)hipDeviceSynchronize();
            std::rethrow_exception(error_);
        }
    }

private:
    struct Times {
        double wait = 0, work = 0;
    };
    // chunk after chunk: wait until ready(k), run the stage, publish `done` = k + 1.  dev >= 0: a side thread, which makes the
    // device current first
    template <class Ready>
    void loop(size_t n_chunks, int dev, const Stage &stage, size_t &done, Ready ready, Times &t)
    {
        const bool timing = host_timing();
        try {
            if (dev >= 0) GDX_HIP(hipSetDevice(dev));
            for (size_t k = 0; k < n_chunks; k++) {
                const double t0 = timing ? now_seconds() : 0.0;
                {
                    std::unique_lock<std::mutex> g(mu_);
                    cv_.wait(g, [&] { return abort_ || ready(k); });
                    if (abort_) return;
                }
                const double t1 = timing ? now_seconds() : 0.0;
                stage(k);
                if (timing) {
                    t.wait += t1 - t0;
                    t.work += now_seconds() - t1;
                }
                {
                    std::lock_guard<std::mutex> g(mu_);
                    done = k + 1;
                }
                cv_.notify_all();
            }
        } catch (...) {
            std::lock_guard<std::mutex> g(mu_);
            if (!error_) error_ = std::current_exception();
            abort_ = true;
            cv_.notify_all();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_;
    size_t staged_ = 0, launched_ = 0, drained_ = 0;  // chunks staged in / with their copy-out enqueued / fully drained
    bool abort_ = false;
    std::exception_ptr error_;
};

// ---- stage in (feeder thread): user memory -> pinned staging -> device, the chunk's kernels enqueued -------------------------
struct StagedChunk {
    bool as_packed = false;    // the chunk is on the device as 2-bit codes (the caller's, or made by the feeder's workers)
    uint64_t uniform_len = 0;  // != 0: every query of the chunk has this many symbols, and no offsets went over
};

// The shared front of every path: host pack, staging copy or pinned pass-through, zero padding, offsets rebase, H2D copies;
// the compute stream then waits for them
StagedChunk stage_queries(HostRun &r, size_t k, WorkerPool &pool)
{
    const HostPlan &p = r.plan;
    const Slot &sl = r.slots[k % kSlots];
    const HostChunk &c = r.chunks[k];
    const uint8_t *qbuf = r.call.qbuf;
    const uint64_t *qoff = r.call.qoff;
    const uint64_t uniform_len = r.call.uniform_len;
    const bool uniform = uniform_len != 0;
    auto off_of = [&](uint64_t i) { return uniform ? i * uniform_len : qoff[i]; };
    bool as_packed = r.call.packed, packed_here = false;  // packed_here: the chunk's codes were made by this thread's workers, in h_in
    uint64_t chunk_uniform = uniform ? uniform_len : 0;
    if (p.host_pack && c.bytes != 0) {
        // the chunk's symbols are packed from ITS first symbol on (symbol j of the chunk in bits 2 (j & 3) of byte j >> 2)
        const uint64_t first = off_of(c.q0), n_sym = off_of(c.q0 + c.nq) - first, nb = div_ceil(n_sym, 4);
        std::atomic<bool> other{false};  // a symbol that is not one of the dense codes 1..4
        std::atomic<bool> ragged{false};
        const uint64_t len0 = uniform ? uniform_len : qoff[c.q0 + 1] - qoff[c.q0];
        uint8_t *out = sl.h_in;
        pool.run([&](unsigned w, unsigned nw) {
            const uint64_t per = (nb / nw + 64) / 64 * 64;
            const uint64_t lo = std::min(nb, per * w), hi = std::min(nb, lo + per);
            pack_range(p.pack_plan, r.io_to_dense, qbuf + first, 0, n_sym, lo, hi, out,
                       [&](uint64_t) { other.store(true, std::memory_order_relaxed); });
            // reads of one length (a sequencer's) need no offsets at all: neither rebased, nor copied, nor read by the kernels
            if (!uniform && len0 != 0) {
                const uint64_t qper = div_ceil(c.nq, nw), q_lo = std::min(c.nq, qper * w), q_hi = std::min(c.nq, q_lo + qper);
                bool same = true;
                for (uint64_t i = q_lo; i < q_hi; i++) same &= qoff[c.q0 + i + 1] - qoff[c.q0 + i] == len0;
                if (!same) ragged.store(true, std::memory_order_relaxed);
            }
        });
        as_packed = packed_here = !other.load();
        if (packed_here && !uniform && len0 != 0 && len0 < (1ull << 21) && !ragged.load()) chunk_uniform = len0;
    }
    // packed (by the caller): the chunk starts at the 16-bit unit that holds its first symbol, offsets are rebased to that unit
    const uint64_t base = (as_packed && !packed_here) ? (off_of(c.q0) & ~7ull) : off_of(c.q0);
    const uint64_t src_byte = as_packed ? base / 4 : base;
    const uint64_t n_bytes = as_packed ? div_ceil(off_of(c.q0 + c.nq) - base, 4) : c.bytes;
    if (!p.pinned_input && !packed_here)
        pool.parallel_range(n_bytes, 64, [&](uint64_t lo, uint64_t hi) { stream_copy(sl.h_in + lo, qbuf + src_byte + lo, hi - lo); });
    if (chunk_uniform == 0)
        pool.parallel_range(c.nq + 1, 8, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t i = lo; i < hi; i++) sl.h_qoff[i] = qoff[c.q0 + i] - base;
        });
    const uint64_t padded = div_ceil(n_bytes + 2, 8) * 8;
    if (p.pinned_input && !packed_here) {  // the caller's buffer is pinned: the device reads it as it is, no staging copy
        if (n_bytes) GDX_HIP(hipMemcpyAsync(sl.d_qbuf, qbuf + src_byte, n_bytes, hipMemcpyHostToDevice, r.st.in));
        GDX_HIP(hipMemsetAsync(sl.d_qbuf + n_bytes, 0, padded - n_bytes, r.st.in));  // windows may read past the last query
    } else {
        std::memset(sl.h_in + n_bytes, 0, padded - n_bytes);
        GDX_HIP(hipMemcpyAsync(sl.d_qbuf, sl.h_in, padded, hipMemcpyHostToDevice, r.st.in));
    }
    if (chunk_uniform == 0) GDX_HIP(hipMemcpyAsync(sl.d_qoff, sl.h_qoff, (c.nq + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, r.st.in));
    GDX_HIP(hipEventRecord(r.st.ev_in[sl.s], r.st.in));
    GDX_HIP(hipStreamWaitEvent(r.st.k, r.st.ev_in[sl.s], 0));
    return StagedChunk{as_packed, chunk_uniform};
}

// the query side of the chunk's search
SearchCall chunk_search_call(const Slot &sl, const HostChunk &c, const StagedChunk &sc)
{
    SearchCall call;
    call.d_qbuf = sl.d_qbuf;
    if (sc.uniform_len != 0) {  // (the chunk starts at its first symbol: it is a uniform batch of its own)
        call.uniform_len = static_cast<uint32_t>(sc.uniform_len);
    } else {
        call.d_qbeg = sl.d_qoff;
        call.d_qend = sl.d_qoff + 1;
    }
    call.nq = c.nq;
    call.packed = sc.as_packed;
    return call;
}

// kIntervals, kCounts: search, then *d_tot |= 1 when a status byte of the chunk is set
void enqueue_flagged(HostRun &r, const Slot &sl, const HostChunk &c, SearchCall call)
{
    if (r.plan.path == Path::kIntervals) {
        call.d_start = sl.d_a;
        call.d_end = sl.d_b;
        call.mode = 0;
    } else {
        call.d_count = sl.d_a;
        call.mode = 1;
    }
    call.d_status = sl.d_status;
    launch_search_call(r.view, call, r.st.k, r.qo);
    GDX_HIP(hipGetLastError());
    GDX_HIP(hipEventRecord(r.st.ev_k[sl.s], r.st.k));
    GDX_HIP(hipMemsetAsync(sl.d_tot, 0, sizeof(unsigned long long), r.st.k));
    hipLaunchKernelGGL(any_status_kernel, dim3(static_cast<unsigned>(std::min<uint64_t>(c.nq / 4096 + 1, 1024))), dim3(256), 0, r.st.k,
                       sl.d_status, c.nq, sl.d_tot);
    GDX_HIP(hipMemcpyAsync(sl.h_total, sl.d_tot, sizeof(uint64_t), hipMemcpyDeviceToHost, r.st.k));
    GDX_HIP(hipEventRecord(r.st.ev_total[sl.s], r.st.k));
}

// kPlainLocate: search into records, status unpack, offsets scan; the chunk's total goes to the host
void enqueue_plain_locate(HostRun &r, const Slot &sl, const HostChunk &c, SearchCall call)
{
    call.d_rec = sl.d_rec;
    call.mode = 1;
    launch_search_call(r.view, call, r.st.k, r.qo);
    GDX_HIP(hipGetLastError());
    const unsigned blocks = static_cast<unsigned>(std::min<uint64_t>((c.nq + 255) / 256, 4096));
    hipLaunchKernelGGL(unpack_status_kernel, dim3(blocks), dim3(256), 0, r.st.k, sl.d_rec, c.nq, sl.d_status);
    // (max_hits_per_query: a query gets slots for its first k rows only -- locate(q).take(k))
    launch_hit_offsets_rec(sl.d_rec, c.nq, sl.d_off, sl.d_scan, r.scan_bytes, r.st.k, r.qo.max_hits_per_query, true);
    GDX_HIP(hipMemcpyAsync(sl.h_total, sl.d_off + c.nq, sizeof(uint64_t), hipMemcpyDeviceToHost, r.st.k));
    GDX_HIP(hipEventRecord(r.st.ev_total[sl.s], r.st.k));
}

// kStepWire: the slot's offsets and hits -> its wire and exceptions; the wire's meta goes to the host behind the totals
void pack_wire(HostRun &r, const Slot &sl, uint64_t chunk_nq)
{
    const WireLayout &wl = r.plan.wl;
    const uint64_t max_nq = r.plan.max_nq;
    uint8_t *w = sl.d_wire, *e = sl.d_exc;
    WireHostForm hf;
    hf.d_exc_hits32 = reinterpret_cast<gdx_hit32_t *>(e + wl.exc_hits);
    hf.d_tile_off = reinterpret_cast<uint32_t *>(w + wl.tile_off);
    hf.d_found_ids = wl.ids ? w + wl.found_ids : nullptr;
    hf.ix = &r.view;
    hf.hits_stored = sl.exc_hits_cap;
    launch_wire_pack(sl.d_cmp, sl.d_off32, true, static_cast<const gdx_hit32_t *>(sl.d_hits), chunk_nq, w + wl.bitmap,
                     reinterpret_cast<uint32_t *>(w + wl.tile_found), reinterpret_cast<uint32_t *>(w + wl.found_pos), max_nq,
                     reinterpret_cast<uint32_t *>(e + wl.exc_reads), reinterpret_cast<uint32_t *>(e + wl.exc_counts), max_nq, nullptr,
                     nullptr, sl.exc_hits_cap, reinterpret_cast<uint32_t *>(w), sl.d_wws, r.st.k, &hf);
    GDX_HIP(hipGetLastError());
    GDX_HIP(hipMemcpyAsync(sl.h_total + 4, w, 16, hipMemcpyDeviceToHost, r.st.k));
}

// kStepDma, kStepWire: the fused step (search, totals, u32 offsets, 8-byte hits), status unpack, (wire pack)
void enqueue_step(HostRun &r, const Slot &sl, const HostChunk &c, const SearchCall &call)
{
    LocateStep step;
    step.call = call;
    step.call.d_rec = sl.d_rec;
    step.call.d_compact = sl.d_cmp;
    step.max_hits = r.qo.max_hits_per_query;
    step.take = true;  // locate(q).take(k)
    step.d_scan_workspace = sl.d_scan;
    step.d_totals = sl.d_tot;
    step.d_hit_offsets = sl.d_off32;
    step.narrow = true;
    step.d_hits = sl.d_hits;  // (sized for n32_cap hit slots; a chunk with more takes the second half again, second_half_again)
    step.hits_capacity = r.plan.n32_cap;
    step.d_workspace = sl.d_ws;
    GDX_HIP(hipMemsetAsync(sl.d_tot + 2, 0, sizeof(unsigned long long), r.st.k));
    launch_locate_step(r.view, step, r.st.k, r.qo);
    GDX_HIP(hipGetLastError());
    launch_unpack_records(sl.d_rec, c.nq, nullptr, sl.d_status, r.st.k, sl.d_cmp, sl.d_tot + 2);
    GDX_HIP(hipMemcpyAsync(sl.h_total, sl.d_tot, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, r.st.k));
    if (r.plan.path == Path::kStepWire) pack_wire(r, sl, c.nq);
    GDX_HIP(hipEventRecord(r.st.ev_total[sl.s], r.st.k));
}

void stage_in(HostRun &r, size_t k, WorkerPool &in_pool)
{
    const Slot &sl = r.slots[k % kSlots];
    const HostChunk &c = r.chunks[k];
    const SearchCall call = chunk_search_call(sl, c, stage_queries(r, k, in_pool));
    switch (r.plan.path) {
    case Path::kIntervals:
    case Path::kCounts: enqueue_flagged(r, sl, c, call); break;
    case Path::kPlainLocate: enqueue_plain_locate(r, sl, c, call); break;
    case Path::kStepDma:
    case Path::kStepWire: enqueue_step(r, sl, c, call); break;
    }
}

// ---- stage mid (calling thread): the chunk's search is done (locate: its total is known) -> locate, then all D2H -------------
void mid_flagged(HostRun &r, Slot &sl, const HostChunk &c)
{
    GDX_HIP(hipEventSynchronize(r.st.ev_total[sl.s]));
    sl.w_status = sl.h_total[0] != 0;
    GDX_HIP(hipStreamWaitEvent(r.st.out, r.st.ev_k[sl.s], 0));
    GDX_HIP(hipMemcpyAsync(sl.h_a, sl.d_a, c.nq * sizeof(uint32_t), hipMemcpyDeviceToHost, r.st.out));
    if (r.plan.path == Path::kIntervals) GDX_HIP(hipMemcpyAsync(sl.h_b, sl.d_b, c.nq * sizeof(uint32_t), hipMemcpyDeviceToHost, r.st.out));
    if (sl.w_status) GDX_HIP(hipMemcpyAsync(sl.h_status, sl.d_status, c.nq, hipMemcpyDeviceToHost, r.st.out));
    GDX_HIP(hipEventRecord(r.st.ev_out[sl.s], r.st.out));
}

void mid_plain_locate(HostRun &r, Slot &sl, HostChunk &c)
{
    const size_t hit_bytes = r.plan.hit_bytes;
    GDX_HIP(hipEventSynchronize(r.st.ev_total[sl.s]));
    c.total = *sl.h_total;
    const bool locate = c.total && !r.plan.sizing_only;
    if (locate) {
        sl.d_hits = sl.device<uint8_t>(kDevHits, c.total * hit_bytes);
        sl.h_hits = sl.pinned<uint8_t>(kPinHits, c.total * hit_bytes);
        sl.d_ws = sl.device<uint8_t>(kDevWs, locate_workspace_bytes(c.total));
        LocateCall loc;
        loc.d_rec = sl.d_rec;
        loc.m = c.nq;
        loc.d_hit_offsets = sl.d_off;
        loc.total_hits = c.total;
        loc.d_hits = sl.d_hits;
        loc.wide = r.plan.wide_hits;
        loc.d_workspace = sl.d_ws;
        launch_locate(r.view, loc, r.st.k, r.qo);
        GDX_HIP(hipGetLastError());
    }
    GDX_HIP(hipEventRecord(r.st.ev_k[sl.s], r.st.k));
    GDX_HIP(hipStreamWaitEvent(r.st.out, r.st.ev_k[sl.s], 0));
    GDX_HIP(hipMemcpyAsync(sl.h_off, sl.d_off, (c.nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, r.st.out));
    GDX_HIP(hipMemcpyAsync(sl.h_status, sl.d_status, c.nq, hipMemcpyDeviceToHost, r.st.out));
    if (locate) GDX_HIP(hipMemcpyAsync(sl.h_hits, sl.d_hits, c.total * hit_bytes, hipMemcpyDeviceToHost, r.st.out));
    GDX_HIP(hipEventRecord(r.st.ev_out[sl.s], r.st.out));
}

// rare: more hits than the chunk's buffers were sized for -- the second half of the step again, with room (and the wire again,
// from the complete hits)
void second_half_again(HostRun &r, Slot &sl, const HostChunk &c, uint64_t rest)
{
    sl.d_hits = sl.device<uint8_t>(kDevHits, c.total * sizeof(gdx_hit32_t));
    sl.d_ws = sl.device<uint8_t>(kDevWs, locate_workspace_bytes(c.total));
    launch_offsets_hits(r.view, sl.d_rec, sl.d_cmp, c.nq, r.qo.max_hits_per_query, true, sl.d_scan, sl.d_off32, true, c.total, rest,
                        sl.d_hits, sl.d_ws, r.st.k, r.qo);
    GDX_HIP(hipGetLastError());
    if (r.plan.path == Path::kStepWire) {
        sl.exc_hits_cap = c.total;
        sl.d_exc = sl.device<uint8_t>(kDevExc, r.plan.wl.exc_hits + sl.exc_hits_cap * sizeof(gdx_hit32_t));
        pack_wire(r, sl, c.nq);
        GDX_HIP(hipStreamSynchronize(r.st.k));
    }
}

// both stepped paths: the chunk's totals, the capacity / hit-limit checks, the second half again where it is needed
void step_totals(HostRun &r, Slot &sl, HostChunk &c)
{
    GDX_HIP(hipEventSynchronize(r.st.ev_total[sl.s]));
    c.total = sl.h_total[0];
    const uint64_t rest = sl.h_total[1];
    const Kind kind = r.call.kind;
    if (kind == Kind::kLocate32 && r.mid_hit_base + c.total >= (1ull << 32))
        fail(GDX_ERR_CAPACITY, "more than 2^32 - 1 hits: 32-bit hit offsets do not hold them (gdx_locate_many_alloc_layout does)");
    if (c.total >= r.plan.hit_limit && kind == Kind::kLocate) throw RetryWithWideOffsets{};  // (the wide call has no such limit)
    if (c.total >= 0xffffffffull)  // (the step counts a chunk's hit slots in 32 bits)
        fail(GDX_ERR_CAPACITY, "%llu queries of the batch have %llu hits, more than a chunk's 32-bit offsets hold: cap them "
             "(gdx_query_options_t.max_hits_per_query), or take the device-written results (environment GDX_HOST_RESULTS=dma)",
             static_cast<unsigned long long>(c.nq), static_cast<unsigned long long>(c.total));
    if (c.total > r.plan.n32_cap) second_half_again(r, sl, c, rest);
}

// kStepDma: u32 offsets (shifted by the hits before the chunk) and hits straight into the sink's pinned arrays
void mid_step_dma(HostRun &r, Slot &sl, HostChunk &c)
{
    Narrow32Sink *narrow = r.call.narrow;
    step_totals(r, sl, c);
    if (r.mid_hit_base + c.total > narrow->cap) {  // the pinned hit array moves: nothing may be on its way into the old one
        GDX_HIP(hipStreamSynchronize(r.st.out));
        narrow->hits = narrow->grow(r.mid_hit_base + c.total, r.mid_hit_base, &narrow->cap);
    }
    if (r.mid_hit_base != 0)
        hipLaunchKernelGGL(add_hit_base_kernel, dim3(static_cast<unsigned>(std::min<uint64_t>((c.nq + 255) / 256, 2048))), dim3(256),
                           0, r.st.k, sl.d_off32 + 1, c.nq, static_cast<uint32_t>(r.mid_hit_base));
    GDX_HIP(hipEventRecord(r.st.ev_k[sl.s], r.st.k));
    GDX_HIP(hipStreamWaitEvent(r.st.out, r.st.ev_k[sl.s], 0));
    GDX_HIP(hipMemcpyAsync(narrow->offsets + c.q0 + 1, sl.d_off32 + 1, c.nq * sizeof(uint32_t), hipMemcpyDeviceToHost, r.st.out));
    GDX_HIP(hipMemcpyAsync(sl.h_status, sl.d_status, c.nq, hipMemcpyDeviceToHost, r.st.out));
    if (c.total)
        GDX_HIP(hipMemcpyAsync(narrow->hits + r.mid_hit_base, sl.d_hits, c.total * sizeof(gdx_hit32_t), hipMemcpyDeviceToHost, r.st.out));
    GDX_HIP(hipEventRecord(r.st.ev_out[sl.s], r.st.out));
    c.hit_base = r.mid_hit_base;
    r.mid_hit_base += c.total;
}

// kStepWire: the wire up to the last found read's position, the ids, the exceptions packed tight, the status bytes if one is set
void mid_step_wire(HostRun &r, Slot &sl, HostChunk &c)
{
    const WireLayout &wl = r.plan.wl;
    step_totals(r, sl, c);
    const uint32_t *meta = reinterpret_cast<const uint32_t *>(sl.h_total + 4);
    sl.w_exc = meta[0], sl.w_exc_hits = meta[1], sl.w_found = meta[2];
    sl.w_status = sl.h_total[2] != 0;
    if (sl.w_exc > r.plan.max_nq || sl.w_exc_hits > sl.exc_hits_cap || sl.w_found + sl.w_exc_hits != c.total)
        fail(GDX_ERR_DEVICE, "internal: the wire of a chunk does not add up (%llu found + %llu exception hits, %llu hits)",
             static_cast<unsigned long long>(sl.w_found), static_cast<unsigned long long>(sl.w_exc_hits),
             static_cast<unsigned long long>(c.total));
    GDX_HIP(hipEventRecord(r.st.ev_k[sl.s], r.st.k));
    GDX_HIP(hipStreamWaitEvent(r.st.out, r.st.ev_k[sl.s], 0));
    GDX_HIP(hipMemcpyAsync(sl.h_wire, sl.d_wire, wl.found_pos + sl.w_found * 4, hipMemcpyDeviceToHost, r.st.out));
    if (wl.ids && sl.w_found != 0)
        GDX_HIP(hipMemcpyAsync(sl.h_wire + wl.found_ids, sl.d_wire + wl.found_ids, sl.w_found, hipMemcpyDeviceToHost, r.st.out));
    if (sl.w_exc != 0) {
        const uint64_t n = sl.w_exc;
        sl.h_exc = sl.pinned<uint8_t>(kPinExc, n * 8 + sl.w_exc_hits * sizeof(gdx_hit32_t));
        GDX_HIP(hipMemcpyAsync(sl.h_exc, sl.d_exc + wl.exc_reads, n * 4, hipMemcpyDeviceToHost, r.st.out));
        GDX_HIP(hipMemcpyAsync(sl.h_exc + n * 4, sl.d_exc + wl.exc_counts, n * 4, hipMemcpyDeviceToHost, r.st.out));
        if (sl.w_exc_hits != 0)
            GDX_HIP(hipMemcpyAsync(sl.h_exc + n * 8, sl.d_exc + wl.exc_hits, sl.w_exc_hits * sizeof(gdx_hit32_t), hipMemcpyDeviceToHost,
                                   r.st.out));
    }
    if (sl.w_status) GDX_HIP(hipMemcpyAsync(sl.h_status, sl.d_status, c.nq, hipMemcpyDeviceToHost, r.st.out));
    GDX_HIP(hipEventRecord(r.st.ev_out[sl.s], r.st.out));
    c.hit_base = r.mid_hit_base;
    r.mid_hit_base += c.total;
}

void stage_mid(HostRun &r, size_t k)
{
    Slot &sl = r.slots[k % kSlots];
    HostChunk &c = r.chunks[k];
    switch (r.plan.path) {
    case Path::kIntervals:
    case Path::kCounts: mid_flagged(r, sl, c); break;
    case Path::kPlainLocate: mid_plain_locate(r, sl, c); break;
    case Path::kStepDma: mid_step_dma(r, sl, c); break;
    case Path::kStepWire: mid_step_wire(r, sl, c); break;
    }
}

// ---- stage out (drainer thread): pinned staging -> the caller's arrays, widened -----------------------------------------------
void out_flagged(HostRun &r, const Slot &sl, const HostChunk &c)
{
    const bool intervals = r.plan.path == Path::kIntervals;
    uint64_t *out_a = intervals ? r.call.out_start : r.call.out_count, *out_b = intervals ? r.call.out_end : nullptr;
    r.pool.parallel_range(c.nq, 8, [&](uint64_t lo, uint64_t hi) {
        if (out_a) widen_u32(sl.h_a + lo, hi - lo, out_a + c.q0 + lo);
        if (out_b) widen_u32(sl.h_b + lo, hi - lo, out_b + c.q0 + lo);
    });
}

// wide locate: room for `need` hits in the caller's array (grown where the library manages it); false from the first chunk on
// that does not fit (gdx_locate_many then reports the size it takes)
bool room_for_hits(HostRun &r, uint64_t need)
{
    if (r.call.grow_hits && need > r.hits_capacity) r.hits = (*r.call.grow_hits)(need, &r.hits_capacity);  // at least `need`
    if (!(r.hits && need <= r.hits_capacity && r.capacity_ok)) r.capacity_ok = false;
    return r.capacity_ok;
}

void out_plain_locate(HostRun &r, const Slot &sl, HostChunk &c)
{
    uint64_t *out_off = r.call.out_hit_offsets;
    c.hit_base = r.hit_base;
    if (out_off) {  // the chunk's offsets (scanned on the device) shifted by the hits of the chunks before it
        const uint64_t *off = sl.h_off;
        const uint64_t shift_by = r.hit_base;
        r.pool.parallel_range(c.nq, 8, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t i = lo; i < hi; i++) out_off[c.q0 + i + 1] = off[i + 1] + shift_by;
        });
    }
    const uint64_t need = r.hit_base + c.total;
    if (room_for_hits(r, need) && !r.plan.sizing_only) {
        gdx_hit_t *dst = r.hits + r.hit_base;
        if (r.plan.wide_hits) {
            const gdx_hit_t *src = static_cast<const gdx_hit_t *>(sl.h_hits);
            r.pool.parallel_range(c.total, 8, [&](uint64_t lo, uint64_t hi) { std::memcpy(dst + lo, src + lo, (hi - lo) * sizeof(gdx_hit_t)); });
        } else {
            const gdx_hit32_t *src = static_cast<const gdx_hit32_t *>(sl.h_hits);
            r.pool.parallel_range(c.total, 8, [&](uint64_t lo, uint64_t hi) {
                for (uint64_t i = lo; i < hi; i++) {
                    dst[i].text_id = src[i].text_id;
                    dst[i].position = src[i].position;
                }
            });
        }
    } else {
        r.capacity_ok = false;
    }
    r.hit_base = need;
}

// kStepWire: the chunk's wire -> offsets and hits in the caller's arrays, tiles shared out among the workers
void out_wire(HostRun &r, const Slot &sl, const HostChunk &c)
{
    const WireLayout &wl = r.plan.wl;
    const uint64_t need = c.hit_base + c.total;
    const HostWire w{sl.h_wire + wl.bitmap,
                     reinterpret_cast<const uint32_t *>(sl.h_wire + wl.tile_found),
                     reinterpret_cast<const uint32_t *>(sl.h_wire + wl.tile_off),
                     reinterpret_cast<const uint32_t *>(sl.h_wire + wl.found_pos),
                     wl.ids ? sl.h_wire + wl.found_ids : nullptr,
                     reinterpret_cast<const uint32_t *>(sl.h_exc),
                     reinterpret_cast<const uint32_t *>(sl.h_exc + sl.w_exc * 4),
                     reinterpret_cast<const gdx_hit32_t *>(sl.h_exc + sl.w_exc * 8),
                     sl.w_exc};
    const uint64_t tiles = div_ceil(c.nq, kHostWireTile);
    auto share = [&](unsigned wk, unsigned nw, uint64_t &lo, uint64_t &hi) {
        const uint64_t per = div_ceil(tiles, nw);
        lo = std::min<uint64_t>(tiles, per * wk), hi = std::min<uint64_t>(tiles, lo + per);
    };
    if (r.call.kind == Kind::kLocate32) {  // narrow: u32 offsets and 8-byte hits in the sink's arrays
        Narrow32Sink *narrow = r.call.narrow;
        if (need > narrow->cap) narrow->hits = narrow->grow(need, c.hit_base, &narrow->cap);  // (only this thread's workers write there)
        uint32_t *offs = narrow->offsets + c.q0;
        gdx_hit32_t *hh = narrow->hits;
        const uint32_t hb = static_cast<uint32_t>(c.hit_base);
        r.pool.run([&](unsigned wk, unsigned nw) {
            uint64_t lo, hi;
            share(wk, nw, lo, hi);
            wire_expand_tiles<uint32_t, gdx_hit32_t>(w, c.nq, lo, hi, hb, offs, hh);
        });
        return;
    }
    // wide: u64 offsets and 16-byte hits; the hits only while the caller's buffer holds them
    uint64_t *offs = r.call.out_hit_offsets ? r.call.out_hit_offsets + c.q0 : nullptr;
    gdx_hit_t *hh = room_for_hits(r, need) ? r.hits : nullptr;
    if (offs != nullptr || hh != nullptr)
        r.pool.run([&](unsigned wk, unsigned nw) {
            uint64_t lo, hi;
            share(wk, nw, lo, hi);
            wire_expand_tiles<uint64_t, gdx_hit_t>(w, c.nq, lo, hi, c.hit_base, offs, hh);
        });
    r.hit_base = need;
}

// the status tail of every path.  bytes_came == false: no read of the chunk has a status, the bytes stayed on the device
void out_status(HostRun &r, const Slot &sl, const HostChunk &c, bool bytes_came)
{
    uint8_t *out_status = r.call.out_status;
    if (!bytes_came) {
        if (out_status) r.pool.parallel_range(c.nq, 64, [&](uint64_t lo, uint64_t hi) { std::memset(out_status + c.q0 + lo, 0, hi - lo); });
        return;
    }
    const uint8_t *stt = sl.h_status;
    r.pool.parallel_range(c.nq, 64, [&](uint64_t lo, uint64_t hi) {
        bool any = false;
        for (uint64_t i = lo; i < hi; i++) any |= stt[i] != 0;
        if (out_status) std::memcpy(out_status + c.q0 + lo, stt + lo, hi - lo);
        if (any) r.any_status.store(true);
    });
}

void stage_out(HostRun &r, size_t k)
{
    const Slot &sl = r.slots[k % kSlots];
    HostChunk &c = r.chunks[k];
    const double t_sync0 = host_timing() ? now_seconds() : 0.0;
    GDX_HIP(hipEventSynchronize(r.st.ev_out[sl.s]));
    if (host_timing()) r.t_out_sync += now_seconds() - t_sync0;
    switch (r.plan.path) {
    case Path::kIntervals:
    case Path::kCounts: out_flagged(r, sl, c); break;
    case Path::kPlainLocate: out_plain_locate(r, sl, c); break;
    case Path::kStepDma: break;  // (offsets and hits are where they belong already)
    case Path::kStepWire: out_wire(r, sl, c); break;
    }
    const bool conditional = r.plan.flagged || r.plan.path == Path::kStepWire;  // (the status bytes cross only if one is set)
    out_status(r, sl, c, !conditional || sl.w_status);
}

}  // namespace

// The pipeline behind every host-pointer call: plan, slots, then the three stages over the chunks
int FmIndex::host_pipeline(const HostCall &call) const
{
    // (more than host_threads() workers did not shorten the expansion -- 13 ms of a 100 M-read call with 7 workers, 11 with 13 --
    // and starved the runtime's own threads on a 16-CPU container)
    WorkerPool pool(host_threads());
    HostPlan plan = make_host_plan(call, *this, pool);
    if (call.out_total) *call.out_total = 0;
    if (call.kind == Kind::kLocate && call.out_hit_offsets) call.out_hit_offsets[0] = 0;
    if (call.kind == Kind::kLocate32 && call.narrow != nullptr && call.narrow->offsets != nullptr) call.narrow->offsets[0] = 0;
    if (call.nq == 0) return GDX_OK;
    make_current();
    HostRun r(call, std::move(plan), *this, pool);
    fill_slots(r, cfg_.device_id);
    WorkerPool in_pool(r.plan.in_threads);
    ThreeStageRunner runner;
    runner.run(r.chunks.size(), cfg_.device_id, [&](size_t k) { stage_in(r, k, in_pool); }, [&](size_t k) { stage_mid(r, k); },
               [&](size_t k) { stage_out(r, k); }, r.t_out_sync);
    GDX_HIP(hipStreamSynchronize(r.st.out));
    if (call.kind == Kind::kLocate32) {
        call.narrow->offsets[0] = 0;
        if (call.out_total) *call.out_total = r.mid_hit_base;
        return r.any_status.load() ? GDX_ERR_QUERY_STATUS : GDX_OK;
    }
    if (call.out_total) *call.out_total = r.hit_base;
    if (call.kind == Kind::kLocate && r.hit_base > 0 && !r.capacity_ok) return GDX_ERR_CAPACITY;
    return r.any_status.load() ? GDX_ERR_QUERY_STATUS : GDX_OK;
}

// A wide locate, and once more on the plain path when a chunk's hits did not fit the fused step's 32-bit offsets.
// refresh (optional): brings the call's hit array up to date before the second run (the first may have grown it)
int FmIndex::locate_wide(HostCall call, const std::function<void(HostCall &)> &refresh) const
{
    try {
        return host_pipeline(call);
    } catch (const RetryWithWideOffsets &) {
        (void)hipDeviceSynchronize();
        if (refresh) refresh(call);
        call.plain_locate_only = true;
        return host_pipeline(call);
    }
}

// ASCII -> 2-bit on the host, by all pool threads; exceptions = the queries that hold a symbol which is not one of
// the dense codes 1..4 (sorted, unique); returns how many there are (the first `capacity` of them are stored)
uint64_t FmIndex::pack_queries_host(const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq, uint8_t *out_packed,
                                    uint64_t *out_exc, uint64_t capacity) const
{
    return pack_queries_with_table(cfg_.io_to_dense, qbuf, qoff, nq, out_packed, out_exc, capacity);
}

// (no index, no device: the alphabet's table is all the packing needs -- gdx_pack_queries_table, for a reader that packs
// what it parses before any index is at hand)
uint64_t pack_queries_with_table(const uint8_t *tab, const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq, uint8_t *out_packed,
                                 uint64_t *out_exc, uint64_t capacity)
{
    if (!tab) fail(GDX_ERR_INVALID_ARGUMENT, "io_to_dense is null");
    // (a call of its own, not a stage of the pipeline: every CPU the process may use, unless GDX_HOST_THREADS says otherwise)
    WorkerPool pool(getenv("GDX_HOST_THREADS") ? host_threads() : std::min(32u, usable_cpus()));
    check_queries(qbuf, qoff, nq, pool, 0);
    if (!out_packed && nq && qoff[nq]) fail(GDX_ERR_INVALID_ARGUMENT, "out_packed is null");
    const uint64_t n_sym = nq ? qoff[nq] : 0;
    const uint64_t n_bytes = div_ceil(n_sym, 4);
    const uint64_t first = nq ? qoff[0] : 0;  // symbols before the first query are not looked at (code 0)
    std::vector<std::vector<uint64_t>> bad(pool.size());
    const PackPlan plan = make_pack_plan(tab);  // (pack_host.hpp: 32 symbols per step where the table has the shape for it)
    pool.run([&](unsigned w, unsigned nw) {
        const uint64_t per = (n_bytes / nw + 64) / 64 * 64;
        const uint64_t lo = std::min(n_bytes, per * w), hi = std::min(n_bytes, lo + per);
        std::vector<uint64_t> &mine = bad[w];
        pack_range(plan, tab, qbuf, first, n_sym, lo, hi, out_packed, [&](uint64_t j) {
            const uint64_t q = static_cast<uint64_t>(std::upper_bound(qoff, qoff + nq + 1, j) - qoff) - 1;
            if (mine.empty() || mine.back() != q) mine.push_back(q);
        });
    });
    std::vector<uint64_t> all;
    for (auto &v : bad) all.insert(all.end(), v.begin(), v.end());
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    for (uint64_t i = 0; i < all.size() && i < capacity; i++) out_exc[i] = all[i];
    return all.size();
}

unsigned fastx_default_threads() { return std::min(32u, usable_cpus()); }

void set_host_chunking(uint64_t queries, uint64_t bytes)
{
    g_chunk_queries.store(queries ? queries : (1ull << 20));
    g_chunk_bytes.store(bytes ? bytes : (32ull << 20));
}

int FmIndex::cursors_for_many_queries(const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq, uint64_t *out_start,
                                      uint64_t *out_end, uint64_t *out_count, uint8_t *out_status, bool packed,
                                      uint64_t uniform_len) const
{
    if (packed) check_packed_supported();
    HostCall call;
    call.qbuf = qbuf, call.qoff = qoff, call.nq = nq, call.packed = packed, call.uniform_len = uniform_len;
    call.out_status = out_status;
    if (out_start || out_end) {
        call.kind = HostCall::Kind::kIntervals;
        call.out_start = out_start;
        call.out_end = out_end;
        const int rc = host_pipeline(call);
        if (out_count && out_start && out_end)
            for (uint64_t i = 0; i < nq; i++) out_count[i] = out_end[i] - out_start[i];
        return rc;
    }
    call.kind = HostCall::Kind::kCounts;
    call.out_count = out_count;
    return host_pipeline(call);
}

int FmIndex::locate_many(const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq, uint64_t *out_hit_offsets,
                         gdx_hit_t *hits, uint64_t hits_capacity, uint64_t *out_total, uint8_t *out_status) const
{
    HostCall call;
    call.kind = HostCall::Kind::kLocate;
    call.qbuf = qbuf, call.qoff = qoff, call.nq = nq;
    call.out_hit_offsets = out_hit_offsets;
    call.out_status = out_status;
    call.hits = hits;
    call.hits_capacity = hits ? hits_capacity : 0;
    call.out_total = out_total;
    return locate_wide(call);
}

// One hit array released with gdx_free_hits is kept for the next gdx_locate_many_alloc: a caller that locates batch
// after batch otherwise pays the first touch of 1.6 GB per 100 M hits in every call (page faults and zeroing inside the
// drainer's copy: 0.08-0.14 of a 0.14 s call, tools/host_timing.py).  At most one array is held, the larger of the two
// when another comes back; it is ordinary malloc memory (a caller may free() it as well).
namespace {
std::mutex g_hits_mutex;
void *g_hits_cached = nullptr;
size_t g_hits_cached_bytes = 0;
constexpr size_t kHitsCacheMin = 16u << 20;  // smaller arrays are not worth holding
}  // namespace

void recycle_hits(gdx_hit_t *hits)
{
    if (!hits) return;
    const size_t bytes = malloc_usable_size(hits);
    void *drop = hits;
    if (bytes >= kHitsCacheMin) {
        std::lock_guard<std::mutex> g(g_hits_mutex);
        if (bytes > g_hits_cached_bytes) {
            drop = g_hits_cached;
            g_hits_cached = hits;
            g_hits_cached_bytes = bytes;
        }
    }
    std::free(drop);
}

static void *take_cached_hits(size_t bytes, size_t *got)
{
    std::lock_guard<std::mutex> g(g_hits_mutex);
    // (only for a request of at least half its size: a ten-query call must not walk away with gigabytes)
    if (g_hits_cached == nullptr || g_hits_cached_bytes < bytes || g_hits_cached_bytes / 2 > bytes) return nullptr;
    void *p = g_hits_cached;
    *got = g_hits_cached_bytes;
    g_hits_cached = nullptr;
    g_hits_cached_bytes = 0;
    return p;
}

int FmIndex::locate_many_alloc(const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq, uint64_t *out_hit_offsets,
                               gdx_hit_t **out_hits, uint64_t *out_total, uint8_t *out_status, bool packed,
                               uint64_t uniform_len) const
{
    if (packed) check_packed_supported();
    if (!out_hits) fail(GDX_ERR_INVALID_ARGUMENT, "out_hits is null");
    *out_hits = nullptr;
    gdx_hit_t *buf = nullptr;
    uint64_t cap = 0;
    // The hit array is large (16 bytes per hit) and written exactly once: 2 MB alignment + MADV_HUGEPAGE keeps the
    // first-touch page faults (one per 4 KB otherwise, ~100 ms per GB single-threaded) out of the pipeline.
    const std::function<gdx_hit_t *(uint64_t, uint64_t *)> grow = [&](uint64_t need, uint64_t *new_cap) {
        const uint64_t want = std::max<uint64_t>(need, cap + cap / 2 + 4096);
        size_t bytes = (want * sizeof(gdx_hit_t) + (2u << 20) - 1) / (2u << 20) * (2u << 20);
        void *p = take_cached_hits(bytes, &bytes);  // (an array a caller gave back: its pages are there already)
        if (p == nullptr) {
            if (posix_memalign(&p, 2u << 20, bytes) != 0 || !p) {
                std::free(buf);
                buf = nullptr;
                fail(GDX_ERR_DEVICE, "out of host memory for %llu hits", static_cast<unsigned long long>(want));
            }
            (void)madvise(p, bytes, MADV_HUGEPAGE);
        }
        if (buf) {  // rare: the first guess (one hit per query and a bit) was too small
            std::memcpy(p, buf, cap * sizeof(gdx_hit_t));
            std::free(buf);
        }
        buf = static_cast<gdx_hit_t *>(p);
        cap = bytes / sizeof(gdx_hit_t);
        if (new_cap) *new_cap = cap;
        return buf;
    };
    int rc;
    try {
        // a first guess from the batch size spares most reallocations (one hit per query is the common shape)
        grow(nq + nq / 8, nullptr);
        HostCall call;
        call.kind = HostCall::Kind::kLocate;
        call.qbuf = qbuf, call.qoff = qoff, call.nq = nq, call.packed = packed, call.uniform_len = uniform_len;
        call.out_hit_offsets = out_hit_offsets;
        call.out_status = out_status;
        call.out_total = out_total;
        call.grow_hits = &grow;
        auto current_array = [&](HostCall &c) { c.hits = buf, c.hits_capacity = cap; };
        current_array(call);
        rc = locate_wide(call, current_array);
    } catch (...) {
        std::free(buf);
        throw;
    }
    *out_hits = buf;
    return rc;
}

// ---- narrow results in library-owned pinned memory (gdx_locate_many_alloc_layout32) ---------------------------------------
// The device writes u32 offsets and 8-byte hits into these arrays by D2H copy; the caller reads them where they are.  Pinning
// host memory costs about a millisecond per 10 MB, so the arrays a caller gives back (gdx_free_hits32) are kept for its next
// call -- one pair, the largest seen -- until gdx_release_cached_hits.
namespace {
struct PinnedBlock {
    void *ptr = nullptr;
    size_t bytes = 0;
};
std::mutex g_pinned_mutex;
PinnedBlock g_pinned_cache[2];  // [0] offsets, [1] hits

void *pinned_take(int which, size_t bytes, size_t *got)
{
    {
        std::lock_guard<std::mutex> g(g_pinned_mutex);
        PinnedBlock &b = g_pinned_cache[which];
        if (b.ptr != nullptr && b.bytes >= bytes) {
            void *p = b.ptr;
            *got = b.bytes;
            b = PinnedBlock{};
            return p;
        }
    }
    void *p = nullptr;
    GDX_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    *got = bytes;
    return p;
}

void pinned_give(int which, void *ptr, size_t bytes)
{
    if (ptr == nullptr) return;
    void *drop = ptr;
    {
        std::lock_guard<std::mutex> g(g_pinned_mutex);
        PinnedBlock &b = g_pinned_cache[which];
        if (bytes > b.bytes) {
            drop = b.ptr;
            b.ptr = ptr;
            b.bytes = bytes;
        }
    }
    if (drop != nullptr) (void)hipHostFree(drop);
}
}  // namespace

int FmIndex::locate_many_alloc32(const uint8_t *qbuf, const uint64_t *qoff, uint64_t nq, gdx_hits32_t *out, uint8_t *out_status,
                                 bool packed, uint64_t uniform_len) const
{
    if (packed) check_packed_supported();
    if (!out) fail(GDX_ERR_INVALID_ARGUMENT, "out is null");
    std::memset(out, 0, sizeof(*out));
    make_current();
    size_t off_bytes = 0, hit_bytes = 0;
    Narrow32Sink sink;
    sink.offsets = static_cast<uint32_t *>(pinned_take(0, (nq + 1) * sizeof(uint32_t) + 64, &off_bytes));
    try {
        // a first guess from the batch size spares most reallocations (one hit per query is the common shape)
        sink.hits = static_cast<gdx_hit32_t *>(pinned_take(1, (nq + nq / 8 + 4096) * sizeof(gdx_hit32_t), &hit_bytes));
    } catch (...) {
        pinned_give(0, sink.offsets, off_bytes);
        throw;
    }
    sink.cap = hit_bytes / sizeof(gdx_hit32_t);
    sink.grow = [&](uint64_t need, uint64_t keep, uint64_t *new_cap) {
        size_t bytes = 0;
        gdx_hit32_t *p = static_cast<gdx_hit32_t *>(pinned_take(1, std::max<uint64_t>(need, sink.cap + sink.cap / 2) * sizeof(gdx_hit32_t), &bytes));
        std::memcpy(p, sink.hits, keep * sizeof(gdx_hit32_t));
        pinned_give(1, sink.hits, hit_bytes);
        hit_bytes = bytes;
        *new_cap = bytes / sizeof(gdx_hit32_t);
        return p;
    };
    uint64_t total = 0;
    int rc;
    try {
        HostCall call;
        call.kind = HostCall::Kind::kLocate32;
        call.qbuf = qbuf, call.qoff = qoff, call.nq = nq, call.packed = packed, call.uniform_len = uniform_len;
        call.out_status = out_status;
        call.out_total = &total;
        call.narrow = &sink;
        rc = host_pipeline(call);
    } catch (...) {
        (void)hipDeviceSynchronize();
        pinned_give(0, sink.offsets, off_bytes);
        pinned_give(1, sink.hits, hit_bytes);
        throw;
    }
    out->hit_offsets = sink.offsets;
    out->hits = sink.hits;
    out->total_hits = total;
    out->nq = nq;
    out->reserved[0] = off_bytes;
    out->reserved[1] = hit_bytes;
    return rc;
}

void recycle_hits32(gdx_hits32_t *r)
{
    if (!r) return;
    pinned_give(0, r->hit_offsets, r->reserved[0]);
    pinned_give(1, r->hits, r->reserved[1]);
    std::memset(r, 0, sizeof(*r));
}

void release_cached_hits()
{
    void *drop[3] = {nullptr, nullptr, nullptr};
    {
        std::lock_guard<std::mutex> g(g_pinned_mutex);
        for (int i = 0; i < 2; i++) {
            drop[i] = g_pinned_cache[i].ptr;
            g_pinned_cache[i] = PinnedBlock{};
        }
    }
    {
        std::lock_guard<std::mutex> g(g_hits_mutex);
        drop[2] = g_hits_cached;
        g_hits_cached = nullptr;
        g_hits_cached_bytes = 0;
    }
    if (drop[0]) (void)hipHostFree(drop[0]);
    if (drop[1]) (void)hipHostFree(drop[1]);
    std::free(drop[2]);
}

}  // namespace gdx
