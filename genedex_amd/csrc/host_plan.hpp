// host_plan.hpp -- the arithmetic of the host-pointer pipeline (host_api.hip) that needs no device: how a batch is cut into
// chunks and where the sections of a chunk's "found bitmap" wire lie.  No HIP in here: tests/host_checks/host_checks.cpp
// compiles it for the CPU under ASan + UBSan.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "errors.hpp"
#include "wire_host.hpp"

namespace gdx {

struct HostChunk {
    uint64_t q0 = 0, nq = 0, bytes = 0;  // queries [q0, q0 + nq) of the batch; bytes: their symbols (qoff's unit)
    uint64_t total = 0, hit_base = 0;    // locate: the chunk's hits, and the hits of the chunks before it (set while the call runs)
};

// Chunk boundaries: at most chunk_bytes of query symbols (qoff's unit) and chunk_queries queries each, in order, without
// gaps; a single query longer than chunk_bytes is a chunk of its own.  uniform_len != 0: query i = symbols [i * uniform_len,
// (i + 1) * uniform_len), qoff is not looked at, and every chunk but the last holds a multiple of 8 queries, so that a chunk
// starts on a 16-bit unit of a packed buffer and on a byte of an ASCII one, and is a uniform batch of its own.
inline std::vector<HostChunk> plan_host_chunks(const uint64_t *qoff, uint64_t nq, uint64_t uniform_len, uint64_t chunk_bytes,
                                               uint64_t chunk_queries)
{
    const bool uniform = uniform_len != 0;
    auto off_of = [&](uint64_t i) { return uniform ? i * uniform_len : qoff[i]; };
    const uint64_t uniform_chunk = uniform ? std::max<uint64_t>(8, std::min(chunk_queries, chunk_bytes / uniform_len) / 8 * 8) : 0;
    std::vector<HostChunk> chunks;
    for (uint64_t q0 = 0; q0 < nq;) {
        uint64_t hi = std::min(nq, q0 + (uniform ? uniform_chunk : chunk_queries));
        if (!uniform && qoff[hi] - qoff[q0] > chunk_bytes) {
            const uint64_t *p = std::upper_bound(qoff + q0 + 1, qoff + hi + 1, qoff[q0] + chunk_bytes);
            hi = static_cast<uint64_t>(p - qoff) - 1;
            if (hi <= q0) hi = q0 + 1;  // a single query longer than a chunk
        }
        HostChunk c;
        c.q0 = q0;
        c.nq = hi - q0;
        c.bytes = off_of(hi) - off_of(q0);
        chunks.push_back(c);
        q0 = hi;
    }
    return chunks;
}

// A slot's wire, byte offsets into its buffer: {meta 16 B | bitmap, 256 B per tile | tile_found | tile_off | found_pos} and --
// collections of more than one text -- the found reads' text ids behind it, the same offsets on the device and in pinned
// memory, so that ONE copy brings everything up to the last found read's position and one more the ids.  The exceptions of a
// slot have a buffer of their own: {read numbers | counts | hits}, max_nq entries of the first two.
struct WireLayout {
    uint64_t bitmap = 0, tile_found = 0, tile_off = 0, found_pos = 0, found_ids = 0, bytes = 0;
    uint64_t exc_reads = 0, exc_counts = 0, exc_hits = 0;
    bool ids = false;  // the found reads' text ids travel (more than one text)
};

inline WireLayout make_wire_layout(uint64_t max_nq, uint64_t n_texts)
{
    WireLayout w;
    const uint64_t tiles = div_ceil_u64(max_nq, kHostWireTile);
    w.ids = n_texts > 1;
    w.bitmap = 256;
    w.tile_found = w.bitmap + tiles * 256;
    w.tile_off = w.tile_found + div_ceil_u64((tiles + 1) * 4, 256) * 256;
    w.found_pos = w.tile_off + div_ceil_u64((tiles + 1) * 4, 256) * 256;
    w.found_ids = w.found_pos + div_ceil_u64(max_nq * 4 + 4, 256) * 256;
    w.bytes = w.found_ids + (w.ids ? max_nq + 1 : 0);
    w.exc_reads = 0;
    w.exc_counts = max_nq * 4;
    w.exc_hits = max_nq * 8;
    return w;
}

}  // namespace gdx
