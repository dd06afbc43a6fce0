// host_checks.cpp -- the parts of libgdx.so's host code that parse untrusted bytes, compiled for the CPU with
// AddressSanitizer + UBSan (tests/test_host_sanitized.py builds and runs this; GPU sanitizers are not available):
//   host_checks fastx <file> <max_records> <buffer_bytes>   reads every batch; prints "ok <records> <symbols> <checksum>"
//   host_checks header <file>                                validates an index file header; prints "ok n=.. texts=.."
//   host_checks pack <file>                                  packs the file's bytes as queries (pack_host.hpp: the AVX2 path and the
//                                                            byte loop) in exactly sized buffers; prints "ok <cases> <exceptions>"
//   host_checks wire <seed> <reads> <texts> [<found of ten> <exceptions: one in>]  expands a random chunk's "found bitmap" wire (wire_host.hpp) in pieces,
//                                                            exactly sized buffers; prints "ok <hits> <exceptions>"
//   host_checks chunks <seed>                              the chunk planner and the wire layout of the host-pointer pipeline (host_plan.hpp);
//                                                            prints "ok <cases> <chunks>"
//   host_checks auxplan <seed>                             which auxiliary structures an index gets (aux_plan.hpp) against the arithmetic
//                                                            it replaced; prints "ok <hand-made> <random> <raised> <default shapes> <shrunk>"
// A malformed input must end in "error: <message>" (exit code 3), never in a sanitizer report.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../genedex_amd/csrc/aux_plan.hpp"
#include "../../genedex_amd/csrc/fastx.hpp"
#include "../../genedex_amd/csrc/host_plan.hpp"
#include "../../genedex_amd/csrc/index_file.hpp"
#include "../../genedex_amd/csrc/pack_host.hpp"
#include "../../genedex_amd/csrc/wire_host.hpp"

int main(int argc, char **argv)
{
    if (argc < 3) {
        std::fprintf(stderr, "usage: host_checks fastx <file> <max_records> <buffer_bytes> | header <file>\n");
        return 2;
    }
    const std::string mode = argv[1];
    try {
        if (mode == "fastx") {
            const uint64_t max_records = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 1000;
            const uint64_t cap = argc > 4 ? std::strtoull(argv[4], nullptr, 10) : (1u << 20);
            gdx::FastxReader reader(argv[2]);
            std::vector<uint8_t> qbuf(cap ? cap : 1);
            std::vector<uint64_t> qoff(max_records + 1);
            uint64_t records = 0, symbols = 0, checksum = 1469598103934665603ull;
            for (;;) {
                const uint64_t n = reader.next_batch(qbuf.data(), cap, qoff.data(), max_records);
                if (n == 0) break;
                records += n;
                symbols += qoff[n];
                for (uint64_t i = 0; i < qoff[n]; i++) checksum = (checksum ^ qbuf[i]) * 1099511628211ull;
                for (uint64_t i = 0; i < n; i++)
                    if (qoff[i + 1] < qoff[i] || qoff[i + 1] > cap) return 4;  // the offsets stay inside the buffer
            }
            std::printf("ok %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", records, symbols, checksum);
        } else if (mode == "fastxmap") {
            // the memory-mapped reader, blocks parsed by `threads` threads (GDX_FASTX_BLOCK_BYTES: the smallest block): the same
            // line as "fastx" prints for the same file, or the same error
            const uint64_t max_records = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 1000;
            const uint64_t cap = argc > 4 ? std::strtoull(argv[4], nullptr, 10) : (1u << 20);
            const unsigned threads = argc > 5 ? static_cast<unsigned>(std::strtoul(argv[5], nullptr, 10)) : 4u;
            std::unique_ptr<gdx::FastxMappedReader> reader(gdx::FastxMappedReader::open(argv[2], threads));
            if (!reader) {  // (an empty or missing file: the streaming reader decides)
                gdx::FastxReader plain(argv[2]);
                std::printf("ok 0 0 %" PRIu64 "\n", static_cast<uint64_t>(1469598103934665603ull));
                return 0;
            }
            std::vector<uint8_t> qbuf(cap ? cap : 1);
            std::vector<uint64_t> qoff(max_records + 1);
            uint64_t records = 0, symbols = 0, checksum = 1469598103934665603ull;
            for (;;) {
                uint64_t ulen = 0;
                const uint64_t n = reader->next_batch(qbuf.data(), cap, qoff.data(), max_records, &ulen);
                if (n == 0) break;
                records += n;
                symbols += qoff[n];
                for (uint64_t i = 0; i < qoff[n]; i++) checksum = (checksum ^ qbuf[i]) * 1099511628211ull;
                for (uint64_t i = 0; i < n; i++) {
                    if (qoff[i + 1] < qoff[i] || qoff[i + 1] > cap) return 4;
                    if (ulen != 0 && qoff[i + 1] - qoff[i] != ulen) return 5;
                }
            }
            std::printf("ok %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", records, symbols, checksum);
        } else if (mode == "header") {
            gdx::IndexFile in(argv[2], "rb");
            const gdx::FileHeader h = gdx::read_index_header(in, argv[2]);
            std::printf("ok n=%" PRIu64 " texts=%" PRIu64 " sigma=%d\n", h.n, h.n_texts, h.sigma);
        } else if (mode == "pack") {
            // the file's bytes as a query buffer, packed in pieces whose borders fall everywhere relative to the 32- and
            // 128-symbol steps of the vector loop; source and destination are heap blocks of exactly the size the contract
            // names, so a read or write one byte outside is a sanitizer report.  Compared with the table applied byte by byte.
            std::vector<uint8_t> data;
            {
                gdx::IndexFile in(argv[2], "rb");
                uint8_t chunk[4096];
                for (;;) {
                    const size_t n = std::fread(chunk, 1, sizeof(chunk), in.f);
                    if (n == 0) break;
                    data.insert(data.end(), chunk, chunk + n);
                }
            }
            uint8_t dna[256] = {0}, clash[256] = {0};
            dna[(int)'A'] = dna[(int)'a'] = 1, dna[(int)'C'] = dna[(int)'c'] = 2, dna[(int)'G'] = dna[(int)'g'] = 3;
            dna[(int)'T'] = dna[(int)'t'] = 4, dna[(int)'N'] = dna[(int)'n'] = 5;
            clash[0x41] = 1, clash[0x51] = 2, clash[0x43] = 3, clash[0x47] = 4;  // no nibble plan: the byte loop
            uint64_t cases = 0, exceptions = 0;
            for (const uint8_t *tab : {dna, clash}) {
                const gdx::PackPlan plan = gdx::make_pack_plan(tab);
                if ((tab == dna) != plan.fast) return 5;
                for (uint64_t first : {uint64_t(0), uint64_t(1), uint64_t(31), uint64_t(33), uint64_t(130)}) {
                    for (uint64_t cut : {uint64_t(0), uint64_t(1), uint64_t(29), uint64_t(127)}) {
                        if (first + cut > data.size()) continue;
                        const uint64_t n_sym = data.size() - cut;
                        if (first > n_sym) continue;
                        const uint64_t n_bytes = (n_sym + 3) / 4;
                        std::unique_ptr<uint8_t[]> src(new uint8_t[n_sym ? n_sym : 1]), out(new uint8_t[n_bytes ? n_bytes : 1]);
                        std::copy(data.begin(), data.begin() + n_sym, src.get());
                        // two halves on a 64-byte border of the output, as the worker threads split it
                        const uint64_t mid = std::min(n_bytes, (n_bytes / 2 + 63) / 64 * 64);
                        std::vector<uint64_t> bad;
                        gdx::pack_range(plan, tab, src.get(), first, n_sym, 0, mid, out.get(), [&](uint64_t j) { bad.push_back(j); });
                        gdx::pack_range(plan, tab, src.get(), first, n_sym, mid, n_bytes, out.get(), [&](uint64_t j) { bad.push_back(j); });
                        std::vector<uint64_t> want_bad;
                        for (uint64_t b = 0; b < n_bytes; b++) {
                            uint32_t w = 0;
                            for (uint32_t k = 0; k < 4; k++) {
                                const uint64_t j = 4 * b + k;
                                if (j < first || j >= n_sym) continue;
                                const uint32_t d = tab[src[j]];
                                if (d - 1u < 4u) w |= (d - 1u) << (2u * k);
                                else want_bad.push_back(j);
                            }
                            if (out[b] != w) return 6;
                        }
                        if (bad != want_bad) return 7;
                        cases++;
                        exceptions += bad.size();
                    }
                }
            }
            std::printf("ok %" PRIu64 " %" PRIu64 "\n", cases, exceptions);
        } else if (mode == "wire") {
            // a chunk of reads with random outcomes -- one hit (nine in ten, or one in ten: argv[5]), none, or an exception with
            // 0..40 hits -- over a collection of `texts` texts; the wire as wire_pack_kernel lays it out, in heap blocks of
            // exactly the sizes the host pipeline copies; expanded by 1, 3 and 7 workers and compared with the plain construction
            uint64_t x = std::strtoull(argv[2], nullptr, 10) * 2654435761ull + 88172645463325252ull;
            auto rnd = [&]() {
                x ^= x << 13, x ^= x >> 7, x ^= x << 17;
                return x;
            };
            const uint64_t nq = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 5000;
            const uint64_t n_texts = argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 3;
            const uint64_t found_in_ten = argc > 5 ? std::strtoull(argv[5], nullptr, 10) : 9;
            const uint64_t exc_one_in = argc > 6 ? std::strtoull(argv[6], nullptr, 10) : 3;  // of the reads that are not found
            const uint64_t n = 1000 + n_texts * 700;
            std::vector<uint64_t> sentinels(n_texts);
            for (uint64_t t = 0; t < n_texts; t++) sentinels[t] = (t + 1) * (n / n_texts) - 1 - (t + 1 < n_texts ? rnd() % 300 : 0);
            sentinels[n_texts - 1] = n - 1;
            auto split = [&](uint32_t g) {
                uint32_t t = 0;
                while (sentinels[t] < g) t++;
                gdx_hit32_t h;
                h.text_id = t;
                h.position = t == 0 ? g : g - static_cast<uint32_t>(sentinels[t - 1]) - 1u;
                return h;
            };
            const uint64_t tiles = (nq + gdx::kHostWireTile - 1) / gdx::kHostWireTile;
            std::vector<uint8_t> bitmap(tiles * 256, 0);
            std::vector<uint32_t> tile_found(tiles + 1), tile_off(tiles + 1), found_pos, exc_q, exc_cnt, want_off(nq + 1);
            std::vector<uint8_t> found_ids;
            std::vector<gdx_hit32_t> exc_hits, want_hits;
            const uint32_t base = 777;
            want_off[0] = base;
            for (uint64_t q = 0; q < nq; q++) {
                if (q % gdx::kHostWireTile == 0) {
                    tile_found[q / gdx::kHostWireTile] = static_cast<uint32_t>(found_pos.size());
                    tile_off[q / gdx::kHostWireTile] = static_cast<uint32_t>(want_hits.size());
                }
                const uint64_t r = rnd() % 100;
                if (r < found_in_ten * 10) {
                    uint32_t g;
                    do g = static_cast<uint32_t>(rnd() % n); while (std::find(sentinels.begin(), sentinels.end(), g) != sentinels.end());
                    bitmap[q / 8] |= static_cast<uint8_t>(1u << (q % 8));
                    found_pos.push_back(split(g).position);
                    found_ids.push_back(static_cast<uint8_t>(split(g).text_id));
                    want_hits.push_back(split(g));
                } else if (rnd() % exc_one_in == 0) {
                    const uint32_t cnt = static_cast<uint32_t>(rnd() % 41);
                    exc_q.push_back(static_cast<uint32_t>(q));
                    exc_cnt.push_back(cnt);
                    for (uint32_t i = 0; i < cnt; i++) {
                        gdx_hit32_t h;
                        h.text_id = static_cast<uint32_t>(rnd() % n_texts), h.position = static_cast<uint32_t>(rnd() % 1000);
                        exc_hits.push_back(h);
                        want_hits.push_back(h);
                    }
                }
                want_off[q + 1] = base + static_cast<uint32_t>(want_hits.size());
            }
            tile_found[tiles] = static_cast<uint32_t>(found_pos.size());
            tile_off[tiles] = static_cast<uint32_t>(want_hits.size());
            found_pos.push_back(0xffffffffu);  // (the one element past the found reads that HostWire asks to be readable)
            found_ids.push_back(0xffu);
            auto exact = [](const auto &v) {  // a heap block of exactly the vector's bytes (at least one)
                using T = typename std::decay<decltype(v[0])>::type;
                std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
                std::copy(v.begin(), v.end(), p.get());
                return p;
            };
            const auto b_bitmap = exact(bitmap);
            const auto b_tf = exact(tile_found), b_to = exact(tile_off), b_fp = exact(found_pos), b_eq = exact(exc_q), b_ec = exact(exc_cnt);
            const auto b_eh = exact(exc_hits);
            const auto b_fi = exact(found_ids);
            const gdx::HostWire w{b_bitmap.get(), b_tf.get(), b_to.get(), b_fp.get(), n_texts > 1 ? b_fi.get() : nullptr,
                                  b_eq.get(), b_ec.get(), b_eh.get(), exc_q.size()};
            for (uint64_t workers : {uint64_t(1), uint64_t(3), uint64_t(7)}) {
                const uint64_t per = (tiles + workers - 1) / workers;
                // the narrow form (u32 offsets, 8-byte hits) ...
                std::unique_ptr<uint32_t[]> off(new uint32_t[nq + 1]);
                std::unique_ptr<gdx_hit32_t[]> hits(new gdx_hit32_t[base + want_hits.size() + 1]);
                std::fill(off.get(), off.get() + nq + 1, 0xdeadbeefu);
                for (uint64_t k = workers; k-- > 0;)  // (in reverse: no piece relies on the one before it)
                    gdx::wire_expand_tiles<uint32_t, gdx_hit32_t>(w, nq, std::min(tiles, per * k), std::min(tiles, per * k + per), base, off.get(),
                                                                  hits.get());
                for (uint64_t q = 0; q <= nq; q++)
                    if (off[q] != want_off[q] && nq != 0) return 8;
                for (uint64_t i = 0; i < want_hits.size(); i++)
                    if (hits[base + i].text_id != want_hits[i].text_id || hits[base + i].position != want_hits[i].position) return 9;
                // ... the wide form (u64 offsets, 16-byte hits), and offsets alone beyond 2^32 (the sizing pass of gdx_locate_many)
                std::unique_ptr<uint64_t[]> off64(new uint64_t[nq + 1]), off_only(new uint64_t[nq + 1]);
                std::unique_ptr<gdx_hit_t[]> hits64(new gdx_hit_t[base + want_hits.size() + 1]);
                const uint64_t far = 5'000'000'000ull;
                for (uint64_t k = workers; k-- > 0;) {
                    gdx::wire_expand_tiles<uint64_t, gdx_hit_t>(w, nq, std::min(tiles, per * k), std::min(tiles, per * k + per), base, off64.get(),
                                                                hits64.get());
                    gdx::wire_expand_tiles<uint64_t, gdx_hit_t>(w, nq, std::min(tiles, per * k), std::min(tiles, per * k + per), far, off_only.get(),
                                                                nullptr);
                    gdx::wire_expand_tiles<uint64_t, gdx_hit_t>(w, nq, std::min(tiles, per * k), std::min(tiles, per * k + per), base, nullptr,
                                                                hits64.get());
                }
                for (uint64_t q = 0; q <= nq; q++)
                    if (nq != 0 && (off64[q] != want_off[q] || off_only[q] != want_off[q] - base + far)) return 10;
                for (uint64_t i = 0; i < want_hits.size(); i++)
                    if (hits64[base + i].text_id != want_hits[i].text_id || hits64[base + i].position != want_hits[i].position) return 11;
            }
            // the staging copy and the widening of counts, on exactly sized blocks at every alignment of source and destination
            for (uint64_t len : {uint64_t(0), uint64_t(1), uint64_t(31), uint64_t(4095), uint64_t(4096), uint64_t(4229), uint64_t(10000)})
                for (uint64_t shift = 0; shift < 40; shift += 13) {
                    std::unique_ptr<uint8_t[]> src(new uint8_t[len + shift + 1]), dst(new uint8_t[len + 40 - shift + 1]);
                    for (uint64_t i = 0; i < len; i++) src[shift + i] = static_cast<uint8_t>(rnd());
                    gdx::stream_copy(dst.get() + (40 - shift), src.get() + shift, len);
                    if (len != 0 && std::memcmp(dst.get() + (40 - shift), src.get() + shift, len) != 0) return 12;
                    const uint64_t n32 = len / 4;
                    std::unique_ptr<uint64_t[]> wide(new uint64_t[n32 + 1]);
                    std::unique_ptr<uint32_t[]> narrow(new uint32_t[n32 + 1]);
                    for (uint64_t i = 0; i < n32; i++) narrow[i] = static_cast<uint32_t>(rnd());
                    gdx::widen_u32(narrow.get() + (shift & 1), n32 - (n32 ? (shift & 1) : 0), wide.get() + (shift & 1));
                    for (uint64_t i = (shift & 1); i < n32; i++)
                        if (wide[i] != narrow[i]) return 13;
                }
            std::printf("ok %zu %zu\n", want_hits.size(), exc_q.size());
        } else if (mode == "chunks") {
            // host_plan.hpp: the chunk planner of the host-pointer pipeline on random and hand-made offset arrays, in heap blocks
            // of exactly nq + 1 entries, and the wire layout.  `expected` is the loop as it stood inside the pipeline before it
            // became a function: boundaries must match list for list.
            uint64_t x = std::strtoull(argv[2], nullptr, 10) * 2654435761ull + 88172645463325252ull;
            auto rnd = [&]() {
                x ^= x << 13, x ^= x >> 7, x ^= x << 17;
                return x;
            };
            auto expected = [](const uint64_t *qoff, uint64_t nq, uint64_t uniform_len, uint64_t kChunkBytes, uint64_t kChunkQueries) {
                const bool uniform = uniform_len != 0;
                auto off_of = [&](uint64_t i) { return uniform ? i * uniform_len : qoff[i]; };
                std::vector<gdx::HostChunk> chunks;
                const uint64_t uniform_chunk = uniform ? std::max<uint64_t>(8, std::min(kChunkQueries, kChunkBytes / uniform_len) / 8 * 8) : 0;
                for (uint64_t q0 = 0; q0 < nq;) {
                    uint64_t hi = std::min(nq, q0 + (uniform ? uniform_chunk : kChunkQueries));
                    if (!uniform && qoff[hi] - qoff[q0] > kChunkBytes) {
                        const uint64_t *p = std::upper_bound(qoff + q0 + 1, qoff + hi + 1, qoff[q0] + kChunkBytes);
                        hi = static_cast<uint64_t>(p - qoff) - 1;
                        if (hi <= q0) hi = q0 + 1;  // a single query longer than a chunk
                    }
                    gdx::HostChunk c;
                    c.q0 = q0;
                    c.nq = hi - q0;
                    c.bytes = off_of(hi) - off_of(q0);
                    chunks.push_back(c);
                    q0 = hi;
                }
                return chunks;
            };
            uint64_t cases = 0, n_chunks = 0;
            // lens == null: a uniform batch (no offsets at all, as the calls allow)
            auto check = [&](const std::vector<uint64_t> *lens, uint64_t nq, uint64_t uniform_len, uint64_t first, uint64_t bytes, uint64_t queries) {
                std::unique_ptr<uint64_t[]> qoff;
                if (lens) {
                    qoff.reset(new uint64_t[nq + 1]);
                    qoff[0] = first;
                    for (uint64_t i = 0; i < nq; i++) qoff[i + 1] = qoff[i] + (*lens)[i];
                }
                auto off_of = [&](uint64_t i) { return lens ? qoff[i] : i * uniform_len; };
                const std::vector<gdx::HostChunk> got = gdx::plan_host_chunks(qoff.get(), nq, uniform_len, bytes, queries);
                const std::vector<gdx::HostChunk> want = expected(qoff.get(), nq, uniform_len, bytes, queries);
                if (got.size() != want.size()) return 20;
                uint64_t next = 0;
                for (size_t k = 0; k < got.size(); k++) {
                    const gdx::HostChunk &c = got[k];
                    if (c.q0 != want[k].q0 || c.nq != want[k].nq || c.bytes != want[k].bytes) return 21;
                    if (c.q0 != next || c.nq == 0) return 22;  // in order, without gaps
                    if (c.bytes != off_of(c.q0 + c.nq) - off_of(c.q0)) return 23;
                    // both limits, except for one over-long query -- and a uniform chunk, which never holds fewer than 8 queries
                    if (c.nq > queries && !(uniform_len != 0 && c.nq <= 8)) return 24;
                    if (c.bytes > bytes && !(c.nq == 1 || (uniform_len != 0 && c.nq <= 8))) return 25;
                    if (uniform_len != 0 && k + 1 < got.size() && c.nq % 8 != 0) return 26;
                    next = c.q0 + c.nq;
                }
                if (next != nq) return 27;
                cases++, n_chunks += got.size();
                return 0;
            };
            auto all_limits = [&](const std::vector<uint64_t> *lens, uint64_t nq, uint64_t uniform_len, uint64_t first) {
                for (uint64_t bytes : {uint64_t(1), uint64_t(600), uint64_t(1500), uint64_t(6000), uint64_t(32) << 20, uint64_t(128) << 20})
                    for (uint64_t queries : {uint64_t(1), uint64_t(8), uint64_t(97), uint64_t(388), uint64_t(1) << 20})
                        if (const int rc = check(lens, nq, uniform_len, first, bytes, queries)) return rc;
                return 0;
            };
            const uint64_t big = 7000;  // longer than every byte limit below 32 MB
            std::vector<std::vector<uint64_t>> made = {std::vector<uint64_t>(1000, 0), {0}, {50}, {big}, {big, 40, 41, 42}, {40, 41, big, 42, 43},
                                                       {40, 41, 42, big}, {big, big, big}, std::vector<uint64_t>(500, 1), {0, 0, big, 0, 0}};
            for (const auto &lens : made)
                for (uint64_t first : {uint64_t(0), uint64_t(13)})
                    if (const int rc = all_limits(&lens, lens.size(), 0, first)) return rc;
            for (int round = 0; round < 40; round++) {
                std::vector<uint64_t> lens(1 + rnd() % 3000);
                for (uint64_t &l : lens) l = rnd() % 100 == 0 ? rnd() % 9000 : 18 + rnd() % 53;
                if (const int rc = all_limits(&lens, lens.size(), 0, rnd() % 100)) return rc;
            }
            for (uint64_t ul : {uint64_t(1), uint64_t(50), (uint64_t(1) << 21) - 1})
                for (uint64_t nq : {uint64_t(1), uint64_t(7), uint64_t(8), uint64_t(9), uint64_t(1000), uint64_t(4001)})
                    if (const int rc = all_limits(nullptr, nq, ul, 0)) return rc;
            // the wire layout: 256-byte aligned sections, in order, each as long as its content at least, `bytes` behind the last
            for (uint64_t max_nq : {uint64_t(1), uint64_t(2047), uint64_t(2048), uint64_t(2049), uint64_t(100000)})
                for (uint64_t n_texts : {uint64_t(1), uint64_t(2)}) {
                    const gdx::WireLayout w = gdx::make_wire_layout(max_nq, n_texts);
                    const uint64_t tiles = (max_nq + gdx::kHostWireTile - 1) / gdx::kHostWireTile;
                    for (uint64_t o : {w.bitmap, w.tile_found, w.tile_off, w.found_pos, w.found_ids})
                        if (o % 256 != 0) return 30;
                    if (w.bitmap < 16) return 31;  // (the meta in front)
                    if (w.tile_found < w.bitmap + tiles * 256 || w.tile_off < w.tile_found + (tiles + 1) * 4 ||
                        w.found_pos < w.tile_off + (tiles + 1) * 4 || w.found_ids < w.found_pos + (max_nq + 1) * 4)
                        return 32;
                    if (w.ids != (n_texts > 1) || w.bytes != w.found_ids + (w.ids ? max_nq + 1 : 0)) return 33;
                    if (w.exc_reads != 0 || w.exc_counts != max_nq * 4 || w.exc_hits != max_nq * 8) return 34;
                    cases++;
                }
            std::printf("ok %" PRIu64 " %" PRIu64 "\n", cases, n_chunks);
        } else if (mode == "auxplan") {
            // aux_plan.hpp: which auxiliary structures an index gets.  `expected` is the arithmetic of FmIndex::build_aux as it
            // stood before the decision became this header -- budget, fit test, k, wants, jump / top wanted, shrink loop --
            // with the environment as AuxEnv and the two hipMemGetInfo readings as arguments: the planner must agree field
            // for field, and raise the same error where that raised.
            using gdx::AuxEnv;
            using gdx::BuildOptions;
            uint64_t x = std::strtoull(argv[2], nullptr, 10) * 2654435761ull + 88172645463325252ull;
            auto rnd = [&]() {
                x ^= x << 13, x ^= x >> 7, x ^= x << 17;
                return x;
            };
            constexpr uint32_t kSeedTagBitsMax = 21;  // (layout.hpp, which needs HIP)
            struct Outcome {
                int status = 0;  // of the error raised, 0: none
                std::string message;
                bool default_shape = false, want_pairs = false, want_text = false, want_sa_full = false, want_isa = false, build_any = false;
                uint32_t seed_k = 0, seed_load_pct = 0, wanted_jump = 0, wanted_top = 0, jump = 0, top = 0;
                uint64_t budget_bytes = 0;
            };
            struct Case {
                uint64_t n = 0;
                int sigma = 6, layout = 0, n_searchable = 4;
                BuildOptions bo;
                AuxEnv env;
                uint64_t free1 = 0, free2 = 0, total = 0;  // the readings before anything is allocated and behind the pair lines
            };
            auto expected = [](const Case &c, Outcome &o) {
                const uint64_t n_ = c.n;
                const BuildOptions &bo = c.bo;
                auto env_int = [](bool set, int value, int fallback) { return set ? value : fallback; };
                int want_pairs = bo.pair_lines;
                if (want_pairs < 0) want_pairs = c.env.no_pair_lines ? 0 : 1;
                bool default_shape = bo.seed_symbols < 0 && bo.jump_bytes < 0 && bo.full_sa < 0 && bo.inverse_sa < 0 && bo.text_units < 0 &&
                                     want_pairs != 0 && c.layout == 0 && c.sigma >= 5 && c.n_searchable >= 4 && n_ > 0;
                if (default_shape && c.env.tables_shape) default_shape = false;
                uint32_t seed_load_pct = bo.seed_load_percent > 0 ? static_cast<uint32_t>(bo.seed_load_percent) : 70u;
                auto auto_seed_k = [&] {
                    uint32_t k = 8;
                    while (k < 24 && (1ull << (2u * (k - 8u))) < n_) k++;
                    return k;
                };
                if (default_shape) {
                    const size_t free_b = c.free1, total_b = c.total;
                    const size_t reserve = total_b / 16 > (4ull << 30) ? total_b / 16 : (4ull << 30);
                    double budget = free_b > reserve ? static_cast<double>(free_b - reserve) : 0.0;
                    if (bo.aux_budget_bytes != 0) {
                        budget = static_cast<double>(bo.aux_budget_bytes) < budget ? static_cast<double>(bo.aux_budget_bytes) : budget;
                    } else {
                        if (budget > static_cast<double>(total_b / 2)) budget = static_cast<double>(total_b / 2);
                        if (c.env.budget_gb != HUGE_VAL) budget = std::min(budget, c.env.budget_gb * 1e9);  // (GDX_AUX_BUDGET_GB is set)
                    }
                    const uint32_t k = auto_seed_k();
                    const uint32_t load = bo.seed_load_percent > 0 ? static_cast<uint32_t>(bo.seed_load_percent) : 60u;
                    double seed_bytes = 16.0 / (load / 100.0) * static_cast<double>(n_);
                    if (2u * k > kSeedTagBitsMax) seed_bytes = std::max(seed_bytes, 128.0 * static_cast<double>(1ull << (2u * k - kSeedTagBitsMax)));
                    const double need = 1.25 * seed_bytes + 8.5 * static_cast<double>(n_);
                    if (need > budget) default_shape = false;
                    else seed_load_pct = load;
                }
                uint32_t seed_k = 0;
                if (default_shape) {
                    seed_k = auto_seed_k();
                } else if (bo.seed_symbols >= 1 && c.sigma >= 5) {
                    if (bo.seed_symbols == 1) seed_k = auto_seed_k();
                    else seed_k = static_cast<uint32_t>(bo.seed_symbols);
                    if (seed_k < 8u || seed_k > 24u) gdx::fail(GDX_ERR_INVALID_ARGUMENT, "seed_symbols must be 1 (automatic) or 8..24");
                }
                const bool want_seed = seed_k != 0;
                const bool want_text = bo.text_units == 1 || want_seed, want_sa_full = bo.full_sa == 1 || default_shape,
                           want_isa = bo.inverse_sa == 1 || default_shape;
                o.default_shape = default_shape, o.want_pairs = want_pairs != 0, o.seed_k = seed_k, o.seed_load_pct = seed_load_pct;
                o.want_text = want_text, o.want_sa_full = want_sa_full, o.want_isa = want_isa;
                if (c.layout == 0 && n_ > 0 && (want_pairs || want_text || want_sa_full || want_isa)) {
                    o.build_any = true;
                    uint32_t jump_bytes = 32;
                    if (default_shape) {
                        jump_bytes = 0;
                    } else if (bo.jump_bytes >= 0) {
                        jump_bytes = static_cast<uint32_t>(bo.jump_bytes);
                    } else {
                        jump_bytes = static_cast<uint32_t>(c.env.jump_bytes);
                        if (c.env.no_jump_table) jump_bytes = 0;
                    }
                    if (jump_bytes != 0 && jump_bytes != 8 && jump_bytes != 16 && jump_bytes != 32)
                        gdx::fail(GDX_ERR_INVALID_ARGUMENT, "jump entry bytes must be 0, 8, 16 or 32");
                    if (!want_pairs) jump_bytes = 0;
                    uint32_t top_depth = 0;
                    while (top_depth < 16 && (1ull << (2u * (top_depth + 2u))) <= 2ull * n_) top_depth += 2;
                    if (bo.top_depth >= 0) top_depth = static_cast<uint32_t>(bo.top_depth);
                    else top_depth = static_cast<uint32_t>(env_int(c.env.has_top_depth, c.env.top_depth, static_cast<int>(top_depth)));
                    if (top_depth > 16u) top_depth = 16u;
                    if (default_shape && bo.top_depth < 0 && top_depth > 14u) top_depth = 14u;
                    if (c.sigma < 5) top_depth = 0;
                    if (!want_pairs && !want_text) top_depth = 0;
                    o.wanted_jump = jump_bytes;
                    o.wanted_top = top_depth;
                    {
                        const size_t free_b = c.free2, total_b = c.total;
                        const size_t reserve = total_b / 16 > (4ull << 30) ? total_b / 16 : (4ull << 30);
                        double budget = free_b > reserve ? static_cast<double>(free_b - reserve) : 0.0;
                        if (bo.aux_budget_bytes != 0) {
                            budget = static_cast<double>(bo.aux_budget_bytes) < budget ? static_cast<double>(bo.aux_budget_bytes) : budget;
                        } else {
                            if (budget > static_cast<double>(total_b / 2)) budget = static_cast<double>(total_b / 2);
                            if (c.env.budget_gb != HUGE_VAL) {
                                const double b = c.env.budget_gb * 1e9;
                                budget = b < budget ? b : budget;
                            }
                        }
                        o.budget_bytes = static_cast<uint64_t>(budget);
                        const double seed_load = seed_load_pct / 100.0;
                        double seed_bytes = 0.0;
                        if (want_seed) {
                            seed_bytes = 16.0 / seed_load * static_cast<double>(n_);
                            if (2u * seed_k > kSeedTagBitsMax) seed_bytes = std::max(seed_bytes, 128.0 * static_cast<double>(1ull << (2u * seed_k - kSeedTagBitsMax)));
                            seed_bytes *= 1.25;
                            if (seed_bytes > budget && bo.seed_symbols > 1)
                                gdx::fail(GDX_ERR_INVALID_ARGUMENT,
                                          "seed_symbols = %u needs a seed table of at least %.1f GB (2^(2k - 21) buckets of 128 bytes, or 16 bytes per "
                                          "k-mer over the load factor), the budget for auxiliary structures is %.1f GB: choose a smaller k or "
                                          "seed_symbols = 1", seed_k, seed_bytes / 1.25 / 1e9, budget / 1e9);
                        }
                        const double fixed = ((want_sa_full ? 4.0 : 0.0) + (want_isa ? 4.0 : 0.0)) * static_cast<double>(n_) + (want_text ? 0.5 : 0.0) * static_cast<double>(n_) +
                                             seed_bytes;
                        auto need = [&] {
                            return fixed + static_cast<double>(jump_bytes) * static_cast<double>(n_) +
                                   (top_depth ? 8.0 * static_cast<double>(1ull << (2u * top_depth)) : 0.0);
                        };
                        while (need() > budget) {
                            if (top_depth > 14) top_depth = 14;
                            else if (jump_bytes == 32) jump_bytes = 16;
                            else if (top_depth > 12) top_depth = 12;
                            else if (jump_bytes == 16) jump_bytes = 8;
                            else if (top_depth > 0) top_depth -= top_depth >= 2 ? 2 : 1;
                            else if (jump_bytes != 0) jump_bytes = 0;
                            else break;
                        }
                    }
                    o.jump = jump_bytes;
                    o.top = top_depth;
                }
            };
            // the planner, called as FmIndex::build_aux calls it
            auto planned = [](const Case &c, Outcome &o) {
                const gdx::AuxPlanInput in = {c.n, c.sigma, c.layout, c.n_searchable, kSeedTagBitsMax, c.bo, c.env};
                const bool asked = gdx::aux_default_shape_asked(in);
                const gdx::AuxShape s = gdx::plan_aux_shape(in, asked ? c.free1 : 0, asked ? c.total : 0);
                o.default_shape = s.default_shape, o.want_pairs = s.want_pairs, o.seed_k = s.seed_k, o.seed_load_pct = s.seed_load_percent;
                o.want_text = s.want_text, o.want_sa_full = s.want_sa_full, o.want_isa = s.want_isa, o.build_any = s.build_any;
                if (!s.build_any) return;
                const gdx::AuxTables t = gdx::plan_aux_tables(in, s, c.free2, c.total);
                o.wanted_jump = t.wanted_jump_bytes, o.wanted_top = t.wanted_top_depth, o.jump = t.jump_bytes, o.top = t.top_depth;
                o.budget_bytes = t.budget_bytes;
            };
            auto outcome = [](const auto &plan, const Case &c) {
                Outcome o;
                try {
                    plan(c, o);
                } catch (const gdx::Error &e) {
                    o.status = e.status;
                    o.message = e.what();
                }
                return o;
            };
            uint64_t cases = 0, raised = 0, default_shapes = 0, shrunk = 0;
            auto check = [&](Case c) {
                c.free2 = c.free1 > 2 * c.n ? c.free1 - 2 * c.n : 0;  // the pair lines: 2 bytes per symbol
                const Outcome want = outcome(expected, c), got = outcome(planned, c);
                if (got.status != want.status || got.message != want.message) return 40;
                if (want.status != 0) {  // (a build that raised holds nothing)
                    cases++, raised++;
                    return 0;
                }
                if (got.default_shape != want.default_shape || got.want_pairs != want.want_pairs || got.seed_k != want.seed_k) return 41;
                if (got.seed_load_pct != want.seed_load_pct) return 42;
                if (got.want_text != want.want_text || got.want_sa_full != want.want_sa_full || got.want_isa != want.want_isa) return 43;
                if (got.build_any != want.build_any) return 44;
                if (got.wanted_jump != want.wanted_jump || got.wanted_top != want.wanted_top) return 45;
                if (got.jump != want.jump || got.top != want.top) return 46;
                if (got.budget_bytes != want.budget_bytes) return 47;
                cases++, default_shapes += want.default_shape;
                shrunk += want.jump != want.wanted_jump || want.top != want.wanted_top;
                return 0;
            };
            const uint64_t gib = 1ull << 30, total288 = 288 * gib;
            // the two worked examples: a 288 GiB device with 300e9 bytes free, sigma 6, 3.1 G symbols, every option at its default
            {
                Case c;
                c.n = 3'100'000'000ull, c.free1 = 300'000'000'000ull, c.total = total288;
                if (const int rc = check(c)) return rc;
                c.free2 = c.free1 - 2 * c.n;
                Outcome o = outcome(planned, c);
                if (gdx::aux_budget(c.free1, c.total, 0, c.env) != 154'618'822'656.0 || o.budget_bytes != 154'618'822'656ull) return 50;
                const double need = gdx::seed_table_estimate(c.n, 24, 60, kSeedTagBitsMax) + 8.5 * static_cast<double>(c.n);
                if (need < 129.67e9 || need > 129.69e9) return 51;
                if (o.status != 0 || !o.default_shape || o.seed_k != 24 || o.seed_load_pct != 60 || !o.want_text || !o.want_sa_full || !o.want_isa ||
                    o.wanted_jump != 0 || o.jump != 0 || o.wanted_top != 14 || o.top != 14)
                    return 52;
                c.bo.aux_budget_bytes = 90'000'000'000ull;
                if (const int rc = check(c)) return rc;
                o = outcome(planned, c);
                if (o.status != 0 || o.default_shape || o.seed_k != 0 || o.want_text || o.want_sa_full || o.want_isa || o.wanted_jump != 32 ||
                    o.wanted_top != 16 || o.jump != 16 || o.top != 14 || o.budget_bytes != 90'000'000'000ull)
                    return 53;
            }
            // build_seed_table's bucket rule through seed_min_buckets, against the two ifs it replaced
            for (uint32_t k = 8; k <= 24; k++)
                for (uint64_t b : {uint64_t(0), uint64_t(1), uint64_t(1) << 10, (uint64_t(1) << 27) - 1, uint64_t(1) << 27, uint64_t(1) << 31}) {
                    uint64_t want = b;
                    if (want < 1) want = 1;
                    if (2u * k > kSeedTagBitsMax && want < (1ull << (2u * k - kSeedTagBitsMax))) want = 1ull << (2u * k - kSeedTagBitsMax);
                    if (std::max<uint64_t>({b, 1, gdx::seed_min_buckets(k, kSeedTagBitsMax)}) != want) return 54;
                }
            // hand-made: every value of one thing at a time around a base, over every text length, alphabet and layout
            const std::vector<uint64_t> lengths = {0, 1, 255, 65536, 65537, 20'000, 1ull << 28, 3'100'000'000ull, 3'700'000'000ull, 0xffffffffull};
            std::vector<BuildOptions> option_sets(1);
            auto vary = [&](int BuildOptions::*field, std::initializer_list<int> values) {
                for (int v : values) {
                    BuildOptions bo;
                    bo.*field = v;
                    option_sets.push_back(bo);
                }
            };
            vary(&BuildOptions::pair_lines, {0, 1});
            vary(&BuildOptions::jump_bytes, {0, 8, 16, 32, 7, 24, 64});
            vary(&BuildOptions::top_depth, {0, 1, 5, 12, 13, 14, 16, 17, 400});
            vary(&BuildOptions::full_sa, {0, 1});
            vary(&BuildOptions::text_units, {0, 1});
            vary(&BuildOptions::seed_symbols, {0, 1, 8, 12, 17, 24, 2, 7, 25, 1000});
            vary(&BuildOptions::seed_load_percent, {20, 40, 100});
            vary(&BuildOptions::inverse_sa, {0, 1});
            vary(&BuildOptions::table_layout, {0, 1, 4});
            {
                BuildOptions lean;  // (the seed index of the smoke test), and a k with a load factor, without pair lines
                lean.jump_bytes = 0, lean.top_depth = 0, lean.full_sa = 1, lean.seed_symbols = 1, lean.inverse_sa = 1;
                option_sets.push_back(lean);
                lean.seed_symbols = 24, lean.seed_load_percent = 40, lean.pair_lines = 0;
                option_sets.push_back(lean);
            }
            std::vector<AuxEnv> envs(1);
            envs.emplace_back().no_pair_lines = true;
            envs.emplace_back().tables_shape = true;
            for (double gb : {0.0003, 50.0, 120.0, 1000.0}) envs.emplace_back().budget_gb = gb;
            for (int jb : {0, 8, 16, 7, -8}) envs.emplace_back().jump_bytes = jb;
            envs.emplace_back().no_jump_table = true;
            for (int td : {0, 6, 13, 16, 20, -1}) envs.emplace_back().has_top_depth = true, envs.back().top_depth = td;
            const std::vector<uint64_t> budgets = {0, 1, 300'000, 90'000'000'000ull, 250'000'000'000ull};
            // free - reserve below half of the device, above it before the pair lines and below it behind them (3.1 G symbols:
            // 6.2 GB), above it; less than the reserve; and a small device, whose reserve is the 4 GB floor
            const std::vector<std::pair<uint64_t, uint64_t>> memory = {
                {100'000'000'000ull, total288}, {total288 / 16 + total288 / 2 + 3'000'000'000ull, total288}, {300'000'000'000ull, total288},
                {1'000'000'000ull, total288}, {15 * gib, 16 * gib}};
            for (uint64_t n : lengths)
                for (int sigma : {4, 5, 6, 9})
                    for (int layout : {0, 1})
                        for (int n_searchable : {3, 4})
                            for (const auto &mem : memory)
                                for (uint64_t budget : budgets) {
                                    Case c;
                                    c.n = n, c.sigma = sigma, c.layout = layout, c.n_searchable = n_searchable;
                                    c.free1 = mem.first, c.total = mem.second;
                                    for (const BuildOptions &bo : option_sets) {
                                        c.bo = bo, c.bo.aux_budget_bytes = budget;
                                        if (const int rc = check(c)) return rc;
                                    }
                                    for (const AuxEnv &env : envs)  // each override alone: on the defaults, and where jump and top are read
                                        for (int text_units : {-1, 0}) {
                                            c.bo = BuildOptions(), c.bo.aux_budget_bytes = budget, c.bo.text_units = text_units, c.env = env;
                                            if (const int rc = check(c)) return rc;
                                        }
                                }
            const uint64_t made = cases;
            // random combinations of all of it
            auto pick = [&](std::initializer_list<int> values) { return values.begin()[rnd() % values.size()]; };
            for (int round = 0; round < 6000; round++) {
                Case c;
                c.n = rnd() % 4 == 0 ? lengths[rnd() % lengths.size()] : (rnd() % 2 ? rnd() % 0x100000000ull : rnd() % 100'000);
                c.sigma = pick({3, 4, 5, 6, 9, 21}), c.layout = pick({0, 0, 1}), c.n_searchable = pick({2, 3, 4, 5});
                c.bo.pair_lines = pick({-1, -1, 0, 1}), c.bo.jump_bytes = pick({-1, -1, -1, 0, 8, 16, 32, 12});
                c.bo.top_depth = pick({-1, -1, -1, 0, 3, 8, 12, 14, 15, 16, 30}), c.bo.full_sa = pick({-1, -1, 0, 1});
                c.bo.text_units = pick({-1, -1, 0, 1}), c.bo.seed_symbols = pick({-1, -1, -1, 0, 1, 9, 16, 22, 24, 3, 30});
                c.bo.seed_load_percent = pick({0, 0, 20, 55, 100}), c.bo.inverse_sa = pick({-1, -1, 0, 1});
                c.bo.aux_budget_bytes = rnd() % 2 ? 0 : (rnd() % 2 ? budgets[rnd() % budgets.size()] : rnd() % 200'000'000'000ull);
                if (rnd() % 3 == 0) c.env = envs[rnd() % envs.size()];
                if (rnd() % 8 == 0) c.env.no_pair_lines = true;
                c.total = rnd() % 4 == 0 ? (8 + rnd() % 300) * gib : total288;
                c.free1 = rnd() % 4 == 0 ? memory[rnd() % 3].first : rnd() % (c.total + 1);
                if (const int rc = check(c)) return rc;
            }
            if (raised == 0 || default_shapes == 0 || shrunk == 0) return 55;
            std::printf("ok %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", made, cases - made, raised, default_shapes, shrunk);
        } else {
            return 2;
        }
    } catch (const gdx::Error &e) {
        std::printf("error: %s\n", e.what());
        return 3;
    }
    return 0;
}
