// aux_plan.hpp -- which auxiliary structures an index gets (FmIndex::build_aux, fm_index.hip): the build options, the debug
// overrides of the environment and the device's free memory decide, in two steps around the two moments the build reads the
// memory at.  No HIP in here: tests/host_checks/host_checks.cpp compiles it for the CPU under ASan + UBSan.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "errors.hpp"

namespace gdx {

// Build-time choices of this implementation that the reference has no counterpart for (gdx_build_options_t).
// Negative / zero = default.  The GDX_* environment variables of AuxEnv only override fields left at their default
// (debugging aid).
struct BuildOptions {
    // (all of jump_bytes / full_sa / text_units / seed_symbols / inverse_sa at -1 and pair lines not switched off: THE DEFAULT
    // SHAPE -- seed table + text units + full and inverse suffix array + pair lines + top table of depth <= 14, no jump table
    // -- when it fits the budget; plan_aux_shape)
    int pair_lines = -1;            // -1 default (on for sigma <= 8), 0 off, 1 on
    int jump_bytes = -1;            // -1 default (none in the default shape, else 32), 0 none, 8, 16, 32
    int top_depth = -1;             // -1 default (largest even D <= 16 with 4^D <= 2n; <= 14 in the default shape), 0 none, 1..16
    uint64_t aux_budget_bytes = 0;  // cap for jump + top table; 0 = min(free HBM - reserve, half of the HBM)
    int full_sa = -1;               // 1: SA[row] of every row as its own array
    int text_units = -1;            // 1: the text itself, 16 bytes per 32 symbols (layout.hpp)
    int seed_symbols = -1;          // -1 / 0 none, 1 = seed table with k chosen from the text length, 8..24 = that k
                                    // (implies text_units)
    int seed_load_percent = 0;      // slots filled on average, 0 = default (70), 20..100
    int table_layout = -1;          // -1 / 0: this implementation's own occurrence table (rank lines for sigma <= 8); 1..4: the
                                    // reference's Condensed64 / Condensed512 / Flat64 / Flat512 layout, queried as it is
    int inverse_sa = -1;            // 1: ISA[position] = row as its own array (4 bytes per symbol): exact intervals through the
                                    // seed table
};

// The environment's debug overrides of the aux build, read at every build (read_aux_env: the only getenv for these six)
struct AuxEnv {
    bool no_pair_lines = false;       // GDX_NO_PAIR_LINES=1
    bool tables_shape = false;        // GDX_DEFAULT_SHAPE=tables: never the default shape
    double budget_gb = HUGE_VAL;      // GDX_AUX_BUDGET_GB (not set: infinite): caps the budget when aux_budget_bytes is 0
    int jump_bytes = 32;              // GDX_JUMP_BYTES
    bool no_jump_table = false;       // GDX_NO_JUMP_TABLE=1
    bool has_top_depth = false;       // GDX_TOP_DEPTH is set, to top_depth
    int top_depth = 0;
};

inline AuxEnv read_aux_env()
{
    auto env_int = [](const char *name, int fallback) {
        const char *e = getenv(name);
        return e ? atoi(e) : fallback;
    };
    AuxEnv env;
    env.no_pair_lines = env_int("GDX_NO_PAIR_LINES", 0) == 1;
    const char *shape = getenv("GDX_DEFAULT_SHAPE");
    env.tables_shape = shape != nullptr && strcmp(shape, "tables") == 0;
    if (const char *e = getenv("GDX_AUX_BUDGET_GB")) env.budget_gb = atof(e);
    env.jump_bytes = env_int("GDX_JUMP_BYTES", 32);
    env.no_jump_table = env_int("GDX_NO_JUMP_TABLE", 0) == 1;
    env.has_top_depth = getenv("GDX_TOP_DEPTH") != nullptr;
    env.top_depth = env_int("GDX_TOP_DEPTH", 0);
    return env;
}

// GDX_SEED_PAIRS=0: no records of the seed table's two- to four-copy repeats (experiments).  Read once per process, when the
// first seed table is built
inline bool env_no_seed_pairs()
{
    static const bool none = [] { const char *e = getenv("GDX_SEED_PAIRS"); return e != nullptr && atoi(e) == 0; }();
    return none;
}

// What the build knows of the index before it plans.  seed_tag_bits_max: kSeedTagBitsMax (layout.hpp, which needs HIP)
struct AuxPlanInput {
    uint64_t n = 0;
    int sigma = 0, layout = 0, n_searchable = 0;  // layout 0: rank lines
    uint32_t seed_tag_bits_max = 0;
    BuildOptions opts;
    AuxEnv env;
};

// The budget for auxiliary structures: BuildOptions::aux_budget_bytes, by default what the device has free minus room for query
// batches and results (1/16 of the memory, at least 4 GB) but never more than half of the device's memory.
inline double aux_budget(uint64_t free_bytes, uint64_t total_bytes, uint64_t aux_budget_bytes, const AuxEnv &env)
{
    const uint64_t reserve = std::max<uint64_t>(total_bytes / 16, 4ull << 30);
    double budget = free_bytes > reserve ? static_cast<double>(free_bytes - reserve) : 0.0;
    if (aux_budget_bytes != 0) return std::min(budget, static_cast<double>(aux_budget_bytes));
    budget = std::min(budget, static_cast<double>(total_bytes / 2));
    return std::min(budget, env.budget_gb * 1e9);
}

// (bucket, tag) must name a k-mer exactly with at most tag_bits_max tag bits: the fewest buckets a seed table of k symbols may
// have (17 GB for k = 24 whatever the text), 0 when any number will do
inline uint64_t seed_min_buckets(uint32_t k, uint32_t tag_bits_max) { return 2u * k > tag_bits_max ? 1ull << (2u * k - tag_bits_max) : 0ull; }

// The seed table's bytes as the other tables have to leave room for them: 16 bytes per distinct k-mer over the load factor --
// about n k-mers -- but never fewer than seed_min_buckets buckets of 128 bytes, and a placement that fails retries with a
// quarter more buckets
inline double seed_table_estimate(uint64_t n, uint32_t k, uint32_t load_percent, uint32_t tag_bits_max)
{
    const double bytes = 16.0 / (load_percent / 100.0) * static_cast<double>(n);
    return 1.25 * std::max(bytes, 128.0 * static_cast<double>(seed_min_buckets(k, tag_bits_max)));
}

// seed table (layout.hpp): k from the text length unless given: ceil(log4 n) + 8, so that a k-mer that occurs at all almost
// always occurs once (3.1 G symbols: 24), at most 24 (k + 32 symbols fit the search window)
inline uint32_t auto_seed_k(uint64_t n)
{
    uint32_t k = 8;
    while (k < 24 && (1ull << (2u * (k - 8u))) < n) k++;
    return k;
}

// top table depth wanted: even (the pair steps that follow consume two symbols each) and as deep as leaves about one row per
// entry (4^D <= 2 n), so that most reads can jump right after it; at most 16 (34 GB).  Measured (search_variants.md section 25):
// 3.1 G symbols: 16 beats 14 by 23 %; 2^28: 14 beats 12; 2^24: 12 beats 10.
inline uint32_t auto_top_depth(uint64_t n)
{
    uint32_t depth = 0;
    while (depth < 16 && (1ull << (2u * (depth + 2u))) <= 2ull * n) depth += 2;
    return depth;
}

// One step of the order jump and top table shrink in, which is the order of what each step costs on the headline workload:
// top 16 -> 14, jump 32 -> 16, top -> 12, jump -> 8, top -> 0, jump -> 0; false: nothing is left to give up
inline bool aux_shrink_step(uint32_t &jump_bytes, uint32_t &top_depth)
{
    if (top_depth > 14) top_depth = 14;
    else if (jump_bytes == 32) jump_bytes = 16;
    else if (top_depth > 12) top_depth = 12;
    else if (jump_bytes == 16) jump_bytes = 8;
    else if (top_depth > 0) top_depth -= top_depth >= 2 ? 2 : 1;
    else if (jump_bytes != 0) jump_bytes = 0;
    else return false;
    return true;
}

// ---- step one: before anything is allocated -------------------------------------------------------------------------------
struct AuxShape {
    bool default_shape = false, want_pairs = false;
    uint32_t seed_k = 0, seed_load_percent = 70;  // seed_k 0: no seed table
    bool want_text = false, want_sa_full = false, want_isa = false;
    bool build_any = false;  // rank-line layout, a text, and something wanted: else the build leaves the index as it is
};

inline bool aux_want_pairs(const AuxPlanInput &in) { return in.opts.pair_lines < 0 ? !in.env.no_pair_lines : in.opts.pair_lines != 0; }

// are the options those of THE DEFAULT SHAPE (below)?  Only then does step one look at the memory
inline bool aux_default_shape_asked(const AuxPlanInput &in)
{
    const BuildOptions &bo = in.opts;
    return bo.seed_symbols < 0 && bo.jump_bytes < 0 && bo.full_sa < 0 && bo.inverse_sa < 0 && bo.text_units < 0 && aux_want_pairs(in) &&
           in.layout == 0 && in.sigma >= 5 && in.n_searchable >= 4 && in.n > 0 && !in.env.tables_shape;
}

// THE DEFAULT SHAPE (round 6): options left at their defaults on a DNA-like alphabet (rank-line layout, dense symbols 1..4
// searchable) build ONE index that serves every call at its best measured speed -- seed table (k from the text length, load
// 60 %) + text units + full suffix array + inverse suffix array + pair lines + a top table of depth <= 14, no jump table:
// count / locate through the seed table (search_seed_lane_kernel), exact intervals and cursors through seed entry / text /
// ISA with the pair lines for the steps that empty an interval (search_exact_kernel4<0, ., ., true>), locate with SA[row]
// one fetch away.  3.1 G symbols: 104 GB.  It needs 8.5 bytes per symbol + the seed table inside the budget for auxiliary
// structures; where that does not fit -- or any of the structures is asked for or switched off explicitly -- the options
// mean what they say and the tables of rounds 1-3 (32-byte jump entries + top table, shrunk to the budget) are the default.
// GDX_DEFAULT_SHAPE=tables: the latter regardless (debugging aid).
// free_bytes / total_bytes: the device's memory before the build allocates (read only when aux_default_shape_asked).
inline AuxShape plan_aux_shape(const AuxPlanInput &in, uint64_t free_bytes, uint64_t total_bytes)
{
    const BuildOptions &bo = in.opts;
    AuxShape s;
    s.want_pairs = aux_want_pairs(in);
    if (bo.seed_load_percent > 0) s.seed_load_percent = static_cast<uint32_t>(bo.seed_load_percent);
    if (aux_default_shape_asked(in)) {  // does it fit?
        const uint32_t load = bo.seed_load_percent > 0 ? s.seed_load_percent : 60u;
        const double need = seed_table_estimate(in.n, auto_seed_k(in.n), load, in.seed_tag_bits_max) + 8.5 * static_cast<double>(in.n);
        if (need <= aux_budget(free_bytes, total_bytes, bo.aux_budget_bytes, in.env)) {
            s.default_shape = true;
            s.seed_load_percent = load;
        }
    }
    if (s.default_shape) {
        s.seed_k = auto_seed_k(in.n);
    } else if (bo.seed_symbols >= 1 && in.sigma >= 5) {
        s.seed_k = bo.seed_symbols == 1 ? auto_seed_k(in.n) : static_cast<uint32_t>(bo.seed_symbols);
        if (s.seed_k < 8u || s.seed_k > 24u) fail(GDX_ERR_INVALID_ARGUMENT, "seed_symbols must be 1 (automatic) or 8..24");
    }
    s.want_text = bo.text_units == 1 || s.seed_k != 0;
    s.want_sa_full = bo.full_sa == 1 || s.default_shape;
    s.want_isa = bo.inverse_sa == 1 || s.default_shape;
    s.build_any = in.layout == 0 && in.n > 0 && (s.want_pairs || s.want_text || s.want_sa_full || s.want_isa);
    return s;
}

// ---- step two: the pair lines are in place ------------------------------------------------------------------------------
struct AuxTables {
    uint32_t wanted_jump_bytes = 0, wanted_top_depth = 0;  // before the budget was applied
    uint32_t jump_bytes = 0, top_depth = 0;                // what is built
    uint64_t budget_bytes = 0;
};

// Jump and top table of an index that builds anything (AuxShape::build_any).  Both are optional and have to fit the budget
// beside what does not shrink (full and inverse suffix array, text units, the seed table's estimate); gdx_index_aux reports
// what was wanted and what was built.  free_bytes / total_bytes: the device's memory now, the pair lines allocated.
inline AuxTables plan_aux_tables(const AuxPlanInput &in, const AuxShape &s, uint64_t free_bytes, uint64_t total_bytes)
{
    const BuildOptions &bo = in.opts;
    const double n = static_cast<double>(in.n);
    AuxTables t;
    // jump table: 32-byte entries by default (BuildOptions::jump_bytes; GDX_JUMP_BYTES / GDX_NO_JUMP_TABLE override the
    // default only)
    uint32_t jump_bytes = 32;
    if (s.default_shape) jump_bytes = 0;  // (the text, SA and ISA stand in for it)
    else if (bo.jump_bytes >= 0) jump_bytes = static_cast<uint32_t>(bo.jump_bytes);
    else jump_bytes = in.env.no_jump_table ? 0u : static_cast<uint32_t>(in.env.jump_bytes);
    if (jump_bytes != 0 && jump_bytes != 8 && jump_bytes != 16 && jump_bytes != 32)
        fail(GDX_ERR_INVALID_ARGUMENT, "jump entry bytes must be 0, 8, 16 or 32");
    if (!s.want_pairs) jump_bytes = 0;  // the jump table belongs to the pair-line kernels
    uint32_t top_depth = auto_top_depth(in.n);
    if (bo.top_depth >= 0) top_depth = static_cast<uint32_t>(bo.top_depth);
    else if (in.env.has_top_depth) top_depth = static_cast<uint32_t>(in.env.top_depth);
    if (top_depth > 16u) top_depth = 16u;
    // (the default shape's top table only starts the reads the seed table does not answer -- absent k-mers, reads shorter
    // than the seed: depth 14 is 2 GB, depth 16 would be 34)
    if (s.default_shape && bo.top_depth < 0 && top_depth > 14u) top_depth = 14u;
    if (in.sigma < 5) top_depth = 0;
    if (!s.want_pairs && !s.want_text) top_depth = 0;  // nothing would read it
    t.wanted_jump_bytes = jump_bytes;
    t.wanted_top_depth = top_depth;
    const double budget = aux_budget(free_bytes, total_bytes, bo.aux_budget_bytes, in.env);
    t.budget_bytes = static_cast<uint64_t>(budget);
    // (the full suffix array and the text units are asked for explicitly: they count, but do not shrink)
    double fixed = ((s.want_sa_full ? 4.0 : 0.0) + (s.want_isa ? 4.0 : 0.0)) * n + (s.want_text ? 0.5 : 0.0) * n;
    if (s.seed_k != 0) {
        const double seed_bytes = seed_table_estimate(in.n, s.seed_k, s.seed_load_percent, in.seed_tag_bits_max);
        if (seed_bytes > budget && bo.seed_symbols > 1)  // an explicit k whose smallest table cannot fit: say so now
            fail(GDX_ERR_INVALID_ARGUMENT,
                 "seed_symbols = %u needs a seed table of at least %.1f GB (2^(2k - 21) buckets of 128 bytes, or 16 bytes per "
                 "k-mer over the load factor), the budget for auxiliary structures is %.1f GB: choose a smaller k or "
                 "seed_symbols = 1", s.seed_k, seed_bytes / 1.25 / 1e9, budget / 1e9);
        fixed += seed_bytes;
    }
    while (fixed + static_cast<double>(jump_bytes) * n + (top_depth ? 8.0 * static_cast<double>(1ull << (2u * top_depth)) : 0.0) > budget)
        if (!aux_shrink_step(jump_bytes, top_depth)) break;
    t.jump_bytes = jump_bytes;
    t.top_depth = top_depth;
    return t;
}

}  // namespace gdx
