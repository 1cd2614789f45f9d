// slim_plan.h -- the host arithmetic of a SLIM-BPR launch: the environment's knobs (SlimKnobs, parsed in ONE place), the grids of the
// two persistent kernels, the sparse store's segment cuts, the sizes of the sorts -- and the constants the kernels share with it.
// Plain C++17 on plain numbers -- no HIP call; the compute-unit count and the occupancy come in as arguments -- so g++ builds it and
// tests/test_slim_plan.py runs it without a GPU.  Included by slim.hip (through slim_flow.cuh).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <optional>
#include <string>
#include <vector>

namespace mi355rec {
namespace {

constexpr int LOSS_SLOTS = 1024;
constexpr int FLOW_THREADS = 1024;                    // 16 wavefronts: the turn takers of an owned row, or 16 independent steps
constexpr int FLOW_WAVES = FLOW_THREADS / 64;
constexpr int FLOW_REGS = 4;                          // profile entries per lane whose cells stay in registers between the passes
constexpr int MAX_OWNERS = 192;
// (the step queue of a workgroup, LocalQueue in slim_flow.cuh: steps fetched per device atomic, chunks the ring holds)
constexpr int LQ_CHUNK = 16, LQ_RING = 8;
// Profiles longer than the FLOW_REGS x 64 entries whose cells a wavefront keeps in registers are walked in BLOCKS of the same
// size with all loads of a block in flight (round 4's first version took them 64 at a time, one dependent round trip each: 14 % of
// the ML-20M users have more than 256 items, and those steps made up most of every critical section).
constexpr int FLOW_BLOCK = 64 * FLOW_REGS;

// The MI355REC_SLIM_* switches (and the lock directory) as one ABI call sees them: parsed when the call begins, because tests and
// scripts change them between calls of one process.  An integer knob that is unset OR EMPTY takes its default; a switch is on as
// soon as the variable exists, whatever it holds.
struct SlimKnobs {
    int nap = 1;                        // NAP: how much longer a waiting wavefront sleeps between polls (SlimParams::nap)
    bool no_presched = false;           // NO_PRESCHED: the next epoch is not scheduled behind the running one
    bool prof = false;                  // PROF: phase clocks of the dataflow kernels, printed after every launch
    bool inject_abort = false;          // INJECT_ABORT (test hook): the abort flag is up before the first step polls it
    int sym_spare_cus = 64;             // SYM_SPARE_CUS: compute units the symmetric kernel leaves to the next epoch's schedule
    std::optional<int> sym_wgs;         // SYM_WGS: its workgroups (default: what fits)
    std::optional<int> sym_long_wgs;    // SYM_LONG_WGS: ... of which for the long profiles (default: a quarter)
    int owners = 128;                   // OWNERS: owned rows of a dense launch, at most MAX_OWNERS
    std::optional<int> cus;             // CUS: compute units a dense launch asks the lease for (default: all)
    int owner_min_steps = 24;           // OWNER_MIN_STEPS: steps of the stream a row needs to get an owner (at least 2)
    bool no_owner_gate = false;         // NO_OWNER_GATE: owners without the device's lock file
    double gate_wait_s = 600.0;         // GATE_WAIT_S: how long a symmetric launch waits for another process's lock
    std::string lock_dir = "/tmp";      // MI355REC_LOCK_DIR, else XDG_RUNTIME_DIR, else /tmp
};

// the only place of slim.hip and its headers that reads the environment
inline SlimKnobs read_slim_knobs() {
    const auto text = [](const char *name) -> const char * {
        const char *v = getenv(name);
        return v && *v ? v : nullptr;
    };
    const auto number = [&](const char *name) { return text(name) ? std::optional<int>(atoi(text(name))) : std::nullopt; };
    const auto is_set = [](const char *name) { return getenv(name) != nullptr; };
    SlimKnobs k;
    k.nap = number("MI355REC_SLIM_NAP").value_or(k.nap);
    k.no_presched = is_set("MI355REC_SLIM_NO_PRESCHED");
    k.prof = is_set("MI355REC_SLIM_PROF");
    k.inject_abort = is_set("MI355REC_SLIM_INJECT_ABORT");
    k.sym_spare_cus = number("MI355REC_SLIM_SYM_SPARE_CUS").value_or(k.sym_spare_cus);
    k.sym_wgs = number("MI355REC_SLIM_SYM_WGS");
    k.sym_long_wgs = number("MI355REC_SLIM_SYM_LONG_WGS");
    k.owners = number("MI355REC_SLIM_OWNERS").value_or(k.owners);
    k.cus = number("MI355REC_SLIM_CUS");
    k.owner_min_steps = number("MI355REC_SLIM_OWNER_MIN_STEPS").value_or(k.owner_min_steps);
    k.no_owner_gate = is_set("MI355REC_SLIM_NO_OWNER_GATE");
    if (const char *w = getenv("MI355REC_SLIM_GATE_WAIT_S")) k.gate_wait_s = atof(w);      // (empty: 0 s, as atof reads it)
    const char *dir = text("MI355REC_LOCK_DIR");
    if (!dir) dir = text("XDG_RUNTIME_DIR");
    if (dir) k.lock_dir = dir;
    return k;
}

// bits a radix sort has to walk to tell n_values values apart (at least 1)
inline int bits_for(unsigned long long n_values) {
    int b = 1;
    while (b < 63 && (1ull << b) < n_values) ++b;
    return b;
}

// the dataflow kernels apply; otherwise slim_ordered_kernel (cell ids of the symmetric store are 32-bit sort keys)
inline bool flow_supported(bool symmetric, int n_items) { return !(symmetric && n_items > 92681); }

// the sparse store cuts an epoch into segments with a pruning pass between them: those are scheduled one after the other
inline bool schedules_ahead(bool sparse_weights, bool symmetric, int n_items, const SlimKnobs &knobs) {
    return !sparse_weights && flow_supported(symmetric, n_items) && !knobs.no_presched;
}

// Capacity of the symmetric store's cell sort and of `pred` once n_cells no longer fit.  (A buffer that grows is handed back to the
// block cache, which waits for the device -- and so for the dataflow kernel this schedule is meant to run behind: sized once, 25 %
// above the expected 2 nnz n / n_users cells of n uniformly drawn users.)
inline size_t roomy_cell_capacity(size_t nnz, int n, int n_users, long long n_cells) {
    return std::max((size_t)(2.5 * (double)nnz * (double)n / (double)n_users) + 1024, (size_t)n_cells + (size_t)(n_cells >> 2));
}

// ---- symmetric store ------------------------------------------------------------------------------------------------------------
struct SymLaunch {
    int long_wgs, grid;     // workgroups that take the long profiles (a workgroup per step); all workgroups
};
// Steps in flight = wavefronts of the grid: more of them only adds pollers once the chain of dependent steps is the bound (every
// workgroup has to be resident: at most what the device holds at once, per_cu per compute unit) ... leaving some compute units to
// the schedule of the next epoch (`ahead`; the kernel is bound by its chain of dependent steps, not by the number of steps in
// flight: 512 of them were as fast as 8 192).
inline SymLaunch plan_sym_launch(int cus, int per_cu, bool ahead, int n, int n_short, const SlimKnobs &knobs) {
    const int spare = ahead ? std::max(0, std::min(cus / 2, knobs.sym_spare_cus)) : 0;
    const int fit = (cus - spare) * per_cu;
    const int most = std::max(2, std::min(knobs.sym_wgs.value_or(fit), fit));
    // a quarter of them for the long profiles (14 % of the steps at the ML-20M shape, a workgroup each)
    const int n_long = n - n_short;
    const int long_wgs = std::min(n_long, std::max(1, std::min(most - 1, knobs.sym_long_wgs.value_or(most / 4))));
    const int short_wgs = (int)(((long long)n_short + FLOW_WAVES - 1) / FLOW_WAVES);
    return {long_wgs, long_wgs + std::max(1, std::min(short_wgs, most - long_wgs))};
}

// ---- dense store ----------------------------------------------------------------------------------------------------------------
// Before the lease: does this launch want owned rows (the busiest rows of its stream, each in the LDS of one workgroup), and how
// many compute units does it ask for.
struct DensePlan {
    bool wanted;
    int want_slots;
    size_t row_bytes;       // one row of S as floats, padded to 16 bytes
};
inline DensePlan plan_dense_launch(int n_items, bool sparse_weights, int cus, const SlimKnobs &knobs) {
    const size_t row_bytes = ((size_t)n_items * sizeof(float) + 15) & ~(size_t)15;
    const bool wanted = std::min(MAX_OWNERS, knobs.owners) > 0 && row_bytes + 4096 <= 160 * 1024 && !sparse_weights;
    return {wanted, std::max(32, std::min(cus, knobs.cus.value_or(cus))), row_bytes};
}

// After the lease (`slots` compute units, 0: none).  With owners: one workgroup per leased compute unit (they must all be resident);
// without: whatever fits (blocks_per_cu_no_lds workgroups per compute unit; not looked at with owners).
struct DenseGrid {
    bool owners;
    size_t lds;
    int grid, max_owners, min_steps;
    bool needs_lds_attribute;       // more dynamic LDS than a kernel gets without hipFuncAttributeMaxDynamicSharedMemorySize
};
inline DenseGrid dense_grid(int slots, int cus, int blocks_per_cu_no_lds, size_t row_bytes, const SlimKnobs &knobs) {
    DenseGrid g;
    g.owners = slots > 0;
    g.lds = g.owners ? row_bytes : 0;
    g.needs_lds_attribute = g.lds > 48 * 1024;
    g.grid = g.owners ? slots : cus * blocks_per_cu_no_lds;
    g.max_owners = std::min(std::min(MAX_OWNERS, knobs.owners), g.grid / 2);
    g.min_steps = std::max(2, knobs.owner_min_steps);
    return g;
}

// ---- sparse store ---------------------------------------------------------------------------------------------------------------
// One epoch of n steps.  Sparse store: the stream is cut after every step whose index is a positive multiple of n / 5 --
// `numCurrentBatch % (totalNumberOfBatch/5) == 0 and numCurrentBatch != 0` with C integer division (.pyx:320-324; the module sets
// cdivision) -- and the rows are pruned there.
struct Segment {
    int first, count;
    bool prune_after;
};
inline std::vector<Segment> sparse_segments(int n, bool sparse_weights) {
    if (!sparse_weights || n < 5) return {{0, n, false}};
    std::vector<Segment> segments;
    const int every = n / 5;
    int first = 0;
    while (first < n) {
        // steps first .. cut (inclusive) run, then the rows are pruned if `cut` is a rebalance point
        const int cut = std::max(1, (first + every - 1) / every) * every;      // next multiple of `every` at or after `first`, never step 0
        const int last = std::min(cut, n - 1);
        segments.push_back({first, last - first + 1, cut <= n - 1});
        first = last + 1;
    }
    return segments;
}

}  // namespace
}  // namespace mi355rec
