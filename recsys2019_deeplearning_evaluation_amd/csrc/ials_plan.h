// ials_plan.h -- the host arithmetic of an IALS half-step: the environment's knobs (IalsKnobs, parsed in ONE place), the tile counts and
// the kernel instance each of them selects, the sizes of the LDS and HBM buffers, the work items of a row range (which rows are split
// into parts, in which order they run), the batches of a two-stage epoch, the accounting -- and the constants the kernels share with it.
// Plain C++17 on plain numbers -- no HIP call; the free memory of the device comes in as an argument -- so g++ builds it and
// tests/test_ials_plan.py runs it without a GPU.  Included by ials.hip (through ials_kernels.cuh).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <optional>
#include <utility>
#include <vector>

#include "ials_tile.h"

#ifdef __HIPCC__
#define MI355REC_IALS_HOST_DEVICE __host__ __device__
#else
#define MI355REC_IALS_HOST_DEVICE
#endif

namespace mi355rec {
namespace {

constexpr int CHUNK = 16;   // profile rows staged per LDS round
#ifndef MI355REC_IALS_GRAM_CHUNK
#define MI355REC_IALS_GRAM_CHUNK 32
#endif
constexpr int GRAM_CHUNK = MI355REC_IALS_GRAM_CHUNK;   // ... by the Gramian stage of a two-stage epoch
constexpr int MAX_KT = 16, MAX_NT = MAX_KT * (MAX_KT + 1) / 2;
constexpr int ROW_THREADS = 512, ROW_WAVES = ROW_THREADS / 64;   // 2 wavefronts per SIMD: 256 VGPRs for the tiles of a wavefront
constexpr int TILE_WAVES = ROW_WAVES - 1;                        // the solve stage: wavefront 0 is the panel wavefront and holds no tile
// The Gramian stage of a two-stage epoch: 1024 threads, tiles over sixteen wavefronts
constexpr int GRAM_THREADS = 1024, GRAM_WAVES = GRAM_THREADS / 64;
// the solve stage holds the tiles on 7 wavefronts: up to 13 slots (k <= 207) fit two workgroups per CU
constexpr int MAX_SOLVE_SLOTS = 13;
constexpr int MAX_PARTS = 64;            // parts a long profile is split into, at most
constexpr int MIN_BATCH_ROWS = 64;       // a systems buffer that cannot be had is halved down to this many slabs, not further

// ---- the environment ------------------------------------------------------------------------------------------------------------
// The MI355REC_IALS_* switches as one ABI call sees them (PHASES: as the create call saw it).  TWO_STAGE, SYSTEM_GIB and PART_ROWS
// are numbers as atoi / atof read them -- an EMPTY value is a 0: two-stage epochs off, the smallest buffer, parts of CHUNK rows;
// the other three are on as soon as the variable exists, whatever it holds.
struct IalsKnobs {
    bool two_stage = true;                  // TWO_STAGE=0: one-kernel epochs
    std::optional<double> system_gib;       // SYSTEM_GIB: size of the two-stage epochs' systems buffer (default: decide_system_gib)
    int part_rows = 4096;                   // PART_ROWS: profile entries per part of a split row, a multiple of CHUNK (tests)
    bool no_split = false;                  // NO_SPLIT: no row is split (tests)
    bool same_panel_wave = false;           // SAME_PANEL_WAVE (diagnostics): every workgroup's panel wavefront is wavefront 0
    bool phases = false;                    // PHASES: shader-clock totals of the kernels' phases, printed after every half-step
};

// the only place of ials.hip and its headers that reads the environment
inline IalsKnobs read_ials_knobs() {
    IalsKnobs k;
    if (const char *v = getenv("MI355REC_IALS_TWO_STAGE")) k.two_stage = atoi(v) != 0;
    if (const char *v = getenv("MI355REC_IALS_SYSTEM_GIB")) k.system_gib = atof(v);
    if (const char *v = getenv("MI355REC_IALS_PART_ROWS")) k.part_rows = std::max(CHUNK, atoi(v) / CHUNK * CHUNK);
    k.no_split = getenv("MI355REC_IALS_NO_SPLIT") != nullptr;
    k.same_panel_wave = getenv("MI355REC_IALS_SAME_PANEL_WAVE") != nullptr;
    k.phases = getenv("MI355REC_IALS_PHASES") != nullptr;
    return k;
}

// ---- tiles and the kernel instances they select -----------------------------------------------------------------------------------
// The augmented system of k factors (the rhs row included) is KT x KT tiles of 16 x 16; its lower triangle has NT of them.
constexpr int KT(int k) { return (k + 1 + 15) / 16; }
constexpr int NT(int k) { return KT(k) * (KT(k) + 1) / 2; }

// The SLOTS (tiles per wavefront) each kernel is compiled for.  dispatch_slots() calls f(std::integral_constant<int, N>) for the N of
// the list that equals n and says whether there was one: the launch code picks its template instance this way from the functions
// below, so the rounding of a slot count to an instance is written once.
template <int... Ns>
struct Slots {};
using RowSlots = Slots<1, 2, 4, 6, 8, 10, 12, 13, 15, 17>;     // ials_row_kernel<N, 0, ROW_THREADS>
using GramSlots = Slots<1, 2, 3, 4, 5, 6, 7, 8>;               // ials_row_kernel<N, 1, GRAM_THREADS>
using SolveSlots = Slots<1, 2, 4, 6, 8, 10, 11, 12, 13>;       // ials_solve_kernel<N>
template <int... Ns, class F>
bool dispatch_slots(Slots<Ns...>, int n, F &&f) {
    return ((n == Ns ? (f(std::integral_constant<int, Ns>{}), true) : false) || ...);
}

// one-kernel epoch, NT tiles over ROW_WAVES wavefronts: the instance's SLOTS, one of RowSlots for every k <= 255 (17: 16 x 16 tiles)
inline int row_slots(int NT) {
    const int need = (NT + ROW_WAVES - 1) / ROW_WAVES;
    if (need <= 2) return need;
    if (need <= 12) return (need + 1) / 2 * 2;
    return need == 13 ? 13 : (need <= 15 ? 15 : 17);
}
// Gramian stage: every count has its instance (one of GramSlots wherever two-stage epochs apply)
inline int gram_slots(int NT) { return (NT + GRAM_WAVES - 1) / GRAM_WAVES; }
// solve stage, NT tiles over TILE_WAVES wavefronts: what it needs, and the instance's SLOTS, one of SolveSlots (the largest where
// even that one does not hold the tiles: two_stage_applies keeps those k away from it)
inline int solve_slots(int NT) { return (NT + TILE_WAVES - 1) / TILE_WAVES; }
inline int solve_instance_slots(int NT) {
    const int need = solve_slots(NT);
    if (need <= 2) return need;
    return need <= 10 ? (need + 1) / 2 * 2 : std::min(need, MAX_SOLVE_SLOTS);
}

// Two-stage epochs: on unless MI355REC_IALS_TWO_STAGE=0 or the solve stage's 13 tile slots do not cover k (k > 207).
inline bool two_stage_applies(int k, const IalsKnobs &knobs) { return knobs.two_stage && solve_slots(NT(k)) <= MAX_SOLVE_SLOTS; }

// ---- buffer sizes ---------------------------------------------------------------------------------------------------------------
// doubles of dynamic LDS a kernel needs for k factors.  stage 0: ials_row_kernel of a one-kernel epoch; 1: the Gramian stage; 2: the
// solve stage (1 and 2 are launched only where two_stage_applies).
inline size_t lds_doubles(int k, int stage) {
    const int kt = KT(k), KP = kt * 16;
    const int first = stage == 2 ? kt * 16 * TP : (stage == 1 ? 2 * GRAM_CHUNK * KP : std::max(2 * CHUNK * KP, kt * 16 * TP));
    return (size_t)first + (size_t)kt * 16 * TP + (size_t)kt * 16 + 3 * (size_t)KP;   // staging | panel, Linv, z / x / acc
}

// doubles of one row's augmented system (or of one part of a split row) as the kernel that builds it lays it out: the Gramian stage
// of a two-stage epoch, else the one kernel
inline size_t slab_doubles(int k, bool two_stage) {
    return two_stage ? (size_t)gram_slots(NT(k)) * 4 * GRAM_THREADS : (size_t)row_slots(NT(k)) * 4 * ROW_THREADS;
}

// ---- batches of a two-stage epoch: how many systems the buffer holds ----------------------------------------------------------------
// MI355REC_IALS_SYSTEM_GIB worth of slabs (default: 8, but never more than a quarter of the memory the device has free when the
// handle first asks -- several handles on one device, or a device shared with PyTorch / RCCL, each take a share instead of 8 GiB;
// a free count nobody could tell comes as SIZE_MAX), ...
inline double decide_system_gib(size_t free_bytes, const IalsKnobs &knobs) {
    double gib = std::min(8.0, (double)free_bytes / 4.0 / 1073741824.0);
    if (knobs.system_gib) gib = *knobs.system_gib;
    return std::max(0.001, gib);
}
// ... at most the longer side
inline int rows_per_batch(double system_gib, int k, size_t longest_side) {
    const size_t sys_bytes = slab_doubles(k, true) * sizeof(double);
    return (int)std::max<size_t>(1, std::min<size_t>(longest_side, (size_t)(system_gib * 1073741824.0) / sys_bytes));
}
// A buffer of per_batch slabs could not be had: the size to try next, or nothing -- MIN_BATCH_ROWS slabs were not to be had either,
// the caller falls back to the one-kernel epoch.
inline std::optional<double> halved_system_gib(int per_batch, int k) {
    if (per_batch <= MIN_BATCH_ROWS) return std::nullopt;
    return std::max(0.001, 0.5 * (double)per_batch * (double)slab_doubles(k, true) * sizeof(double) / 1073741824.0);
}

// ---- work items -----------------------------------------------------------------------------------------------------------------
// what the kernels read as an int4: {row, part, n_parts, first part slot}
struct WorkItem {
    int x, y, z, w;
};

// The profile entries part `part` of `n_parts` takes of a row's [beg, end): equal slices rounded up to whole chunks of the kernel that
// runs it (trailing parts may be empty).
struct PartRange {
    int beg, end;
};
MI355REC_IALS_HOST_DEVICE inline PartRange part_range(int beg, int end, int part, int n_parts, int chunk) {
    const int per = (((end - beg + n_parts - 1) / n_parts) + chunk - 1) / chunk * chunk;
    beg = end < beg + part * per ? end : beg + part * per;
    return {beg, end < beg + per ? end : beg + per};
}

struct WorkPlan {
    std::vector<int> rows;              // the warm rows of the range, longest profile first
    std::vector<WorkItem> items;        // most expensive first
    int n_split = 0, part_slots = 0;    // rows that were split, parts of all of them
    double nnz_rows = 0;                // profile entries of `rows`
};
// Rows [r0, r1) of the side whose CSR row pointer is `ptr` and whose rows, longest profile first, are `order`.
// Warm rows only (IALSRecommender.py:78-82).  Work items, most expensive first.  cost(row) = L k^2 (Gramian) + k^3 / 3 (solve), in
// units of k^2: L + k / 3.  A row with more than 2 x PART_ROWS profile entries is split into parts of PART_ROWS (at most 64 parts);
// the part that arrives last merges and solves (ials_row_kernel).  The split depends on the row alone -- not on what else the call
// holds -- so a row-sharded epoch adds every row up in the same order as the single-GPU epoch.
inline WorkPlan plan_work_items(const int *ptr, const std::vector<int> &order, int r0, int r1, int k, const IalsKnobs &knobs) {
    WorkPlan w;
    for (int r : order)
        if (r >= r0 && r < r1 && ptr[r + 1] > ptr[r]) {
            w.rows.push_back(r);
            w.nnz_rows += ptr[r + 1] - ptr[r];
        }
    const double solve_cost = k / 3.0;
    std::vector<std::pair<double, int>> keyed;
    for (int r : w.rows) {
        const int L = ptr[r + 1] - ptr[r];
        int parts = 1;
        if (!knobs.no_split && L > 2 * knobs.part_rows) parts = std::min(MAX_PARTS, (L + knobs.part_rows - 1) / knobs.part_rows);
        if (parts > 1) {
            for (int q = 0; q < parts; ++q) {
                keyed.emplace_back((double)L / parts + (q == 0 ? solve_cost : 0.0), (int)w.items.size());
                w.items.push_back({r, q, parts, w.part_slots});
            }
            w.part_slots += parts;
            ++w.n_split;
        } else {
            keyed.emplace_back(L + solve_cost, (int)w.items.size());
            w.items.push_back({r, 0, 1, 0});
        }
    }
    if (w.n_split) {        // (without a split row the length order is the cost order)
        std::stable_sort(keyed.begin(), keyed.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
        std::vector<WorkItem> sorted(keyed.size());
        for (size_t i = 0; i < keyed.size(); ++i) sorted[i] = w.items[keyed[i].second];
        w.items.swap(sorted);
    }
    return w;
}

// Two-stage epochs: the rows of the half-step, in cost order, in batches of per_batch rows whose systems share the buffer; per batch
// the items that build the systems (the batch's rows and parts, still most expensive first), then one item per row that solves.
struct Batch {
    int gram_off, gram_n, solve_off, solve_n;       // into `items` / `sys_slot`
};
struct BatchPlan {
    std::vector<WorkItem> items;        // of all batches, one after the other
    std::vector<int> sys_slot;          // slab of every item's row in the systems buffer
    std::vector<Batch> batches;
};
inline BatchPlan plan_batches(const std::vector<int> &rows, const std::vector<WorkItem> &items, int per_batch, int n_side) {
    const int n_local = (int)rows.size(), n_batches = (n_local + per_batch - 1) / per_batch;
    BatchPlan plan;
    // position of every row in the cost order -> (batch, slab)
    std::vector<int> pos_of_row((size_t)n_side, -1);
    for (int i = 0; i < n_local; ++i) pos_of_row[rows[i]] = i;
    // stage-1 items per batch (the sorted list filtered), then one stage-2 item per row
    std::vector<std::vector<WorkItem>> gram_items((size_t)n_batches);
    for (const WorkItem &it : items) gram_items[(size_t)(pos_of_row[it.x] / per_batch)].push_back(it);
    for (int b = 0; b < n_batches; ++b) {
        Batch batch;
        batch.gram_off = (int)plan.items.size();
        batch.gram_n = (int)gram_items[b].size();
        for (const WorkItem &it : gram_items[b]) {
            plan.items.push_back(it);
            plan.sys_slot.push_back(pos_of_row[it.x] % per_batch);
        }
        batch.solve_off = (int)plan.items.size();
        const int r_end = std::min(n_local, (b + 1) * per_batch);
        batch.solve_n = r_end - b * per_batch;
        for (int i = b * per_batch; i < r_end; ++i) {
            plan.items.push_back({rows[i], 0, 1, 0});
            plan.sys_slot.push_back(i % per_batch);
        }
        plan.batches.push_back(batch);
    }
    return plan;
}

// ---- accounting -----------------------------------------------------------------------------------------------------------------
// ALGORITHMIC work of a half-step, SURVEY.md section 8(d): Gramian 2 * nnz * k^2 flop per pass (+ the k x k base Gramian 2 n k^2),
// solve k^3/3 + 2 k^2 per row; bytes: gathered factor rows + confidences + the solved rows.
struct HalfStepWork {
    double flops, bytes;
};
inline HalfStepWork half_step_work(double nnz_rows, int n_local, int n_other, int n_factors) {
    const double k = n_factors;
    return {2.0 * nnz_rows * k * k + (double)n_local * (k * k * k / 3.0 + 2.0 * k * k) + 2.0 * (double)n_other * k * k,
            nnz_rows * (8.0 * k + 8.0) + (double)n_local * 8.0 * k};
}

}  // namespace
}  // namespace mi355rec
