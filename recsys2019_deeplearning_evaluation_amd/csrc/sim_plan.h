// sim_plan.h -- the column schedule of one similarity build call: which columns the call computes (ColumnSelection), which of the
// two launches takes each of them, how heavy columns are split, in what order the work items are queued (plan_columns).
// Host arithmetic on host arrays only -- no HIP runtime call, nothing read from the environment -- so a plain C++17 compiler
// builds it and tests/test_sim_plan.py runs it without a GPU.  Included by sim.hip (through sim_kernels.cuh, which shares the
// constants below with the host).
#pragma once

#include "../../include/mi355rec.h"

#include <hip/hip_vector_types.h>

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace mi355rec {
namespace {

// what the accumulator cells of the column kernels hold (sim_kernels.cuh, sim_column_kernel's MODE)
enum { ACC_COUNTS = 0, ACC_INT32 = 1, ACC_WIDE = 2 };

// (2.0e6 until pieces of a multi-GPU part were measured on their own: the 512 most expensive columns of an 8-way part of the ML-20M
// shape, 1.07 M pair-adds per column, took 0.51 ms packed against 0.23 ms on the 32-bit kernel -- a few long columns and nothing to
// interleave them with --, columns [0, 4096) of the whole shape, 1.05 M, 1.51 against 1.45 ms; at 0.87 M and below packed wins)
constexpr double PACKED_MAX_PAIRS_PER_COLUMN = 1.0e6;
constexpr int PACKED_PART_ENTRIES = 49152;      // walk entries (>= users) of one part of a column with 65 536 users or more: its counts stay below 2^16

// Interleaved parts (multi-GPU): the columns in cost order are dealt to the parts in serpentine order -- position p of the
// cost order belongs to group p / n_parts and, inside the group, to part p % n_parts (even groups) or its mirror image (odd
// groups) -- so every part receives the same NUMBER of columns (+-1) and the same COST (the heavy head of the order is
// spread over all parts).  A part's output rows are its groups, in order.
inline int part_of_position(long long pos, int n_parts) {
    const long long group = pos / n_parts;
    const int within = (int)(pos % n_parts);
    return (group & 1) ? n_parts - 1 - within : within;
}

// The columns of one call: the contiguous range [start, end) (n_parts == 0), or interleaved part `part` of `n_parts`, of whose
// columns (in output order) only slots [slot_first, slot_first + slot_count) are built, into output rows 0 .. slot_count - 1 (a
// sharded build computes its part in pieces; the wide top-K path walks a part in blocks).
struct ColumnSelection {
    int start = 0, end = 0;
    int part = 0, n_parts = 0, slot_first = 0, slot_count = 0x7fffffff;
    static ColumnSelection range(int start, int end) {
        ColumnSelection s;
        s.start = start;
        s.end = end;
        return s;
    }
    static ColumnSelection part_of(int part, int n_parts, int slot_first = 0, int slot_count = 0x7fffffff) {
        ColumnSelection s;
        s.part = part;
        s.n_parts = n_parts;
        s.slot_first = slot_first;
        s.slot_count = slot_count;
        return s;
    }
};

// a selection's columns in output order (`cost_order`: all columns, most expensive first)
inline std::vector<int> selection_columns(const ColumnSelection &sel, const std::vector<int> &cost_order) {
    std::vector<int> columns;
    if (sel.n_parts == 0) {
        for (int c = sel.start; c < sel.end; ++c) columns.push_back(c);
        return columns;
    }
    int seen = 0;
    for (long long pos = 0; pos < (long long)cost_order.size(); ++pos)
        if (part_of_position(pos, sel.n_parts) == sel.part) {
            if (seen >= sel.slot_first && (int)columns.size() < sel.slot_count) columns.push_back(cost_order[(size_t)pos]);
            ++seen;
        }
    return columns;
}

// the environment's switches of a build call, as the caller has parsed them (once per call: tests and scripts set them between calls)
struct SimKnobs {
    bool one_wg_per_cu = false;     // MI355REC_SIM_ONE_WG_PER_CU is set
    int min_part_users = 0;         // MI355REC_SIM_MIN_PART_USERS: max(64, its value); 0 = not set
    bool fast_topk = true;          // false: MI355REC_SIM_FAST_TOPK=0
    int packed = -1;                // MI355REC_SIM_PACKED: 1 / 0 = its value is non-zero / zero; -1 = not set
    bool no_packed = false;         // MI355REC_SIM_NO_PACKED is set
    bool packed_heavy = true;       // false: MI355REC_SIM_PACKED_HEAVY=0
    int packed_demote = -1;         // MI355REC_SIM_PACKED_DEMOTE: like `packed`
    bool phases = false;            // MI355REC_SIM_PHASES is set
};

struct ColumnPlanInput {
    // per column, from the constructor: pair-adds, the columns most expensive first, [n_cols + 1] users, [n_cols + 1] walk entries
    const std::vector<long long> &cost;
    const std::vector<int> &cost_order, &csc_ptr_host, &walk_ptr_host;
    int n_cols, tile_w, n_tiles, acc_mode, group_lanes;
    int topK;                       // of this call (0: dense columns)
    bool dense;
    int similarity, shrink;         // the configuration, where the threshold-first selection depends on it
    float tversky_alpha, tversky_beta;
    int cus;
    size_t lds_fixed, lds_packed_fixed;     // bytes of LDS next to the accumulator: the 32-bit kernel's, the packed-counts kernel's
    ColumnSelection sel;
    SimKnobs knobs;
};

struct ColumnPlan {
    int threads = 0, max_grid = 0;          // launch shape of the 32-bit kernel
    size_t lds = 0, lds_packed = 0;
    int acc_words = 0, packed_words = 0;
    bool fast_topk = false;
    // work lists in their device layout: [the packed kernel's items | the 32-bit kernel's items, the merge items last | (on the
    // device) room for every packed item handed over]
    int n_packed = 0, n_legacy = 0;
    std::vector<int4> items;                // {column, part, n_parts, first part slot}, see SimParams::items
    std::vector<int2> ranges;               // per item, the column's [begin, end) in the walk arrays
    int part_slots = 0, n_split = 0;
    int n_local = 0;                        // columns of the call = rows of its output
    int start = 0, end = 0;                 // the range the kernel's output rows count from (an interleaved part: all columns)
    long long cost_sum = 0;
    double nnz_range = 0;
    std::vector<int> out_slot;              // interleaved parts: [n_cols] output row of every column, -1 outside the call
};

// threshold-first selection (fast_column_topk in the kernel): positive denominators only (the set-based modes and tversky's
// alpha / beta inside the range the approximation's error bound was derived for), K well below the number of thread maxima
inline bool fast_topk_for(const ColumnPlanInput &in, int n_threads) {
    const bool unit_kernel = in.acc_mode != ACC_WIDE;
    const bool tversky_ok = in.similarity != MI355REC_SIM_TVERSKY ||
                            (in.tversky_alpha >= 0.f && in.tversky_alpha <= 4.f && in.tversky_beta >= 0.f && in.tversky_beta <= 4.f);
    return in.knobs.fast_topk && unit_kernel && in.n_tiles == 1 && in.topK > 0 && 4 * in.topK <= n_threads &&
           in.similarity != MI355REC_SIM_EUCLIDEAN && in.shrink >= 0 && tversky_ok;
}

// work items most expensive first (stable): keyed = (item cost, index into items)
inline void sort_items_by_cost(std::vector<std::pair<long long, int>> &keyed, std::vector<int4> &items) {
    std::stable_sort(keyed.begin(), keyed.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
    std::vector<int4> sorted(keyed.size());
    for (size_t i = 0; i < keyed.size(); ++i) sorted[i] = items[keyed[i].second];
    items.swap(sorted);
}

// The columns of the call (in_call) that the packed-counts launch takes (is_packed), and the pair-adds of the two launches.
inline void choose_packed_columns(const ColumnPlanInput &in, const std::vector<char> &in_call, int packed_grid, std::vector<char> &is_packed,
                                  long long &packed_cost, long long &legacy_cost) {
    const bool heavy_parts = in.knobs.packed_heavy;
    is_packed.assign((size_t)in.n_cols, 0);
    for (int c : in.cost_order) {
        if (!in_call[c]) continue;
        // (columns of 65 536 users or more: accumulated there in parts of fewer users each, added up by the 32-bit launch; more
        // than 64 such parts: left to the 32-bit kernel)
        const int n_c = in.walk_ptr_host[c + 1] - in.walk_ptr_host[c];
        const bool many = in.csc_ptr_host[c + 1] - in.csc_ptr_host[c] >= 65536;
        if ((many ? heavy_parts && n_c <= 64 * PACKED_PART_ENTRIES : true) && in.cost[c] >= 16ll * std::max(1, in.topK)) {
            is_packed[(size_t)c] = 1;
            packed_cost += in.cost[c];
        } else {
            legacy_cost += in.cost[c];
        }
    }
    // HEAVY columns gain nothing from the packed launch -- what it offers is a second workgroup's accumulation beside a column's
    // selection phases, and a heavy column is nearly all accumulation, on workgroups of 8 wavefronts instead of 16 (the 8 heaviest
    // columns of an 8-way part of the ML-20M shape: 0.37 ms packed against 0.125 ms; 504 columns of 0.93 M pair-adds: 0.245 against
    // 0.204 ms; 715 of 0.26 M: 0.102 against 0.115 ms -- packed wins).  Heavy = more than a quarter of a packed workgroup's fair share
    // of the call, and at least 0.5 M pair-adds.  Where such columns are a large share of the call (a part of an 8-way build: 60 %
    // of its pair-adds; the whole shape: 14 %, where a second launch of that size only adds a tail -- measured 3.05 against 3.00 ms)
    // they go to the 32-bit launch behind this one: slowest part of 8 0.56 -> 0.45-0.47 ms, identical output.
    // MI355REC_SIM_PACKED_DEMOTE=0 / 1 forces it off / on.
    const long long heavy = std::max<long long>(500000, packed_cost / ((long long)packed_grid * 4));
    long long heavy_cost = 0;
    for (int c : in.cost_order)
        if (in_call[c] && is_packed[(size_t)c] && in.cost[c] > heavy) heavy_cost += in.cost[c];
    const bool demote = in.knobs.packed_demote >= 0 ? in.knobs.packed_demote != 0 : (double)heavy_cost >= 0.4 * (double)packed_cost;
    if (demote)
        for (int c : in.cost_order) {
            if (!in_call[c] || !is_packed[(size_t)c] || in.cost[c] <= heavy) continue;
            is_packed[(size_t)c] = 0;
            packed_cost -= in.cost[c];
            legacy_cost += in.cost[c];
        }
}

// The packed launch's work items; merge_items / merge_parts: the items of the 32-bit launch that add up the packed parts of a
// column of 65 536 users or more, and how many parts each has.  Counts the part slots and split columns in `plan`.
inline std::vector<int4> packed_work_list(const ColumnPlanInput &in, const std::vector<char> &in_call, const std::vector<char> &is_packed,
                                          long long packed_cost, int packed_grid, ColumnPlan &plan, std::vector<int4> &merge_items,
                                          std::vector<int> &merge_parts) {
    int &part_slots = plan.part_slots, &n_split = plan.n_split;
    std::vector<int4> packed_items;
    // its heavy columns are split like the 32-bit kernel's: a part is at most 1/4 of a workgroup's fair share (its workgroups have
    // 8 wavefronts: an unsplit column of 1/2 share kept one of them busy for a third of the launch)
    const long long plimit = std::max<long long>(1, packed_cost / ((long long)packed_grid * 4));
    std::vector<std::pair<long long, int>> pkeyed;
    for (int c : in.cost_order) {
        if (!in_call[c] || !is_packed[(size_t)c]) continue;
        const int n_c = in.walk_ptr_host[c + 1] - in.walk_ptr_host[c];
        const bool many_users = in.csc_ptr_host[c + 1] - in.csc_ptr_host[c] >= 65536;
        long long parts = 1;
        if (in.cost[c] > plimit) parts = std::max<long long>(1, std::min<long long>({(in.cost[c] + plimit - 1) / plimit, (long long)n_c / (4 * 512), 64ll}));
        if (many_users) parts = std::max<long long>(parts, (n_c + PACKED_PART_ENTRIES - 1) / PACKED_PART_ENTRIES);
        for (int q = 0; q < (int)parts; ++q) {
            pkeyed.emplace_back(in.cost[c] / parts, (int)packed_items.size());
            packed_items.push_back(make_int4(c, q, (int)parts | (many_users ? 1 << 16 : 0), parts > 1 || many_users ? part_slots : 0));
        }
        if (many_users) merge_items.push_back(make_int4(c, 0, 1, -(1 + part_slots)));
        if (many_users) merge_parts.push_back((int)parts);
        if (parts > 1 || many_users) {
            part_slots += (int)parts;
            ++n_split;
        }
    }
    if (n_split) sort_items_by_cost(pkeyed, packed_items);
    return packed_items;
}

// The 32-bit launch's own work items: the columns of the call that are not packed, split where they exceed `limit`.
inline std::vector<int4> legacy_work_list(const ColumnPlanInput &in, const std::vector<char> &in_call, const std::vector<char> &is_packed,
                                          long long limit, int min_part_users, ColumnPlan &plan) {
    int &part_slots = plan.part_slots, &n_split = plan.n_split;
    const int n_split_packed = n_split;
    std::vector<int4> items;
    items.reserve((size_t)plan.n_local + 8 * (size_t)plan.max_grid);
    std::vector<std::pair<long long, int>> keyed;   // (item cost, index into items)
    keyed.reserve(items.capacity());
    for (int c : in.cost_order) {
        if (!in_call[c]) continue;
        if (!is_packed.empty() && is_packed[(size_t)c]) continue;
        const int n_c = in.walk_ptr_host[c + 1] - in.walk_ptr_host[c];      // entries of the column's walk list
        long long parts = 1;
        if (in.n_tiles == 1 && in.cost[c] > limit)
            parts = std::max<long long>(1, std::min<long long>({(in.cost[c] + limit - 1) / limit, (long long)n_c / min_part_users, 64ll}));
        if (parts > 1) {
            for (int q = 0; q < (int)parts; ++q) {
                keyed.emplace_back(in.cost[c] / parts, (int)items.size());
                items.push_back(make_int4(c, q, (int)parts, part_slots));
            }
            part_slots += (int)parts;
            ++n_split;
        } else {
            keyed.emplace_back(in.cost[c], (int)items.size());
            // .w of an unsplit column: 1 = LIGHT -- fewer than 16 K pair-adds cannot leave K positive thread maxima behind (real
            // catalogues: half of ML-20M's items have fewer than 20 ratings), so the threshold-first selection would scan the
            // accumulator twice only to hand the column to the full path, which is quick on such columns anyway (all-zero quads
            // are skipped, nothing to select among fewer than K positives)
            items.push_back(make_int4(c, 0, 1, in.cost[c] < 16ll * std::max(1, in.topK) ? 1 : 0));
        }
    }
    if (n_split > n_split_packed) sort_items_by_cost(keyed, items);
    return items;
}

inline ColumnPlan plan_columns(const ColumnPlanInput &in) {
    ColumnPlan plan;
    const ColumnSelection &sel = in.sel;
    const SimKnobs &knobs = in.knobs;
    const std::vector<int> columns = selection_columns(sel, in.cost_order);
    const int n_local = plan.n_local = (int)columns.size();
    std::vector<char> in_call((size_t)in.n_cols, 0);
    for (int c : columns) in_call[(size_t)c] = 1;
    plan.start = sel.start;
    plan.end = sel.end;
    if (sel.n_parts > 0) {
        plan.out_slot.assign((size_t)in.n_cols, -1);
        for (int i = 0; i < n_local; ++i) plan.out_slot[(size_t)columns[(size_t)i]] = i;
        plan.start = 0;
        plan.end = in.n_cols;
    }
    const bool unit_kernel = in.acc_mode != ACC_WIDE;          // 4-byte cells
    plan.acc_words = (in.tile_w + 4) * (unit_kernel ? 1 : 2);
    const size_t lds = plan.lds = (size_t)plan.acc_words * 4 + in.lds_fixed;
    const int cus = in.cus;
    int threads = 1024, max_grid = cus;   // one 16-wave workgroup per CU when the accumulator owns the LDS
    if (lds <= 72 * 1024 && !knobs.one_wg_per_cu) {       // (the variable: measurements of one 16-wave workgroup against several 8-wave ones)
        const int per_cu = std::max(1, std::min(4, (int)((160 * 1024) / (lds + 1024))));
        threads = 512;
        max_grid = cus * per_cu;
    }
    plan.threads = threads;
    plan.max_grid = max_grid;
    plan.fast_topk = fast_topk_for(in, threads);

    // ---- schedule: work items, most expensive first (LPT).  A column whose cost exceeds 1/2 of a workgroup's fair
    //      share is split into parts (contiguous runs of its users) that different workgroups accumulate; otherwise
    //      the head items bound the build as soon as the range is spread over many CUs (at ML-20M shape the top
    //      column is 0.49 of a CU's share on one GPU, 3.9 on eight).  Not combined with accumulator tiling.
    long long cost_sum = 0;
    double nnz_range = 0;
    for (int c : columns) {
        cost_sum += in.cost[c];
        nnz_range += (double)(in.csc_ptr_host[c + 1] - in.csc_ptr_host[c]);
    }
    plan.cost_sum = cost_sum;
    plan.nnz_range = nnz_range;
    int min_part_users = 4 * threads;
    if (knobs.min_part_users) min_part_users = knobs.min_part_users;
    // The packed-counts kernel (sim_packed_kernel: two 512-thread workgroups per CU) takes the columns it can: all-ones data, one
    // tile, the threshold-first selection applicable, fewer than 65 536 users, not light, cheap enough not to be split over its grid.
    // Everything else -- and whatever that kernel hands over -- goes to the 32-bit kernel's launch behind it.
    plan.packed_words = ((in.tile_w / 2 + 2) + 3) & ~3;
    const size_t lds_packed = plan.lds_packed = (size_t)plan.packed_words * 4 + in.lds_packed_fixed;
    // ... and only where a column's fixed phases weigh something next to its accumulation: below PACKED_MAX_PAIRS_PER_COLUMN
    // pair-adds per column of the call (ML-20M shape: 0.29 M, kernel 3.80 -> 3.03-3.10 ms; 138 493 x 9 000 with the same stored
    // values: 0.87 M, 2.44 -> 2.09-2.17 ms; Netflix shape: 3.0 M, accumulation 92 % of the kernel, 16.5 -> 17.0 ms: not packed; the
    // head of an 8-way part, 1.07 M: 0.51 against 0.23 ms: not packed).
    // MI355REC_SIM_PACKED=1 / 0 forces it on (where it applies) / off.
    const bool packed_pays = knobs.packed >= 0 ? knobs.packed != 0 : (double)cost_sum < PACKED_MAX_PAIRS_PER_COLUMN * (double)std::max(1, n_local);
    const bool packed = in.acc_mode == ACC_COUNTS && in.n_tiles == 1 && !in.dense && threads == 1024 && fast_topk_for(in, 512) &&
                        2 * (lds_packed + 1024) <= 160 * 1024 && (in.group_lanes == 4 || in.group_lanes == 8 || in.group_lanes == 16) &&
                        packed_pays && !knobs.no_packed;
    const int packed_grid = 2 * cus;
    std::vector<int4> packed_items, merge_items;       // merge_items: 32-bit launch, columns whose packed parts it adds up
    std::vector<int> merge_parts;
    std::vector<char> is_packed;
    long long legacy_cost = 0, packed_cost = 0;
    if (packed) {
        choose_packed_columns(in, in_call, packed_grid, is_packed, packed_cost, legacy_cost);
        packed_items = packed_work_list(in, in_call, is_packed, packed_cost, packed_grid, plan, merge_items, merge_parts);
    }
    const int n_packed = plan.n_packed = (int)packed_items.size();
    if (!n_packed) is_packed.clear();
    // (the 32-bit launch behind a packed one splits ITS columns -- the heaviest of the call -- over its whole grid)
    const long long limit = std::max<long long>(1, (n_packed ? legacy_cost : cost_sum) / ((long long)max_grid * 2));
    std::vector<int4> &items = plan.items = legacy_work_list(in, in_call, is_packed, limit, min_part_users, plan);
    items.insert(items.end(), merge_items.begin(), merge_items.end());        // (cheap: nothing to accumulate)
    // device layout of the work lists: [the packed kernel's items | the 32-bit kernel's items | room for every packed item handed over]
    plan.n_legacy = (int)items.size();
    items.insert(items.begin(), packed_items.begin(), packed_items.end());
    const int n_items = (int)items.size();
    plan.ranges.resize((size_t)n_items);
    for (int i = 0; i < n_items; ++i) {
        const int c = items[i].x;
        plan.ranges[i] = make_int2(in.walk_ptr_host[c], in.walk_ptr_host[c + 1]);
        if (i >= n_packed && items[i].w < 0) {            // a column added up from packed parts: the empty list [parts, parts)
            const int parts = merge_parts[(size_t)(i - (n_items - (int)merge_items.size()))];
            plan.ranges[i] = make_int2(parts, parts);
        }
    }
    return plan;
}

}  // namespace
}  // namespace mi355rec
