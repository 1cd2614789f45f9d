// extern "C" wrapper around plan_columns (csrc/sim_plan.h) for tests/test_sim_plan.py, which compiles it with g++ and calls it
// through ctypes: no GPU, no HIP runtime.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/sim_plan.h"

#include <cstdint>

using namespace mi355rec;

extern "C" void sim_plan_constants(int64_t *out) {
    out[0] = PACKED_PART_ENTRIES;
    out[1] = (int64_t)PACKED_MAX_PAIRS_PER_COLUMN;
    out[2] = ACC_COUNTS;
    out[3] = ACC_INT32;
    out[4] = ACC_WIDE;
}

// ip: n_cols, tile_w, n_tiles, acc_mode, group_lanes, topK, dense, similarity, shrink, cus, lds_fixed, lds_packed_fixed,
//     start, end, part, n_parts, slot_first, slot_count, then the eight SimKnobs fields in their order; fp: tversky alpha, beta.
// Returns the number of work items (-1: more than `cap`); items_out [cap][4], ranges_out [cap][2], out_slot [n_cols].
extern "C" int sim_plan_shim(const int64_t *cost, const int32_t *cost_order, const int32_t *csc_ptr, const int32_t *walk_ptr, const int32_t *ip,
                             const float *fp, int64_t *scalars, int32_t *items_out, int32_t *ranges_out, int32_t *out_slot, int32_t cap) {
    const int n = ip[0];
    const std::vector<long long> cost_v(cost, cost + n);
    const std::vector<int> order_v(cost_order, cost_order + n), csc_v(csc_ptr, csc_ptr + n + 1), walk_v(walk_ptr, walk_ptr + n + 1);
    ColumnPlanInput in{cost_v, order_v, csc_v, walk_v};
    in.n_cols = n;
    in.tile_w = ip[1];
    in.n_tiles = ip[2];
    in.acc_mode = ip[3];
    in.group_lanes = ip[4];
    in.topK = ip[5];
    in.dense = ip[6] != 0;
    in.similarity = ip[7];
    in.shrink = ip[8];
    in.tversky_alpha = fp[0];
    in.tversky_beta = fp[1];
    in.cus = ip[9];
    in.lds_fixed = (size_t)ip[10];
    in.lds_packed_fixed = (size_t)ip[11];
    in.sel = ip[15] > 0 ? ColumnSelection::part_of(ip[14], ip[15], ip[16], ip[17]) : ColumnSelection::range(ip[12], ip[13]);
    in.knobs.one_wg_per_cu = ip[18] != 0;
    in.knobs.min_part_users = ip[19];
    in.knobs.fast_topk = ip[20] != 0;
    in.knobs.packed = ip[21];
    in.knobs.no_packed = ip[22] != 0;
    in.knobs.packed_heavy = ip[23] != 0;
    in.knobs.packed_demote = ip[24];
    in.knobs.phases = ip[25] != 0;
    const ColumnPlan plan = plan_columns(in);
    const int n_items = (int)plan.items.size();
    if (n_items > cap) return -1;
    const int64_t s[18] = {plan.threads, plan.max_grid, (int64_t)plan.lds, (int64_t)plan.lds_packed, plan.acc_words, plan.packed_words,
                           plan.fast_topk ? 1 : 0, plan.n_packed, plan.n_legacy, n_items, plan.part_slots, plan.n_split, plan.n_local,
                           plan.cost_sum, (int64_t)plan.nnz_range, plan.start, plan.end, plan.out_slot.empty() ? 0 : 1};
    for (int i = 0; i < 18; ++i) scalars[i] = s[i];
    for (int i = 0; i < n_items; ++i) {
        const int4 it = plan.items[(size_t)i];
        const int2 r = plan.ranges[(size_t)i];
        items_out[4 * i] = it.x;
        items_out[4 * i + 1] = it.y;
        items_out[4 * i + 2] = it.z;
        items_out[4 * i + 3] = it.w;
        ranges_out[2 * i] = r.x;
        ranges_out[2 * i + 1] = r.y;
    }
    for (int c = 0; c < n; ++c) out_slot[c] = plan.out_slot.empty() ? -1 : plan.out_slot[(size_t)c];
    return n_items;
}
