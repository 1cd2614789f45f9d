// sim.hip -- Compute_Similarity on MI355X (gfx950).
//
// Replaces Base/Similarity/Cython/Compute_Similarity_Cython.pyx (reference): __init__ :72-213 (pre-processing,
// column norms, CSR+CSC views), computeItemSimilarities :325-406 (the hot loop), compute_similarity :411-607
// (normalisation :473-504, per-column top-K :523-562).
//
// Also serves Compute_Similarity_Euclidean.py (euclidean_cell below), the boolean-transpose products of P3alpha / RP3beta
// (unit_column_side) and the Gram step of EASE_R (dense output).
//
// Design: one persistent workgroup per CU pulls work items (columns, or parts of heavy
// columns) from a cost-ordered queue; the per-column accumulator `this_item_weights` lives in LDS (uint32 counts for
// all-ones data, exact int32 sums for quantised ratings, int64 fixed-point or float64 sums otherwise), the co-occurrence products are accumulated with LDS atomics from a padded
// uint16 profile stream, normalised in place and reduced to the top-K by an in-LDS radix select with early exit
// (bank-replicated histograms) and a counting rank of the survivors.  The URM is read through L2 / Infinity Cache;
// nothing but the K results per column (and the partial accumulators of split columns) is written to HBM.
//
// This file: the handle, the launchers, a build call (plan -> upload -> SimParams -> launch -> stats), the wide top-K path, the
// constructor's stages, the C entry points.  sim_kernels.cuh: the column kernels; sim_setup.cuh: the constructor's kernels;
// sim_plan.h: the schedule of a call, host arithmetic only.
#include "common.h"
#include "topk.cuh"

#include <rocprim/rocprim.hpp>

#include <chrono>

#include <algorithm>
#include <memory>
#include <type_traits>
#include <numeric>

#include "sim_kernels.cuh"
#include "sim_setup.cuh"

using namespace mi355rec;

struct mi355rec_sim : Handle {     // `timer`: start/stop events carried by the column-kernel dispatch itself; `call_timer`: events
                                   // around the whole call (H2D of the schedule, kernel, D2H of the result)
    mi355rec_sim_config cfg{};
    int n_rows = 0, n_cols = 0;
    size_t nnz = 0;
    bool unit_values = false;
    DeviceBuffer<int> csr_ptr, csr_idx, csc_ptr, csc_idx;
    DeviceBuffer<int4> items;
    DeviceBuffer<uint32_t> part_buf;
    DeviceBuffer<unsigned> part_count;
    DeviceBuffer<unsigned long long> phase_ticks;
    DeviceBuffer<unsigned long long> selection_counts;   // [0] columns finished by the threshold-first selection, [1] their candidates, [2] fall-backs after its scan
    DeviceBuffer<int> csr_key, csr_key_sorted, csr_pos, csr_pos_sorted, csr_indptr, csr_indices;   // mi355rec_sim_compute_csr
    DeviceBuffer<float> csr_data;
    DeviceBuffer<char> csr_sort_tmp;
    ColumnPlan plan;                // schedule of the current call (and the host staging of its work lists)
    DeviceBuffer<int2> item_range;
    DeviceBuffer<unsigned short> seg_idx16;
    DeviceBuffer<int> seg_ptr;
    DeviceBuffer<float> seg_val;
    DeviceBuffer<short> seg_val16;
    DeviceBuffer<int> row_tile_ptr, cand_idx;
    DeviceBuffer<float> cand_val;
    int tile_w = 0, n_tiles = 1;
    DeviceBuffer<float> csr_val, csc_val, row_w, norm, norm_alpha, norm_1ma;
    DeviceBuffer<int> out_slot;         // interleaved parts: output row per column
    DeviceBuffer<float> weighted_val;   // feature_weighting: the re-weighted values as handed back to the recommender
    DeviceBuffer<unsigned> queue;
    DeviceBuffer<int> out_idx;
    DeviceBuffer<float> out_val;
    std::vector<long long> cost;   // host copy
    std::vector<int> csc_ptr_host;
    DeviceBuffer<int> walk4;            // walk lists of the column kernel (all-ones data), see SimParams::walk4
    DeviceBuffer<uint2> walk_tab;       //   ... and the bounds of the slices they name
    DeviceBuffer<uint4> walk16;         // walk lists with the column-side weight (valued data)
    std::vector<int> walk_ptr_host;     // [n_cols + 1] a column's entries in the walk arrays
    std::vector<int> cost_order;   // all columns, most expensive first
    int group_lanes = 64;
    double fixed_scale = 0.0;      // real-valued data: power-of-two scale of the int64 fixed-point accumulator (0: float64 sums)
    bool wide_topk = false;
    double wide_kernel_ms = -1.0, wide_call_ms = 0.0;   // >= 0 after a build with topK > MAX_TOPK (several launches: the event pair of the last one is not the build)
    int int_shift = -1;            // >= 0: every stored value times 2^int_shift is a small integer -> exact int32 sums (ACC_INT32)
    int acc_mode() const { return unit_values && !row_w.ptr ? ACC_COUNTS : (int_shift >= 0 ? ACC_INT32 : ACC_WIDE); }
    // last call
    int last_start = -1, last_end = -1;

    ~mi355rec_sim() { shutdown(); }
};

namespace {

template <int THREADS, int G>
void launch_sim(mi355rec_sim *h, const SimParams &p, int grid, size_t lds, hipEvent_t e0, hipEvent_t e1) {
    auto go = [&](auto k) {
        MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipExtLaunchKernelGGL(k, dim3(grid), dim3(THREADS), (unsigned)lds, h->stream, e0, e1, 0, p);
    };
    switch (h->acc_mode()) {
        case ACC_COUNTS: go(sim_column_kernel<THREADS, G, ACC_COUNTS>); break;
        case ACC_INT32: go(sim_column_kernel<THREADS, G, ACC_INT32>); break;
        default: go(sim_column_kernel<THREADS, G, ACC_WIDE>); break;
    }
    MI_HIP(hipGetLastError());
}

template <int THREADS>
void launch_sim_g(mi355rec_sim *h, const SimParams &p, int grid, size_t lds, hipEvent_t e0, hipEvent_t e1) {
    switch (h->group_lanes) {
        case 4: launch_sim<THREADS, 4>(h, p, grid, lds, e0, e1); break;
        case 8: launch_sim<THREADS, 8>(h, p, grid, lds, e0, e1); break;
        case 16: launch_sim<THREADS, 16>(h, p, grid, lds, e0, e1); break;
        case 32: launch_sim<THREADS, 32>(h, p, grid, lds, e0, e1); break;
        default: launch_sim<THREADS, 64>(h, p, grid, lds, e0, e1); break;
    }
}

// the packed-counts kernel (all-ones data, one tile, 512 threads, two workgroups per CU)
void launch_packed(mi355rec_sim *h, const SimParams &p, int grid, size_t lds, hipEvent_t e0, hipEvent_t e1) {
    auto go = [&](auto k) {
        MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipExtLaunchKernelGGL(k, dim3(grid), dim3(512), (unsigned)lds, h->stream, e0, e1, 0, p);
    };
    switch (h->group_lanes) {
        case 4: go(sim_packed_kernel<512, 4>); break;
        case 16: go(sim_packed_kernel<512, 16>); break;
        default: go(sim_packed_kernel<512, 8>); break;
    }
    MI_HIP(hipGetLastError());
}

void clamp_range(const mi355rec_sim *h, int32_t &s, int32_t &e) {
    // same rule as .pyx:447-451: out-of-range bounds fall back to the full range
    int32_t s_in = s, e_in = e;
    s = 0;
    e = h->n_cols;
    if (s_in > 0 && s_in < h->n_cols) s = s_in;
    if (e_in > s && e_in < h->n_cols) e = e_in;
}

// valid after the stream has been synchronised past the last build
void read_timers(mi355rec_sim *h) {
    if (h->wide_kernel_ms >= 0.0) {
        h->stats.kernel_ms = h->wide_kernel_ms;
        h->stats.call_ms = h->wide_call_ms;
    } else {
        h->stats.kernel_ms = h->timer.elapsed_ms();
        h->stats.call_ms = h->call_timer.elapsed_ms();
    }
}

// the environment's switches of a build call, read at every call (tests and scripts set them between calls)
SimKnobs read_sim_knobs() {
    auto on_off = [](const char *name) {        // 1 / 0: set to a non-zero / zero value; -1: not set
        const char *v = getenv(name);
        return v ? (atoi(v) != 0 ? 1 : 0) : -1;
    };
    SimKnobs k;
    k.one_wg_per_cu = getenv("MI355REC_SIM_ONE_WG_PER_CU") != nullptr;
    if (getenv("MI355REC_SIM_MIN_PART_USERS")) k.min_part_users = std::max(64, atoi(getenv("MI355REC_SIM_MIN_PART_USERS")));
    k.fast_topk = on_off("MI355REC_SIM_FAST_TOPK") != 0;
    k.packed = on_off("MI355REC_SIM_PACKED");
    k.no_packed = getenv("MI355REC_SIM_NO_PACKED") != nullptr;
    k.packed_heavy = on_off("MI355REC_SIM_PACKED_HEAVY") != 0;
    k.packed_demote = on_off("MI355REC_SIM_PACKED_DEMOTE");
    k.phases = getenv("MI355REC_SIM_PHASES") != nullptr;
    return k;
}

ColumnPlanInput plan_input(const mi355rec_sim *h, const ColumnSelection &sel, int topK, bool dense, const SimKnobs &knobs) {
    ColumnPlanInput in{h->cost, h->cost_order, h->csc_ptr_host, h->walk_ptr_host};
    in.n_cols = h->n_cols;
    in.tile_w = h->tile_w;
    in.n_tiles = h->n_tiles;
    in.acc_mode = h->acc_mode();
    in.group_lanes = h->group_lanes;
    in.topK = topK;
    in.dense = dense;
    in.similarity = h->cfg.similarity;
    in.shrink = h->cfg.shrink;
    in.tversky_alpha = h->cfg.tversky_alpha;
    in.tversky_beta = h->cfg.tversky_beta;
    in.cus = multiprocessor_count();
    in.lds_fixed = (size_t)AUX_WORDS * 4 + sizeof(SimShared);
    in.lds_packed_fixed = (size_t)PACKED_AUX_WORDS * 4 + sizeof(SimShared);
    in.sel = sel;
    in.knobs = knobs;
    return in;
}

// the work lists of h->plan, the queue counters and the partial accumulators of its split columns
void upload_plan(mi355rec_sim *h) {
    const ColumnPlan &plan = h->plan;
    const int n_items = (int)plan.items.size(), n_packed = plan.n_packed, part_slots = plan.part_slots;
    if (h->items.count < (size_t)n_items + (size_t)n_packed) {
        h->items.alloc((size_t)n_items + (size_t)n_packed + 1024);
        h->item_range.alloc((size_t)n_items + (size_t)n_packed + 1024);
    }
    MI_HIP(hipMemcpyAsync(h->items.ptr, plan.items.data(), sizeof(int4) * n_items, hipMemcpyHostToDevice, h->stream));
    MI_HIP(hipMemcpyAsync(h->item_range.ptr, plan.ranges.data(), sizeof(int2) * n_items, hipMemcpyHostToDevice, h->stream));
    MI_HIP(hipMemsetAsync(h->queue.ptr, 0, 4 * sizeof(unsigned), h->stream));           // [0] the 32-bit launch's queue, [1] the packed launch's, [2] items of the 32-bit launch
    if (n_packed) MI_HIP(hipMemcpyAsync(h->queue.ptr + 2, &plan.n_legacy, sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (part_slots) {
        const size_t pub_words = (size_t)h->tile_w * (h->acc_mode() != ACC_WIDE ? 1 : 2);
        if (h->part_buf.count < (size_t)part_slots * pub_words) h->part_buf.alloc((size_t)part_slots * pub_words);
        if (h->part_count.count < (size_t)part_slots) h->part_count.alloc((size_t)part_slots);
        MI_HIP(hipMemsetAsync(h->part_count.ptr, 0, sizeof(unsigned) * part_slots, h->stream));
    }
}

// the 32-bit launch's parameters for h->plan (the packed launch's are derived from them); zeroes the diagnostics they point to and
// uploads a part's output rows
SimParams fill_params(mi355rec_sim *h, int topK, int *d_idx, float *d_val, float *d_dense, const SimKnobs &knobs) {
    const ColumnPlan &plan = h->plan;
    SimParams p{};
    p.n_rows = h->n_rows;
    p.n_cols = h->n_cols;
    p.n_cols_pad = h->tile_w;          // neighbour cells of the LDS accumulator
    p.acc_cells = h->tile_w + 4;
    p.acc_words = plan.acc_words;
    p.tile_w = h->tile_w;
    p.n_tiles = h->n_tiles;
    p.topK = topK;
    p.kind = h->cfg.similarity;
    p.normalize = h->cfg.normalize;
    p.unit_col = h->cfg.unit_column_side;
    p.avg_row = h->cfg.normalize_avg_row;
    p.euclid_mode = h->cfg.euclidean_mode;
    p.shrink = (float)h->cfg.shrink;
    p.tversky_alpha = h->cfg.tversky_alpha;
    p.tversky_beta = h->cfg.tversky_beta;
    p.csr_ptr = h->csr_ptr.ptr;
    p.seg_ptr = h->seg_ptr.ptr;
    p.seg_idx16 = h->seg_idx16.ptr;
    p.seg_val = h->seg_val.ptr;
    p.seg_val16 = h->seg_val16.ptr;
    p.csc_ptr = h->csc_ptr.ptr;
    p.csc_idx = h->csc_idx.ptr;
    p.csc_val = h->csc_val.ptr;
    p.walk4 = h->walk4.ptr;
    p.walk_tab = h->walk_tab.ptr;
    p.walk16 = h->walk16.ptr;
    p.row_w = h->row_w.ptr;
    p.norm = h->norm.ptr;
    p.norm_alpha = h->norm_alpha.ptr;
    p.norm_1ma = h->norm_1ma.ptr;
    p.items = h->items.ptr + plan.n_packed;
    p.item_range = h->item_range.ptr + plan.n_packed;
    p.n_items = plan.n_legacy;
    p.part_buf = h->part_buf.ptr;
    p.part_count = h->part_count.ptr;
    if (knobs.phases) {
        if (!h->phase_ticks.ptr) h->phase_ticks.alloc(16);
        MI_HIP(hipMemsetAsync(h->phase_ticks.ptr, 0, 16 * sizeof(unsigned long long), h->stream));
        MI_HIP(hipMemsetAsync(h->phase_ticks.ptr + 8, 0xFF, sizeof(unsigned long long), h->stream));      // [8]: a minimum
        p.phase_ticks = h->phase_ticks.ptr;
    }
    if (!h->selection_counts.ptr) h->selection_counts.alloc(4);
    MI_HIP(hipMemsetAsync(h->selection_counts.ptr, 0, 4 * sizeof(unsigned long long), h->stream));
    p.fast_stats = h->selection_counts.ptr;
    p.fast_topk = plan.fast_topk;
    p.fixed_scale = h->acc_mode() != ACC_WIDE ? 0.0 : h->fixed_scale;
    p.int_scale = h->int_shift >= 0 ? (float)(1 << (2 * h->int_shift)) : 1.f;
    p.int_half = h->int_shift >= 0 ? (float)(1 << h->int_shift) : 1.f;
    p.int_inv = 1.f / p.int_scale;
    p.fixed_inv = p.fixed_scale > 0.0 ? 1.0 / p.fixed_scale : 0.0;
    p.start_col = plan.start;
    p.out_slot = nullptr;
    if (!plan.out_slot.empty()) {
        if (h->out_slot.count < (size_t)h->n_cols) h->out_slot.alloc((size_t)h->n_cols);
        MI_HIP(hipMemcpyAsync(h->out_slot.ptr, plan.out_slot.data(), sizeof(int) * (size_t)h->n_cols, hipMemcpyHostToDevice, h->stream));
        MI_HIP(hipStreamSynchronize(h->stream));
        p.out_slot = h->out_slot.ptr;
    }
    p.queue = h->queue.ptr;
    p.out_idx = d_idx;
    p.out_val = d_val;
    p.out_dense = d_dense;
    return p;
}

// the packed-counts launch, where the plan has one, and the 32-bit launch (behind it)
void launch_columns(mi355rec_sim *h, SimParams p) {
    const ColumnPlan &plan = h->plan;
    const int n_packed = plan.n_packed;
    const int grid = n_packed ? plan.max_grid : std::min(plan.n_legacy, plan.max_grid);      // (behind a packed launch the list may grow)
    if (h->n_tiles > 1 && p.topK > 0) {
        const size_t need = (size_t)grid * h->n_tiles * p.topK;
        if (h->cand_idx.count < need) {
            h->cand_idx.alloc(need);
            h->cand_val.alloc(need);
        }
    }
    p.cand_idx = h->cand_idx.ptr;
    p.cand_val = h->cand_val.ptr;
    h->call_timer.start(h->stream);
    if (n_packed) {
        SimParams q = p;
        q.items = h->items.ptr;
        q.item_range = h->item_range.ptr;
        q.n_items = n_packed;
        q.acc_words = plan.packed_words;
        q.queue = h->queue.ptr + 1;
        q.retry_count = reinterpret_cast<int *>(h->queue.ptr + 2);
        q.retry_items = h->items.ptr + n_packed;
        q.retry_ranges = h->item_range.ptr + n_packed;
        launch_packed(h, q, std::min(n_packed, 2 * multiprocessor_count()), plan.lds_packed, h->timer.t0, nullptr);
        p.n_items_dev = reinterpret_cast<const int *>(h->queue.ptr + 2);
        launch_sim_g<1024>(h, p, grid, plan.lds, nullptr, h->timer.t1);
    } else if (plan.threads == 1024) {
        launch_sim_g<1024>(h, p, grid, plan.lds, h->timer.t0, h->timer.t1);
    } else {
        launch_sim_g<512>(h, p, grid, plan.lds, h->timer.t0, h->timer.t1);
    }
    h->call_timer.stop(h->stream);
}

void write_stats(mi355rec_sim *h, int topK) {
    const ColumnPlan &plan = h->plan;
    h->stats.n_launches = plan.n_packed ? 2 : 1;
    h->stats.n_timed = 1;
    h->stats.n_units = plan.n_local;
    // ALGORITHMIC bytes, SURVEY.md section 8(d): per column c, its CSC column (8 B x n_c) + the CSR row of each of its users
    // (8 B x L_u) + topK x 8 B of output, i.e. 8 * (nnz_range + cost_range) + 8 * n_local * topK.  (The kernel's own
    // layout moves less -- uint16 ids, no values for all-ones data -- see DESIGN.md section 4.)
    h->stats.algorithmic_bytes = 8.0 * (plan.nnz_range + (double)plan.cost_sum) + 8.0 * (double)plan.n_local * (double)topK;
    h->stats.algorithmic_flops = 0;
    h->last_start = plan.start;
    h->last_end = plan.end;
}

// Runs the column kernel for the selection's columns with the call's topK (0: dense columns), leaving results in d_idx/d_val (or
// d_dense when topK == 0).
void run_columns_lds(mi355rec_sim *h, const ColumnSelection &sel, int topK, int *d_idx, float *d_val, float *d_dense) {
    const SimKnobs knobs = read_sim_knobs();
    h->plan = plan_columns(plan_input(h, sel, topK, d_dense != nullptr, knobs));
    upload_plan(h);
    const SimParams p = fill_params(h, topK, d_idx, d_val, d_dense, knobs);
    launch_columns(h, p);
    write_stats(h, topK);
}

// topK beyond the in-LDS selection (MAX_TOPK = 4096 candidates): the reference only clamps topK to n_cols (.pyx:146).  The columns
// are built DENSE into HBM (the kernel's topK == 0 path), every column is sorted by descending value with one segmented radix sort
// (rocPRIM; stable: equal values keep ascending neighbour ids, the in-LDS path's tie rule) and the K largest cells of the full
// column -- zeros compete, then are dropped (.pyx:523-555) -- are emitted.  Blocks of columns bound the scratch memory.
__global__ __launch_bounds__(256) void wide_topk_emit_kernel(const float *sorted_val, const int *sorted_id, int n_cols, int topK, int *out_idx,
                                                             float *out_val) {
    __shared__ int s_npos, s_nnonneg;
    const float *val = sorted_val + (size_t)blockIdx.x * n_cols;
    const int *id = sorted_id + (size_t)blockIdx.x * n_cols;
    if (threadIdx.x < 2) {           // first position whose value is <= 0 (thread 0) / < 0 (thread 1): descending order
        int lo = 0, hi = n_cols;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const bool before = threadIdx.x == 0 ? val[mid] > 0.f : val[mid] >= 0.f;
            if (before) lo = mid + 1; else hi = mid;
        }
        if (threadIdx.x == 0) s_npos = lo; else s_nnonneg = lo;
    }
    __syncthreads();
    const int npos = s_npos, nzero = s_nnonneg - s_npos;
    const int take_pos = min(topK, npos), take_neg = max(0, min(topK - npos - nzero, n_cols - npos - nzero));
    int *oi = out_idx + (size_t)blockIdx.x * topK;
    float *ov = out_val + (size_t)blockIdx.x * topK;
    for (int r = threadIdx.x; r < topK; r += 256) {
        int src = -1;
        if (r < take_pos) src = r;
        else if (r < take_pos + take_neg) src = npos + nzero + (r - take_pos);
        oi[r] = src >= 0 ? id[src] : -1;
        ov[r] = src >= 0 ? val[src] : 0.f;
    }
}

__global__ void wide_iota_kernel(int *ids, unsigned *offsets, int n_rows, int n_cols) {
    const size_t n = (size_t)n_rows * n_cols;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) ids[e] = (int)(e % n_cols);
    for (size_t r = blockIdx.x * (size_t)blockDim.x + threadIdx.x; r <= (size_t)n_rows; r += (size_t)gridDim.x * blockDim.x)
        offsets[r] = (unsigned)(r * n_cols);
}

void run_columns_wide_topk(mi355rec_sim *h, const ColumnSelection &sel, int *d_idx, float *d_val) {
    const int topK = h->cfg.topK, n_cols = h->n_cols;
    // rows of the output, in output order: a contiguous range, or (a piece of) one interleaved part (whose rows the kernel places by out_slot)
    const int n_local = (int)selection_columns(sel, h->cost_order).size();
    if (n_local == 0) return;
    // 4 GiB per float buffer (MI355REC_SIM_WIDE_CELLS: a smaller bound, for tests of the block walk)
    const size_t cells_cap = getenv("MI355REC_SIM_WIDE_CELLS") ? (size_t)std::max(1ll, atoll(getenv("MI355REC_SIM_WIDE_CELLS"))) : (size_t)1 << 30;
    int block = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_local, cells_cap / (size_t)n_cols));
    DeviceBuffer<float> dense, sorted_val;
    DeviceBuffer<int> ids, sorted_id;
    DeviceBuffer<unsigned> offsets;
    DeviceBuffer<unsigned char> tmp;
    dense.alloc((size_t)block * n_cols); sorted_val.alloc((size_t)block * n_cols);
    ids.alloc((size_t)block * n_cols); sorted_id.alloc((size_t)block * n_cols);
    offsets.alloc((size_t)block + 1);
    hipStream_t s = h->stream;
    hipLaunchKernelGGL(wide_iota_kernel, dim3(4096), dim3(256), 0, s, ids.ptr, offsets.ptr, block, n_cols);
    size_t tmp_bytes = 0;
    MI_HIP(rocprim::segmented_radix_sort_pairs_desc(nullptr, tmp_bytes, dense.ptr, sorted_val.ptr, ids.ptr, sorted_id.ptr,
                                                    (unsigned)((size_t)block * n_cols), (unsigned)block, offsets.ptr, offsets.ptr + 1, 0, 32, s));
    tmp.alloc(tmp_bytes + 256);
    double kernel_ms = 0, units = 0, bytes = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    MI_HIP(hipEventCreate(&t0));
    MI_HIP(hipEventCreate(&t1));
    MI_HIP(hipEventRecord(t0, s));
    try {
        for (int done = 0; done < n_local; done += block) {
            const int here = std::min(block, n_local - done);
            // dense columns: the call's topK is 0, whatever the handle's
            const ColumnSelection rows = sel.n_parts > 0 ? ColumnSelection::part_of(sel.part, sel.n_parts, sel.slot_first + done, here)
                                                         : ColumnSelection::range(sel.start + done, sel.start + done + here);
            run_columns_lds(h, rows, 0, nullptr, nullptr, dense.ptr);
            MI_HIP(hipStreamSynchronize(s));
            kernel_ms += h->timer.elapsed_ms();
            units += h->stats.n_units;
            bytes += h->stats.algorithmic_bytes;
            size_t bytes_now = tmp_bytes;
            MI_HIP(rocprim::segmented_radix_sort_pairs_desc(tmp.ptr, bytes_now, dense.ptr, sorted_val.ptr, ids.ptr, sorted_id.ptr,
                                                            (unsigned)((size_t)here * n_cols), (unsigned)here, offsets.ptr, offsets.ptr + 1, 0, 32, s));
            hipLaunchKernelGGL(wide_topk_emit_kernel, dim3(here), dim3(256), 0, s, sorted_val.ptr, sorted_id.ptr, n_cols, topK,
                               d_idx + (size_t)done * topK, d_val + (size_t)done * topK);
            MI_HIP(hipGetLastError());
        }
    } catch (...) {
        (void)hipEventDestroy(t0);
        (void)hipEventDestroy(t1);
        throw;
    }
    // the handle's timers are read by the callers after this returns: make them cover the whole wide build
    MI_HIP(hipEventRecord(t1, s));
    MI_HIP(hipStreamSynchronize(s));
    float whole_ms = 0.f;
    MI_HIP(hipEventElapsedTime(&whole_ms, t0, t1));
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    h->wide_kernel_ms = kernel_ms;
    h->wide_call_ms = whole_ms;
    h->stats.n_units = (int64_t)units;
    h->stats.algorithmic_bytes = bytes + 8.0 * (double)n_local * topK;
}

// d_dense: dense columns (the call's topK is 0); otherwise the handle's topK, by the route it needs
void run_columns(mi355rec_sim *h, const ColumnSelection &sel, int *d_idx, float *d_val, float *d_dense) {
    h->wide_kernel_ms = -1.0;
    if (!d_dense && h->wide_topk && h->cfg.topK > 0) run_columns_wide_topk(h, sel, d_idx, d_val);
    else run_columns_lds(h, sel, d_dense ? 0 : h->cfg.topK, d_idx, d_val, d_dense);
}

}  // namespace

namespace {

// What the constructor's stages hand to one another.  The device buffers are scratch that more than one stage touches, or whose
// block a stage must not hand back while the stream still works on it: all of it is released when the constructor returns.
struct SimCreate {
    mi355rec_sim *h;
    const mi355rec_sim_config *cfg;
    int n_rows, n_cols;
    size_t nnz;
    hipStream_t s;
    const float *row_weights;
    bool set_based, euclid;
    int eb = 256, eg = 0;               // launch shape of the element-wise kernels over the stored values
    unsigned info0[3] = {0xFu, 0u, 1u}; // value_scan_kernel's words for the values as they came in
    bool stream_order = true;
    bool walk_only = false;             // all-ones data: the walk list is the column view (one sort of 4-byte entries instead of the CSC's sort + the list's)
    int n_walk_entries = 0;
    DeviceBuffer<float> row_mean;
    // the walk lists' sorted column keys and the scan of the rows' lengths by first slice: what the columns' costs and user counts
    // of all-ones data are summed from (build_walk)
    DeviceBuffer<int> walk_keys, walk_len_ptr;
    DeviceBuffer<float> mean;
    DeviceBuffer<double> sumsq;
    DeviceBuffer<long long> cost;
    DeviceBuffer<int> key_out, row_of;                  // CSR -> CSC: the sorted column keys, the row of every cell
    DeviceBuffer<unsigned long long> cell_in, cell_out;
    DeviceBuffer<char> sort_tmp;
    DeviceBuffer<int> user_count;
    DeviceBuffer<unsigned long long> packed;
    DeviceBuffer<long long> cost_sorted;
    DeviceBuffer<int> col_ids, col_order;
    DeviceBuffer<char> order_tmp;
    // MI355REC_SIM_CREATE_PHASES=1: wall clock of the constructor's phases on stderr (each one drained before the next starts)
    bool phases = false;
    std::chrono::steady_clock::time_point t_phase;
    void phase(const char *what) {
        if (!phases) return;
        (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[sim create] %-34s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_phase).count());
        t_phase = now;
    }
};

// `resident`: the three CSR arrays are device memory -- copied at HBM speed instead of over PCIe
// (the handle keeps its own copy either way: the values are re-weighted / centred in place and the arrays are padded)
void create_upload(SimCreate &c, const int32_t *csr_indptr, const int32_t *csr_indices, const float *csr_data, bool resident) {
    mi355rec_sim *h = c.h;
    hipStream_t s = c.s;
    const size_t nnz = c.nnz;
    const hipMemcpyKind in_kind = resident ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    h->csr_ptr.alloc((size_t)c.n_rows + 1);
    MI_HIP(hipMemcpyAsync(h->csr_ptr.ptr, csr_indptr, ((size_t)c.n_rows + 1) * sizeof(int), in_kind, s));
    // padding: the column kernel reads the profiles in aligned 16-byte chunks, a whole lane group at a time
    h->csr_idx.alloc(nnz + 520);                 // (only the padding needs the zeros)
    h->csr_val.alloc(nnz + 520);
    MI_HIP(hipMemsetAsync(h->csr_idx.ptr + nnz, 0, 520 * sizeof(int), s));
    MI_HIP(hipMemsetAsync(h->csr_val.ptr + nnz, 0, 520 * sizeof(float), s));
    MI_HIP(hipMemcpyAsync(h->csr_idx.ptr, csr_indices, nnz * sizeof(int), in_kind, s));
    MI_HIP(hipMemcpyAsync(h->csr_val.ptr, csr_data, nnz * sizeof(float), in_kind, s));
    if (c.row_weights) h->row_w.upload(c.row_weights, c.n_rows, s);
    c.phase(resident ? "allocate + copy of the resident URM" : "allocate + upload (PCIe)");
}

// optional pre-pass: BM25 / TF-IDF on the stored values (what the KNN recommenders do to the matrix before the build)
void create_feature_weighting(SimCreate &c) {
    mi355rec_sim *h = c.h;
    const mi355rec_sim_config *cfg = c.cfg;
    hipStream_t s = c.s;
    const int n_rows = c.n_rows, n_cols = c.n_cols;
    MI_REQUIRE(cfg->feature_weighting == MI355REC_WEIGHT_BM25 || cfg->feature_weighting == MI355REC_WEIGHT_TFIDF,
               "Value for 'feature_weighting' not recognized (%d)", cfg->feature_weighting);
    if (cfg->feature_weighting == MI355REC_WEIGHT_BM25) {
        MI_REQUIRE(cfg->bm25_b > 0.f && cfg->bm25_b < 1.f, "okapi_BM_25: B must be in (0,1)");
        MI_REQUIRE(cfg->bm25_k1 > 0.f, "okapi_BM_25: K1 must be > 0");
    }
    DeviceBuffer<double> row_sum, col_sum, total;
    DeviceBuffer<int> col_cnt;
    row_sum.alloc((size_t)n_rows);
    col_sum.alloc_zero((size_t)n_cols, s);
    col_cnt.alloc_zero((size_t)n_cols, s);
    total.alloc_zero(64, s);
    const int wg = div_up((int64_t)n_rows * 64, 256);
    hipLaunchKernelGGL(weighting_stats_kernel, dim3(wg), dim3(256), 0, s, h->csr_ptr.ptr, h->csr_idx.ptr, h->csr_val.ptr, n_rows,
                       row_sum.ptr, col_sum.ptr, col_cnt.ptr, total.ptr);
    hipLaunchKernelGGL(weighting_apply_kernel, dim3(wg), dim3(256), 0, s, h->csr_ptr.ptr, h->csr_idx.ptr, h->csr_val.ptr, n_rows, n_cols,
                       row_sum.ptr, col_sum.ptr, col_cnt.ptr, total.ptr, cfg->feature_weighting, cfg->weighting_documents,
                       (double)cfg->bm25_k1, (double)cfg->bm25_b);
    MI_HIP(hipGetLastError());
    h->weighted_val.alloc(c.nnz);
    MI_HIP(hipMemcpyAsync(h->weighted_val.ptr, h->csr_val.ptr, c.nnz * sizeof(float), hipMemcpyDeviceToDevice, s));
    MI_HIP(hipStreamSynchronize(s));            // (the statistics buffers go out of scope here)
}

// the finiteness check, the weighting, and what the values are: all ones? on a 2^s grid?
void create_value_checks(SimCreate &c) {
    mi355rec_sim *h = c.h;
    const mi355rec_sim_config *cfg = c.cfg;
    hipStream_t s = c.s;
    const size_t nnz = c.nnz;
    const int eb = c.eb, eg = c.eg;
    // One pass over the values as they came in: the reference's dispatcher asserts that they are finite (Compute_Similarity.py:34-36,
    // np.isfinite over the whole array: 9 of the 18 ms of an ItemKNN fit at ML-20M shape when the front-end did it on the host) -- the
    // largest |value|'s bits say so here -- and, where nothing re-writes the values before the build, the same pass answers "all
    // ones?" and "which 2^s grid?" below.
    unsigned *info0 = c.info0;
    {
        DeviceBuffer<unsigned> scan;
        scan.alloc_zero(3, s);
        hipLaunchKernelGGL(value_scan_kernel, dim3(eg), dim3(eb), 0, s, h->csr_val.ptr, nnz, scan.ptr);
        MI_HIP(hipGetLastError());
        scan.download(info0, 3, s);
        MI_HIP(hipStreamSynchronize(s));
        if (info0[1] >= 0x7F800000u) fail(MI355REC_E_INVALID, "Compute_Similarity: Data matrix contains non finite values");
    }

    if (cfg->feature_weighting != MI355REC_WEIGHT_NONE) create_feature_weighting(c);
    // pre-processing of the stored values (.pyx:158-164)
    if (c.set_based) hipLaunchKernelGGL(fill_kernel, dim3(eg), dim3(eb), 0, s, h->csr_val.ptr, nnz, 1.0f);
    // All-ones data (implicit URMs, every set-based similarity) takes the integer-count kernel, which never reads
    // the value arrays; mean-centred data never qualifies.
    h->unit_values = c.set_based;
    // Quantised values (star ratings, half stars, counts): if every stored value times 2^s (s <= 3) is an integer of at most
    // 2048 and n_rows products of that size cannot overflow an int32, the column sums are exact integers (ACC_INT32).  Not for
    // mean-centred data (adjusted / pearson centre the values later) nor with row weights.  One pass answers both questions.
    if (!c.set_based && cfg->similarity != MI355REC_SIM_ADJUSTED && cfg->similarity != MI355REC_SIM_PEARSON) {
        // [0] bit s set: some value times 2^s is not an integer; [1] bits of max |value|; [2] not all ones
        unsigned info[3] = {info0[0], info0[1], info0[2]};
        if (cfg->feature_weighting != MI355REC_WEIGHT_NONE) {          // (the weighting has re-written the values: look again)
            DeviceBuffer<unsigned> scan;
            scan.alloc_zero(3, s);
            hipLaunchKernelGGL(value_scan_kernel, dim3(eg), dim3(eb), 0, s, h->csr_val.ptr, nnz, scan.ptr);
            MI_HIP(hipGetLastError());
            info[0] = 0xFu; info[1] = 0u; info[2] = 1u;
            scan.download(info, 3, s);
            MI_HIP(hipStreamSynchronize(s));
        }
        h->unit_values = (info[2] == 0);
        if (!h->unit_values && !c.row_weights && !getenv("MI355REC_SIM_F64_SUMS") && !getenv("MI355REC_SIM_NO_INT32")) {
            float vmax_f;
            memcpy(&vmax_f, &info[1], sizeof(float));
            for (int sh = 0; sh <= 3; ++sh) {
                const double m = (double)vmax_f * (double)(1 << sh);
                if (!((info[0] >> sh) & 1u) && m <= 2048.0 && (double)c.n_rows * m * m < 2147483648.0) {
                    h->int_shift = sh;
                    break;
                }
            }
        }
    }
    c.phase("value checks (weighting, units, grid)");
}

// the accumulator's tiles (they follow from the cell size the value checks have settled) and the row centring of adjusted cosine
void create_tiles_and_row_centring(SimCreate &c) {
    mi355rec_sim *h = c.h;
    const int n_rows = c.n_rows, n_cols = c.n_cols;
    // accumulator tiling: the LDS holds MAX_TILE 4-byte cells (counts, exact integer sums) or MAX_TILE_F64 8-byte cells (other
    // real-valued data, row weights) next to the 32 KiB selection scratch
    const int max_tile = h->acc_mode() != ACC_WIDE ? MAX_TILE : MAX_TILE_F64;
    h->tile_w = n_cols <= max_tile ? ((n_cols + 3) & ~3) : max_tile;
    h->n_tiles = (n_cols + h->tile_w - 1) / h->tile_w;
    // topK beyond the in-LDS selection, or per-tile candidates (n_tiles x topK) beyond the merge buffer: dense columns + segmented sort
    h->wide_topk = h->cfg.topK > MAX_TOPK || (long long)h->n_tiles * h->cfg.topK > h->tile_w;
    if (c.cfg->similarity == MI355REC_SIM_ADJUSTED) {
        c.row_mean.alloc((size_t)n_rows);
        hipLaunchKernelGGL(segment_mean_kernel, dim3(div_up(n_rows, 256)), dim3(256), 0, c.s, h->csr_ptr.ptr, h->csr_val.ptr,
                           n_rows, c.row_mean.ptr);
        hipLaunchKernelGGL(row_center_kernel, dim3(div_up((int64_t)n_rows * 64, 256)), dim3(256), 0, c.s, h->csr_ptr.ptr,
                           h->csr_val.ptr, n_rows, c.row_mean.ptr);
    }
}

// the profile stream: (row, tile) segments padded to whole 16-byte chunks, from the pre-processed values.  Its offsets
// (build_seg_ptr) depend on the row lengths alone; its contents (fill_stream) on the pre-processed values and on group_lanes
void build_seg_ptr(SimCreate &c) {
    mi355rec_sim *h = c.h;
    hipStream_t s = c.s;
    const long long n_seg = (long long)c.n_rows * h->n_tiles;
    DeviceBuffer<int> len_pad;
    DeviceBuffer<char> scan_tmp;
    len_pad.alloc((size_t)n_seg + 1);
    h->seg_ptr.alloc((size_t)n_seg + 1);
    hipLaunchKernelGGL(seg_len_kernel, dim3(div_up(n_seg + 1, 256)), dim3(256), 0, s, h->csr_ptr.ptr, h->row_tile_ptr.ptr,
                       c.n_rows, h->n_tiles, len_pad.ptr);
    size_t scan_bytes = 0;
    MI_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, len_pad.ptr, h->seg_ptr.ptr, 0, (size_t)(n_seg + 1), rocprim::plus<int>(), s));
    scan_tmp.alloc(scan_bytes);
    MI_HIP(rocprim::exclusive_scan(scan_tmp.ptr, scan_bytes, len_pad.ptr, h->seg_ptr.ptr, 0, (size_t)(n_seg + 1), rocprim::plus<int>(), s));
}

void fill_stream(SimCreate &c) {
    mi355rec_sim *h = c.h;
    hipStream_t s = c.s;
    const long long n_seg = (long long)c.n_rows * h->n_tiles;
    const size_t seg_cap = c.nnz + 7 * (size_t)n_seg + 520;     // every segment grows by at most 7 entries
    MI_REQUIRE(seg_cap < (size_t)INT32_MAX, "matrix too large for 32-bit segment offsets");
    h->seg_idx16.alloc_zero(seg_cap, s);
    const bool int16_values = h->acc_mode() == ACC_INT32;      // (ids + int16 values: 4 B per entry instead of 6)
    if (int16_values) h->seg_val16.alloc_zero(seg_cap, s);
    else if (h->acc_mode() != ACC_COUNTS) h->seg_val.alloc_zero(seg_cap, s);     // (the counts kernel reads ids only)
    hipLaunchKernelGGL(seg_fill_kernel, dim3(div_up(n_seg * 64, 256)), dim3(256), 0, s, h->csr_ptr.ptr, h->row_tile_ptr.ptr,
                       h->csr_idx.ptr, h->csr_val.ptr, h->seg_ptr.ptr, c.n_rows, h->n_tiles, h->tile_w, h->seg_idx16.ptr,
                       h->seg_val.ptr, c.stream_order ? h->group_lanes : 0, h->seg_val16.ptr, (float)(1 << std::max(0, h->int_shift)));
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(s));      // the temporaries above go out of scope
}

// the walk lists (what the column kernel's accumulation walks instead of the CSC arrays): slices of the profile segments,
// every column's longest first.  All-ones data: 4-byte entries (slice numbers) -- the sorted list is the column view itself,
// `walk_keys` (its sorted column keys) and `walk_len_ptr` (scan of the rows' lengths by first slice) are what the columns'
// costs and user counts are then summed from, and no CSC is ever built (walk_only).
void build_walk(SimCreate &c) {
    mi355rec_sim *h = c.h;
    const mi355rec_sim_config *cfg = c.cfg;
    hipStream_t s = c.s;
    const int n_rows = c.n_rows, n_cols = c.n_cols;
    const size_t nnz = c.nnz;
    DeviceBuffer<int> &walk_len_ptr = c.walk_len_ptr;
    const int tiled = h->n_tiles > 1;
    const bool wide = h->acc_mode() != ACC_COUNTS;
    DeviceBuffer<int> n_slices, slice_off, rec_len, first_len, out_off, key_in, key_sorted, walk_ptr;
    DeviceBuffer<unsigned> rec_key, rec_key_sorted;
    DeviceBuffer<unsigned long long> rec, rec_sorted;
    DeviceBuffer<char> tmp;
    n_slices.alloc((size_t)n_rows + 1);
    slice_off.alloc((size_t)n_rows + 1);
    MI_HIP(hipMemsetAsync(n_slices.ptr + n_rows, 0, sizeof(int), s));
    hipLaunchKernelGGL(walk_row_slices_kernel, dim3(div_up(n_rows, 256)), dim3(256), 0, s, h->csr_ptr.ptr, h->seg_ptr.ptr, n_rows, tiled, n_slices.ptr);
    size_t bytes = 0;
    MI_HIP(rocprim::exclusive_scan(nullptr, bytes, n_slices.ptr, slice_off.ptr, 0, (size_t)n_rows + 1, rocprim::plus<int>(), s));
    tmp.alloc(bytes + 16);
    MI_HIP(rocprim::exclusive_scan(tmp.ptr, bytes, n_slices.ptr, slice_off.ptr, 0, (size_t)n_rows + 1, rocprim::plus<int>(), s));
    int n_rec = 0;
    MI_HIP(hipMemcpyAsync(&n_rec, slice_off.ptr + n_rows, sizeof(int), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    MI_REQUIRE(n_rec > 0, "matrix has no stored values");
    rec_key.alloc((size_t)n_rec); rec_key_sorted.alloc((size_t)n_rec);
    rec.alloc((size_t)n_rec); rec_sorted.alloc((size_t)n_rec);
    hipLaunchKernelGGL(walk_slice_records_kernel, dim3(div_up(n_rows, 256)), dim3(256), 0, s, h->csr_ptr.ptr, h->seg_ptr.ptr, slice_off.ptr, n_rows,
                       tiled, h->n_tiles, rec_key.ptr, rec.ptr);
    bytes = 0;
    MI_HIP(rocprim::radix_sort_pairs_desc(nullptr, bytes, rec_key.ptr, rec_key_sorted.ptr, rec.ptr, rec_sorted.ptr, (size_t)n_rec, 0, 8, s));
    DeviceBuffer<char> tmp2;
    tmp2.alloc(bytes + 16);
    MI_HIP(rocprim::radix_sort_pairs_desc(tmp2.ptr, bytes, rec_key.ptr, rec_key_sorted.ptr, rec.ptr, rec_sorted.ptr, (size_t)n_rec, 0, 8, s));
    rec_len.alloc((size_t)n_rec + 1);
    first_len.alloc((size_t)n_rec + 1);
    out_off.alloc((size_t)n_rec + 1);
    if (!wide && !tiled) h->walk_tab.alloc((size_t)n_rec);
    hipLaunchKernelGGL(walk_record_lengths_kernel, dim3(div_up(n_rec + 1, 256)), dim3(256), 0, s, rec_sorted.ptr, h->csr_ptr.ptr, h->seg_ptr.ptr,
                       n_rec, (int)(wide || tiled), rec_len.ptr, first_len.ptr, h->walk_tab.ptr);
    bytes = 0;
    MI_HIP(rocprim::exclusive_scan(nullptr, bytes, rec_len.ptr, out_off.ptr, 0, (size_t)n_rec + 1, rocprim::plus<int>(), s));
    DeviceBuffer<char> tmp3;
    tmp3.alloc(bytes + 16);
    MI_HIP(rocprim::exclusive_scan(tmp3.ptr, bytes, rec_len.ptr, out_off.ptr, 0, (size_t)n_rec + 1, rocprim::plus<int>(), s));
    if (!wide && !tiled) {         // (tiled: the entries are rows, whose lengths the CSR pointers give)
        walk_len_ptr.alloc((size_t)n_rec + 1);
        bytes = tmp3.count;
        MI_HIP(rocprim::exclusive_scan(tmp3.ptr, bytes, first_len.ptr, walk_len_ptr.ptr, 0, (size_t)n_rec + 1, rocprim::plus<int>(), s));
    }
    int n_walk = 0;
    MI_HIP(hipMemcpyAsync(&n_walk, out_off.ptr + n_rec, sizeof(int), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    MI_REQUIRE(n_walk > 0 && (size_t)n_walk >= nnz, "walk list: %d entries for %zu stored values", n_walk, nnz);
    key_in.alloc((size_t)n_walk); key_sorted.alloc((size_t)n_walk);
    walk_ptr.alloc((size_t)n_cols + 1);
    int key_bits = 1;
    while ((1ll << key_bits) < (long long)n_cols) ++key_bits;
    DeviceBuffer<char> tmp4;
    if (wide) {
        DeviceBuffer<uint4> gen;
        gen.alloc((size_t)n_walk);
        h->walk16.alloc((size_t)n_walk);
        hipLaunchKernelGGL(walk_generate_kernel<true>, dim3(n_rec), dim3(256), 0, s, rec_sorted.ptr, out_off.ptr, h->csr_ptr.ptr, h->csr_idx.ptr,
                           h->csr_val.ptr, h->seg_ptr.ptr, h->row_w.ptr, (int)cfg->unit_column_side, tiled, key_in.ptr, (void *)gen.ptr);
        bytes = 0;
        MI_HIP(rocprim::radix_sort_pairs(nullptr, bytes, key_in.ptr, key_sorted.ptr, gen.ptr, h->walk16.ptr, (size_t)n_walk, 0, key_bits, s));
        tmp4.alloc(bytes + 16);
        MI_HIP(rocprim::radix_sort_pairs(tmp4.ptr, bytes, key_in.ptr, key_sorted.ptr, gen.ptr, h->walk16.ptr, (size_t)n_walk, 0, key_bits, s));
        MI_HIP(hipStreamSynchronize(s));       // (gen goes out of scope)
    } else {
        DeviceBuffer<int> gen;
        gen.alloc((size_t)n_walk);
        h->walk4.alloc((size_t)n_walk);
        hipLaunchKernelGGL(walk_generate_kernel<false>, dim3(n_rec), dim3(256), 0, s, rec_sorted.ptr, out_off.ptr, h->csr_ptr.ptr, h->csr_idx.ptr,
                           h->csr_val.ptr, h->seg_ptr.ptr, h->row_w.ptr, (int)cfg->unit_column_side, tiled, key_in.ptr, (void *)gen.ptr);
        bytes = 0;
        MI_HIP(rocprim::radix_sort_pairs(nullptr, bytes, key_in.ptr, key_sorted.ptr, gen.ptr, h->walk4.ptr, (size_t)n_walk, 0, key_bits, s));
        tmp4.alloc(bytes + 16);
        MI_HIP(rocprim::radix_sort_pairs(tmp4.ptr, bytes, key_in.ptr, key_sorted.ptr, gen.ptr, h->walk4.ptr, (size_t)n_walk, 0, key_bits, s));
        MI_HIP(hipStreamSynchronize(s));
    }
    hipLaunchKernelGGL(csc_ptr_kernel, dim3(div_up(n_cols + 1, 256)), dim3(256), 0, s, key_sorted.ptr, (size_t)n_walk, n_cols, walk_ptr.ptr);
    MI_HIP(hipGetLastError());
    h->walk_ptr_host.resize((size_t)n_cols + 1);
    walk_ptr.download(h->walk_ptr_host.data(), (size_t)n_cols + 1, s);
    MI_HIP(hipStreamSynchronize(s));
    c.n_walk_entries = n_walk;
    c.walk_keys.swap(key_sorted);
}

// the column view of the pre-processed values: the walk lists themselves (all-ones data), or CSR -> CSC
void create_column_view(SimCreate &c) {
    mi355rec_sim *h = c.h;
    hipStream_t s = c.s;
    const int n_rows = c.n_rows, n_cols = c.n_cols, eb = c.eb, eg = c.eg;
    const size_t nnz = c.nnz;
    DeviceBuffer<int> &key_out = c.key_out, &row_of = c.row_of;
    DeviceBuffer<unsigned long long> &cell_in = c.cell_in, &cell_out = c.cell_out;
    DeviceBuffer<char> &sort_tmp = c.sort_tmp;
    const bool walk_only = c.walk_only;
    if (!walk_only) {
        h->csc_idx.alloc(nnz);
        h->csc_val.alloc(nnz);
    }
    if (h->n_tiles > 1) {
        h->row_tile_ptr.alloc((size_t)n_rows * (h->n_tiles + 1));
        hipLaunchKernelGGL(row_tile_ptr_kernel, dim3(div_up((int64_t)n_rows * (h->n_tiles + 1), 256)), dim3(256), 0, s,
                           h->csr_ptr.ptr, h->csr_idx.ptr, n_rows, h->tile_w, h->n_tiles, h->row_tile_ptr.ptr);
    }
    // CSR -> CSC (.pyx:203-207), on the device: stable radix sort of the pre-processed cells by column.  All-ones data sorts the
    // row ids alone (the values of the column view are a fill); valued data sorts (row id, value) words and splits them.
    // (Measured and rejected: the sort on a second stream behind the upload of the values -- the upload of pageable memory and
    // the sort's kernels got into each other's way, 5.96 ms for the two against 2.92 + 1.16 ms one after the other.)
    if (walk_only) {
        build_seg_ptr(c);
        build_walk(c);
    } else {
        h->csc_ptr.alloc((size_t)n_cols + 1);
        key_out.alloc(nnz);
        int key_bits = 1;
        while ((1ll << key_bits) < (long long)n_cols) ++key_bits;
        size_t tmp_bytes = 0;
        const int rg = div_up((int64_t)n_rows * 64, 256);
        if (h->unit_values) {
            row_of.alloc(nnz);
            hipLaunchKernelGGL(expand_rows_kernel, dim3(rg), dim3(256), 0, s, h->csr_ptr.ptr, n_rows, row_of.ptr);
            MI_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, h->csr_idx.ptr, key_out.ptr, row_of.ptr, h->csc_idx.ptr,
                                                      (int)nnz, 0, key_bits, s));
            sort_tmp.alloc(tmp_bytes);
            MI_HIP(rocprim::radix_sort_pairs(sort_tmp.ptr, tmp_bytes, h->csr_idx.ptr, key_out.ptr, row_of.ptr, h->csc_idx.ptr,
                                                      (int)nnz, 0, key_bits, s));
            hipLaunchKernelGGL(fill_kernel, dim3(eg), dim3(eb), 0, s, h->csc_val.ptr, nnz, 1.0f);
        } else {
            cell_in.alloc(nnz);
            cell_out.alloc(nnz);
            hipLaunchKernelGGL(expand_cells_kernel, dim3(rg), dim3(256), 0, s, h->csr_ptr.ptr, h->csr_val.ptr, n_rows, cell_in.ptr);
            MI_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, h->csr_idx.ptr, key_out.ptr, cell_in.ptr, cell_out.ptr,
                                                      (int)nnz, 0, key_bits, s));
            sort_tmp.alloc(tmp_bytes);
            MI_HIP(rocprim::radix_sort_pairs(sort_tmp.ptr, tmp_bytes, h->csr_idx.ptr, key_out.ptr, cell_in.ptr, cell_out.ptr,
                                                      (int)nnz, 0, key_bits, s));
            hipLaunchKernelGGL(split_cells_kernel, dim3(eg), dim3(eb), 0, s, cell_out.ptr, nnz, h->csc_idx.ptr, h->csc_val.ptr);
        }
        hipLaunchKernelGGL(csc_ptr_kernel, dim3(div_up(n_cols + 1, 256)), dim3(256), 0, s, key_out.ptr, nnz, n_cols, h->csc_ptr.ptr);
        MI_HIP(hipGetLastError());
    }
    c.phase(walk_only ? "walk lists = the column view (slices, radix sort of the entries)" : "CSR -> CSC (allocations, radix sort of the cells)");
}

// pearson's column centring, every column's cost, users and norm, and the columns by descending cost -- with their host copies
void create_costs_and_norms(SimCreate &c) {
    mi355rec_sim *h = c.h;
    const mi355rec_sim_config *cfg = c.cfg;
    hipStream_t s = c.s;
    const int n_rows = c.n_rows, n_cols = c.n_cols, eb = c.eb, eg = c.eg;
    const size_t nnz = c.nnz;
    const bool walk_only = c.walk_only, set_based = c.set_based, euclid = c.euclid;
    DeviceBuffer<float> &mean = c.mean;
    DeviceBuffer<double> &sumsq = c.sumsq;
    DeviceBuffer<long long> &cost = c.cost, &cost_sorted = c.cost_sorted;
    DeviceBuffer<int> &key_out = c.key_out, &walk_keys = c.walk_keys, &walk_len_ptr = c.walk_len_ptr, &user_count = c.user_count;
    DeviceBuffer<unsigned long long> &packed = c.packed;
    DeviceBuffer<int> &col_ids = c.col_ids, &col_order = c.col_order;
    DeviceBuffer<char> &order_tmp = c.order_tmp;
    const int n_walk_entries = c.n_walk_entries;
    const int cg = div_up((int64_t)n_cols * 64, 256);
    if (cfg->similarity == MI355REC_SIM_PEARSON) {
        mean.alloc((size_t)n_cols);
        hipLaunchKernelGGL(segment_mean_kernel, dim3(div_up(n_cols, 256)), dim3(256), 0, s, h->csc_ptr.ptr, h->csc_val.ptr, n_cols,
                           mean.ptr);
        hipLaunchKernelGGL(col_center_kernel, dim3(eg), dim3(eb), 0, s, h->csr_idx.ptr, h->csr_val.ptr, nnz, mean.ptr);
        hipLaunchKernelGGL(col_center_csc_kernel, dim3(cg), dim3(256), 0, s, h->csc_ptr.ptr, h->csc_val.ptr, n_cols, mean.ptr);
    }
    sumsq.alloc((size_t)n_cols);
    cost.alloc((size_t)n_cols);
    MI_HIP(hipMemsetAsync(cost.ptr, 0, sizeof(long long) * (size_t)n_cols, s));
    if (walk_only) {
        // cost and users of every column from the sorted entries: the rows' lengths filed under their first slices (tiled: rows)
        const size_t n_walk = (size_t)n_walk_entries;
        packed.alloc_zero((size_t)n_cols, s);
        user_count.alloc((size_t)n_cols);
        hipLaunchKernelGGL(column_cost_kernel<true>, dim3(div_up((int64_t)div_up((int64_t)n_walk, COST_CHUNK) * 64, 256)), dim3(256), 0, s, walk_keys.ptr,
                           h->walk4.ptr, h->n_tiles > 1 ? h->csr_ptr.ptr : walk_len_ptr.ptr, n_walk, packed.ptr);
        hipLaunchKernelGGL(walk_unpack_cost_kernel, dim3(div_up(n_cols, 256)), dim3(256), 0, s, packed.ptr, n_cols, cost.ptr, sumsq.ptr, user_count.ptr);
    } else
    hipLaunchKernelGGL(column_cost_kernel<false>, dim3(div_up((int64_t)div_up((int64_t)nnz, COST_CHUNK) * 64, 256)), dim3(256), 0, s, key_out.ptr,
                       h->csc_idx.ptr, h->csr_ptr.ptr, nnz, reinterpret_cast<unsigned long long *>(cost.ptr));
    MI_REQUIRE(cfg->norm_sum_order == 0 || cfg->norm_sum_order == 1, "norm_sum_order must be 0 (CSR order) or 1 (CSC order)");
    if (walk_only) {
        // (sumsq = the users counted above)
    } else if (h->unit_values && n_rows < (1 << 24))
        hipLaunchKernelGGL(column_count_sumsq_kernel, dim3(div_up(n_cols, 256)), dim3(256), 0, s, h->csc_ptr.ptr, n_cols, sumsq.ptr);
    else if (cfg->norm_sum_order == 0)
        hipLaunchKernelGGL(column_sumsq_f32_rowwise_kernel, dim3(div_up((int64_t)n_cols * 64, 256)), dim3(256), 0, s, h->csc_ptr.ptr,
                           h->csc_val.ptr, n_cols, sumsq.ptr);
    else
        hipLaunchKernelGGL(column_sumsq_f32_kernel, dim3(div_up(n_cols, 64)), dim3(64), 0, s, h->csc_ptr.ptr, h->csc_val.ptr, n_cols,
                           cfg->norm_sum_order, sumsq.ptr);
    h->norm.alloc_zero((size_t)n_cols + NORM_PAD, s);
    const bool asym = cfg->similarity == MI355REC_SIM_ASYMMETRIC;
    if (euclid) h->norm_alpha.alloc_zero((size_t)n_cols + NORM_PAD, s);     // sums of squares
    if (asym) {
        h->norm_alpha.alloc_zero((size_t)n_cols + NORM_PAD, s);
        h->norm_1ma.alloc_zero((size_t)n_cols + NORM_PAD, s);
    }
    hipLaunchKernelGGL(norms_kernel, dim3(div_up(n_cols, 256)), dim3(256), 0, s, sumsq.ptr, n_cols, (int)set_based,
                       (int)asym, (int)euclid, cfg->asymmetric_alpha, h->norm.ptr, h->norm_alpha.ptr, h->norm_1ma.ptr);
    MI_HIP(hipGetLastError());
    // columns by descending cost (stable: ties keep ascending column ids), sorted where the costs are
    cost_sorted.alloc((size_t)n_cols); col_ids.alloc((size_t)n_cols); col_order.alloc((size_t)n_cols);
    hipLaunchKernelGGL(iota_kernel, dim3(div_up(n_cols, 256)), dim3(256), 0, s, col_ids.ptr, n_cols);
    size_t order_bytes = 0;
    int cost_bits = 1;                          // a column's cost counts every stored cell at most once: cost <= nnz
    while ((1ull << cost_bits) <= (unsigned long long)nnz) ++cost_bits;
    MI_HIP(rocprim::radix_sort_pairs_desc(nullptr, order_bytes, cost.ptr, cost_sorted.ptr, col_ids.ptr, col_order.ptr, (size_t)n_cols, 0, cost_bits, s));
    order_tmp.alloc(order_bytes + 16);
    MI_HIP(rocprim::radix_sort_pairs_desc(order_tmp.ptr, order_bytes, cost.ptr, cost_sorted.ptr, col_ids.ptr, col_order.ptr, (size_t)n_cols, 0, cost_bits, s));
    h->cost_order.resize(n_cols);
    col_order.download(h->cost_order.data(), (size_t)n_cols, s);
    h->cost.resize(n_cols);
    cost.download(h->cost.data(), n_cols, s);
    h->csc_ptr_host.resize((size_t)n_cols + 1);
    if (walk_only) {
        user_count.download(h->csc_ptr_host.data() + 1, (size_t)n_cols, s);
        MI_HIP(hipStreamSynchronize(s));
        h->csc_ptr_host[0] = 0;
        for (int col = 0; col < n_cols; ++col) h->csc_ptr_host[col + 1] += h->csc_ptr_host[col];
        MI_REQUIRE((size_t)h->csc_ptr_host[n_cols] == nnz, "walk lists: %d users counted for %zu stored values", h->csc_ptr_host[n_cols], nnz);
    } else {
        h->csc_ptr.download(h->csc_ptr_host.data(), (size_t)n_cols + 1, s);
        MI_HIP(hipStreamSynchronize(s));
    }
    c.phase("column costs + norms + downloads");
}

// lanes per user profile
void choose_group_lanes(SimCreate &c) {
    mi355rec_sim *h = c.h;
    long long total_cost = 0;
    for (long long k : h->cost) total_cost += k;
    // each lane covers 8 profile entries per load: G lanes span 8*G entries
    // (with the walk lists a lane group never sees more than WALK_SLICE chunks at once and the groups of a round get slices of
    // the same length: 8 lanes per slice are fastest at every shape measured -- ML-20M shape 3.76 ms against 3.77 / 3.91 / 4.48 with
    // 16 / 32 / 64, Netflix shape 15.7 against 16.2 / 17.8 with 16 / 32, star ratings 5.16 against 5.31 / 5.88 / 7.39)
    h->group_lanes = 8;
    // (where the packed-counts kernel will run -- see plan_columns -- sixteen: 3.03 against 3.10 ms at ML-20M shape)
    if (h->acc_mode() == ACC_COUNTS && h->n_tiles == 1 && (double)total_cost < PACKED_MAX_PAIRS_PER_COLUMN * (double)c.n_cols) h->group_lanes = 16;
    // the float64 kernel has half the loads in flight per lane (DEPTH 2)
    if (h->acc_mode() == ACC_WIDE) h->group_lanes = 16;
    if (getenv("MI355REC_SIM_G")) h->group_lanes = atoi(getenv("MI355REC_SIM_G"));
    MI_REQUIRE(h->group_lanes == 4 || h->group_lanes == 8 || h->group_lanes == 16 || h->group_lanes == 32 || h->group_lanes == 64,
               "MI355REC_SIM_G must be 4, 8, 16, 32 or 64");
}

void create_stream_and_walk(SimCreate &c) {
    if (!c.walk_only) build_seg_ptr(c);
    fill_stream(c);
    c.phase("profile stream");
    if (!c.walk_only) {
        build_walk(c);
        c.phase("walk lists");
    }
}

// Real-valued data: can the column sums be kept as int64 fixed point (ds_add_u64 is 1.8x faster than ds_add_f64)?
// Every product is at most P = max weight * max |column-side value| * max |value|; a cell sums at most N = longest
// column of them.  Scale 2^S with P * 2^S <= 2^50 (the float64 rounding trick needs |x| < 2^51) and N * P * 2^S <= 2^62.
// A cell is then off by at most N / 2 units of 2^-S.  What that error is measured against:
//   normalised similarities, Euclidean distances: the smallest denominator a cell can meet, the smallest non-zero column norm
//     squared (a distance is measured against the sum of two of them: the same bar, conservative);
//   every other un-normalised build (the results are the sums themselves, or the sums over a denominator that does not depend on
//     the data's scale): the smallest non-zero CELL, which is at least the smallest non-zero product -- smallest weight * smallest
//     |value| (unit column side: the P3alpha / RP3beta walk) or * smallest |value| squared.  A column's norm says nothing here: one
//     large entry carries it while a cell sums the column's tiny entries (values of sign-mixed data can cancel below any such
//     bound, in float64 as well).
// Accept when that WORST-CASE error stays below 1e-6 (a tenth of the parity bar; rounding errors of random sign add up to
// ~sqrt(N), not N), otherwise keep float64.
void create_fixed_point(SimCreate &c) {
    mi355rec_sim *h = c.h;
    const mi355rec_sim_config *cfg = c.cfg;
    hipStream_t s = c.s;
    const int n_rows = c.n_rows, n_cols = c.n_cols, eb = c.eb, eg = c.eg;
    const size_t nnz = c.nnz;
    const float *row_weights = c.row_weights;
    DeviceBuffer<double> &sumsq = c.sumsq;
    if (h->acc_mode() == ACC_WIDE && !getenv("MI355REC_SIM_F64_SUMS")) {
        // (h->cfg: the set-based measures have had their `normalize` cleared)
        const bool by_smallest_cell = !h->cfg.normalize && !c.euclid;
        DeviceBuffer<unsigned> d_vmax, d_vmin;
        d_vmax.alloc_zero(1, s);
        hipLaunchKernelGGL(absmax_kernel, dim3(eg), dim3(eb), 0, s, h->csc_val.ptr, nnz, d_vmax.ptr);
        MI_HIP(hipGetLastError());
        unsigned vbits = 0, vmin_bits = 0xFFFFFFFFu;
        d_vmax.download(&vbits, 1, s);
        if (by_smallest_cell) {
            d_vmin.alloc(1);
            MI_HIP(hipMemsetAsync(d_vmin.ptr, 0xFF, sizeof(unsigned), s));
            hipLaunchKernelGGL(absmin_nonzero_kernel, dim3(eg), dim3(eb), 0, s, h->csc_val.ptr, nnz, d_vmin.ptr);
            MI_HIP(hipGetLastError());
            d_vmin.download(&vmin_bits, 1, s);
        }
        std::vector<double> sq((size_t)n_cols);
        sumsq.download(sq.data(), (size_t)n_cols, s);
        MI_HIP(hipStreamSynchronize(s));
        float vmax_f;
        memcpy(&vmax_f, &vbits, sizeof(float));
        const double vmax = (double)vmax_f;
        double vmin = 0.0;                  // smallest non-zero |value| (0: none)
        if (vmin_bits != 0xFFFFFFFFu) {
            float vmin_f;
            memcpy(&vmin_f, &vmin_bits, sizeof(float));
            vmin = (double)vmin_f;
        }
        double wmax = 1.0, wmin = 1.0;      // wmin: smallest non-zero |weight|
        if (row_weights) {
            wmin = 0.0;
            for (int r = 0; r < n_rows; ++r) {
                const double w = (double)std::fabs(row_weights[r]);
                wmax = std::max(wmax, w);
                if (w > 0.0 && (wmin == 0.0 || w < wmin)) wmin = w;
            }
        }
        double longest = 1.0, min_sq = 0.0;
        for (int col = 0; col < n_cols; ++col) {
            longest = std::max(longest, (double)(h->csc_ptr_host[col + 1] - h->csc_ptr_host[col]));
            if (sq[col] > 0.0 && (min_sq == 0.0 || sq[col] < min_sq)) min_sq = sq[col];
        }
        const double prod = wmax * (cfg->unit_column_side ? 1.0 : vmax) * vmax;
        if (prod > 0.0 && std::isfinite(prod)) {
            const int S = (int)std::floor(std::min(50.0 - std::log2(prod), 62.0 - std::log2(prod * longest)));
            const double unit = std::ldexp(1.0, -S);
            // denominators: norm_c * norm_j >= min_sq (normalised); otherwise the smallest non-zero cell (see above)
            const double floor_of_results = by_smallest_cell ? wmin * (cfg->unit_column_side ? 1.0 : vmin) * vmin : min_sq;
            const double worst = 0.5 * longest * unit / std::max(floor_of_results, 1e-300);
            if (S > -1000 && S < 1000 && worst <= 1e-6) h->fixed_scale = std::ldexp(1.0, S);
        }
    }
}

}  // namespace

// `resident`: the three CSR arrays are device memory (mi355rec_sim_create_resident) -- copied at HBM speed instead of over PCIe
static int sim_create_from(mi355rec_sim_t *out, const mi355rec_sim_config *cfg, int32_t n_rows, int32_t n_cols,
                           const int32_t *csr_indptr, const int32_t *csr_indices, const float *csr_data,
                           const float *row_weights, bool resident) {
    return guarded([&] {
        MI_REQUIRE(out && cfg && csr_indptr && csr_indices && csr_data, "NULL argument");
        MI_REQUIRE(n_rows > 0 && n_cols > 0, "empty matrix (%d x %d)", n_rows, n_cols);
        MI_REQUIRE(cfg->similarity >= MI355REC_SIM_COSINE && cfg->similarity <= MI355REC_SIM_EUCLIDEAN,
                   "Cosine_Similarity: value for parameter 'mode' not recognized (%d)", cfg->similarity);
        const bool euclid = cfg->similarity == MI355REC_SIM_EUCLIDEAN;
        if (euclid) {
            MI_REQUIRE(cfg->euclidean_mode >= MI355REC_EUCLID_LIN && cfg->euclidean_mode <= MI355REC_EUCLID_EXP,
                       "Compute_Similarity_Euclidean: value for parameter 'mode' not recognized (%d)", cfg->euclidean_mode);
            // the reference multiplies the distances to the n_cols columns by the n_rows weights (Euclidean.py:174-175): NumPy refuses
            // that for any other shape ("operands could not be broadcast together")
            if (row_weights)
                MI_REQUIRE(n_rows == n_cols, "Compute_Similarity_Euclidean: row_weights need a square dataMatrix (the reference multiplies the "
                           "%d column distances by the %d row weights: operands could not be broadcast together)", n_cols, n_rows);
        }
        MI_REQUIRE(cfg->topK >= 0, "topK must be >= 0");
        const auto t_enter = std::chrono::steady_clock::now();
        ensure_device();
        std::unique_ptr<mi355rec_sim> h(new mi355rec_sim());
        h->cfg = *cfg;
        h->cfg.topK = std::min(cfg->topK, n_cols);  // .pyx:146
        // (topK > MAX_TOPK, the in-LDS selection's candidate buffer: dense columns + segmented sort, run_columns_wide_topk)
        const bool set_based = cfg->similarity == MI355REC_SIM_JACCARD || cfg->similarity == MI355REC_SIM_DICE ||
                               cfg->similarity == MI355REC_SIM_TVERSKY;
        if (set_based) h->cfg.normalize = 0;  // .pyx:124-135
        h->n_rows = n_rows;
        h->n_cols = n_cols;
        int32_t nnz_in = 0;
        if (resident) MI_HIP(hipMemcpy(&nnz_in, csr_indptr + n_rows, sizeof(int32_t), hipMemcpyDeviceToHost));
        else nnz_in = csr_indptr[n_rows];
        h->nnz = (size_t)nnz_in;
        MI_REQUIRE(nnz_in > 0, "matrix has no stored values");
        h->open(2, StreamFrom::Pool);
        ReleaseScope scope(h->stream);          // the constructor's temporaries wait for this stream, not for the device
        SimCreate c{h.get(), cfg, n_rows, n_cols, h->nnz, h->stream, row_weights, set_based, euclid};
        c.eg = std::min<size_t>((c.nnz + c.eb - 1) / c.eb, 4096);
        c.phases = getenv("MI355REC_SIM_CREATE_PHASES") != nullptr;
        c.t_phase = t_enter;
        c.phase("device, stream, events, nnz");
        create_upload(c, csr_indptr, csr_indices, csr_data, resident);
        create_value_checks(c);
        create_tiles_and_row_centring(c);
        c.stream_order = !(getenv("MI355REC_SIM_STREAM_ORDER") && atoi(getenv("MI355REC_SIM_STREAM_ORDER")) == 0);
        c.walk_only = h->acc_mode() == ACC_COUNTS && n_rows < (1 << 23) && !getenv("MI355REC_SIM_WALK_WITH_CSC");
        create_column_view(c);
        create_costs_and_norms(c);
        choose_group_lanes(c);
        create_stream_and_walk(c);
        create_fixed_point(c);
        // the column view has served (norms, costs, value range): the accumulation walks the lists above
        h->csc_idx.release();
        h->csc_val.release();
        h->queue.alloc(4);
        c.phase("fixed-point check + cost order (host)");
        *out = h.release();
    });
}

extern "C" int mi355rec_sim_create(mi355rec_sim_t *out, const mi355rec_sim_config *cfg, int32_t n_rows, int32_t n_cols,
                                   const int32_t *csr_indptr, const int32_t *csr_indices, const float *csr_data,
                                   const float *row_weights) {
    return sim_create_from(out, cfg, n_rows, n_cols, csr_indptr, csr_indices, csr_data, row_weights, false);
}

extern "C" int mi355rec_sim_create_resident(mi355rec_sim_t *out, const mi355rec_sim_config *cfg, int32_t n_rows, int32_t n_cols,
                                            const int32_t *d_csr_indptr, const int32_t *d_csr_indices, const float *d_csr_data,
                                            const float *row_weights) {
    return sim_create_from(out, cfg, n_rows, n_cols, d_csr_indptr, d_csr_indices, d_csr_data, row_weights, true);
}

extern "C" int mi355rec_sim_compute_device(mi355rec_sim_t h, int32_t start_col, int32_t end_col, int32_t *d_nbr_idx,
                                           float *d_nbr_val) {
    return guarded([&] {
        MI_REQUIRE(h && d_nbr_idx && d_nbr_val, "NULL argument");
        MI_REQUIRE(h->cfg.topK > 0, "topK == 0: use mi355rec_sim_compute_dense");
        ensure_device();
        clamp_range(h, start_col, end_col);
        ReleaseScope scope(h->stream);
        run_columns(h, ColumnSelection::range(start_col, end_col), d_nbr_idx, d_nbr_val, nullptr);
    });
}

extern "C" int mi355rec_sim_compute_part_device(mi355rec_sim_t h, int32_t part, int32_t n_parts, int32_t *d_nbr_idx, float *d_nbr_val) {
    return guarded([&] {
        MI_REQUIRE(h && d_nbr_idx && d_nbr_val, "NULL argument");
        MI_REQUIRE(n_parts >= 1 && part >= 0 && part < n_parts, "part %d of %d", part, n_parts);
        if (h->cfg.topK == 0) fail(MI355REC_E_INVALID, "topK == 0: use mi355rec_sim_compute_dense");
        ensure_device();
        run_columns(h, ColumnSelection::part_of(part, n_parts), d_nbr_idx, d_nbr_val, nullptr);
    });
}

extern "C" int mi355rec_sim_compute_part_chunk_device(mi355rec_sim_t h, int32_t part, int32_t n_parts, int32_t slot_first, int32_t slot_count,
                                                      int32_t *d_nbr_idx, float *d_nbr_val) {
    return guarded([&] {
        MI_REQUIRE(h && d_nbr_idx && d_nbr_val, "NULL argument");
        MI_REQUIRE(n_parts >= 1 && part >= 0 && part < n_parts, "part %d of %d", part, n_parts);
        MI_REQUIRE(slot_first >= 0 && slot_count >= 0, "rows %d + %d of a part", slot_first, slot_count);
        if (h->cfg.topK == 0) fail(MI355REC_E_INVALID, "topK == 0: use mi355rec_sim_compute_dense");
        ensure_device();
        if (slot_count == 0) return;
        // (topK beyond the in-LDS selection, or more per-tile candidates than the merge buffer holds: dense columns + segmented sort,
        // walking the same rows of the part)
        run_columns(h, ColumnSelection::part_of(part, n_parts, slot_first, slot_count), d_nbr_idx, d_nbr_val, nullptr);
    });
}

// The 6-byte cells of the sharded build's exchange (n_cols <= 65 535): n_cells float32 values, then n_cells 16-bit neighbour ids
// (0xFFFF = the empty slot's -1), the whole padded to 4-byte words.  Two cells per thread: one packed id word per store.
__global__ void sim_pack_slab_kernel(const int *idx, const float *val, long long n_cells, float *out_val, unsigned *out_ids) {
    const long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;          // pair number
    const long long q = 2 * p;
    if (q >= n_cells) return;
    const bool two = q + 1 < n_cells;
    const unsigned lo = (unsigned)idx[q] & 0xFFFFu, hi = two ? ((unsigned)idx[q + 1] & 0xFFFFu) : 0xFFFFu;
    out_val[q] = val[q];
    if (two) out_val[q + 1] = val[q + 1];
    out_ids[p] = lo | (hi << 16);
}
__global__ void sim_unpack_slab_kernel(const float *in_val, const unsigned *in_ids, long long n_cells, int *idx, float *val) {
    const long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long q = 2 * p;
    if (q >= n_cells) return;
    const unsigned w = in_ids[p];
    const unsigned lo = w & 0xFFFFu, hi = w >> 16;
    idx[q] = lo == 0xFFFFu ? -1 : (int)lo;
    val[q] = in_val[q];
    if (q + 1 < n_cells) {
        idx[q + 1] = hi == 0xFFFFu ? -1 : (int)hi;
        val[q + 1] = in_val[q + 1];
    }
}

extern "C" int mi355rec_sim_pack_slab_device(mi355rec_sim_t h, const int32_t *d_nbr_idx, const float *d_nbr_val, int64_t n_cells, void *d_packed) {
    return guarded([&] {
        MI_REQUIRE(h && d_nbr_idx && d_nbr_val && d_packed, "NULL argument");
        MI_REQUIRE(n_cells >= 0, "n_cells = %lld", (long long)n_cells);
        MI_REQUIRE(h->n_cols <= 65535, "n_cols = %d: neighbour ids do not fit 16 bits", h->n_cols);
        ensure_device();
        if (n_cells == 0) return;
        const long long pairs = (n_cells + 1) / 2;
        hipLaunchKernelGGL(sim_pack_slab_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, h->stream, d_nbr_idx, d_nbr_val, (long long)n_cells,
                           (float *)d_packed, (unsigned *)d_packed + n_cells);
        MI_HIP(hipGetLastError());
    });
}

extern "C" int mi355rec_sim_unpack_slab_device(mi355rec_sim_t h, const void *d_packed, int64_t n_cells, int32_t *d_nbr_idx, float *d_nbr_val) {
    return guarded([&] {
        MI_REQUIRE(h && d_nbr_idx && d_nbr_val && d_packed, "NULL argument");
        MI_REQUIRE(n_cells >= 0, "n_cells = %lld", (long long)n_cells);
        ensure_device();
        if (n_cells == 0) return;
        const long long pairs = (n_cells + 1) / 2;
        hipLaunchKernelGGL(sim_unpack_slab_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, h->stream, (const float *)d_packed,
                           (const unsigned *)d_packed + n_cells, (long long)n_cells, d_nbr_idx, d_nbr_val);
        MI_HIP(hipGetLastError());
    });
}

extern "C" int mi355rec_sim_part_columns(mi355rec_sim_t h, int32_t part, int32_t n_parts, int32_t *columns, int32_t *n_columns) {
    return guarded([&] {
        MI_REQUIRE(h && n_columns, "NULL argument");
        MI_REQUIRE(n_parts >= 1 && part >= 0 && part < n_parts, "part %d of %d", part, n_parts);
        const std::vector<int> mine = selection_columns(ColumnSelection::part_of(part, n_parts), h->cost_order);
        if (columns) std::copy(mine.begin(), mine.end(), columns);
        *n_columns = (int32_t)mine.size();
    });
}

extern "C" int mi355rec_sim_get_weighted_values(mi355rec_sim_t h, float *csr_data) {
    return guarded([&] {
        MI_REQUIRE(h && csr_data, "NULL argument");
        MI_REQUIRE(h->weighted_val.ptr, "the handle was created without feature_weighting");
        ensure_device();
        h->weighted_val.download(csr_data, h->nnz, h->stream);
        MI_HIP(hipStreamSynchronize(h->stream));
    });
}

extern "C" int mi355rec_sim_compute(mi355rec_sim_t h, int32_t start_col, int32_t end_col, int32_t *nbr_idx, float *nbr_val) {
    return guarded([&] {
        MI_REQUIRE(h && nbr_idx && nbr_val, "NULL argument");
        MI_REQUIRE(h->cfg.topK > 0, "topK == 0: use mi355rec_sim_compute_dense");
        ensure_device();
        clamp_range(h, start_col, end_col);
        ReleaseScope scope(h->stream);
        const size_t n = (size_t)(end_col - start_col) * h->cfg.topK;
        if (h->out_idx.count < n) {
            h->out_idx.alloc(n);
            h->out_val.alloc(n);
        }
        run_columns(h, ColumnSelection::range(start_col, end_col), h->out_idx.ptr, h->out_val.ptr, nullptr);
        h->out_idx.download(nbr_idx, n, h->stream);
        h->out_val.download(nbr_val, n, h->stream);
        MI_HIP(hipStreamSynchronize(h->stream));
        read_timers(h);
        if (h->phase_ticks.ptr && getenv("MI355REC_SIM_PHASES")) {
            unsigned long long t[12], w[16];
            h->phase_ticks.download(w, 16, h->stream);
            h->selection_counts.download(t + 8, 4, h->stream);
            MI_HIP(hipStreamSynchronize(h->stream));
            memcpy(t, w, 8 * sizeof(unsigned long long));
            fprintf(stderr, "[mi355rec sim spans] first start to last end %.3f ms; workgroups' own spans %.2f workgroup-ms; longest work item %.3f ms (column %llu)\n",
                    (double)(w[9] - w[8]) * 1e-5, (double)w[10] * 1e-5, (double)w[11] * 1e-5, w[12]);
            fprintf(stderr, "[mi355rec sim phases, workgroup-ms] fetch+clear %.2f  accumulate %.2f  split-merge %.2f  normalise %.2f  topk %.2f  (kernel %.3f ms)"
                            "  threshold-first: maxima scan %.2f  (K-th maximum under `normalise`)  survivor scan %.2f  (exact values + rank + emit under `topk`)"
                            "  columns %llu (candidates %.1f per column), full-selection fall-backs after the scan %llu (%llu: buffer full); wait for the scan's slowest wavefront %.2f (instrumented runs only)\n",
                    t[0] * 1e-5, t[1] * 1e-5, t[2] * 1e-5, t[3] * 1e-5, t[4] * 1e-5, h->stats.kernel_ms, t[5] * 1e-5, t[6] * 1e-5, t[8],
                    t[8] ? (double)t[9] / (double)t[8] : 0.0, t[10], t[11], t[7] * 1e-5);
        }
    });
}

extern "C" int mi355rec_sim_compute_csr(mi355rec_sim_t h, int32_t start_col, int32_t end_col, int32_t *indptr, int32_t *indices,
                                        float *data, int64_t *nnz_out) {
    return guarded([&] {
        MI_REQUIRE(h && indptr && indices && data && nnz_out, "NULL argument");
        MI_REQUIRE(h->cfg.topK > 0, "topK == 0: use mi355rec_sim_compute_dense");
        ensure_device();
        clamp_range(h, start_col, end_col);
        ReleaseScope scope(h->stream);
        const size_t n = (size_t)(end_col - start_col) * h->cfg.topK;
        MI_REQUIRE(n < (size_t)INT32_MAX, "result too large for 32-bit CSR offsets");
        if (h->out_idx.count < n) {
            h->out_idx.alloc(n);
            h->out_val.alloc(n);
        }
        if (h->csr_key.count < n) {
            h->csr_key.alloc(n); h->csr_key_sorted.alloc(n); h->csr_pos.alloc(n); h->csr_pos_sorted.alloc(n);
            h->csr_indices.alloc(n); h->csr_data.alloc(n);
        }
        if (!h->csr_indptr.ptr) h->csr_indptr.alloc((size_t)h->n_cols + 1);
        hipStream_t s = h->stream;
        run_columns(h, ColumnSelection::range(start_col, end_col), h->out_idx.ptr, h->out_val.ptr, nullptr);
        const int eb = 256, eg = (int)std::min<size_t>((n + eb - 1) / eb, 4096);
        hipLaunchKernelGGL(csr_keys_kernel, dim3(eg), dim3(eb), 0, s, h->out_idx.ptr, n, h->n_cols, h->csr_key.ptr, h->csr_pos.ptr);
        int key_bits = 1;
        while ((1ll << key_bits) < (long long)h->n_cols + 1) ++key_bits;
        size_t tmp_bytes = 0;
        MI_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, h->csr_key.ptr, h->csr_key_sorted.ptr, h->csr_pos.ptr,
                                                  h->csr_pos_sorted.ptr, (int)n, 0, key_bits, s));
        if (h->csr_sort_tmp.count < tmp_bytes) h->csr_sort_tmp.alloc(tmp_bytes);
        MI_HIP(rocprim::radix_sort_pairs(h->csr_sort_tmp.ptr, tmp_bytes, h->csr_key.ptr, h->csr_key_sorted.ptr,
                                                  h->csr_pos.ptr, h->csr_pos_sorted.ptr, (int)n, 0, key_bits, s));
        // indptr[r] = first sorted position whose key is >= r; indptr[n_cols] = number of real entries (padding sorts last)
        hipLaunchKernelGGL(csc_ptr_kernel, dim3(div_up(h->n_cols + 1, 256)), dim3(256), 0, s, h->csr_key_sorted.ptr, n, h->n_cols,
                           h->csr_indptr.ptr);
        hipLaunchKernelGGL(csr_gather_kernel, dim3(eg), dim3(eb), 0, s, h->csr_pos_sorted.ptr, h->out_val.ptr, n, h->cfg.topK,
                           start_col, h->csr_indices.ptr, h->csr_data.ptr);
        MI_HIP(hipGetLastError());
        h->csr_indptr.download(indptr, (size_t)h->n_cols + 1, s);
        MI_HIP(hipStreamSynchronize(s));
        const size_t nnz = (size_t)indptr[h->n_cols];
        *nnz_out = (int64_t)nnz;
        h->csr_indices.download(indices, nnz, s);
        h->csr_data.download(data, nnz, s);
        MI_HIP(hipStreamSynchronize(s));
        read_timers(h);
    });
}

extern "C" int mi355rec_sim_compute_dense(mi355rec_sim_t h, int32_t start_col, int32_t end_col, float *W, int64_t ld) {
    return guarded([&] {
        MI_REQUIRE(h && W, "NULL argument");
        ensure_device();
        clamp_range(h, start_col, end_col);
        ReleaseScope scope(h->stream);
        const int n_local = end_col - start_col;
        MI_REQUIRE(ld >= n_local, "ld (%lld) < number of columns (%d)", (long long)ld, n_local);
        DeviceBuffer<float> slab, slab_t;
        slab.alloc((size_t)n_local * h->n_cols);
        slab_t.alloc((size_t)n_local * h->n_cols);
        run_columns(h, ColumnSelection::range(start_col, end_col), nullptr, nullptr, slab.ptr);
        hipLaunchKernelGGL(transpose_kernel, dim3(div_up(h->n_cols, 32), div_up(n_local, 32)), dim3(32, 8), 0, h->stream,
                           slab.ptr, slab_t.ptr, n_local, h->n_cols);
        MI_HIP(hipGetLastError());
        MI_HIP(hipMemcpy2DAsync(W, (size_t)ld * sizeof(float), slab_t.ptr, (size_t)n_local * sizeof(float),
                                (size_t)n_local * sizeof(float), (size_t)h->n_cols, hipMemcpyDeviceToHost, h->stream));
        MI_HIP(hipStreamSynchronize(h->stream));
        read_timers(h);
    });
}

extern "C" int mi355rec_sim_compute_dense_device(mi355rec_sim_t h, int32_t start_col, int32_t end_col, float *d_W, int64_t ld) {
    return guarded([&] {
        MI_REQUIRE(h && d_W, "NULL argument");
        ensure_device();
        clamp_range(h, start_col, end_col);
        ReleaseScope scope(h->stream);
        const int n_local = end_col - start_col;
        MI_REQUIRE(ld >= h->n_cols, "ld (%lld) < length of a column (%d)", (long long)ld, h->n_cols);
        if (ld == h->n_cols) {
            run_columns(h, ColumnSelection::range(start_col, end_col), nullptr, nullptr, d_W);
        } else {            // (the column kernel's own pitch is n_cols)
            DeviceBuffer<float> slab;
            slab.alloc((size_t)n_local * h->n_cols);
            run_columns(h, ColumnSelection::range(start_col, end_col), nullptr, nullptr, slab.ptr);
            MI_HIP(hipMemcpy2DAsync(d_W, (size_t)ld * sizeof(float), slab.ptr, (size_t)h->n_cols * sizeof(float),
                                    (size_t)h->n_cols * sizeof(float), (size_t)n_local, hipMemcpyDeviceToDevice, h->stream));
        }
        MI_HIP(hipStreamSynchronize(h->stream));
        read_timers(h);
    });
}

namespace mi355rec {
// what ease.hip checks before it asks a handle for its Gram matrix
void sim_shape(const mi355rec_sim *h, int *n_cols, int *topK) {
    *n_cols = h->n_cols;
    *topK = h->cfg.topK;
}
}  // namespace mi355rec

extern "C" int mi355rec_sim_column_costs(mi355rec_sim_t h, int64_t *cost) {
    return guarded([&] {
        MI_REQUIRE(h && cost, "NULL argument");
        for (int c = 0; c < h->n_cols; ++c) cost[c] = h->cost[c];
    });
}

extern "C" int mi355rec_sim_schedule_info(mi355rec_sim_t h, int32_t *n_items, int32_t *n_split_columns, int32_t *n_parts) {
    return guarded([&] {
        MI_REQUIRE(h && n_items && n_split_columns && n_parts, "NULL argument");
        *n_items = (int32_t)h->plan.items.size();
        *n_split_columns = h->plan.n_split;
        *n_parts = h->plan.part_slots;
    });
}

extern "C" int mi355rec_sim_selection_info(mi355rec_sim_t h, int64_t *threshold_first_columns, int64_t *candidates, int64_t *fallbacks) {
    return guarded([&] {
        MI_REQUIRE(h && threshold_first_columns && candidates && fallbacks, "NULL argument");
        unsigned long long t[4] = {0, 0, 0, 0};
        if (h->selection_counts.ptr) {
            ensure_device();
            h->selection_counts.download(t, 4, h->stream);
            MI_HIP(hipStreamSynchronize(h->stream));
        }
        *threshold_first_columns = (int64_t)t[0];
        *candidates = (int64_t)t[1];
        *fallbacks = (int64_t)t[2];
    });
}

extern "C" int mi355rec_sim_accumulator_info(mi355rec_sim_t h, int32_t *kind, double *fixed_scale) {
    return guarded([&] {
        MI_REQUIRE(h && kind && fixed_scale, "NULL argument");
        const int mode = h->acc_mode();
        *kind = mode == ACC_COUNTS ? 0 : (mode == ACC_INT32 ? 3 : (h->fixed_scale > 0.0 ? 1 : 2));
        *fixed_scale = mode == ACC_COUNTS ? 0.0 : (mode == ACC_INT32 ? (double)(1 << (2 * h->int_shift)) : h->fixed_scale);
    });
}

// ---- the bound the column kernel is priced against, measured on the device at hand -----------------------------------------
// ds_add_u32 lane-adds per second of the whole device: one 1024-thread workgroup per CU adding to pseudo-random cells of a 128 KiB LDS
// array (uniformly random addresses: the bank conflicts of a random scatter are part of the figure; scripts/micro/lds_atomics.hip is
// the same loop stand-alone, 21.6 lane-adds per ns and CU in round 1).
namespace {
__global__ __launch_bounds__(1024) void lds_atomic_rate_kernel(int iters, unsigned *sink) {
    extern __shared__ __attribute__((aligned(16))) unsigned rate_cells[];
    constexpr unsigned CELLS = 128 * 1024 / sizeof(unsigned);
    for (unsigned i = threadIdx.x; i < CELLS; i += 1024) rate_cells[i] = 0u;
    __syncthreads();
    unsigned s = threadIdx.x * 2654435761u + blockIdx.x * 40503u + 1u;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            s = s * 1664525u + 1013904223u;
            atomicAdd(&rate_cells[(s >> 8) % CELLS], s & 7u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) sink[blockIdx.x] = rate_cells[blockIdx.x % CELLS];
}
}  // namespace

extern "C" int mi355rec_lds_atomic_rate(double *lane_adds_per_second) {
    return guarded([&] {
        MI_REQUIRE(lane_adds_per_second, "NULL argument");
        ensure_device();
        const int cus = multiprocessor_count(), iters = 2048;
        DeviceBuffer<unsigned> sink;
        sink.alloc((size_t)cus);
        auto kern = lds_atomic_rate_kernel;
        MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
        hipEvent_t a = pooled_event(), b = pooled_event();
        hipLaunchKernelGGL(kern, dim3(cus), dim3(1024), 128 * 1024, 0, 64, sink.ptr);             // warm-up
        double best = 0.0;
        for (int rep = 0; rep < 3; ++rep) {
            MI_HIP(hipEventRecord(a, 0));
            hipLaunchKernelGGL(kern, dim3(cus), dim3(1024), 128 * 1024, 0, iters, sink.ptr);
            MI_HIP(hipEventRecord(b, 0));
            MI_HIP(hipEventSynchronize(b));
            float ms = 0.f;
            MI_HIP(hipEventElapsedTime(&ms, a, b));
            if (ms > 0.f) best = std::max(best, (double)cus * 1024.0 * iters * 8.0 / (ms * 1e-3));
        }
        MI_HIP(hipGetLastError());
        pooled_event_return(a);
        pooled_event_return(b);
        *lane_adds_per_second = best;
    });
}

extern "C" int mi355rec_sim_sync(mi355rec_sim_t h) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL handle");
        MI_HIP(hipStreamSynchronize(h->stream));
        if (h->last_start >= 0) read_timers(h);
    });
}

extern "C" int mi355rec_sim_get_stats(mi355rec_sim_t h, mi355rec_stats *stats) { return handle_get_stats(h, stats); }

extern "C" void mi355rec_sim_destroy(mi355rec_sim_t h) { handle_destroy(h); }
