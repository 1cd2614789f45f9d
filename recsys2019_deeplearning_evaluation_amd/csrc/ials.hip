// ials.hip -- IALS solve step on MI355X (gfx950).
//
// Replaces MatrixFactorization/IALSRecommender.py (reference, pure NumPy): _run_epoch :137-166 (user pass against
// V and V^T V, then item pass against the UPDATED U and U^T U) and _update_row :170-201
//      x = inv(YtY + Y_I^T (C_I - 1) Y_I + reg I) . (Y_I^T c_I).
//
// Design.  This is the one dense contraction on the hot path; it is done in float64 like the
// reference (the systems are ill-conditioned for small `reg`, fp32 cannot meet the 1e-5 parity bar), on the FP64 MATRIX pipe
// (v_mfma_f64_16x16x4_f64; on CDNA4 its peak equals the FP64 vector peak, 78.6 TFLOP/s, but one instruction carries 512
// multiply-adds and needs 2 LDS operand reads, against 14 reads per 28 multiply-adds on the vector pipe).
//   gram_kernel      G = Y^T Y, register tiles + double atomics (tiny: n * k^2).
//   ials_row_kernel  one 512-thread workgroup per row, rows pulled longest-profile-first from a queue; see the comment above
//                    the kernel: augmented system in 16 x 16 register tiles, Gramian and trailing updates as MFMAs, blocked
//                    Cholesky with an in-register diagonal-tile factorisation, back substitution through the tile inverses.
// This file: the handle, the launches and the C ABI.  The kernels are in ials_kernels.cuh and ials_solve.cuh (the diagonal tile in
// ials_diag.cuh); every host decision -- knobs, tile counts and kernel instances, buffer sizes, work items, batches -- is a function
// of ials_plan.h, which builds and is tested without a GPU.
#include "common.h"
#include "score.h"
#include "ials_solve.cuh"

#include <cstdint>
#include <memory>
#include <numeric>

using namespace mi355rec;

static_assert(sizeof(WorkItem) == sizeof(int4), "the kernels read a work item as an int4");

struct mi355rec_ials : Handle {
    int n_users = 0, n_items = 0, k = 0;
    double reg = 0;
    size_t nnz = 0;
    IalsKnobs knobs;                       // as the running ABI call found them (begin_call)
    DeviceBuffer<int> u_ptr, u_idx, i_ptr, i_idx;
    DeviceBuffer<int4> items;
    DeviceBuffer<double> part_buf;
    DeviceBuffer<unsigned> part_count;
    DeviceBuffer<double> systems;          // two-stage epochs: the augmented systems of one batch of rows
    DeviceBuffer<int> sys_slot;
    double system_gib = 0.0;             // size of the two-stage epochs' systems buffer (0: not decided yet, see batch_rows)
    WorkPlan work;                         // of the last half-step
    int n_split_rows = 0, n_part_items = 0;
    DeviceBuffer<float> u_conf, i_conf;
    DeviceBuffer<double> U, V, G;
    DeviceBuffer<unsigned> queue;
    DeviceBuffer<unsigned long long> phases;
    std::vector<int> user_order, item_order;     // longest profile first
    std::vector<int> u_ptr_host, i_ptr_host;
    double flops_acc = 0, bytes_acc = 0;
    long long rows_acc = 0, launches_acc = 0;

    ~mi355rec_ials() { shutdown(); }
};

namespace {

// f(std::integral_constant<int, SLOTS>) for the kernel instance the plan's slot count names
template <class List, class F>
void launch_instance(List list, int slots, F &&f) {
    MI_REQUIRE(dispatch_slots(list, slots, f), "ials: no kernel instance with %d tile slots", slots);
}

void launch_gram(mi355rec_ials *h, const double *Y, int n) {
    MI_HIP(hipMemsetAsync(h->G.ptr, 0, sizeof(double) * h->k * h->k, h->stream));
    const int grid = std::max(1, std::min(2 * multiprocessor_count(), (n + 63) / 64));
    const auto launch = [&](auto kt16, int a0, int b0) {
        hipLaunchKernelGGL(gram_kernel<decltype(kt16)::value>, dim3(grid), dim3(256), 0, h->stream, Y, n, h->k, h->G.ptr, a0, b0);
    };
    const int tiles = (h->k + 15) / 16;        // per side of G (no rhs row here)
    if (dispatch_slots(Slots<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14>{}, tiles, [&](auto kt16) { launch(kt16, 0, 0); })) return;
    for (int a0 = 0; a0 < 16; a0 += 8)         // 15 or 16 tiles per side: four quadrants of 8 x 8 tiles
        for (int b0 = 0; b0 < 16; b0 += 8) launch(std::integral_constant<int, 8>{}, a0, b0);
}

template <int SLOTS, int STAGE, int THREADS>
void launch_rows_ts(mi355rec_ials *h, const IalsParams &p, int grid, hipEvent_t e0, hipEvent_t e1) {
    const size_t lds = sizeof(double) * lds_doubles(h->k, STAGE);
    auto kern = ials_row_kernel<SLOTS, STAGE, THREADS>;
    MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipExtLaunchKernelGGL(kern, dim3(grid), dim3(THREADS), (unsigned)lds, h->stream, e0, e1, 0, p);
}

// the one-kernel epoch: 512 threads, lower-triangle tiles over eight wavefronts
void launch_rows(mi355rec_ials *h, const IalsParams &p, int grid, hipEvent_t e0, hipEvent_t e1) {
    launch_instance(RowSlots{}, row_slots(NT(h->k)),
                    [&](auto slots) { launch_rows_ts<decltype(slots)::value, 0, ROW_THREADS>(h, p, grid, e0, e1); });
}

// The Gramian stage of a two-stage epoch: 1024 threads, tiles over sixteen wavefronts
void launch_gram_stage(mi355rec_ials *h, const IalsParams &p, int grid, hipEvent_t e0, hipEvent_t e1) {
    launch_instance(GramSlots{}, gram_slots(NT(h->k)),
                    [&](auto slots) { launch_rows_ts<decltype(slots)::value, 1, GRAM_THREADS>(h, p, grid, e0, e1); });
}

template <int SLOTS>
void launch_solve_t(mi355rec_ials *h, const IalsParams &p, int grid, hipEvent_t e0, hipEvent_t e1) {
    const size_t lds = sizeof(double) * lds_doubles(h->k, 2);
    auto kern = ials_solve_kernel<SLOTS>;
    MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipExtLaunchKernelGGL(kern, dim3(grid), dim3(ROW_THREADS), (unsigned)lds, h->stream, e0, e1, 0, p, gram_slots(NT(h->k)),
                          (int)GRAM_THREADS);
}

void launch_solve(mi355rec_ials *h, const IalsParams &p, int grid, hipEvent_t e0, hipEvent_t e1) {
    launch_instance(SolveSlots{}, solve_instance_slots(NT(h->k)),
                    [&](auto slots) { launch_solve_t<decltype(slots)::value>(h, p, grid, e0, e1); });
}

// Rows whose systems the buffer holds at a time (ials_plan.h: decide_system_gib, rows_per_batch); the size is decided when the handle
// first asks.  A buffer that cannot be had is halved (ensure_systems).
int batch_rows(mi355rec_ials *h) {
    if (h->system_gib <= 0.0) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            (void)hipGetLastError();
            free_b = SIZE_MAX;
        }
        h->system_gib = decide_system_gib(free_b, h->knobs);
    }
    return rows_per_batch(h->system_gib, h->k, (size_t)std::max(h->n_users, h->n_items));
}

// The systems buffer for half-steps of up to `rows` rows: min(rows, batch_rows) slabs.  Blocks above 1 GiB bypass the block cache,
// so this is a real hipMalloc -- done once per handle (and again only if a larger half-step arrives).  If the device cannot give it,
// the batch is halved (more, smaller batches: same results) down to 64 slabs; below that the caller falls back to the one-kernel epoch.
bool ensure_systems(mi355rec_ials *h, int rows) {
    const size_t slab = slab_doubles(h->k, true);
    for (;;) {
        const int per_batch = std::min(std::max(1, rows), batch_rows(h));
        if (h->systems.count >= (size_t)per_batch * slab) return true;
        try {
            h->systems.alloc((size_t)per_batch * slab);
            return true;
        } catch (const Error &) {
            (void)hipGetLastError();
            const std::optional<double> smaller = halved_system_gib(per_batch, h->k);
            if (!smaller) return false;
            h->system_gib = *smaller;
        }
    }
}

// the partial systems of split rows, laid out by the kernel that builds them (two_stage: the Gramian stage), and their arrival counters
void ensure_parts(mi355rec_ials *h, int part_slots, bool two_stage) {
    if (!part_slots) return;
    const size_t part_doubles = slab_doubles(h->k, two_stage);
    if (h->part_buf.count < (size_t)part_slots * part_doubles) h->part_buf.alloc((size_t)part_slots * part_doubles);
    if (h->part_count.count < (size_t)part_slots) h->part_count.alloc((size_t)part_slots);
    MI_HIP(hipMemsetAsync(h->part_count.ptr, 0, sizeof(unsigned) * part_slots, h->stream));
}

void upload_items(mi355rec_ials *h, const std::vector<WorkItem> &items) {
    if (h->items.count < items.size()) h->items.alloc(items.size() + 1024);
    MI_HIP(hipMemcpyAsync(h->items.ptr, items.data(), sizeof(int4) * items.size(), hipMemcpyHostToDevice, h->stream));
}

// what every launch of a half-step has in common
IalsParams side_params(mi355rec_ials *h, bool users) {
    IalsParams p{};
    p.k = h->k;
    p.reg = h->reg;
    p.ptr = users ? h->u_ptr.ptr : h->i_ptr.ptr;
    p.idx = users ? h->u_idx.ptr : h->i_idx.ptr;
    p.conf = users ? h->u_conf.ptr : h->i_conf.ptr;
    p.Y = users ? h->V.ptr : h->U.ptr;
    p.G = h->G.ptr;
    p.X = users ? h->U.ptr : h->V.ptr;
    p.part_buf = h->part_buf.ptr;         // (ensure_parts has run; items and sys_slot: whoever uploads them, the buffers may move)
    p.part_count = h->part_count.ptr;
    p.queue = h->queue.ptr;
    p.phases = h->phases.ptr;
    return p;
}

// one launch, a workgroup per compute unit pulling the work items from the queue
void run_one_kernel(mi355rec_ials *h, IalsParams p) {
    upload_items(h, h->work.items);
    p.items = h->items.ptr;
    p.n_local = (int)h->work.items.size();
    MI_HIP(hipMemsetAsync(h->queue.ptr, 0, sizeof(unsigned), h->stream));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    h->dispatch_timers.reserve(h->dispatch_timers.used + 1);
    h->dispatch_timers.next(e0, e1, 1 << 30);
    launch_rows(h, p, std::min(p.n_local, multiprocessor_count()), e0, e1);
    MI_HIP(hipGetLastError());
}

// Two-stage epochs (ials_row_kernel STAGE 1, ials_solve_kernel): the rows of the half-step, in cost order, in batches whose systems
// fit the buffer (MI355REC_IALS_SYSTEM_GIB, default 8: 43 000 rows at k = 200); per batch one launch builds the systems (work items =
// the batch's rows and parts, still most expensive first) and one solves them, two workgroups per CU.  Same arithmetic as the
// one-kernel epoch (tests/test_ials_gpu.py::test_two_stage_epochs_equal_one_kernel_epochs: 1e-12).
void run_two_stage(mi355rec_ials *h, IalsParams p, int n_side) {
    const int n_local = (int)h->work.rows.size(), grid_cap = multiprocessor_count();
    const int per_batch = (int)std::min<size_t>((size_t)std::min(std::max(1, n_local), batch_rows(h)), h->systems.count / slab_doubles(h->k, true));
    const BatchPlan plan = plan_batches(h->work.rows, h->work.items, per_batch, n_side);
    upload_items(h, plan.items);
    if (h->sys_slot.count < plan.sys_slot.size()) h->sys_slot.alloc(plan.sys_slot.size() + 1024);
    MI_HIP(hipMemcpyAsync(h->sys_slot.ptr, plan.sys_slot.data(), sizeof(int) * plan.sys_slot.size(), hipMemcpyHostToDevice, h->stream));
    MI_HIP(hipStreamSynchronize(h->stream));         // (`plan` is a local)
    h->dispatch_timers.reserve(h->dispatch_timers.used + 2 * (int)plan.batches.size());
    p.systems = h->systems.ptr;
    p.same_panel_wave = h->knobs.same_panel_wave;
    for (const Batch &b : plan.batches) {
        for (int stage = 1; stage <= 2; ++stage) {
            p.items = h->items.ptr + (stage == 1 ? b.gram_off : b.solve_off);
            p.sys_slot = h->sys_slot.ptr + (stage == 1 ? b.gram_off : b.solve_off);
            p.n_local = stage == 1 ? b.gram_n : b.solve_n;
            MI_HIP(hipMemsetAsync(h->queue.ptr, 0, sizeof(unsigned), h->stream));
            hipEvent_t e0 = nullptr, e1 = nullptr;
            h->dispatch_timers.next(e0, e1, 1 << 30);
            if (stage == 1) launch_gram_stage(h, p, std::min(p.n_local, grid_cap), e0, e1);
            else launch_solve(h, p, std::min(p.n_local, 2 * grid_cap), e0, e1);
            MI_HIP(hipGetLastError());
        }
    }
}

// MI355REC_IALS_PHASES=1: the kernels' shader-clock totals of the half-step that was just queued (waits for it)
void print_phases(mi355rec_ials *h, bool users) {
    unsigned long long ph[8];
    MI_HIP(hipMemcpyAsync(ph, h->phases.ptr, sizeof(ph), hipMemcpyDeviceToHost, h->stream));
    MI_HIP(hipStreamSynchronize(h->stream));
    fprintf(stderr, "[ials phases] %s half: %llu rows; shader cycles per row: base %.0f, Gramian %.0f, Cholesky %.0f (diagonal tiles %.0f, panel solves %.0f, "
                    "trailing updates of wavefront 0 %.0f), back-substitution %.0f\n",
            users ? "user" : "item", ph[4], (double)ph[0] / ph[4], (double)ph[1] / ph[4], (double)ph[2] / ph[4], (double)ph[5] / ph[4], (double)ph[6] / ph[4],
            (double)ph[7] / ph[4], (double)ph[3] / ph[4]);
    MI_HIP(hipMemsetAsync(h->phases.ptr, 0, sizeof(ph), h->stream));
}

// Solve the rows [r0, r1) of one side.
void half_step(mi355rec_ials *h, bool users, int r0, int r1) {
    const int n_side = users ? h->n_users : h->n_items, n_other = users ? h->n_items : h->n_users;
    MI_REQUIRE(r0 >= 0 && r1 <= n_side && r0 <= r1, "row range [%d,%d) outside [0,%d)", r0, r1, n_side);
    launch_gram(h, users ? h->V.ptr : h->U.ptr, n_other);
    h->work = plan_work_items((users ? h->u_ptr_host : h->i_ptr_host).data(), users ? h->user_order : h->item_order, r0, r1, h->k, h->knobs);
    const int n_local = (int)h->work.rows.size();
    if (n_local == 0) return;
    h->n_split_rows = h->work.n_split;
    h->n_part_items = h->work.part_slots;
    // (no memory for 64 systems: the one-kernel epoch)
    const bool two_stage = two_stage_applies(h->k, h->knobs) && ensure_systems(h, n_local);
    ensure_parts(h, h->work.part_slots, two_stage);
    const IalsParams p = side_params(h, users);
    if (two_stage) run_two_stage(h, p, n_side);
    else run_one_kernel(h, p);
    if (h->phases.ptr) print_phases(h, users);
    const HalfStepWork done = half_step_work(h->work.nnz_rows, n_local, n_other, h->k);
    h->flops_acc += done.flops;
    h->bytes_acc += done.bytes;
    h->rows_acc += n_local;
    h->launches_acc += 1;
}

// `rows`: the longest half-step the call will run
void begin_call(mi355rec_ials *h, int rows) {
    h->knobs = read_ials_knobs();
    // (the buffer of the two-stage epochs is allocated here, before the call's clock starts: 8 GiB of hipMalloc took 0.4 s of the
    // first epoch's "call_ms" when half_step did it)
    if (two_stage_applies(h->k, h->knobs)) (void)ensure_systems(h, rows);
    h->dispatch_timers.reset();
    h->flops_acc = h->bytes_acc = 0;
    h->rows_acc = h->launches_acc = 0;
    h->timer.start(h->stream);
}

// the stats of what the call has run so far (the stream has been waited for)
void fill_stats(mi355rec_ials *h) {
    h->stats.call_ms = h->timer.elapsed_ms();
    h->stats.kernel_ms = h->dispatch_timers.total_ms();
    h->stats.n_timed = h->dispatch_timers.used;
    h->stats.n_launches = h->launches_acc;
    h->stats.n_units = h->rows_acc;
    h->stats.algorithmic_bytes = h->bytes_acc;
    h->stats.algorithmic_flops = h->flops_acc;
}

void end_call(mi355rec_ials *h, bool sync) {
    h->timer.stop(h->stream);
    if (!sync) return;
    MI_HIP(hipStreamSynchronize(h->stream));
    fill_stats(h);
    h->stats.loss = 0;
}

// item-major view of the confidence matrix (the reference keeps C_csc, IALSRecommender.py:106), built on the device
void build_item_view(mi355rec_ials *h) {
    hipStream_t s = h->stream;
    const size_t nnz = h->nnz;
    DeviceBuffer<int> cnt, cursor;
    cnt.alloc_zero((size_t)h->n_items, s);
    cursor.alloc((size_t)h->n_items);
    h->i_ptr.alloc((size_t)h->n_items + 1);
    h->i_idx.alloc(nnz);
    h->i_conf.alloc(nnz);
    const int eb = 256, eg = (int)std::min<size_t>((nnz + eb - 1) / eb, 4096);
    hipLaunchKernelGGL(ials_count_kernel, dim3(eg), dim3(eb), 0, s, h->u_idx.ptr, nnz, cnt.ptr);
    hipLaunchKernelGGL(ials_scan_kernel, dim3(1), dim3(1024), 0, s, cnt.ptr, h->i_ptr.ptr, cursor.ptr, h->n_items);
    hipLaunchKernelGGL(ials_scatter_kernel, dim3(div_up((int64_t)h->n_users * 64, 256)), dim3(256), 0, s, h->u_ptr.ptr,
                       h->u_idx.ptr, h->u_conf.ptr, h->n_users, cursor.ptr, h->i_idx.ptr, h->i_conf.ptr);
    MI_HIP(hipGetLastError());
    h->i_ptr_host.resize((size_t)h->n_items + 1);
    h->i_ptr.download(h->i_ptr_host.data(), (size_t)h->n_items + 1, s);
    MI_HIP(hipStreamSynchronize(s));                 // (cnt and cursor are locals; the caller reads i_ptr_host)
}

// rows of a CSR pointer, longest profile first
std::vector<int> by_length(const std::vector<int> &ptr, int n) {
    std::vector<int> o(n);
    std::iota(o.begin(), o.end(), 0);
    std::stable_sort(o.begin(), o.end(), [&](int a, int b) { return ptr[a + 1] - ptr[a] > ptr[b + 1] - ptr[b]; });
    return o;
}

}  // namespace

extern "C" int mi355rec_ials_create(mi355rec_ials_t *out, int32_t n_users, int32_t n_items, int32_t n_factors, double reg,
                                    const int32_t *indptr, const int32_t *indices, const float *confidence, const double *U0,
                                    const double *V0) {
    return guarded([&] {
        MI_REQUIRE(out && indptr && indices && confidence && V0, "NULL argument");
        MI_REQUIRE(n_users > 0 && n_items > 0, "empty URM");
        MI_REQUIRE(n_factors >= 1, "num_factors must be >= 1");
        if (n_factors > 255)   // 16 x 16 tiles of 16 (the rhs row included): 17 tiles per wavefront; the search space stops at 200
            fail(MI355REC_E_UNSUPPORTED, "num_factors = %d: the register-resident solver covers num_factors <= 255", n_factors);
        ensure_device();
        std::unique_ptr<mi355rec_ials> h(new mi355rec_ials());
        h->n_users = n_users;
        h->n_items = n_items;
        h->k = n_factors;
        h->reg = reg;
        h->nnz = (size_t)indptr[n_users];
        MI_REQUIRE(h->nnz > 0, "URM has no interactions");
        h->open(1);
        h->dispatch_timers.reserve(8);
        hipStream_t s = h->stream;
        h->u_ptr.upload(indptr, (size_t)n_users + 1, s);
        h->u_idx.upload(indices, h->nnz, s);
        h->u_conf.upload(confidence, h->nnz, s);
        const size_t nu = (size_t)n_users * h->k, ni = (size_t)n_items * h->k;
        if (U0) h->U.upload(U0, nu, s); else h->U.alloc_zero(nu, s);
        h->V.upload(V0, ni, s);
        h->G.alloc((size_t)h->k * h->k);
        h->queue.alloc(1);
        if (read_ials_knobs().phases) h->phases.alloc_zero(8, s);
        h->u_ptr_host.assign(indptr, indptr + n_users + 1);
        build_item_view(h.get());
        h->user_order = by_length(h->u_ptr_host, n_users);
        h->item_order = by_length(h->i_ptr_host, n_items);
        *out = h.release();
    });
}

extern "C" int mi355rec_ials_run_epochs(mi355rec_ials_t h, int32_t n_epochs) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL handle");
        MI_REQUIRE(n_epochs >= 0, "n_epochs must be >= 0");
        ensure_device();
        ReleaseScope scope(h->stream);
        h->dispatch_timers.reserve(2 * std::max(1, n_epochs));
        begin_call(h, std::max(h->n_users, h->n_items));
        for (int e = 0; e < n_epochs; ++e) {
            half_step(h, true, 0, h->n_users);      // fit user factors against V     (IALSRecommender.py:141-152)
            half_step(h, false, 0, h->n_items);     // then item factors against the UPDATED U (:156-166)
        }
        end_call(h, true);
    });
}

extern "C" int mi355rec_ials_user_half(mi355rec_ials_t h, int32_t u0, int32_t u1) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL handle");
        ensure_device();
        ReleaseScope scope(h->stream);
        h->dispatch_timers.reserve(2);
        begin_call(h, std::max(0, u1 - u0));
        half_step(h, true, u0, u1);
        end_call(h, false);
    });
}

extern "C" int mi355rec_ials_item_half(mi355rec_ials_t h, int32_t i0, int32_t i1) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL handle");
        ensure_device();
        ReleaseScope scope(h->stream);
        h->dispatch_timers.reserve(2);
        begin_call(h, std::max(0, i1 - i0));
        half_step(h, false, i0, i1);
        end_call(h, false);
    });
}

extern "C" int mi355rec_ials_device_factors(mi355rec_ials_t h, double **d_U, double **d_V) {
    return guarded([&] {
        MI_REQUIRE(h && d_U && d_V, "NULL argument");
        *d_U = h->U.ptr;
        *d_V = h->V.ptr;
    });
}

extern "C" int mi355rec_ials_sync(mi355rec_ials_t h) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL handle");
        ensure_device();
        MI_HIP(hipStreamSynchronize(h->stream));
        fill_stats(h);                              // (a loss the stats held before stays)
    });
}

extern "C" int mi355rec_ials_get_factors(mi355rec_ials_t h, double *U, double *V) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL handle");
        ensure_device();
        if (U) h->U.download(U, (size_t)h->n_users * h->k, h->stream);
        if (V) h->V.download(V, (size_t)h->n_items * h->k, h->stream);
        MI_HIP(hipStreamSynchronize(h->stream));
    });
}

// (the conversion kernel is handoff.hip's: this file's device code is the epoch's alone)
extern "C" int mi355rec_scorer_update_from_ials(mi355rec_scorer_t scorer, mi355rec_ials_t h) {
    return guarded([&] {
        MI_REQUIRE(scorer && h, "NULL handle");
        hand_off_check(scorer, "IALS", h->n_users, h->n_items, h->k, 0);
        ensure_device();
        const size_t nu = (size_t)h->n_users * h->k, ni = (size_t)h->n_items * h->k;
        hand_off_begin(scorer, h->stream);
        f64_to_f32_enqueue(h->U.ptr, scorer->U.ptr, nu, h->stream);
        f64_to_f32_enqueue(h->V.ptr, scorer->V.ptr, ni, h->stream);
        hand_off_end(scorer, h->stream, 12.0 * (double)(nu + ni), 2);
    });
}

extern "C" int mi355rec_ials_schedule_info(mi355rec_ials_t h, int32_t *n_split_rows, int32_t *n_parts) {
    return guarded([&] {
        MI_REQUIRE(h && n_split_rows && n_parts, "NULL argument");
        *n_split_rows = h->n_split_rows;
        *n_parts = h->n_part_items;
    });
}

extern "C" int mi355rec_ials_get_stats(mi355rec_ials_t h, mi355rec_stats *stats) { return handle_get_stats(h, stats); }

extern "C" void mi355rec_ials_destroy(mi355rec_ials_t h) { handle_destroy(h); }
