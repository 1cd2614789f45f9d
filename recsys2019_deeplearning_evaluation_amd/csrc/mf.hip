// mf.hip -- BPR-MF, FunkSVD and AsySVD mini-batch SGD epochs on MI355X (gfx950).
//
// Replaces MatrixFactorization/Cython/MatrixFactorization_Cython_Epoch.pyx (reference):
//   epochIteration_Cython_BPR_SGD :580-649, epochIteration_Cython_FUNK_SVD_SGD :286-361,
//   sampleBPR_Cython :940-985, sampleMSE_Cython :878-935, _add_*_sample_in_minibatch :737-766,
//   _apply_minibatch_updates_to_latent_factors :770-829, adaptive_gradient :835-873, ASY_SVD :393-541.
//
// Design.  The reference's mini-batch rule -- every gradient of a batch is taken against the
// start-of-batch factors, the gradients of a row are summed, the sum is applied once -- has two consequences:
//   (1) the samples of a batch are independent, and
//   (2) the sample stream does not depend on the factors, so everything about WHO touches WHICH row WHEN is known
//       before the first mini-batch runs.
// Round 1 used (1) only: a scatter kernel (float atomics into accumulators, first-toucher flags) and an apply kernel per
// mini-batch, i.e. two dependent launches and five dependent memory round trips per batch (10.2 us per batch of 1000).
// This version uses (2) as well and turns the batch into ONE gather kernel with no atomics, no flags and no
// accumulators:
//   mf_sample_kernel   one thread per sample of the epoch (counter-based RNG, binary-search rejection) -- or, for an epoch that goes
//                      through one in-LDS schedule, the same draw inside that schedule's workgroups (schedule_draws);
//   schedule           the epoch's (row, batch) incidences are grouped (in-LDS radix sort per mini-batch, or one rocPRIM sort of
//                      the whole stream) into TASKS: one task per row touched
//                      in a batch, holding the list of that batch's samples which touch the row.  Because every
//                      row's tasks are ordered by batch, the VERSION of a row each sample must read is static: factor
//                      rows live in two buffers, version v of a row in buffer (v & 1); a task reads version v of
//                      every row it needs and writes version v + 1 of its own row into the other buffer, which no
//                      reader of the same batch looks at.  Parities are baked into the sample records;
//   mf_batch_kernel    one wavefront per task: for each sample of the list, gather the 3 (BPR) / 2 (FunkSVD) rows at
//                      their parities, x_uij by DPP / v_permlane swap reduction inside a LPR-lane group (16-byte
//                      loads; a 64-lane wavefront works on 64/LPR samples at a time), own-row gradient summed in
//                      registers in sample order (deterministic), then mean over batch_size, optimiser, += lr * step,
//                      one store of the new row version.
// One dependent launch and three dependent memory round trips per mini-batch (task header -> rows -> store).
// Round 3: rows touched by ONE sample of the mini-batch (most of them) no longer get tasks of their own -- the sample's user
// task updates them too (fused sample tasks), and neighbouring single-sample tasks share a wavefront (pair tasks): 7 row
// transfers per sample instead of 12, HBM traffic 1.22 x the algorithmic 24 k bytes (was 1.84 x); mf_group_batch_kernel runs
// mini-batch b of R independent models as one grid (mi355rec_mf_group_*).  The arithmetic type is the storage type: float32 for plain sgd (north_star),
// float64 factors + moments for adagrad / rmsprop / adam, whose per-component normalisation amplifies float32 rounding
// to O(lr); outputs are float32 either way.
// There is no dense contraction here, hence no MFMA.
#include "common.h"
#include "score.h"
#include "asy_estimate.h"
#include "asy_estimate_plan.h"
#include "sampling.cuh"
#include "wave.cuh"

#include <rocprim/rocprim.hpp>

#include <memory>

// One translation unit, split by stage: mf_plan.h holds every decision as host-only arithmetic on plain numbers (and the constants the
// kernels share with it), the four .cuh headers the device code (parameters + optimiser step + sampler | schedules | mini-batch
// kernels | AsySVD); this file holds the handles, the launches, the graphs and the C ABI.
#include "mf_plan.h"
#include "mf_core.cuh"
#include "mf_schedule.cuh"
#include "mf_batch.cuh"
#include "mf_asy.cuh"


using namespace mi355rec;

struct mi355rec_mf : Handle {
    mi355rec_mf_config cfg{};
    int n_users = 0, n_items = 0, k = 0;
    int n_u_rows = 0;                 // rows of U: n_users, or n_items for AsySVD
    bool f64 = false;                 // storage / arithmetic type of factors and moments
    size_t nnz = 0;
    DeviceBuffer<int> indptr, indices;
    DeviceBuffer<float> data, stage;
    // T-typed arrays (float or double by `f64`), held as bytes
    DeviceBuffer<unsigned char> U[2], V[2], bu[2], bi[2], c1U, c2U, c1V, c2V, c1_bu, c2_bu, c1_bi, c2_bi;
    DeviceBuffer<unsigned char> mu_state, mu_acc, asy_mu, asy_c_mu;
    DeviceBuffer<unsigned char> par;
    DeviceBuffer<double> loss_slots;
    DeviceBuffer<MfState> state;
    DeviceBuffer<unsigned long long> ticks;         // MI355REC_MF_TICKS: the mini-batch kernel's phase stamps
    DeviceBuffer<int> asy_order;                    // mi355rec_mf_asy_user_factors: the users longest profile first, made by its first call
    long long batches_done = 0;      // batches executed since create (device state mirrors this)
    long long last_call_samples = 0; // samples in the stream buffer after the last native call
    int max_timed = 0;
    std::vector<double> host_loss;

    // the sample stream and what every schedule makes of it: task headers and records (sized by BufferPlan)
    struct StreamBuffers {
        DeviceBuffer<int> su, si, sj;
        DeviceBuffer<float> sr;
        DeviceBuffer<TaskHeader> tasks;
        DeviceBuffer<int4> recs, slot_recs;
        size_t capacity = 0;             // samples
        long long batch_capacity = 0;    // mini-batches the task arrays can hold
    } buf;
    // the radix-sort schedule of a whole stream
    struct RadixSchedule {
        DeviceBuffer<unsigned long long> keys, keys_sorted;
        DeviceBuffer<int> slots, slots_sorted, head, head_scan, task_at, batch_count;
        DeviceBuffer<unsigned char> spar, cub_tmp;
        size_t cub_tmp_bytes = 0;
        size_t capacity = 0;             // samples its buffers hold
    } radix;
    // the in-LDS schedule
    struct LdsSchedule {
        bool fast_schedule = false;              // available to this handle (cached: see MfShape::fast_schedule)
        bool bit_rows = false, bit_rows_decided = false;      // bit rows in place of the bitmap (cached like fast_schedule, decided once)
        DeviceBuffer<unsigned> touched;          // (row, mini-batch) bitmap: only without bit rows
        DeviceBuffer<unsigned> bit_rows_buf;     // [mini-batches of one schedule][row words]
        DeviceBuffer<int> sorted_slot, qtask, used;
        DeviceBuffer<unsigned long long> ticks;  // MI355REC_MF_TICKS: the sort kernel's phase stamps
    } lds;
    // exact multi-GPU mode: this rank's share of every mini-batch and the exchange slabs
    struct Shard {
        DeviceBuffer<unsigned char> send, recv;
        int rank = -1, world = 0, slots_per_rank = 0;
        long long batches = 0;
    } shard;
    // one native epoch: sampler, schedule, n_batches mini-batch kernels -- in graphs of up to GRAPH_SEGMENT mini-batches each
    struct Graphs {
        std::vector<hipGraphExec_t> epoch;
        bool failed = false;
    } graphs;

    void drop_graphs() {
        for (hipGraphExec_t g : graphs.epoch) (void)hipGraphExecDestroy(g);
        graphs.epoch.clear();
    }
    ~mi355rec_mf() { shutdown([&] { drop_graphs(); }); }
};

namespace {

// the plain numbers mf_plan.h decides on (taken when needed: a call may set lds.fast_schedule on its way)
MfShape shape_of(const mi355rec_mf *h) {
    MfShape s;
    s.algorithm = h->cfg.algorithm;
    s.n_users = h->n_users;
    s.n_items = h->n_items;
    s.nnz = (long long)h->nnz;
    s.k = h->k;
    s.f64 = h->f64;
    s.batch_size = h->cfg.batch_size;
    s.sharded = h->shard.rank >= 0;
    s.fast_schedule = h->lds.fast_schedule;
    s.bit_rows = h->lds.bit_rows;
    return s;
}

template <class T> T *as(const DeviceBuffer<unsigned char> &b) { return reinterpret_cast<T *>(b.ptr); }

// One launch: with per-dispatch events when `e0` is set, else the plain (capturable) form.
template <class... P, class... A>
void launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1, const A &...args) {
    if (e0) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, s, e0, e1, 0, static_cast<P>(args)...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, s, static_cast<P>(args)...);
}

// `enqueue`'s launches on `s` as an executable graph; null on any failure (the error is cleared: plain launches remain correct, only
// slower)
template <class F>
hipGraphExec_t capture_graph(hipStream_t s, F &&enqueue) {
    hipGraph_t g = nullptr;
    hipGraphExec_t exec = nullptr;
    hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        try {
            enqueue();
        } catch (...) {
            (void)hipStreamEndCapture(s, &g);
            if (g) (void)hipGraphDestroy(g);
            (void)hipGetLastError();
            return nullptr;
        }
        e = hipStreamEndCapture(s, &g);
    }
    if (e == hipSuccess) e = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    if (g) (void)hipGraphDestroy(g);
    if (e == hipSuccess) return exec;
    (void)hipGetLastError();
    return nullptr;
}

template <class T>
void fill_config(const mi355rec_mf *h, MfParams<T> &p) {
    const auto &c = h->cfg;
    p.n_users = h->n_users; p.n_items = h->n_items; p.k = h->k; p.batch_size = c.batch_size;
    p.use_bias = c.use_bias && c.algorithm != MI355REC_MF_BPR;
    p.sgd_mode = c.sgd_mode;
    p.sample_negatives = c.negative_interactions_quota != 0.0;
    p.lr = (T)c.learning_rate; p.user_reg = (T)c.user_reg; p.item_reg = (T)c.item_reg; p.bias_reg = (T)c.bias_reg;
    p.positive_reg = (T)c.positive_reg; p.negative_reg = (T)c.negative_reg;
    p.inv_batch = (T)1 / (T)c.batch_size;
    p.quota = (float)c.negative_interactions_quota;
    p.gamma = (T)c.gamma; p.beta_1 = (T)c.beta_1; p.beta_2 = (T)c.beta_2;
    p.one_m_gamma = (T)(1.0 - c.gamma); p.one_m_beta_1 = (T)(1.0 - c.beta_1); p.one_m_beta_2 = (T)(1.0 - c.beta_2);
    p.beta_1_d = c.beta_1; p.beta_2_d = c.beta_2;
    p.seed = c.random_seed;
}

template <class T>
void fill_params(mi355rec_mf *h, MfParams<T> &p) {
    const MfShape s = shape_of(h);
    fill_config(h, p);
    p.tasks_per_batch = tasks_per_batch(s);
    p.indptr = h->indptr.ptr; p.indices = h->indices.ptr; p.data = h->data.ptr;
    p.U0 = as<T>(h->U[0]); p.U1 = as<T>(h->U[1]); p.V0 = as<T>(h->V[0]); p.V1 = as<T>(h->V[1]);
    p.bu0 = as<T>(h->bu[0]); p.bu1 = as<T>(h->bu[1]); p.bi0 = as<T>(h->bi[0]); p.bi1 = as<T>(h->bi[1]);
    p.c1U = as<T>(h->c1U); p.c2U = as<T>(h->c2U); p.c1V = as<T>(h->c1V); p.c2V = as<T>(h->c2V);
    p.c1_bu = as<T>(h->c1_bu); p.c2_bu = as<T>(h->c2_bu); p.c1_bi = as<T>(h->c1_bi); p.c2_bi = as<T>(h->c2_bi);
    p.mu_state = reinterpret_cast<MuState<T> *>(h->mu_state.ptr);
    p.mu_acc = as<T>(h->mu_acc);
    p.asy_mu = as<T>(h->asy_mu); p.asy_c_mu = as<T>(h->asy_c_mu);
    p.par = h->par.ptr;
    p.loss_slots = h->loss_slots.ptr; p.state = h->state.ptr;
    p.su = h->buf.su.ptr; p.si = h->buf.si.ptr; p.sj = h->buf.sj.ptr; p.sr = h->buf.sr.ptr;
    p.samples_per_epoch = batches_per_epoch(s) * (long long)s.batch_size;
    p.tasks = h->buf.tasks.ptr; p.recs = h->buf.recs.ptr;
    p.slot_recs = h->buf.slot_recs.ptr;
    p.slot_rec_stride = slot_rec_stride(s);
    p.used = nullptr;                       // (only the group's launch reads it: group_member_table)
    p.ticks = h->ticks.ptr;
    p.wg_base = 0;
    p.wg_stride = 1;
}

// ---- kernel selection: the instance comes from mf_plan.h's row-width table ------------------------------------------------------------
template <int ALGO, class T, int VEC, int LPR, int KI>
void launch_batch_as(mi355rec_mf *h, const MfParams<T> &p, int grid, int batch_local, hipEvent_t e0, hipEvent_t e1) {
    // what the header's address is made of goes in front of the parameter block (see mf_batch_kernel); constants of the launch, and
    // of the captured graph node, like batch_local
    const TaskHeader *hdr = p.tasks + (size_t)batch_local * p.tasks_per_batch;
    const int4 *slot = p.slot_recs + (size_t)batch_local * p.slot_rec_stride;
    const int stamps = p.ticks != nullptr;
    auto go = [&](auto kernel) {
        launch(kernel, dim3(grid), dim3(256), 0, h->stream, e0, e1, hdr, slot, p.tasks_per_batch, p.wg_base, p.wg_stride, stamps, p, batch_local);
    };
    if (p.sgd_mode == MI355REC_SGD) go(mf_batch_kernel<ALGO, T, VEC, LPR, KI, true>);
    else go(mf_batch_kernel<ALGO, T, VEC, LPR, KI, false>);
}

template <int ALGO, class T>
void launch_batch(mi355rec_mf *h, const MfParams<T> &p, int batch_local, bool timed, int wg_count = -1) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int grid = wg_count >= 0 ? wg_count : div_up(p.tasks_per_batch, 4);       // (p.wg_base names the first one)
    if (grid == 0) return;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (timed) h->dispatch_timers.next(e0, e1, h->max_timed);
    const bool found = dispatch_width(row_width(h->k, sizeof(T) == 8).klass, [&](auto lpr, auto ki) {
        launch_batch_as<ALGO, T, VEC, decltype(lpr)::value, decltype(ki)::value>(h, p, grid, batch_local, e0, e1);
    });
    if (!found) launch(mf_batch_generic_kernel<ALGO, T>, dim3(grid), dim3(256), 0, h->stream, e0, e1, p, batch_local);
}

template <int ALGO, class T>
void launch_group_batch(hipStream_t s, const MfParams<T> *table, int klass, int wgs, int n_models, int batch_local, bool plain_sgd,
                        hipEvent_t e0, hipEvent_t e1) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const dim3 grid(wgs, n_models);
    // (a 64-VGPR build for 8 wavefronts per SIMD was measured twice and is gone: 20 spilled registers, 422 M against 678 M samples/s)
    dispatch_width(klass, [&](auto lpr, auto ki) {
        constexpr int LPR = decltype(lpr)::value, KI = decltype(ki)::value;
        if (plain_sgd) launch(mf_group_batch_kernel<ALGO, T, VEC, LPR, KI, true>, grid, dim3(256), 0, s, e0, e1, table, batch_local);
        else launch(mf_group_batch_kernel<ALGO, T, VEC, LPR, KI, false>, grid, dim3(256), 0, s, e0, e1, table, batch_local);
    });
}

template <class T>
void launch_sampler(mi355rec_mf *h, const MfParams<T> &p, hipStream_t on = nullptr) {
    const int grid = div_up(p.samples_per_epoch, 256);
    hipStream_t s = on ? on : h->stream;
    if (h->cfg.algorithm == MI355REC_MF_BPR) hipLaunchKernelGGL((mf_sample_kernel<MI355REC_MF_BPR, T>), dim3(grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((mf_sample_kernel<MI355REC_MF_FUNK_SVD, T>), dim3(grid), dim3(256), 0, s, p);
    hipLaunchKernelGGL(mf_epoch_advance_kernel, dim3(1), dim3(64), 0, s, p.state);
}

// ---- schedules ------------------------------------------------------------------------------------------------------------------
size_t sched_lds(int np) { return sched_lds_bytes(np, sched_sort_storage_bytes(np)); }
// ... of a launch: with the mini-batch's bit row behind the flags
size_t sched_lds(const FastSchedParams &f) { return sched_lds(f.np) + (f.bit_rows ? sizeof(unsigned) * (size_t)f.row_words : 0); }

// what bit_rows_fit() needs of the current device: the LDS a workgroup may have, and what the sort kernels declare statically
// (the block scan's scratch; the one-model and the group kernel share the body)
struct SchedLdsLimits {
    size_t limit, static_bytes;
};
SchedLdsLimits sched_lds_limits() {
    static SchedLdsLimits cached[64] = {};
    int dev = 0, limit = 0;
    MI_HIP(hipGetDevice(&dev));
    if (dev >= 0 && dev < 64 && cached[dev].limit) return cached[dev];
    MI_HIP(hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    hipFuncAttributes one{}, group{};
    MI_HIP(hipFuncGetAttributes(&one, reinterpret_cast<const void *>(mf_sched_sort_kernel)));
    MI_HIP(hipFuncGetAttributes(&group, reinterpret_cast<const void *>(mf_group_sched_sort_kernel)));
    const SchedLdsLimits l{(size_t)std::max(limit, 0), std::max(one.sharedSizeBytes, group.sharedSizeBytes)};
    if (dev >= 0 && dev < 64) cached[dev] = l;
    return l;
}

// (everything a workgroup may have: the largest mini-batch without a bit row, and every bit row bit_rows_fit() lets through)
void set_sched_sort_attribute(const void *kernel, bool (&attr_set)[64]) {
    int dev = 0;
    MI_HIP(hipGetDevice(&dev));                 // the attribute is per DEVICE, not per process
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        const SchedLdsLimits l = sched_lds_limits();
        const size_t bytes = std::max(sched_lds(FAST_MAX_SLOTS), l.limit > l.static_bytes ? l.limit - l.static_bytes : 0);
        MI_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
}

FastSchedParams fast_sched_params(mi355rec_mf *h, const MfKnobs &knobs, long long n_samples) {
    const MfShape s = shape_of(h);
    const FastSchedNumbers n = fast_sched_numbers_bit_rows(s, knobs, sched_sort_storage_bytes(sched_np(tasks_per_batch(s))));
    FastSchedParams f;
    memset(&f, 0, sizeof(f));                   // (padding bytes included: the group compares tables bytewise)
    f.n_samples = n_samples;
    f.per = per_sample(s);
    f.n_users = h->n_users;
    f.n_entries = h->n_users + h->n_items;
    f.batch_size = h->cfg.batch_size;
    f.tasks_per_batch = tasks_per_batch(s);
    f.np = n.np; f.slot_bits = n.slot_bits; f.entry_bits = n.entry_bits; f.mid_bytes = n.mid_bytes;
    f.words = n.words; f.group = n.group; f.fuse = n.fuse; f.fill_all = n.fill_all;
    f.su = h->buf.su.ptr; f.si = h->buf.si.ptr; f.sj = h->buf.sj.ptr; f.sr = h->buf.sr.ptr;
    f.touched = h->lds.touched.ptr; f.par = h->par.ptr;
    f.row_words = n.row_words;
    f.bit_rows = n.bit_rows ? h->lds.bit_rows_buf.ptr : nullptr;
    f.sorted_slot = h->lds.sorted_slot.ptr; f.qtask = h->lds.qtask.ptr; f.used = h->lds.used.ptr;
    f.tasks = h->buf.tasks.ptr; f.recs = h->buf.recs.ptr; f.slot_recs = h->buf.slot_recs.ptr;
    f.ticks = h->lds.ticks.ptr;
    return f;
}

// the schedule's workgroups draw the epoch's samples themselves (schedule_draws)
template <class T>
void set_draw(FastSchedParams &f, const MfParams<T> &p) {
    f.draw = 1;
    f.advance_epoch = 1;
    f.bpr = f.per == 3;
    f.sample_negatives = p.sample_negatives;
    f.n_items = p.n_items;
    f.quota = p.quota;
    f.seed = p.seed;
    f.samples_per_epoch = p.samples_per_epoch;
    f.first_sample = 0;
    f.state = p.state;
    f.indptr = p.indptr; f.indices = p.indices; f.data = p.data;
}

void enqueue_fast_schedule(mi355rec_mf *h, const FastSchedParams &f, long long n_batches) {
    hipStream_t s = h->stream;
    static bool attr_set[64] = {};
    set_sched_sort_attribute(reinterpret_cast<const void *>(mf_sched_sort_kernel), attr_set);
    hipLaunchKernelGGL(mf_sched_sort_kernel, dim3((unsigned)n_batches), dim3(SCHED_THREADS), sched_lds(f), s, f);
    if (f.bit_rows) hipLaunchKernelGGL(mf_sched_parity_kernel, dim3(div_up(f.row_words, 64)), dim3(PARITY_THREADS), 0, s, f, (int)n_batches);
    hipLaunchKernelGGL(mf_sched_emit_kernel, dim3(div_up(f.batch_size, 256), (unsigned)n_batches), dim3(256), 0, s, f);
    if (!f.bit_rows) hipLaunchKernelGGL(mf_sched_finish_kernel, dim3(div_up(f.n_entries, 256)), dim3(256), 0, s, f);
}

SchedParams radix_sched_params(mi355rec_mf *h, const GeneralSched &g, long long n_samples) {
    const MfShape s = shape_of(h);
    const long long n = n_samples * per_sample(s);
    auto &r = h->radix;
    SchedParams sp{};
    sp.n_samples = n_samples;
    sp.per = per_sample(s);
    sp.n_users = h->n_users;
    sp.batch_size = h->cfg.batch_size;
    sp.batch_bits = g.batch_bits;
    sp.tasks_per_batch = tasks_per_batch(s);
    sp.su = h->buf.su.ptr; sp.si = h->buf.si.ptr; sp.sj = h->buf.sj.ptr; sp.sr = h->buf.sr.ptr;
    sp.keys = r.keys.ptr; sp.slots = r.slots.ptr;
    sp.keys_sorted = r.keys_sorted.ptr; sp.slots_sorted = r.slots_sorted.ptr;
    sp.head = r.head.ptr; sp.head_scan = r.head_scan.ptr; sp.task_at = r.task_at.ptr;
    sp.spar = r.spar.ptr; sp.par = h->par.ptr;
    sp.batch_count = g.by_rank ? nullptr : r.batch_count.ptr;
    // (the unsorted keys are dead after the sort: their buffer holds the first-incidence flags and their scan, n ints each)
    sp.slot_flag = reinterpret_cast<int *>(r.keys.ptr);
    sp.slot_rank = reinterpret_cast<int *>(r.keys.ptr) + n;
    sp.tasks = h->buf.tasks.ptr; sp.recs = h->buf.recs.ptr;
    return sp;
}

// Stream buffers -> tasks (all on the handle's stream, no host synchronisation: capturable).
void enqueue_schedule(mi355rec_mf *h, const MfKnobs &knobs, long long n_samples, long long n_batches) {
    const MfShape shape = shape_of(h);
    if (runs_fast_schedule(shape, knobs, n_batches)) {
        enqueue_fast_schedule(h, fast_sched_params(h, knobs, n_samples), n_batches);
        return;
    }
    hipStream_t s = h->stream;
    auto &r = h->radix;
    const GeneralSched g = general_sched(shape, n_batches);
    const SchedParams sp = radix_sched_params(h, g, n_samples);
    const long long n = n_samples * sp.per;
    MI_REQUIRE(g.fits, "sample stream too long for the schedule keys");
    MI_HIP(hipMemsetAsync(r.batch_count.ptr, 0, sizeof(int) * (size_t)n_batches, s));
    MI_HIP(hipMemsetAsync(h->buf.tasks.ptr, 0, sizeof(TaskHeader) * (size_t)n_batches * sp.tasks_per_batch, s));
    hipLaunchKernelGGL(mf_keys_kernel, dim3(div_up(n_samples, 256)), dim3(256), 0, s, sp);
    size_t bytes = r.cub_tmp_bytes;
    MI_HIP(rocprim::radix_sort_pairs(r.cub_tmp.ptr, bytes, r.keys.ptr, r.keys_sorted.ptr, r.slots.ptr, r.slots_sorted.ptr, (int)n, 0, g.end_bit, s));
    MI_HIP(hipMemsetAsync(sp.slot_flag, 0, sizeof(int) * (size_t)n, s));
    hipLaunchKernelGGL(mf_heads_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, sp);
    bytes = r.cub_tmp_bytes;
    MI_HIP(rocprim::inclusive_scan(r.cub_tmp.ptr, bytes, r.head.ptr, r.head_scan.ptr, (size_t)n, rocprim::plus<int>(), s));
    bytes = r.cub_tmp_bytes;
    MI_HIP(rocprim::exclusive_scan(r.cub_tmp.ptr, bytes, sp.slot_flag, reinterpret_cast<int *>(r.keys.ptr) + n, 0, (size_t)n, rocprim::plus<int>(), s));
    hipLaunchKernelGGL(mf_tasks_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, sp);
    hipLaunchKernelGGL(mf_recs_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, sp);
}

// the schedule a step of the stream walk asks for (StreamStep::sched)
template <class T>
void enqueue_step_schedule(mi355rec_mf *h, const MfKnobs &knobs, const MfParams<T> &p, const StreamStep &st) {
    if (st.sched == SCHED_WHOLE) {
        enqueue_schedule(h, knobs, st.sched_samples, st.sched_batches);
        return;
    }
    FastSchedParams f = fast_sched_params(h, knobs, st.sched_samples);
    if (st.sched == SCHED_DRAW) set_draw(f, p);
    f.su += st.sample_offset; f.si += st.sample_offset; f.sj += st.sample_offset; f.sr += st.sample_offset;     // (a part: a stream of its own)
    enqueue_fast_schedule(h, f, st.sched_batches);
}

// mini-batches first .. last - 1 of a stream of n_batches, with the schedules and stream ends that fall into that range
template <class T>
void enqueue_stream(mi355rec_mf *h, const MfKnobs &knobs, const MfParams<T> &p, long long n_samples, long long n_batches, bool timed,
                    long long first = 0, long long last = -1, bool draw = false) {
    const bool bpr = h->cfg.algorithm == MI355REC_MF_BPR;
    const long long span = schedule_span(shape_of(h), knobs, n_batches), B = h->cfg.batch_size;
    if (last < 0) last = n_batches;
    for (long long b = first; b < last; ++b) {
        const StreamStep st = stream_step(n_samples, n_batches, span, B, draw, b);
        if (st.sched != SCHED_NONE) enqueue_step_schedule(h, knobs, p, st);
        if (bpr) launch_batch<MI355REC_MF_BPR, T>(h, p, st.local, timed);
        else launch_batch<MI355REC_MF_FUNK_SVD, T>(h, p, st.local, timed);
        if (st.end_batches) hipLaunchKernelGGL(mf_stream_end_kernel<T>, dim3(1), dim3(64), 0, h->stream, p, st.end_batches);
    }
}

template <class T>
void enqueue_asy_steps(mi355rec_mf *h, const MfParams<T> &p, long long n_steps, bool timed) {
    for (long long first = 0; first < n_steps; first += ASY_CHUNK) {
        const int count = (int)std::min<long long>(ASY_CHUNK, n_steps - first);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (timed) h->dispatch_timers.next(e0, e1, h->max_timed);
        auto go = [&](auto kernel) { launch(kernel, dim3(1), dim3(1024), 0, h->stream, e0, e1, p, first, count); };
        if (h->k <= 64) go(mf_asy_kernel<T, 1>);
        else if (h->k <= 128) go(mf_asy_kernel<T, 2>);
        else go(mf_asy_kernel<T, 4>);
    }
}

// One native epoch as plain launches (the first `max_timed` mini-batch launches carry per-dispatch events when `timed`) -- or the
// part of it that holds mini-batches first .. last - 1: sampler and schedule go with the first part.
template <class T>
void enqueue_epoch(mi355rec_mf *h, const MfKnobs &knobs, const MfParams<T> &p, bool timed, long long first = 0, long long last = -1) {
    const MfShape s = shape_of(h);
    const bool draw = schedule_draws(s, knobs);
    if (first == 0 && !draw) launch_sampler(h, p);
    if (h->cfg.algorithm == MI355REC_MF_ASY_SVD) {
        enqueue_asy_steps(h, p, p.samples_per_epoch, timed);
        return;
    }
    enqueue_stream(h, knobs, p, p.samples_per_epoch, batches_per_epoch(s), timed, first, last, draw);
}

// Capture one epoch into graphs of up to GRAPH_SEGMENT mini-batches (once per handle; re-captured only if the stream buffers are
// re-allocated).
template <class T>
void ensure_epoch_graph(mi355rec_mf *h, const MfKnobs &knobs, const MfParams<T> &p) {
    if (!h->graphs.epoch.empty() || h->graphs.failed) return;
    const long long nb = graph_batches(shape_of(h));
    for (long long i = 0; i < graph_segments(nb); ++i) {
        const BatchRange r = graph_segment(nb, i);
        hipGraphExec_t exec = capture_graph(h->stream, [&] { enqueue_epoch(h, knobs, p, false, r.first, r.last); });
        if (!exec) {                 // remember and go on with plain launches
            h->drop_graphs();
            h->graphs.failed = true;
            return;
        }
        h->graphs.epoch.push_back(exec);
    }
}

// ---- buffers (what and how much: BufferPlan) ------------------------------------------------------------------------------------------
void alloc_radix_buffers(mi355rec_mf *h, const BufferPlan &b, size_t n_samples) {
    h->drop_graphs();
    const size_t n = b.incidences;
    MI_REQUIRE(b.incidences_fit, "sample stream too long (%zu incidences)", n);
    auto &r = h->radix;
    r.keys.alloc(n); r.keys_sorted.alloc(n);
    r.slots.alloc(n); r.slots_sorted.alloc(n);
    r.head.alloc(n); r.head_scan.alloc(n); r.task_at.alloc(n);
    r.spar.alloc(n);
    size_t sort_bytes = 0, scan_bytes = 0;
    MI_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, r.keys.ptr, r.keys_sorted.ptr, r.slots.ptr, r.slots_sorted.ptr, (int)n, 0, 64, h->stream));
    MI_HIP(rocprim::inclusive_scan(nullptr, scan_bytes, r.head.ptr, r.head_scan.ptr, (size_t)n, rocprim::plus<int>(), h->stream));
    r.cub_tmp_bytes = std::max(sort_bytes, scan_bytes) + 256;
    r.cub_tmp.alloc(r.cub_tmp_bytes);
    r.capacity = n_samples;
}

void alloc_task_tables(mi355rec_mf *h, const BufferPlan &b) {
    h->drop_graphs();
    h->radix.batch_count.alloc(b.batch_count);
    h->buf.tasks.alloc(b.tasks);
    MI_HIP(hipMemsetAsync(h->buf.tasks.ptr, 0, sizeof(TaskHeader) * b.tasks, h->stream));
    h->buf.recs.alloc(b.recs);
    h->lds.fast_schedule = b.fast1;
    h->buf.slot_recs.alloc_zero(b.slot_recs, h->stream);
    if (b.fast1) {
        h->lds.sorted_slot.alloc(b.sorted_slot);
        h->lds.qtask.alloc(b.qtask);
        h->lds.used.alloc(b.used);
        if (b.touched && !h->lds.touched.ptr) h->lds.touched.alloc_zero(b.touched, h->stream);
        if (h->lds.bit_rows_buf.count < b.bit_rows) h->lds.bit_rows_buf.alloc(b.bit_rows);      // (every row a stream reads, it has written)
    }
    h->buf.batch_capacity = b.table_batches;
}

// `whole_stream`: the caller schedules the stream in one piece whatever its length (group members, exact multi-GPU mode)
void ensure_stream_capacity(mi355rec_mf *h, const MfKnobs &knobs, size_t n_samples, long long n_batches, bool whole_stream = false) {
    // bit rows or the per-row bitmap: decided by the handle's first call that plans buffers, for good (both leave the same par[])
    if (!h->lds.bit_rows_decided && h->cfg.algorithm != MI355REC_MF_ASY_SVD) {
        const MfShape s = shape_of(h);
        if (fast_schedule_fits(s, knobs, 1)) {
            const SchedLdsLimits l = sched_lds_limits();
            h->lds.bit_rows = bit_rows_fit(s, knobs, sched_sort_storage_bytes(sched_np(tasks_per_batch(s))), l.static_bytes, l.limit);
        }
        h->lds.bit_rows_decided = true;
    }
    const BufferPlan b = buffer_plan_bit_rows(shape_of(h), knobs, n_samples, n_batches, whole_stream);
    if (h->buf.capacity < n_samples) {
        h->drop_graphs();       // they hold the old buffer addresses
        h->buf.su.alloc(n_samples);
        h->buf.si.alloc(n_samples);
        h->buf.sj.alloc(n_samples);
        h->buf.sr.alloc(n_samples);
        h->buf.capacity = n_samples;
    }
    if (b.asy) return;
    if (b.general && h->radix.capacity < n_samples) alloc_radix_buffers(h, b, n_samples);   // only for streams that schedule will actually see
    if (h->buf.batch_capacity < b.table_batches) alloc_task_tables(h, b);
}

// ---- calls ----------------------------------------------------------------------------------------------------------------------
void begin_call(mi355rec_mf *h) {
    MI_HIP(hipMemsetAsync(h->loss_slots.ptr, 0, sizeof(double) * h->loss_slots.count, h->stream));
    MI_HIP(hipMemsetAsync(&h->state.ptr->asy_loss, 0, sizeof(double), h->stream));
    h->dispatch_timers.reset();
}

// the sum of the loss slots, once everything on the handle's stream is done
double read_loss(mi355rec_mf *h) {
    h->host_loss.resize(h->loss_slots.count);
    h->loss_slots.download(h->host_loss.data(), h->loss_slots.count, h->stream);
    MI_HIP(hipStreamSynchronize(h->stream));
    double loss = 0;
    for (double v : h->host_loss) loss += v;
    return loss;
}

void finish_call(mi355rec_mf *h, long long n_samples, long long n_launches) {
    MI_HIP(hipGetLastError());
    double loss = read_loss(h);
    if (h->cfg.algorithm == MI355REC_MF_ASY_SVD) {
        MfState st{};
        MI_HIP(hipMemcpy(&st, h->state.ptr, sizeof(MfState), hipMemcpyDeviceToHost));
        loss = st.asy_loss;
    }
    h->stats.call_ms = h->timer.elapsed_ms();
    h->stats.kernel_ms = h->dispatch_timers.total_ms();
    h->stats.n_timed = h->dispatch_timers.used;
    h->stats.n_launches = n_launches;           // launches of the dominant (mini-batch) kernel
    h->stats.n_units = n_samples;
    h->stats.algorithmic_bytes = bytes_per_sample(shape_of(h)) * (double)n_samples;
    h->stats.algorithmic_flops = 0;
    h->stats.loss = loss;
}

template <class T>
void create_typed(mi355rec_mf *h, const void *U0, const void *V0) {
    hipStream_t s = h->stream;
    const auto &cfg = h->cfg;
    const size_t nu = (size_t)h->n_u_rows * h->k, ni = (size_t)h->n_items * h->k, ts = sizeof(T);
    for (int b = 0; b < 2; ++b) {
        h->U[b].upload(static_cast<const unsigned char *>(U0), nu * ts, s);
        h->V[b].upload(static_cast<const unsigned char *>(V0), ni * ts, s);
        h->bu[b].alloc_zero((size_t)h->n_users * ts, s);
        h->bi[b].alloc_zero((size_t)h->n_items * ts, s);
    }
    if (cfg.sgd_mode != MI355REC_SGD) {
        h->c1U.alloc_zero(nu * ts, s);
        h->c1V.alloc_zero(ni * ts, s);
        h->c1_bu.alloc_zero((size_t)h->n_users * ts, s);
        h->c1_bi.alloc_zero((size_t)h->n_items * ts, s);
        if (cfg.sgd_mode == MI355REC_ADAM) {
            h->c2U.alloc_zero(nu * ts, s);
            h->c2V.alloc_zero(ni * ts, s);
            h->c2_bu.alloc_zero((size_t)h->n_users * ts, s);
            h->c2_bi.alloc_zero((size_t)h->n_items * ts, s);
        }
    }
    h->mu_state.alloc_zero(3 * sizeof(MuState<T>), s);
    h->mu_acc.alloc_zero(3 * MU_SLOTS * ts, s);
    h->asy_mu.alloc_zero(ts, s);
    h->asy_c_mu.alloc_zero(2 * ts, s);
}

void check_config(const mi355rec_mf_config *cfg, int32_t n_users, int32_t n_items) {
    MI_REQUIRE(n_users > 0 && n_items > 0, "empty URM");
    MI_REQUIRE(cfg->algorithm >= MI355REC_MF_BPR && cfg->algorithm <= MI355REC_MF_ASY_SVD,
               "Value for 'algorithm_name' not recognized (%d)", cfg->algorithm);
    const bool asy = cfg->algorithm == MI355REC_MF_ASY_SVD;
    MI_REQUIRE(!asy || cfg->batch_size == 1, "Batch size other than 1 not supported for ASY_SVD");
    if (asy && cfg->n_factors > ASY_KMAX)
        fail(MI355REC_E_UNSUPPORTED, "ASY_SVD: n_factors = %d exceeds %d", cfg->n_factors, ASY_KMAX);
    MI_REQUIRE(cfg->sgd_mode >= MI355REC_SGD && cfg->sgd_mode <= MI355REC_ADAM, "Value for 'sgd_mode' not recognized (%d)",
               cfg->sgd_mode);
    MI_REQUIRE(cfg->n_factors >= 1, "n_factors must be >= 1");
    if (cfg->n_factors > 512) fail(MI355REC_E_UNSUPPORTED, "n_factors = %d exceeds 512", cfg->n_factors);
    MI_REQUIRE(cfg->batch_size >= 1, "batch_size must be >= 1");
    MI_REQUIRE(cfg->precision == MI355REC_F32 || cfg->precision == MI355REC_F64, "precision must be MI355REC_F32 or MI355REC_F64");
}

// what create allocates beside the factors: parities, tick buffers (MI355REC_MF_TICKS as this call sees it), loss slots, device state
void create_state(mi355rec_mf *h, const MfKnobs &knobs) {
    hipStream_t s = h->stream;
    const MfShape shape = shape_of(h);
    h->par.alloc_zero((size_t)h->n_users + h->n_items, s);
    if (knobs.ticks) {
        h->ticks.alloc_zero(tick_count(shape), s);
        h->lds.ticks.alloc_zero(sched_tick_count(), s);
    }
    h->loss_slots.alloc_zero(loss_slot_count(shape), s);
    h->state.alloc_zero(1, s);
    MfState init{};     // Adam's running beta powers start at beta^1 (.pyx:217-218)
    init.beta_1_power = h->cfg.beta_1;
    init.beta_2_power = h->cfg.beta_2;
    MI_HIP(hipMemcpyAsync(h->state.ptr, &init, sizeof(MfState), hipMemcpyHostToDevice, s));
    MI_HIP(hipStreamSynchronize(s));
}

template <class T>
void run_epochs_typed(mi355rec_mf *h, const MfKnobs &knobs, int n_epochs) {
    const long long B = h->cfg.batch_size;
    const long long per_epoch = batches_per_epoch(shape_of(h));
    ensure_stream_capacity(h, knobs, (size_t)(per_epoch * B), per_epoch);
    const MfShape s = shape_of(h);
    MfParams<T> p{};
    fill_params(h, p);
    begin_call(h);
    const long long timed = timed_epochs(h->max_timed, per_epoch, n_epochs);
    bool graph = use_graph(s, knobs, per_epoch, n_epochs, timed);
    if (graph) {
        ensure_epoch_graph(h, knobs, p);
        graph = !h->graphs.epoch.empty();
    }
    h->timer.start(h->stream);
    for (long long e = 0; e < n_epochs; ++e) {
        if (e < timed || !graph) enqueue_epoch(h, knobs, p, e < timed);
        else for (hipGraphExec_t g : h->graphs.epoch) MI_HIP(hipGraphLaunch(g, h->stream));
    }
    h->timer.stop(h->stream);
    h->batches_done += per_epoch * n_epochs;
    h->last_call_samples = n_epochs > 0 ? per_epoch * B : 0;
    finish_call(h, per_epoch * n_epochs * B, n_launches(s, per_epoch, n_epochs));
}

template <class T>
void run_samples_typed(mi355rec_mf *h, const MfKnobs &knobs, int64_t n) {
    const MfShape s = shape_of(h);
    const bool asy = h->cfg.algorithm == MI355REC_MF_ASY_SVD;
    MfParams<T> p{};
    fill_params(h, p);
    const long long n_batches = asy ? n : ceil_div(n, h->cfg.batch_size);      // (AsySVD: single-sample steps)
    begin_call(h);
    h->timer.start(h->stream);
    if (asy) enqueue_asy_steps(h, p, n, true);
    else enqueue_stream(h, knobs, p, n, n_batches, true);
    h->timer.stop(h->stream);
    h->batches_done += n_batches;
    finish_call(h, n, n_launches(s, n_batches, 1));
}

// O = float (the float32 matrices north_star speaks of) or double (what the reference's getters return, .pyx:685-702: exact when
// the device state is float64)
template <class T, class O>
void get_factors_typed(mi355rec_mf *h, O *U, O *V, O *bu, O *bi, O *mu) {
    hipStream_t s = h->stream;
    MfParams<T> p{};
    fill_params(h, p);
    const size_t nu = (size_t)h->n_u_rows * h->k, ni = (size_t)h->n_items * h->k;
    const size_t need = std::max(std::max(nu, ni), (size_t)std::max(h->n_users, h->n_items)) * (sizeof(O) / sizeof(float));
    if (h->stage.count < need) h->stage.alloc(need);
    O *stage = reinterpret_cast<O *>(h->stage.ptr);
    // rows of U are entries [0, n_u_rows) of `par` for BPR / FunkSVD; AsySVD never flips a buffer (par stays 0)
    const unsigned char *par_u = h->par.ptr, *par_v = h->par.ptr + h->n_users;
    auto gather = [&](const T *b0, const T *b1, const unsigned char *par, size_t rows, int k, O *host) {
        hipLaunchKernelGGL((mf_gather_rows_kernel<T, O>), dim3(div_up((long long)rows * k, 256)), dim3(256), 0, s, b0, b1, par,
                           (long long)rows, k, stage);
        MI_HIP(hipMemcpyAsync(host, stage, rows * k * sizeof(O), hipMemcpyDeviceToHost, s));
        MI_HIP(hipStreamSynchronize(s));
    };
    const bool asy = h->cfg.algorithm == MI355REC_MF_ASY_SVD;
    if (U) gather(p.U0, p.U1, asy ? par_v : par_u, h->n_u_rows, h->k, U);   // AsySVD: item-sized, par is all zero anyway
    if (V) gather(p.V0, p.V1, par_v, h->n_items, h->k, V);
    if (bu) gather(p.bu0, p.bu1, par_u, h->n_users, 1, bu);
    if (bi) gather(p.bi0, p.bi1, par_v, h->n_items, 1, bi);
    if (!mu) return;
    if (asy) {
        T v;
        MI_HIP(hipMemcpyAsync(&v, p.asy_mu, sizeof(T), hipMemcpyDeviceToHost, s));
        MI_HIP(hipStreamSynchronize(s));
        *mu = (O)v;
    } else {
        hipLaunchKernelGGL((mf_final_mu_kernel<T, O>), dim3(1), dim3(64), 0, s, p, stage);
        MI_HIP(hipMemcpyAsync(mu, stage, sizeof(O), hipMemcpyDeviceToHost, s));
        MI_HIP(hipStreamSynchronize(s));
    }
}

// mi355rec_scorer_update_from_mf: get_factors_typed<T, float> with the scorer's buffers in the place of `stage` and the host -- the
// same kernel instances, so the scorer ends with float32(what the getters return), bit for bit
template <class T>
void scorer_update_typed(mi355rec_mf *h, mi355rec_scorer *sc) {
    hipStream_t s = h->stream;
    MfParams<T> p{};
    fill_params(h, p);
    const bool bias = sc->use_bias != 0;
    if (bias && h->stage.count < 1) h->stage.alloc(1);
    const unsigned char *par_u = h->par.ptr, *par_v = h->par.ptr + h->n_users;
    int launches = 0;
    auto gather = [&](const T *b0, const T *b1, const unsigned char *par, size_t rows, int k, float *out) {
        hipLaunchKernelGGL((mf_gather_rows_kernel<T, float>), dim3(div_up((long long)rows * k, 256)), dim3(256), 0, s, b0, b1, par,
                           (long long)rows, k, out);
        ++launches;
    };
    hand_off_begin(sc, s);
    gather(p.U0, p.U1, par_u, h->n_users, h->k, sc->U.ptr);
    gather(p.V0, p.V1, par_v, h->n_items, h->k, sc->V.ptr);
    float mu = 0.f;
    if (bias) {
        gather(p.bu0, p.bu1, par_u, h->n_users, 1, sc->bu.ptr);
        gather(p.bi0, p.bi1, par_v, h->n_items, 1, sc->bi.ptr);
        hipLaunchKernelGGL((mf_final_mu_kernel<T, float>), dim3(1), dim3(64), 0, s, p, h->stage.ptr);
        ++launches;
        MI_HIP(hipMemcpyAsync(&mu, h->stage.ptr, sizeof(float), hipMemcpyDeviceToHost, s));
    }
    const double cells = ((double)h->n_users + h->n_items) * (h->k + (bias ? 1 : 0));
    hand_off_end(sc, s, cells * (sizeof(T) + sizeof(float)) + (double)h->n_users + h->n_items, launches);
    if (bias) sc->mu = mu;
}

}  // namespace

extern "C" int mi355rec_mf_create(mi355rec_mf_t *out, const mi355rec_mf_config *cfg, int32_t n_users, int32_t n_items,
                                  const int32_t *indptr, const int32_t *indices, const float *data, const void *U0,
                                  const void *V0) {
    return guarded([&] {
        MI_REQUIRE(out && cfg && indptr && indices && data && U0 && V0, "NULL argument");
        check_config(cfg, n_users, n_items);
        const MfKnobs knobs = read_mf_knobs();
        ensure_device();
        std::unique_ptr<mi355rec_mf> h(new mi355rec_mf());
        h->cfg = *cfg;
        h->n_users = n_users;
        h->n_items = n_items;
        h->k = cfg->n_factors;
        h->n_u_rows = cfg->algorithm == MI355REC_MF_ASY_SVD ? n_items : n_users;
        h->f64 = cfg->precision == MI355REC_F64;
        h->nnz = (size_t)indptr[n_users];
        MI_REQUIRE(h->nnz > 0, "URM has no interactions");
        h->open(1);
        hipStream_t s = h->stream;
        h->indptr.upload(indptr, (size_t)n_users + 1, s);
        h->indices.upload(indices, h->nnz, s);
        h->data.upload(data, h->nnz, s);
        if (h->f64) create_typed<double>(h.get(), U0, V0); else create_typed<float>(h.get(), U0, V0);
        create_state(h.get(), knobs);
        *out = h.release();
    });
}

extern "C" int mi355rec_mf_run_epochs(mi355rec_mf_t h, int32_t n_epochs) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL handle");
        MI_REQUIRE(n_epochs >= 0, "n_epochs must be >= 0");
        const MfKnobs knobs = read_mf_knobs();
        ensure_device();
        ReleaseScope scope(h->stream);
        if (h->f64) run_epochs_typed<double>(h, knobs, n_epochs); else run_epochs_typed<float>(h, knobs, n_epochs);
    });
}

extern "C" int mi355rec_mf_run_samples(mi355rec_mf_t h, const int32_t *u, const int32_t *i, const int32_t *j,
                                       const float *rating, int64_t n) {
    return guarded([&] {
        MI_REQUIRE(h && u && i, "NULL argument");
        const bool bpr = h->cfg.algorithm == MI355REC_MF_BPR;
        MI_REQUIRE(bpr ? j != nullptr : rating != nullptr, "%s", bpr ? "BPR replay needs the negative items" : "FunkSVD / AsySVD replay needs the ratings");
        MI_REQUIRE(n >= 0, "n must be >= 0");
        // the kernels index the factor matrices, the bit rows and par[] with these ids as they come: one pass on the host in front of
        // everything (AsySVD: u is a user id there, too -- its profile is what the step walks)
        const auto check_ids = [n](const int32_t *ids, int32_t limit, const char *what) {
            for (int64_t t = 0; t < n; ++t)
                if (ids[t] < 0 || ids[t] >= limit) fail(MI355REC_E_INVALID, "sample %lld: %s id %d out of range [0, %d)", (long long)t, what, ids[t], limit);
        };
        check_ids(u, h->n_users, "user");
        check_ids(i, h->n_items, "item");
        if (bpr) check_ids(j, h->n_items, "negative item");
        const MfKnobs knobs = read_mf_knobs();
        ensure_device();
        if (n == 0) return;
        const long long B = h->cfg.batch_size;
        const long long per_epoch = batches_per_epoch(shape_of(h));
        ensure_stream_capacity(h, knobs, (size_t)std::max<long long>(n, per_epoch * B), std::max<long long>(ceil_div(n, B), per_epoch));
        hipStream_t s = h->stream;
        MI_HIP(hipMemcpyAsync(h->buf.su.ptr, u, sizeof(int) * n, hipMemcpyHostToDevice, s));
        MI_HIP(hipMemcpyAsync(h->buf.si.ptr, i, sizeof(int) * n, hipMemcpyHostToDevice, s));
        if (bpr) MI_HIP(hipMemcpyAsync(h->buf.sj.ptr, j, sizeof(int) * n, hipMemcpyHostToDevice, s));
        else MI_HIP(hipMemcpyAsync(h->buf.sr.ptr, rating, sizeof(float) * n, hipMemcpyHostToDevice, s));
        h->last_call_samples = 0;
        if (h->f64) run_samples_typed<double>(h, knobs, n); else run_samples_typed<float>(h, knobs, n);
    });
}

// ---- exact multi-GPU mini-batches ---------------------------------------------------------------------------------------
namespace {

template <class T>
void shard_begin_typed(mi355rec_mf *h, const MfKnobs &knobs) {
    const long long B = h->cfg.batch_size, per_epoch = batches_per_epoch(shape_of(h));
    ensure_stream_capacity(h, knobs, (size_t)(per_epoch * B), per_epoch, true);
    MfParams<T> p{};
    fill_params(h, p);
    begin_call(h);
    h->timer.start(h->stream);
    launch_sampler(h, p);                                   // the same stream on every rank: the generator is counter based
    enqueue_schedule(h, knobs, p.samples_per_epoch, per_epoch);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(h->stream));
}

template <class T>
void shard_batch_typed(mi355rec_mf *h, int b) {
    MfParams<T> p{};
    fill_params(h, p);
    const ShardPlan sh = shard_plan(shape_of(h), p.tasks_per_batch, h->shard.rank, h->shard.world);
    p.wg_base = h->shard.rank;
    p.wg_stride = h->shard.world;
    launch_batch<MI355REC_MF_BPR, T>(h, p, b, true, sh.rank_wgs);
    hipLaunchKernelGGL((mf_shard_rows_kernel<T, true>), dim3(sh.wgs), dim3(256), 0, h->stream, p, b, h->shard.rank, h->shard.world,
                       h->shard.slots_per_rank, as<T>(h->shard.send));
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(h->stream));                // the caller's collective may run on any stream
}

template <class T>
void shard_merge_typed(mi355rec_mf *h, int b) {
    MfParams<T> p{};
    fill_params(h, p);
    hipLaunchKernelGGL((mf_shard_rows_kernel<T, false>), dim3(div_up(p.tasks_per_batch, 4)), dim3(256), 0, h->stream, p, b, h->shard.rank,
                       h->shard.world, h->shard.slots_per_rank, as<T>(h->shard.recv));
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(h->stream));                // the slab may be overwritten by the next exchange
}

template <class T>
void shard_end_typed(mi355rec_mf *h) {
    const MfShape s = shape_of(h);
    const long long B = h->cfg.batch_size, per_epoch = batches_per_epoch(s);
    MfParams<T> p{};
    fill_params(h, p);
    hipLaunchKernelGGL(mf_stream_end_kernel<T>, dim3(1), dim3(64), 0, h->stream, p, per_epoch);
    h->timer.stop(h->stream);
    h->batches_done += per_epoch;
    h->last_call_samples = per_epoch * B;
    finish_call(h, per_epoch * B, n_launches(s, per_epoch, 1));               // (the loss is this rank's share)
}

// An error inside an exact multi-GPU epoch ends that epoch: the handle leaves the sharded state, so the next call is refused with
// "begin_epoch has not been called" (or a plain epoch may follow) instead of continuing on a half-exchanged mini-batch.
struct ShardEpochGuard {
    mi355rec_mf *h;
    bool ok = false;
    ~ShardEpochGuard() { if (!ok) h->shard.rank = -1; }
};

}  // namespace

extern "C" int mi355rec_mf_shard_begin_epoch(mi355rec_mf_t h, int32_t rank, int32_t world, void **d_send, void **d_recv,
                                             uint64_t *bytes_per_rank, int32_t *n_batches) {
    return guarded([&] {
        MI_REQUIRE(h && d_send && d_recv && bytes_per_rank && n_batches, "NULL argument");
        MI_REQUIRE(world >= 1 && rank >= 0 && rank < world, "rank %d of %d", rank, world);
        if (h->cfg.algorithm != MI355REC_MF_BPR || h->cfg.sgd_mode != MI355REC_SGD)
            fail(MI355REC_E_UNSUPPORTED, "the exact multi-GPU mode covers MF_BPR with sgd (optimiser moments and the FunkSVD global bias are not exchanged)");
        const MfKnobs knobs = read_mf_knobs();
        ensure_device();
        const ShardPlan sh = shard_plan(shape_of(h), tasks_per_batch(shape_of(h)), rank, world);
        ShardEpochGuard guard{h};
        h->shard.rank = rank;
        h->shard.world = world;
        h->shard.slots_per_rank = sh.slots_per_rank;
        if (h->shard.send.count < sh.bytes_per_rank) h->shard.send.alloc_zero(sh.bytes_per_rank, h->stream);
        if (h->shard.recv.count < sh.bytes_per_rank * world) h->shard.recv.alloc_zero(sh.bytes_per_rank * world, h->stream);
        if (h->f64) shard_begin_typed<double>(h, knobs); else shard_begin_typed<float>(h, knobs);
        h->shard.batches = batches_per_epoch(shape_of(h));
        *d_send = h->shard.send.ptr;
        *d_recv = h->shard.recv.ptr;
        *bytes_per_rank = sh.bytes_per_rank;
        *n_batches = (int32_t)h->shard.batches;
        guard.ok = true;
    });
}

extern "C" int mi355rec_mf_shard_batch(mi355rec_mf_t h, int32_t batch) {
    return guarded([&] {
        MI_REQUIRE(h && h->shard.rank >= 0, "mi355rec_mf_shard_begin_epoch has not been called");
        MI_REQUIRE(batch >= 0 && batch < h->shard.batches, "mini-batch %d of %lld", batch, h->shard.batches);
        ensure_device();
        ShardEpochGuard guard{h};
        if (h->f64) shard_batch_typed<double>(h, batch); else shard_batch_typed<float>(h, batch);
        guard.ok = true;
    });
}

extern "C" int mi355rec_mf_shard_merge(mi355rec_mf_t h, int32_t batch) {
    return guarded([&] {
        MI_REQUIRE(h && h->shard.rank >= 0, "mi355rec_mf_shard_begin_epoch has not been called");
        MI_REQUIRE(batch >= 0 && batch < h->shard.batches, "mini-batch %d of %lld", batch, h->shard.batches);
        ensure_device();
        ShardEpochGuard guard{h};
        if (h->f64) shard_merge_typed<double>(h, batch); else shard_merge_typed<float>(h, batch);
        guard.ok = true;
    });
}

extern "C" int mi355rec_mf_shard_end_epoch(mi355rec_mf_t h) {
    return guarded([&] {
        MI_REQUIRE(h && h->shard.rank >= 0, "mi355rec_mf_shard_begin_epoch has not been called");
        ensure_device();
        ShardEpochGuard guard{h};                            // (ends the sharded state on success too)
        if (h->f64) shard_end_typed<double>(h); else shard_end_typed<float>(h);
    });
}

// ---- replica-batched epochs: R independent models, one launch per mini-batch index ---------------------------------------------
struct mi355rec_mf_group : Handle {
    std::vector<mi355rec_mf *> members;      // not owned
    bool f64 = false;
    int algorithm = 0, klass = 0, tasks_per_batch = 0;      // klass: position of the shared instance in mf_plan.h's RowWidths
    bool plain_sgd = false;                 // every member runs sgd_mode "sgd"
    long long batches_per_epoch = 0;
    int max_timed = 0;
    DeviceBuffer<unsigned char> table;       // MfParams<T>[R]
    std::vector<unsigned char> host_table;
    DeviceBuffer<FastSchedParams> sched_table;   // valid when every member is on the in-LDS schedule (all_fast)
    std::vector<FastSchedParams> host_sched_table;
    bool all_fast = false;
    // Look-ahead schedule (all_fast): the sampler, sort, emit and finish launches of epoch e + 1 -- 38 % of a group epoch, and they read
    // nothing the mini-batch kernels write -- run on `side` while the mini-batch launches of epoch e run on `stream`.  What the
    // mini-batch kernels READ of a schedule (task headers, records, pair records, slots in use) exists twice per member: set A is the
    // member's own, set B belongs to the group; the tables below are the A tables with the four pointers swapped.
    struct SetB {
        DeviceBuffer<TaskHeader> tasks;
        DeviceBuffer<int4> recs, slot_recs;
        DeviceBuffer<int> used;
    };
    std::vector<std::unique_ptr<SetB>> set_b;
    DeviceBuffer<unsigned char> table_b;
    DeviceBuffer<FastSchedParams> sched_table_b;
    hipEvent_t ahead_fork = nullptr, ahead_join = nullptr;
    hipEvent_t fork = nullptr;
    std::vector<hipEvent_t> join;
    hipGraphExec_t graph = nullptr;
    bool graph_failed = false;

    void drop_graph() {
        if (graph) (void)hipGraphExecDestroy(graph);
        graph = nullptr;
    }
    ~mi355rec_mf_group() {
        shutdown([&] {
            if (ahead_fork) (void)hipEventDestroy(ahead_fork);
            if (ahead_join) (void)hipEventDestroy(ahead_join);
            drop_graph();
            if (fork) (void)hipEventDestroy(fork);
            for (auto e : join) (void)hipEventDestroy(e);
        });
    }
};

namespace {

template <class T>
const MfParams<T> *params_table(const DeviceBuffer<unsigned char> &table) { return reinterpret_cast<const MfParams<T> *>(table.ptr); }

// sampler + schedule of all members (all on the in-LDS schedule): four launches
template <class T>
void group_enqueue_schedule(mi355rec_mf_group *g, const MfParams<T> *table, const FastSchedParams *sched_table, hipStream_t s) {
    const long long nb = g->batches_per_epoch;
    const int R = (int)g->members.size();
    mi355rec_mf *h0 = g->members[0];
    const FastSchedParams &f0 = g->host_sched_table[0];
    const dim3 sgrid(div_up(nb * (long long)h0->cfg.batch_size, 256), R);
    if (g->algorithm == MI355REC_MF_BPR) hipLaunchKernelGGL((mf_group_sample_kernel<MI355REC_MF_BPR, T>), sgrid, dim3(256), 0, s, table);
    else hipLaunchKernelGGL((mf_group_sample_kernel<MI355REC_MF_FUNK_SVD, T>), sgrid, dim3(256), 0, s, table);
    hipLaunchKernelGGL(mf_group_epoch_advance_kernel<T>, dim3(div_up(R, 64)), dim3(64), 0, s, table, R);
    static bool attr_set[64] = {};
    set_sched_sort_attribute(reinterpret_cast<const void *>(mf_group_sched_sort_kernel), attr_set);
    // (all members on bit rows or none: group_sched_table; the rows' lengths are the members' own)
    int max_entries = 0, max_row_words = 0;
    size_t lds = 0;
    for (const auto &f : g->host_sched_table) {
        max_entries = std::max(max_entries, f.n_entries);
        max_row_words = std::max(max_row_words, f.row_words);
        lds = std::max(lds, sched_lds(f));
    }
    const bool bit_rows = f0.bit_rows != nullptr;
    hipLaunchKernelGGL(mf_group_sched_sort_kernel, dim3((unsigned)nb, R), dim3(SCHED_THREADS), lds, s, sched_table);
    if (bit_rows) hipLaunchKernelGGL(mf_group_sched_parity_kernel, dim3(div_up(max_row_words, 64), R), dim3(PARITY_THREADS), 0, s, sched_table, (int)nb);
    hipLaunchKernelGGL(mf_group_sched_emit_kernel, dim3(div_up(f0.batch_size, 256), (unsigned)nb, R), dim3(256), 0, s, sched_table);
    if (!bit_rows) hipLaunchKernelGGL(mf_group_sched_finish_kernel, dim3(div_up(max_entries, 256), R), dim3(256), 0, s, sched_table);
}

// the shared chain of mini-batch launches of one epoch, on the group's stream
template <class T>
void group_enqueue_batches(mi355rec_mf_group *g, const MfParams<T> *table, bool timed) {
    const long long nb = g->batches_per_epoch;
    const int wgs = group_workgroups(g->tasks_per_batch), R = (int)g->members.size();
    for (long long b = 0; b < nb; ++b) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (timed) g->dispatch_timers.next(e0, e1, g->max_timed);
        if (g->algorithm == MI355REC_MF_BPR) launch_group_batch<MI355REC_MF_BPR, T>(g->stream, table, g->klass, wgs, R, (int)b, g->plain_sgd, e0, e1);
        else launch_group_batch<MI355REC_MF_FUNK_SVD, T>(g->stream, table, g->klass, wgs, R, (int)b, g->plain_sgd, e0, e1);
    }
    hipLaunchKernelGGL(mf_group_stream_end_kernel<T>, dim3(div_up(R, 64)), dim3(64), 0, g->stream, table, R, nb);
}

// samplers and schedules on the members' own streams (parallel branches, also when captured)
template <class T>
void group_enqueue_member_schedules(mi355rec_mf_group *g, const MfKnobs &knobs) {
    MI_HIP(hipEventRecord(g->fork, g->stream));
    for (size_t m = 0; m < g->members.size(); ++m) {
        mi355rec_mf *h = g->members[m];
        MI_HIP(hipStreamWaitEvent(h->stream, g->fork, 0));
        MfParams<T> p{};
        fill_params(h, p);
        launch_sampler(h, p);
        enqueue_schedule(h, knobs, p.samples_per_epoch, g->batches_per_epoch);
        MI_HIP(hipEventRecord(g->join[m], h->stream));
        MI_HIP(hipStreamWaitEvent(g->stream, g->join[m], 0));
    }
}

// One epoch of every member: sampler and schedule, then the shared chain of mini-batch launches on the group's stream.
template <class T>
void group_enqueue_epoch(mi355rec_mf_group *g, const MfKnobs &knobs, bool timed) {
    if (g->all_fast) group_enqueue_schedule<T>(g, params_table<T>(g->table), g->sched_table.ptr, g->stream);
    else group_enqueue_member_schedules<T>(g, knobs);
    group_enqueue_batches<T>(g, params_table<T>(g->table), timed);
}

// Stage 1: every member's buffers and parameter block, as the bytes of MfParams<T>[R].
template <class T>
std::vector<unsigned char> group_member_table(mi355rec_mf_group *g, const MfKnobs &knobs) {
    const long long nb = g->batches_per_epoch;
    const int R = (int)g->members.size();
    std::vector<unsigned char> table(sizeof(MfParams<T>) * (size_t)R);
    for (int m = 0; m < R; ++m) {
        mi355rec_mf *h = g->members[m];
        MI_REQUIRE(h->shard.rank < 0, "member %d is inside an exact multi-GPU epoch", m);
        ensure_stream_capacity(h, knobs, (size_t)(nb * h->cfg.batch_size), nb, true);
        MfParams<T> p;
        memset(&p, 0, sizeof(p));
        fill_params(h, p);
        p.used = reads_used_slots(shape_of(h), knobs) ? h->lds.used.ptr : nullptr;
        memcpy(table.data() + sizeof(MfParams<T>) * (size_t)m, &p, sizeof(MfParams<T>));
        begin_call(h);
        MI_HIP(hipStreamSynchronize(h->stream));      // (its clears and first-touch memsets run on the member's own stream)
    }
    return table;
}

// Stage 2: the members' in-LDS schedule tables; `all_fast` says whether every member is on that schedule (the tables of the members
// in front of the first one that is not are filled, as ever: the change detection below compares them only when all_fast).
std::vector<FastSchedParams> group_sched_table(mi355rec_mf_group *g, const MfKnobs &knobs, bool &all_fast) {
    const long long nb = g->batches_per_epoch;
    std::vector<FastSchedParams> sched(g->members.size());
    all_fast = !knobs.group_per_member_schedule;
    for (size_t m = 0; m < g->members.size(); ++m) {
        mi355rec_mf *h = g->members[m];
        all_fast = all_fast && runs_fast_schedule(shape_of(h), knobs, nb);
        // one launch runs either the parity kernel in front of the emit kernel or the finish kernel behind it: members that disagree
        // about bit rows (one too large for LDS, or created under MI355REC_MF_ROW_BITMAP) schedule on their own streams, as a whole
        all_fast = all_fast && h->lds.bit_rows == g->members[0]->lds.bit_rows;
        if (!all_fast) continue;
        sched[m] = fast_sched_params(h, knobs, nb * (long long)h->cfg.batch_size);
        // (the group's mini-batch kernel reads `used` and never looks at a slot past the last workgroup in use: two thirds of the
        // header slots of a fused BPR mini-batch are not zero-filled -- 150 MB of 16-byte stores per 32-model epoch)
        sched[m].fill_all = 0;
    }
    return sched;
}

// Stage 3: what changed since the last call goes to the device, and the graph that holds the old addresses goes away.
void group_publish_tables(mi355rec_mf_group *g, const std::vector<unsigned char> &table, const std::vector<FastSchedParams> &sched, bool all_fast) {
    const bool sched_changed = all_fast != g->all_fast || (all_fast && (g->host_sched_table.size() != sched.size() ||
                               memcmp(g->host_sched_table.data(), sched.data(), sizeof(FastSchedParams) * sched.size()) != 0));
    if (sched_changed) {
        g->drop_graph();
        MI_HIP(hipStreamSynchronize(g->stream));
        g->all_fast = all_fast;
        g->host_sched_table = sched;
        if (all_fast) {
            if (g->sched_table.count < sched.size()) g->sched_table.alloc(sched.size());
            MI_HIP(hipMemcpy(g->sched_table.ptr, sched.data(), sizeof(FastSchedParams) * sched.size(), hipMemcpyHostToDevice));
        }
    }
    if (table != g->host_table) {                 // a member re-allocated its stream buffers
        g->drop_graph();
        MI_HIP(hipStreamSynchronize(g->stream));
        if (g->table.count < table.size()) g->table.alloc(table.size());
        MI_HIP(hipMemcpy(g->table.ptr, table.data(), table.size(), hipMemcpyHostToDevice));
        g->host_table = table;
    }
}

// Stage 4 (look-ahead only): set B (once per group, again when a member's buffers moved) ...
void group_ensure_set_b(mi355rec_mf_group *g) {
    const size_t R = g->members.size();
    bool fresh = g->set_b.size() != R;
    for (size_t m = 0; m < R && !fresh; ++m) {
        const mi355rec_mf *h = g->members[m];
        const mi355rec_mf_group::SetB &b = *g->set_b[m];
        fresh = b.tasks.count != h->buf.tasks.count || b.recs.count != h->buf.recs.count || b.slot_recs.count != h->buf.slot_recs.count ||
                b.used.count != h->lds.used.count;
    }
    if (!fresh) return;
    MI_HIP(hipStreamSynchronize(g->stream));
    g->open_side();
    if (!g->ahead_fork) MI_HIP(hipEventCreateWithFlags(&g->ahead_fork, hipEventDisableTiming));
    if (!g->ahead_join) MI_HIP(hipEventCreateWithFlags(&g->ahead_join, hipEventDisableTiming));
    g->set_b.clear();
    for (const mi355rec_mf *h : g->members) {
        std::unique_ptr<mi355rec_mf_group::SetB> b(new mi355rec_mf_group::SetB());
        b->tasks.alloc_zero(h->buf.tasks.count, g->stream);
        b->recs.alloc(h->buf.recs.count);
        b->slot_recs.alloc_zero(h->buf.slot_recs.count, g->stream);
        b->used.alloc(h->lds.used.count);
        g->set_b.push_back(std::move(b));
    }
}

// ... and its tables: the A tables with the four pointers swapped
template <class T>
void group_publish_tables_b(mi355rec_mf_group *g, std::vector<unsigned char> table_b, std::vector<FastSchedParams> sched_b) {
    for (size_t m = 0; m < g->members.size(); ++m) {
        MfParams<T> pb;
        memcpy(&pb, table_b.data() + sizeof(MfParams<T>) * m, sizeof(pb));
        const mi355rec_mf_group::SetB &b = *g->set_b[m];
        pb.tasks = b.tasks.ptr; pb.recs = b.recs.ptr; pb.slot_recs = b.slot_recs.ptr; pb.used = b.used.ptr;
        memcpy(table_b.data() + sizeof(MfParams<T>) * m, &pb, sizeof(pb));
        sched_b[m].tasks = b.tasks.ptr; sched_b[m].recs = b.recs.ptr; sched_b[m].slot_recs = b.slot_recs.ptr; sched_b[m].used = b.used.ptr;
    }
    if (g->table_b.count < table_b.size()) g->table_b.alloc(table_b.size());
    if (g->sched_table_b.count < sched_b.size()) g->sched_table_b.alloc(sched_b.size());
    MI_HIP(hipMemcpyAsync(g->table_b.ptr, table_b.data(), table_b.size(), hipMemcpyHostToDevice, g->stream));
    MI_HIP(hipMemcpyAsync(g->sched_table_b.ptr, sched_b.data(), sizeof(FastSchedParams) * sched_b.size(), hipMemcpyHostToDevice, g->stream));
    MI_HIP(hipStreamSynchronize(g->stream));           // (the two vectors are locals)
}

// Stage 5, look-ahead: epoch e + 1's schedule on `side` beside epoch e's mini-batches, the two table sets in turn
template <class T>
void group_run_ahead(mi355rec_mf_group *g, long long n_epochs, long long timed) {
    const MfParams<T> *tab[2] = {params_table<T>(g->table), params_table<T>(g->table_b)};
    const FastSchedParams *sch[2] = {g->sched_table.ptr, g->sched_table_b.ptr};
    group_enqueue_schedule<T>(g, tab[0], sch[0], g->stream);                   // the call's first epoch: nothing to hide it behind
    for (long long e = 0; e < n_epochs; ++e) {
        const int cur = (int)(e & 1);
        if (e + 1 < n_epochs) {
            MI_HIP(hipEventRecord(g->ahead_fork, g->stream));                   // (behind epoch e's schedule and epoch e - 1's mini-batches)
            MI_HIP(hipStreamWaitEvent(g->side, g->ahead_fork, 0));
            group_enqueue_schedule<T>(g, tab[cur ^ 1], sch[cur ^ 1], g->side);
            MI_HIP(hipEventRecord(g->ahead_join, g->side));
        }
        group_enqueue_batches<T>(g, tab[cur], e < timed);
        if (e + 1 < n_epochs) MI_HIP(hipStreamWaitEvent(g->stream, g->ahead_join, 0));
    }
}

// Stage 5, otherwise: timed epochs as plain launches, the rest replays one graph (captured once per group) or plain launches, too
template <class T>
bool group_ensure_graph(mi355rec_mf_group *g, const MfKnobs &knobs) {
    if (!g->graph && !g->graph_failed) {
        g->graph = capture_graph(g->stream, [&] { group_enqueue_epoch<T>(g, knobs, false); });
        g->graph_failed = g->graph == nullptr;
    }
    return g->graph != nullptr;
}

template <class T>
void group_run_plain(mi355rec_mf_group *g, const MfKnobs &knobs, long long n_epochs, long long timed, bool graph) {
    for (long long e = 0; e < n_epochs; ++e) {
        if (e < timed || !graph) group_enqueue_epoch<T>(g, knobs, e < timed);
        else MI_HIP(hipGraphLaunch(g->graph, g->stream));
    }
}

// Stage 6: the group's stats and every member's
void group_account(mi355rec_mf_group *g, long long n_epochs) {
    const long long nb = g->batches_per_epoch;
    mi355rec_stats &st = g->stats;
    st = mi355rec_stats{};
    st.call_ms = g->timer.elapsed_ms();
    st.kernel_ms = g->dispatch_timers.total_ms();
    st.n_timed = g->dispatch_timers.used;
    st.n_launches = nb * n_epochs;
    for (mi355rec_mf *h : g->members) {
        const long long n = nb * n_epochs * (long long)h->cfg.batch_size;
        const double loss = read_loss(h);
        h->batches_done += nb * n_epochs;
        h->last_call_samples = n_epochs > 0 ? nb * (long long)h->cfg.batch_size : 0;
        h->stats = mi355rec_stats{};
        h->stats.call_ms = st.call_ms;
        h->stats.n_launches = st.n_launches;
        h->stats.n_units = n;
        h->stats.algorithmic_bytes = bytes_per_sample(shape_of(h)) * (double)n;
        h->stats.loss = loss;
        st.n_units += n;
        st.algorithmic_bytes += h->stats.algorithmic_bytes;
        st.loss += loss;
    }
}

template <class T>
void group_run_epochs_typed(mi355rec_mf_group *g, const MfKnobs &knobs, int n_epochs) {
    const long long nb = g->batches_per_epoch;
    bool all_fast = false;
    const std::vector<unsigned char> table = group_member_table<T>(g, knobs);
    const std::vector<FastSchedParams> sched = group_sched_table(g, knobs, all_fast);
    group_publish_tables(g, table, sched, all_fast);
    g->dispatch_timers.reset();
    const long long timed = timed_epochs(g->max_timed, nb, n_epochs);
    const bool ahead = group_ahead(g->all_fast, n_epochs, knobs);
    bool graph = group_use_graph(ahead, knobs, nb, n_epochs, timed);
    if (ahead) {
        group_ensure_set_b(g);
        group_publish_tables_b<T>(g, table, sched);
    } else if (graph) {
        graph = group_ensure_graph<T>(g, knobs);
    }
    g->timer.start(g->stream);
    if (ahead) group_run_ahead<T>(g, n_epochs, timed);
    else group_run_plain<T>(g, knobs, n_epochs, timed, graph);
    g->timer.stop(g->stream);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(g->stream));
    group_account(g, n_epochs);
}

// the group's shared numbers come from member 0
void group_adopt_first(mi355rec_mf_group *g, const mi355rec_mf *first) {
    const MfShape s = shape_of(first);
    if (s.algorithm == MI355REC_MF_ASY_SVD) fail(MI355REC_E_UNSUPPORTED, "ASY_SVD has no mini-batches to share a launch");
    g->f64 = s.f64;
    g->algorithm = s.algorithm;
    g->klass = row_width(s.k, s.f64).klass;
    if (g->klass < 0)
        fail(MI355REC_E_UNSUPPORTED, "n_factors = %d runs on the any-k kernel, which has no replica-batched form (use a multiple of %d up to %d)",
             s.k, vec_of(s.f64), widest_chunks(RowWidths{}) * vec_of(s.f64));
    g->tasks_per_batch = tasks_per_batch(s);
    g->batches_per_epoch = batches_per_epoch(s);
}

}  // namespace

extern "C" int mi355rec_mf_group_create(mi355rec_mf_group_t *out, const mi355rec_mf_t *members, int32_t n_members) {
    return guarded([&] {
        MI_REQUIRE(out && members, "NULL argument");
        MI_REQUIRE(n_members >= 1 && n_members <= 65535, "n_members = %d out of range", n_members);
        ensure_device();
        std::unique_ptr<mi355rec_mf_group> g(new mi355rec_mf_group());
        MI_REQUIRE(members[0], "member 0 is NULL");
        group_adopt_first(g.get(), members[0]);
        g->plain_sgd = true;
        for (int m = 0; m < n_members; ++m) {
            mi355rec_mf *h = members[m];
            MI_REQUIRE(h, "member %d is NULL", m);
            for (int o = 0; o < m; ++o) MI_REQUIRE(members[o] != h, "member %d is listed twice", m);
            const GroupMismatch mismatch = group_mismatch(shape_of(members[0]), shape_of(h));
            MI_REQUIRE(mismatch != GROUP_OTHER_INSTANCE,
                       "member %d runs a different kernel instance (algorithm, precision or n_factors class) than member 0", m);
            MI_REQUIRE(mismatch != GROUP_OTHER_BATCHES, "member %d has a different batch_size or number of mini-batches per epoch than member 0", m);
            g->members.push_back(h);
            g->plain_sgd = g->plain_sgd && h->cfg.sgd_mode == MI355REC_SGD;
        }
        g->open(1);
        MI_HIP(hipEventCreateWithFlags(&g->fork, hipEventDisableTiming));
        g->join.resize(n_members, nullptr);
        for (auto &e : g->join) MI_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        *out = g.release();
    });
}

extern "C" int mi355rec_mf_group_run_epochs(mi355rec_mf_group_t g, int32_t n_epochs) {
    return guarded([&] {
        MI_REQUIRE(g, "NULL handle");
        MI_REQUIRE(n_epochs >= 0, "n_epochs must be >= 0");
        const MfKnobs knobs = read_mf_knobs();
        ensure_device();
        if (g->f64) group_run_epochs_typed<double>(g, knobs, n_epochs); else group_run_epochs_typed<float>(g, knobs, n_epochs);
    });
}

extern "C" int mi355rec_mf_group_set_profiling(mi355rec_mf_group_t g, int32_t max_timed_launches) {
    return guarded([&] {
        MI_REQUIRE(g, "NULL handle");
        MI_REQUIRE(max_timed_launches >= 0 && max_timed_launches <= 65536, "max_timed_launches out of range");
        ensure_device();
        g->max_timed = max_timed_launches;
        g->dispatch_timers.reserve(max_timed_launches);
    });
}

extern "C" int mi355rec_mf_group_get_stats(mi355rec_mf_group_t g, mi355rec_stats *stats) { return handle_get_stats(g, stats); }

extern "C" void mi355rec_mf_group_destroy(mi355rec_mf_group_t g) { handle_destroy(g); }

extern "C" int mi355rec_mf_get_factors(mi355rec_mf_t h, float *U, float *V, float *bu, float *bi, float *mu) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL handle");
        ensure_device();
        if (h->f64) get_factors_typed<double, float>(h, U, V, bu, bi, mu); else get_factors_typed<float, float>(h, U, V, bu, bi, mu);
    });
}

extern "C" int mi355rec_mf_get_factors_f64(mi355rec_mf_t h, double *U, double *V, double *bu, double *bi, double *mu) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL handle");
        ensure_device();
        if (h->f64) get_factors_typed<double, double>(h, U, V, bu, bi, mu); else get_factors_typed<float, double>(h, U, V, bu, bi, mu);
    });
}

// Host code only: the handle struct is private to this file, the kernel is asy_estimate.hip's.
extern "C" int mi355rec_mf_asy_user_factors(mi355rec_mf_t h, const double *row_divisor, double *out) {
    static_assert(asy_estimate_plan::KMAX == ASY_KMAX, "the estimate takes every k an ASY_SVD handle takes");
    return guarded([&] {
        MI_REQUIRE(h && row_divisor && out, "NULL argument");
        if (h->cfg.algorithm != MI355REC_MF_ASY_SVD)
            fail(MI355REC_E_UNSUPPORTED, "user factors are estimated from Y for ASY_SVD only: this handle's user factors are its model");
        if (!h->f64) fail(MI355REC_E_UNSUPPORTED, "the user-factor estimate is float64 arithmetic: this ASY_SVD handle keeps its state in float32");
        ensure_device();
        hipStream_t s = h->stream;
        ReleaseScope scope(s);
        if (!h->asy_order.count) {
            std::vector<int32_t> indptr((size_t)h->n_users + 1);
            h->indptr.download(indptr.data(), indptr.size(), s);
            MI_HIP(hipStreamSynchronize(s));
            asy_estimate_upload_order(h->n_users, indptr.data(), h->asy_order, s);
        }
        MfParams<double> p{};
        fill_params(h, p);              // (Y is p.U0: AsySVD never flips a buffer)
        DeviceBuffer<double> divisor, estimate;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        h->dispatch_timers.reserve(1);
        h->dispatch_timers.reset();
        h->dispatch_timers.next(e0, e1, 1);
        h->timer.start(s);
        divisor.upload(row_divisor, (size_t)h->n_users, s);
        estimate.alloc((size_t)h->n_users * h->k);
        asy_estimate_enqueue(h->n_users, h->k, {h->indptr.ptr, h->indices.ptr, h->data.ptr, p.U0, divisor.ptr, h->asy_order.ptr, estimate.ptr}, s,
                             e0, e1);
        estimate.download(out, estimate.count, s);
        h->timer.stop(s);
        MI_HIP(hipStreamSynchronize(s));
        h->stats = mi355rec_stats{};
        h->stats.call_ms = h->timer.elapsed_ms();
        h->stats.kernel_ms = h->dispatch_timers.total_ms();
        h->stats.n_launches = h->stats.n_timed = 1;
        h->stats.n_units = (int64_t)h->n_users * h->k;
        h->stats.algorithmic_bytes = asy_estimate_plan::bytes((long long)h->nnz, h->n_users, h->k);
    });
}

extern "C" int mi355rec_scorer_update_from_mf(mi355rec_scorer_t scorer, mi355rec_mf_t h) {
    return guarded([&] {
        MI_REQUIRE(scorer && h, "NULL handle");
        if (h->cfg.algorithm == MI355REC_MF_ASY_SVD)
            fail(MI355REC_E_UNSUPPORTED, "an ASY_SVD handle cannot be handed to a scorer: its user rows are item-sized and the user "
                                         "factors are estimated on the host");
        hand_off_check(scorer, "MF", h->n_users, h->n_items, h->k, h->cfg.use_bias);
        ensure_device();
        ReleaseScope scope(h->stream);
        if (h->f64) scorer_update_typed<double>(h, scorer); else scorer_update_typed<float>(h, scorer);
    });
}

extern "C" int mi355rec_mf_get_last_samples(mi355rec_mf_t h, int32_t *u, int32_t *i, int32_t *j, float *rating, int64_t cap,
                                            int64_t *n) {
    return guarded([&] {
        MI_REQUIRE(h && n, "NULL argument");
        ensure_device();
        *n = h->last_call_samples;
        const size_t m = (size_t)std::min<long long>(cap, h->last_call_samples);
        hipStream_t s = h->stream;
        if (u) h->buf.su.download(u, m, s);
        if (i) h->buf.si.download(i, m, s);
        if (j && h->cfg.algorithm == MI355REC_MF_BPR) h->buf.sj.download(j, m, s);
        if (rating && h->cfg.algorithm != MI355REC_MF_BPR) h->buf.sr.download(rating, m, s);
        MI_HIP(hipStreamSynchronize(s));
    });
}

extern "C" int mi355rec_mf_set_profiling(mi355rec_mf_t h, int32_t max_timed_launches) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL handle");
        MI_REQUIRE(max_timed_launches >= 0 && max_timed_launches <= 65536, "max_timed_launches out of range");
        ensure_device();
        h->max_timed = max_timed_launches;
        h->dispatch_timers.reserve(max_timed_launches);
    });
}

namespace {

void copy_ticks(mi355rec_mf *h, const DeviceBuffer<unsigned long long> &ticks, uint64_t *out, int64_t cap, int64_t *n) {
    MI_REQUIRE(h && n, "NULL argument");
    ensure_device();
    *n = (int64_t)ticks.count;
    if (out && cap > 0) {
        MI_HIP(hipStreamSynchronize(h->stream));
        MI_HIP(hipMemcpy(out, ticks.ptr, sizeof(uint64_t) * std::min<size_t>((size_t)cap, ticks.count), hipMemcpyDeviceToHost));
    }
}

}  // namespace

extern "C" int mi355rec_mf_get_phase_ticks(mi355rec_mf_t h, uint64_t *out, int64_t cap, int64_t *n) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL argument");
        copy_ticks(h, h->ticks, out, cap, n);
    });
}

extern "C" int mi355rec_mf_get_schedule_ticks(mi355rec_mf_t h, uint64_t *out, int64_t cap, int64_t *n) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL argument");
        copy_ticks(h, h->lds.ticks, out, cap, n);
    });
}

extern "C" int mi355rec_mf_get_stats(mi355rec_mf_t h, mi355rec_stats *stats) { return handle_get_stats(h, stats); }

// (a group's launches on the group's stream have been waited for by the call that made them)
extern "C" void mi355rec_mf_destroy(mi355rec_mf_t h) { handle_destroy(h); }
