// slim.hip -- SLIM-BPR epoch on MI355X (gfx950).
//
// Replaces SLIM_BPR/Cython/SLIM_BPR_Cython_Epoch.pyx (reference): epochIteration_Cython :212-317 with the dense
// store (:129) and the symmetric triangular store (Triangular_Matrix :1226-1330), sampleBPR_Cython :439-483,
// adaptive_gradient :398-436, get_S :343-391.  The wrapper hard-codes batch_size = 1
// (SLIM_BPR/Cython/SLIM_BPR_Cython.py:140), so an epoch is n_users + 1 STRICTLY ORDERED SGD steps.
//
// Design.  The sample stream does not depend on S, so WHICH earlier step a step has to wait for is
// known before the first step runs, and an epoch is ONE persistent kernel that executes the stream as a dataflow graph.  What
// bounds it is the longest chain of dependent steps (the steps on the busiest item row: 1 214 of 138 494 at the ML-20M shape),
// i.e. the price of ONE hand-off between two steps -- not bytes.  Round 4 rebuilds both stores around that price:
//   dense store       step t owns rows i_t and j_t.  The BUSIEST rows (top-H items by their number of steps in this stream,
//                     chosen on the device) are kept in the LDS of an OWNING workgroup for the whole launch: its 16 wavefronts
//                     take the row's steps in turn, each prefetching everything that does not depend on the row (profile,
//                     the other row's cells once that row's ticket has come up) before its turn; a link of the chain is then
//                     an LDS gather + wavefront reduction + LDS scatter (a few hundred cycles) instead of ticket poll ->
//                     gather -> write-through -> drain -> ticket through L2 (4.8 us per link under load in round 3).
//                     All other steps are run by "cold" wavefronts (one step per wavefront, no barriers), ordered per item by
//                     numbered tickets as before.  Two busy rows in one step talk through a two-word mailbox.
//   symmetric store   cell (r, c) aliases (c, r), so ownership is per CELL and no row can be owned.  Every cell of the packed
//                     lower triangle is an 8-byte GRANULE {float value, tag of the step that wrote it}, written by ONE
//                     write-through store: a reader that knows which step wrote the cell last (`pred`, from a sort of the
//                     stream's (cell, step) pairs) polls THE CELL until the tag matches -- one round trip per link instead of
//                     done-flag poll + gather + drain + flag store, and no step ever drains its stores.  The per-item
//                     optimiser cells travel the same way (two granules per float64).  Steps with profiles of more than 256
//                     entries are run by a whole workgroup (all their granules in flight at once), the others by a wavefront.
// The sample stream of epoch e + 1 is drawn and scheduled on a second stream while the kernel of epoch e runs (StreamSet x 2).
// Steps are claimed from an in-order queue, so a waiting step only ever waits for steps that are already running: no deadlock
// whatever the residency (the owners of the dense store are the exception: they are leased to one launch at a time, see
// OwnerLease).  Exact sequential semantics (1e-5 element-wise against the float64 oracle for all four optimisers, both stores,
// at the full BASELINE config-3 shape).  4-byte gathers / scatters, no dense contraction: no MFMA.
//
// Source layout.  This file is the translation unit and holds the host side: the handle, the schedules' and launches' HIP calls, the
// epoch loop, the C ABI.  Device code: slim_flow.cuh (shared types and helpers, dense store), slim_sym_flow.cuh (symmetric store,
// ordered fallback), slim_schedule.cuh (sampler, dependencies of a stream), slim_readout.cuh (get_S, prune / list, W).  Host code
// that makes no HIP call: slim_plan.h (knobs, grids, segment cuts), slim_gate.h (owner gate, compute-unit lease).
#include "common.h"
#include "score.h"

#include "sampling.cuh"
#include "topk.cuh"
#include "wave.cuh"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <memory>
#include <type_traits>

#include "slim_flow.cuh"
#include "slim_sym_flow.cuh"
#include "slim_schedule.cuh"
#include "slim_readout.cuh"
#include "slim_gate.h"

using namespace mi355rec;

// What the schedule of ONE stream of steps hands to the launch that runs it.  There are two: the sample stream of an epoch does not
// depend on S, so while the dataflow kernel of epoch e runs, epoch e + 1 is drawn and scheduled on a second HIP stream (the item
// sort, the 40 M-pair cell sort of the symmetric store: 0.35 / 3.7 ms of a 2.1 / 18.9 ms epoch at the ML-20M shape) -- also across
// calls: the reference's fit loop asks for one epoch per call.
struct StreamSet {
    DeviceBuffer<int> su, si, sj, seq, iprev, len2, item_vals, pred, run_start;
    DeviceBuffer<unsigned long long> item_keys;          // (item, step) pairs in sorted order: the owned rows' lists are runs of it
    DeviceBuffer<long long> cellptr;
    DeviceBuffer<StepDesc> desc;                         // symmetric store: one descriptor per step ...
    DeviceBuffer<int> order, n_short_dev;                // ... and the two queues: short profiles in stream order, then the long ones backwards
    int n_short = 0;
    DeviceBuffer<unsigned> item_cnt;
    size_t capacity = 0, pred_capacity = 0;
    long long epoch = -1;                                // the native epoch this set is scheduled for (-1: none / a replayed stream)
    int n = 0;
    long long n_cells = 0;
};

struct mi355rec_slim : Handle {                        // `side`: schedules of the next epoch
    mi355rec_slim_config cfg{};
    int n_users = 0, n_items = 0;
    bool f64 = false;           // arithmetic type; storage type of the dense store and its optimiser cells
    size_t nnz = 0;
    StreamSet set[2];
    int cur = 0;                                        // the set whose stream ran last
    bool last_native = false;                           // ... and whether that was an epoch of the on-device sampler
    DeviceBuffer<int> indptr, indices, ticket, queue;
    // scratch of the schedules (one schedule at a time)
    DeviceBuffer<int> vals, vals_sorted;
    DeviceBuffer<unsigned long long> keys, keys_sorted;
    DeviceBuffer<unsigned char> sched_tmp;
    size_t sort_capacity = 0;
    DeviceBuffer<unsigned char> S, c1, c2;              // dense store: S, c1, c2 are float or double by `f64`
    DeviceBuffer<Granule> G, oc;                        // symmetric store: packed triangle of granules, [n_items][4] optimiser granules
    DeviceBuffer<double> loss_slots;
    // dense store, filled at launch time on the main stream: owned rows, descriptors, the cold queue
    DeviceBuffer<int> hot_rank, hot_tables, counters, iota, item_by_cnt;     // hot_tables: item | first | length
    DeviceBuffer<StepDesc> desc, cold_desc, own_desc;
    DeviceBuffer<unsigned> cnt_sorted;
    DeviceBuffer<unsigned char> cold_flag, launch_tmp;
    DeviceBuffer<unsigned long long> mail;              // [2][launch_capacity]
    size_t launch_capacity = 0;
    DeviceBuffer<unsigned long long> prof;              // MI355REC_SLIM_PROF=1: phase clocks of the last launch
    long long steps_done = 0, epochs_done = 0;
    bool aborted = false;                               // a launch gave up on a hand-off: S holds part of an epoch, every later call refuses
    unsigned tag_base = 0;                              // symmetric store: tags handed out so far
    int last_owners = 0, last_cold = 0;                 // owned rows / steps on rows in HBM of the last dense launch (diagnostics)
    std::vector<double> h_loss;
    SlimKnobs knobs;                                    // the environment as the ABI call in progress found it (enter_call)

    ~mi355rec_slim() { shutdown(); }
};

namespace {

// First thing of every ABI call that launches a kernel of this file: binds the device and reads the knobs -- once per call, not once
// per process (tests and scripts change them between calls), and not once per launch.
void enter_call(mi355rec_slim *h) {
    ensure_device();
    h->knobs = read_slim_knobs();
}

template <class T>
void fill_params(mi355rec_slim *h, const StreamSet &st, SlimParams<T> &p) {
    const auto &c = h->cfg;
    p.n_users = h->n_users; p.n_items = h->n_items; p.symmetric = c.symmetric; p.sgd_mode = c.sgd_mode;
    p.lr = (T)c.learning_rate; p.li_reg = (T)c.li_reg; p.lj_reg = (T)c.lj_reg;
    p.gamma = (T)c.gamma; p.beta_1 = (T)c.beta_1; p.beta_2 = (T)c.beta_2;
    p.one_m_gamma = (T)(1.0 - c.gamma); p.one_m_beta_1 = (T)(1.0 - c.beta_1); p.one_m_beta_2 = (T)(1.0 - c.beta_2);
    p.beta_1_d = c.beta_1; p.beta_2_d = c.beta_2;
    p.seed = c.random_seed;
    p.indptr = h->indptr.ptr; p.indices = h->indices.ptr;
    p.S = reinterpret_cast<T *>(h->S.ptr); p.c1 = reinterpret_cast<T *>(h->c1.ptr); p.c2 = reinterpret_cast<T *>(h->c2.ptr);
    p.G = h->G.ptr; p.oc = h->oc.ptr;
    p.su = st.su.ptr; p.si = st.si.ptr; p.sj = st.sj.ptr;
    p.seq = st.seq.ptr; p.iprev = st.iprev.ptr; p.cellptr = st.cellptr.ptr; p.pred = st.pred.ptr;
    p.ticket = h->ticket.ptr; p.queue = h->queue.ptr;
    p.loss_slots = h->loss_slots.ptr;
    p.epoch = h->epochs_done;
    p.steps_before = h->steps_done;
    p.n_steps = 0;
    p.tag_base = h->tag_base;
    p.hot_rank = h->hot_rank.ptr;
    p.hot_item = h->hot_tables.ptr; p.lst_begin = h->hot_tables.ptr + MAX_OWNERS; p.lst_len = h->hot_tables.ptr + 2 * MAX_OWNERS;
    p.n_hot = h->counters.ptr; p.n_cold = h->counters.ptr + 1;
    p.desc = c.symmetric ? st.desc.ptr : h->desc.ptr; p.cold_desc = h->cold_desc.ptr; p.own_desc = h->own_desc.ptr;
    p.order = st.order.ptr; p.n_short = st.n_short;
    p.nap = h->knobs.nap;
    p.prof = h->prof.ptr;
    p.mail_x = h->mail.ptr; p.mail_g = h->mail.ptr + h->launch_capacity;
}

bool flow_supported(const mi355rec_slim *h) { return mi355rec::flow_supported(h->cfg.symmetric != 0, h->n_items); }
bool schedules_ahead(const mi355rec_slim *h) {
    return mi355rec::schedules_ahead(h->cfg.train_with_sparse_weights != 0, h->cfg.symmetric != 0, h->n_items, h->knobs);
}

void ensure_set_capacity(mi355rec_slim *h, StreamSet &st, size_t n) {
    if (st.capacity >= n) return;
    MI_HIP(hipStreamSynchronize(h->stream));
    MI_HIP(hipStreamSynchronize(h->side));
    st.su.alloc(n); st.si.alloc(n); st.sj.alloc(n);
    st.seq.alloc(2 * n); st.iprev.alloc(2 * n); st.len2.alloc(n + 1); st.cellptr.alloc(n + 1);
    st.item_keys.alloc(std::max<size_t>(2 * n, 1024)); st.item_vals.alloc(std::max<size_t>(2 * n, 1024));
    if (h->cfg.symmetric) {
        st.desc.alloc(n);
        st.order.alloc(n);
        if (!st.n_short_dev.ptr) st.n_short_dev.alloc(2);      // [1]: first step with a seen negative item
    }
    if (!st.run_start.ptr) {
        st.run_start.alloc((size_t)h->n_items);
        st.item_cnt.alloc((size_t)h->n_items);
    }
    st.capacity = n;
    st.epoch = -1;
    st.n = 0;
}

void ensure_launch_capacity(mi355rec_slim *h, size_t n) {      // dense store
    if (h->cfg.symmetric || h->launch_capacity >= n) return;
    MI_HIP(hipStreamSynchronize(h->stream));
    h->desc.alloc(n);
    h->cold_desc.alloc(n);
    h->own_desc.alloc(2 * n);
    h->cold_flag.alloc(n);
    h->mail.alloc(2 * n);
    h->launch_capacity = n;
}

void ensure_sort_capacity(mi355rec_slim *h, size_t n, hipStream_t s) {
    if (h->sort_capacity >= n) return;
    MI_HIP(hipStreamSynchronize(s));
    h->keys.alloc(n); h->vals.alloc(n);
    if (h->cfg.symmetric) { h->keys_sorted.alloc(n); h->vals_sorted.alloc(n); }      // (the item pass sorts into the set's own arrays)
    h->sort_capacity = n;
}

// The rocprim two-call idiom: `call(scratch, bytes, count)` is asked for its scratch size (scratch == nullptr, count = n_sized), the
// block grows if it has to, then the call runs on n elements.  Quarter: the block grows by a quarter more than asked for, so that it
// does not grow from call to call, and the call is told the whole block; Exact: a one-off block of what the call asks for.
enum class Grow { Quarter, Exact };
template <class Call>
void run_with_scratch(DeviceBuffer<unsigned char> &tmp, Grow grow, hipStream_t s, size_t n_sized, size_t n, Call call) {
    size_t bytes = 0;
    MI_HIP(call(nullptr, bytes, n_sized));
    if (grow == Grow::Exact) {
        if (bytes + 16 > tmp.count) tmp.alloc(bytes + 16);
    } else {
        if (tmp.count < bytes) {
            MI_HIP(hipStreamSynchronize(s));                // (earlier work of the stream may still use the old block)
            tmp.alloc(bytes + (bytes >> 2) + 256);
        }
        bytes = tmp.count;
    }
    MI_HIP(call(tmp.ptr, bytes, n));
}

void sort_pairs(mi355rec_slim *h, unsigned long long *keys_out, int *vals_out, size_t n, int end_bit, hipStream_t s) {
    // (sized for the scratch arrays' capacity: it does not grow from epoch to epoch)
    run_with_scratch(h->sched_tmp, Grow::Quarter, s, std::max(n, h->sort_capacity), n, [&](void *tmp, size_t &bytes, size_t count) {
        return rocprim::radix_sort_pairs(tmp, bytes, h->keys.ptr, keys_out, h->vals.ptr, vals_out, count, 0, end_bit, s);
    });
}

// the one HIP call the owner gate needs: the device's PCI bus id names its lock file
std::string device_bus_id() {
    int dev = 0;
    char bus[64] = "unknown";
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetPCIBusId(bus, (int)sizeof(bus), dev);
    return bus;
}

template <class Kernel>
int blocks_per_cu(Kernel k, size_t lds) {
    int per_cu = 0;
    MI_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, FLOW_THREADS, lds));
    return std::max(1, std::min(per_cu, 2));            // (2048 threads per compute unit)
}

DepParams dep_params(mi355rec_slim *h, StreamSet &st, int n, int first) {
    DepParams d{};
    d.n_steps = n; d.n_items = h->n_items;
    d.indptr = h->indptr.ptr; d.indices = h->indices.ptr; d.su = st.su.ptr + first; d.si = st.si.ptr + first; d.sj = st.sj.ptr + first;
    d.keys = h->keys.ptr; d.vals = h->vals.ptr; d.keys_sorted = st.item_keys.ptr; d.vals_sorted = st.item_vals.ptr;
    d.seq = st.seq.ptr; d.iprev = st.iprev.ptr; d.len2 = st.len2.ptr; d.cellptr = st.cellptr.ptr; d.pred = st.pred.ptr;
    d.run_start = st.run_start.ptr; d.item_cnt = st.item_cnt.ptr; d.cnt_sorted = h->cnt_sorted.ptr; d.item_by_cnt = h->item_by_cnt.ptr;
    d.hot_rank = h->hot_rank.ptr;
    d.hot_item = h->hot_tables.ptr; d.lst_begin = h->hot_tables.ptr + MAX_OWNERS; d.lst_len = h->hot_tables.ptr + 2 * MAX_OWNERS;
    d.n_hot = h->counters.ptr;
    d.cold_flag = h->cold_flag.ptr;
    d.desc = h->cfg.symmetric ? st.desc.ptr : h->desc.ptr; d.own_desc = h->own_desc.ptr;
    return d;
}

template <class T>
void draw_epoch(mi355rec_slim *h, StreamSet &st, long long epoch, int n, hipStream_t s) {
    SlimParams<T> p{};
    fill_params(h, st, p);
    p.epoch = epoch;
    p.n_steps = n;
    hipLaunchKernelGGL(slim_sample_kernel<T>, dim3(div_up(n, 256)), dim3(256), 0, s, p, st.su.ptr, st.si.ptr, st.sj.ptr);
    st.epoch = -1;
    st.n = 0;
}

// The item pass of a schedule: ticket numbers and previous steps per item (a sort of the 2n (item, step) pairs), cell slots, and --
// symmetric store -- the two queues.  Returns with `s` drained (the number of cells sizes the cell sort).
void schedule_items(mi355rec_slim *h, StreamSet &st, const DepParams &d, int n, hipStream_t s) {
    MI_HIP(hipMemsetAsync(st.item_cnt.ptr, 0, sizeof(unsigned) * (size_t)h->n_items, s));
    hipLaunchKernelGGL(slim_item_keys_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, d);
    sort_pairs(h, st.item_keys.ptr, st.item_vals.ptr, 2 * (size_t)n, 32 + bits_for((unsigned long long)h->n_items), s);
    hipLaunchKernelGGL(slim_seq_kernel, dim3(div_up(2 * n, 256)), dim3(256), 0, s, d);
    // profile lengths -> cell slots (also the algorithmic byte count of the call)
    MI_HIP(hipMemsetAsync(st.len2.ptr + n, 0, sizeof(int), s));
    run_with_scratch(h->sched_tmp, Grow::Quarter, s, (size_t)(n + 1), (size_t)(n + 1), [&](void *tmp, size_t &bytes, size_t count) {
        return rocprim::exclusive_scan(tmp, bytes, st.len2.ptr, st.cellptr.ptr, 0ll, count, rocprim::plus<long long>(), s);
    });
    long long n_cells = 0;
    int n_short = n;
    if (h->cfg.symmetric) {
        // the two queues of the symmetric store's kernel: profiles of up to FLOW_BLOCK entries (a wavefront each), longer ones (a workgroup each)
        const ShortProfile is_short{st.len2.ptr};
        run_with_scratch(h->sched_tmp, Grow::Quarter, s, (size_t)n, (size_t)n, [&](void *tmp, size_t &bytes, size_t count) {
            return rocprim::partition(tmp, bytes, rocprim::counting_iterator<int>(0), st.order.ptr, st.n_short_dev.ptr, count, is_short, s);
        });
        MI_HIP(hipMemcpyAsync(&n_short, st.n_short_dev.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
    }
    MI_HIP(hipMemcpyAsync(&n_cells, st.cellptr.ptr + n, sizeof(long long), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    st.n_cells = n_cells;
    st.n_short = n_short;
}

// The cell pass (symmetric store): per cell the step that touched it last -- a sort of the (cell, step) pairs of the stream -- and the
// step descriptors.  Returns with `s` drained.
void schedule_cells(mi355rec_slim *h, StreamSet &st, int n, int first, hipStream_t s) {
    const long long n_cells = st.n_cells;
    MI_REQUIRE(n_cells < (1ll << 31), "stream too long for the cell sort (%lld cells)", n_cells);
    const size_t roomy = roomy_cell_capacity(h->nnz, n, h->n_users, n_cells);
    if (h->sort_capacity < (size_t)n_cells) ensure_sort_capacity(h, roomy, s);
    if (st.pred_capacity < (size_t)n_cells) {
        MI_HIP(hipStreamSynchronize(h->stream));
        st.pred.alloc(roomy);
        st.pred_capacity = st.pred.count;
    }
    DepParams d = dep_params(h, st, n, first);
    d.keys_sorted = h->keys_sorted.ptr; d.vals_sorted = h->vals_sorted.ptr;
    d.n_cells = n_cells;
    d.step_bits = bits_for((unsigned long long)n);
    const int cell_bits = bits_for((unsigned long long)h->n_items * ((unsigned long long)h->n_items + 1) / 2 + 1);
    d.no_cell = (unsigned)((1ull << cell_bits) - 1ull);
    d.bad_step = st.n_short_dev.ptr + 1;
    MI_HIP(hipMemsetAsync(d.bad_step, 0x7F, sizeof(int), s));
    hipLaunchKernelGGL(slim_cell_keys_kernel, dim3(div_up(n, 4)), dim3(256), 0, s, d);
    sort_pairs(h, h->keys_sorted.ptr, h->vals_sorted.ptr, (size_t)n_cells, cell_bits + d.step_bits, s);
    hipLaunchKernelGGL(slim_pred_kernel, dim3(div_up(n_cells, 256)), dim3(256), 0, s, d);
    hipLaunchKernelGGL(slim_desc_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, d, 1);
    MI_HIP(hipGetLastError());
    int bad = 0;
    MI_HIP(hipMemcpyAsync(&bad, d.bad_step, sizeof(int), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    if (bad < n)
        fail(MI355REC_E_INVALID, "sample %d: the negative item is in the user's profile (the symmetric store holds cell (i, j) and cell (j, i) "
             "as one cell; the reference's sampler never draws a seen item)", first + bad);
}

// Everything about steps first .. first + n - 1 of st.su / si / sj that does not depend on S, on stream `s`: the item pass and --
// symmetric store -- the cell pass.  Returns with `s` drained.
void schedule_stream(mi355rec_slim *h, StreamSet &st, int n, int first, hipStream_t s) {
    if (!flow_supported(h)) {
        st.n = n;
        st.n_cells = 0;
        return;
    }
    ensure_sort_capacity(h, std::max<size_t>(2 * (size_t)n, 1024), s);
    schedule_items(h, st, dep_params(h, st, n, first), n, s);
    if (h->cfg.symmetric) schedule_cells(h, st, n, first, s);
    st.n = n;
}

struct Launched {
    OwnerLease lease;
    bool dense = false, profile = false, serial = false;
    hipStream_t stream = nullptr;          // set once the dataflow kernel is enqueued
    void end_serial() {
        if (serial) owner_gate().release_blocking();
        serial = false;
    }
    // (error paths end here with the kernel possibly still running: it is waited for BEFORE the gate and the leased compute units go
    // back -- finish_stream has already drained the stream on the regular path, where this costs nothing)
    ~Launched() {
        if (stream && (serial || lease.slots > 0)) (void)hipStreamSynchronize(stream);
        end_serial();
    }
};

// What every launch ends with: the kernel's parameters for steps first .. first + n - 1 of the set, and the dispatch's timer events.
template <class T>
SlimParams<T> stream_params(mi355rec_slim *h, const StreamSet &st, int n, int first, hipEvent_t &e0, hipEvent_t &e1) {
    SlimParams<T> p{};
    fill_params(h, st, p);
    p.su += first; p.si += first; p.sj += first;
    p.n_steps = n;
    h->dispatch_timers.next(e0, e1, 1 << 30);
    return p;
}

// (the symmetric store computes in float64 whatever the handle's precision: its two kernels exist for double only)
template <class T>
void launch_ordered(mi355rec_slim *h, StreamSet &st, int n, int first) {
    if constexpr (std::is_same<T, double>::value) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        const SlimParams<T> p = stream_params<T>(h, st, n, first, e0, e1);
        hipExtLaunchKernelGGL(slim_ordered_kernel, dim3(1), dim3(1024), 0, h->stream, e0, e1, 0, p);
    }
}

template <class T>
void launch_symmetric(mi355rec_slim *h, StreamSet &st, int n, int first, Launched &L) {
    if constexpr (std::is_same<T, double>::value) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        const SlimParams<T> p = stream_params<T>(h, st, n, first, e0, e1);
        h->tag_base += (unsigned)n;                  // (wraps after 4 G steps; a tag is compared only with the tag of a step of the same call)
        const SymLaunch g = plan_sym_launch(multiprocessor_count(), blocks_per_cu(slim_sym_flow_kernel, 0), schedules_ahead(h), n, st.n_short, h->knobs);
        try {
            L.serial = owner_gate().acquire_blocking(h->knobs, device_bus_id());              // one symmetric dataflow kernel per device at a time
        } catch (const GateTimeout &t) {
            fail(MI355REC_E_HIP, "SLIM-BPR (symmetric store): another process has held this device's launch lock for more than %.0f s", t.wait_s);
        }
        hipExtLaunchKernelGGL(slim_sym_flow_kernel, dim3(g.grid), dim3(FLOW_THREADS), 0, h->stream, e0, e1, 0, p, g.long_wgs);
    }
}

// What a dense launch's kernel reads besides the schedule, on the main stream: the busiest rows of this stream get owners (if the
// launch got compute units leased), every step its descriptor, the steps on no owned row their queue.
void prepare_dense_queues(mi355rec_slim *h, StreamSet &st, int n, int first, const DenseGrid &g, hipStream_t s) {
    DepParams d = dep_params(h, st, n, first);
    MI_HIP(hipMemsetAsync(h->hot_rank.ptr, 0xFF, sizeof(int) * (size_t)h->n_items, s));
    MI_HIP(hipMemsetAsync(h->counters.ptr, 0, sizeof(int) * 2, s));
    if (g.owners) {
        run_with_scratch(h->launch_tmp, Grow::Quarter, s, (size_t)h->n_items, (size_t)h->n_items, [&](void *tmp, size_t &bytes, size_t count) {
            return rocprim::radix_sort_pairs_desc(tmp, bytes, st.item_cnt.ptr, h->cnt_sorted.ptr, h->iota.ptr, h->item_by_cnt.ptr, count, 0, 32, s);
        });
        d.max_owners = g.max_owners;
        d.min_steps = g.min_steps;
        hipLaunchKernelGGL(slim_owners_kernel, dim3(1), dim3(256), 0, s, d);
        MI_HIP(hipMemsetAsync(h->mail.ptr, 0xFF, sizeof(unsigned long long) * 2 * h->launch_capacity, s));
    }
    hipLaunchKernelGGL(slim_desc_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, d, 0);
    if (g.owners) hipLaunchKernelGGL(slim_owner_desc_kernel, dim3(div_up(2 * n, 256)), dim3(256), 0, s, d);
    run_with_scratch(h->launch_tmp, Grow::Quarter, s, (size_t)n, (size_t)n, [&](void *tmp, size_t &bytes, size_t count) {
        return rocprim::select(tmp, bytes, h->desc.ptr, h->cold_flag.ptr, h->cold_desc.ptr, h->counters.ptr + 1, count, s);
    });
}

template <class T>
void launch_dense(mi355rec_slim *h, StreamSet &st, int n, int first, Launched &L) {
    hipStream_t s = h->stream;
    L.dense = true;
    ensure_launch_capacity(h, st.capacity);
    auto kernel = slim_dense_flow_kernel<T>;
    const int cus = multiprocessor_count();
    const DensePlan plan = plan_dense_launch(h->n_items, h->cfg.train_with_sparse_weights != 0, cus, h->knobs);
    L.lease.take(plan.wanted, plan.want_slots, cus, h->knobs, plan.wanted ? device_bus_id() : std::string());
    const DenseGrid g = dense_grid(L.lease.slots, cus, L.lease.slots > 0 ? 0 : blocks_per_cu(kernel, 0), plan.row_bytes, h->knobs);
    if (g.needs_lds_attribute)
        MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
    prepare_dense_queues(h, st, n, first, g, s);
    MI_HIP(hipMemsetAsync(h->ticket.ptr, 0, sizeof(int) * (size_t)h->n_items, s));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const SlimParams<T> p = stream_params<T>(h, st, n, first, e0, e1);
    hipExtLaunchKernelGGL(kernel, dim3(g.grid), dim3(FLOW_THREADS), g.lds, s, e0, e1, 0, p, g.owners ? 1 : 0);
}

// The dataflow kernel of a scheduled stream, enqueued on the handle's main stream.
template <class T>
void launch_stream(mi355rec_slim *h, StreamSet &st, int n, int first, Launched &L) {
    hipStream_t s = h->stream;
    L.stream = s;
    L.profile = h->knobs.prof;
    if (L.profile) {
        if (!h->prof.ptr) h->prof.alloc(8 * (MAX_OWNERS + 1));
        MI_HIP(hipMemsetAsync(h->prof.ptr, 0, sizeof(unsigned long long) * h->prof.count, s));
    }
    MI_HIP(hipMemsetAsync(h->queue.ptr, 0, sizeof(int) * 4, s));
    if (h->knobs.inject_abort) {                      // (test hook: the abort flag is up before the first step polls it)
        const int one = 1;
        MI_HIP(hipMemcpyAsync(h->queue.ptr + 1, &one, sizeof(int), hipMemcpyHostToDevice, s));
        MI_HIP(hipStreamSynchronize(s));
    }
    if (!flow_supported(h)) launch_ordered<T>(h, st, n, first);
    else if (h->cfg.symmetric) launch_symmetric<T>(h, st, n, first, L);
    else launch_dense<T>(h, st, n, first, L);
    h->stats.n_launches += 1;
    MI_HIP(hipGetLastError());
}

// MI355REC_SLIM_PROF=1: the phase clocks of the launch that has just finished
void print_profile(mi355rec_slim *h) {
    std::vector<unsigned long long> c(h->prof.count);
    MI_HIP(hipMemcpy(c.data(), h->prof.ptr, sizeof(unsigned long long) * c.size(), hipMemcpyDeviceToHost));
    if (h->cfg.symmetric) {
        fprintf(stderr, "[slim prof] symmetric: %llu steps by a wavefront, mean cycles: until all tags were there %.0f, rest %.0f; %.2f extra polling rounds per step\n",
                c[0], (double)c[1] / std::max(1ull, c[0]), (double)c[2] / std::max(1ull, c[0]), (double)c[3] / std::max(1ull, c[0]));
        fprintf(stderr, "[slim prof] symmetric: %llu steps by a workgroup, mean cycles: until all tags were there %.0f, rest %.0f; %.2f extra polling rounds per step\n",
                c[4], (double)c[5] / std::max(1ull, c[4]), (double)c[6] / std::max(1ull, c[4]), (double)c[7] / std::max(1ull, c[4]));
    } else {
        for (int o = 0; o < h->last_owners; o += std::max(1, h->last_owners / 8)) {
            const unsigned long long *q = c.data() + 8 * o;
            const double e = (double)std::max(1ull, q[0]);
            fprintf(stderr, "[slim prof] owner %3d: %5llu entries, mean cycles: ticket %.0f, gather %.0f, wait for turn %.0f, turn %.0f (row sum %.0f, sigmoid + optimiser %.0f, "
                    "row update + release %.0f), write-back %.0f\n", o, q[0], q[1] / e, q[2] / e, q[3] / e, q[4] / e, q[6] / e, q[7] / e, (q[4] - q[6] - q[7]) / e, q[5] / e);
        }
        const unsigned long long *q = c.data() + 8 * MAX_OWNERS;
        fprintf(stderr, "[slim prof] cold: %llu steps, mean cycles: ids + tickets %.0f, gather .. tickets passed on %.0f\n", q[0],
                (double)q[1] / std::max(1ull, q[0]), (double)q[2] / std::max(1ull, q[0]));
    }
}

// Waits for the launch, gives the leased compute units back, fails if the kernel gave up on a hand-off.
void finish_stream(mi355rec_slim *h, Launched &L, int n) {
    hipStream_t s = h->stream;
    int flags[2] = {0, 0}, counters[2] = {0, 0};
    MI_HIP(hipMemcpyAsync(flags, h->queue.ptr, sizeof(flags), hipMemcpyDeviceToHost, s));
    if (L.dense) MI_HIP(hipMemcpyAsync(counters, h->counters.ptr, sizeof(counters), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    L.lease.give_back();
    L.end_serial();
    if (L.dense) {
        h->last_owners = counters[0];
        h->last_cold = counters[1];
    }
    if (flags[1]) {
        // Steps of the epoch have been applied, others not, and nothing records which: the model is neither the one before the call nor a
        // trained one.  There is no copy to roll back to (S is n_items^2 cells), so the handle says so from now on instead of training on.
        h->aborted = true;
        fail(MI355REC_E_HIP, "SLIM-BPR: a hand-off between steps did not arrive (dataflow kernel aborted); S holds part of an epoch -- this handle "
                             "refuses further calls, create a new one");
    }
    if (L.profile) print_profile(h);
    h->steps_done += n;
}

// Steps first .. first + n - 1 of a set, scheduled and run on the main stream, one thing after the other.
template <class T>
void run_stream(mi355rec_slim *h, StreamSet &st, int n, double &sum_profile, int first = 0) {
    schedule_stream(h, st, n, first, h->stream);
    sum_profile += 0.5 * (double)st.n_cells;
    Launched L;
    launch_stream<T>(h, st, n, first, L);
    finish_stream(h, L, n);
    st.epoch = -1;
}

void prune_rows(mi355rec_slim *h, int with_diag) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    h->dispatch_timers.next(e0, e1, 1 << 30);
    hipExtLaunchKernelGGL(slim_prune_kernel, dim3(std::min(h->n_items, multiprocessor_count() * 8)), dim3(PRUNE_THREADS), 0, h->stream,
                          e0, e1, 0, reinterpret_cast<unsigned long long *>(h->S.ptr), h->n_items, h->cfg.topK, with_diag);
    h->stats.n_launches += 1;
    MI_HIP(hipGetLastError());
}

// One epoch of n steps of a set, scheduled and run on the main stream; the sparse store's epoch in segments with the rows pruned
// between them (sparse_segments).
template <class T>
void run_epoch_stream(mi355rec_slim *h, StreamSet &st, int n, double &sum_profile) {
    for (const Segment &seg : sparse_segments(n, h->cfg.train_with_sparse_weights != 0)) {
        run_stream<T>(h, st, seg.count, sum_profile, seg.first);
        if (seg.prune_after) prune_rows(h, 0);
    }
}

void require_consistent(const mi355rec_slim *h) {
    if (h->aborted) fail(MI355REC_E_HIP, "SLIM-BPR: an earlier call on this handle was aborted inside an epoch; its model is inconsistent -- create a new handle");
}

void begin_call(mi355rec_slim *h) {
    require_consistent(h);
    MI_HIP(hipMemsetAsync(h->loss_slots.ptr, 0, sizeof(double) * LOSS_SLOTS, h->stream));
    h->dispatch_timers.reset();
    h->stats = mi355rec_stats{};
    h->timer.start(h->stream);
}

void end_call(mi355rec_slim *h, long long n_steps, double sum_profile) {
    h->timer.stop(h->stream);
    h->h_loss.resize(LOSS_SLOTS);
    h->loss_slots.download(h->h_loss.data(), LOSS_SLOTS, h->stream);
    MI_HIP(hipStreamSynchronize(h->stream));
    double loss = 0;
    for (double v : h->h_loss) loss += v;
    h->stats.call_ms = h->timer.elapsed_ms();
    h->stats.kernel_ms = h->dispatch_timers.total_ms();
    h->stats.n_timed = h->dispatch_timers.used;
    h->stats.n_units = n_steps;
    // ALGORITHMIC bytes, SURVEY.md section 8(d): 20 * L_u per step (profile ids + 2 gathered rows read + 2 rows written)
    h->stats.algorithmic_bytes = 20.0 * sum_profile;
    h->stats.loss = loss;
}

// an epoch of the on-device sampler has been applied to S: the set it ran from is the current one
void epoch_applied(mi355rec_slim *h) {
    h->cur ^= 1;
    h->epochs_done += 1;
    h->last_native = true;
}

template <class T>
void run_epochs_typed(mi355rec_slim *h, int n_epochs) {
    const int n = h->n_users + 1;                            // totalNumberOfBatch with batch_size 1 (.pyx:215)
    ensure_set_capacity(h, h->set[0], (size_t)n);
    ensure_set_capacity(h, h->set[1], (size_t)n);
    begin_call(h);
    double sum_profile = 0;
    const bool ahead = schedules_ahead(h);
    for (int e = 0; e < n_epochs; ++e) {
        const long long epoch = h->epochs_done;
        StreamSet &st = h->set[h->cur ^ 1];
        if (!ahead) {
            draw_epoch<T>(h, st, epoch, n, h->stream);
            run_epoch_stream<T>(h, st, n, sum_profile);
        } else {
            if (!(st.epoch == epoch && st.n == n)) {            // (first epoch of the handle, or a replayed stream took the set)
                draw_epoch<T>(h, st, epoch, n, h->side);
                schedule_stream(h, st, n, 0, h->side);
                st.epoch = epoch;
            }
            sum_profile += 0.5 * (double)st.n_cells;
            Launched L;
            launch_stream<T>(h, st, n, 0, L);
            // ... and while it runs: the next epoch's stream, into the other set (kept for the next call if this was the last)
            StreamSet &nx = h->set[h->cur];
            try {
                draw_epoch<T>(h, nx, epoch + 1, n, h->side);
                schedule_stream(h, nx, n, 0, h->side);
                nx.epoch = epoch + 1;
            } catch (...) {
                // The look-ahead failed (allocation, a HIP error) while this epoch's kernel is in flight: finish the epoch first --
                // drain, return the lease, advance the counters (S has moved) -- and drop the half-made set; only then report
                // (the lease went back with owners still resident and the epoch would have been applied twice).
                nx.epoch = -1;
                nx.n = 0;
                finish_stream(h, L, n);
                epoch_applied(h);
                throw;
            }
            finish_stream(h, L, n);
        }
        epoch_applied(h);
    }
    end_call(h, (long long)n * n_epochs, sum_profile);
}

template <class T>
void topk_slabs_on_device(mi355rec_slim *h, int topK, DeviceBuffer<int> &d_idx, DeviceBuffer<float> &d_val);

// W = similarityMatrixTopK(get_S(), topK) as it stands in device buffers after build_w_on_device: the canonical CSR is d_indptr
// [n_items + 1] and the first d_indptr[n_items] entries of d_indices / val2_sorted (each n_items * topK long), rows with strictly
// ascending columns; d_idx / d_val are the per-row slabs of get_S().  The rest is scratch of the build, alive until the caller lets go.
struct WBuild {
    DeviceBuffer<int> d_idx, slot, slot_sorted, col_start, d_indptr, d_indices;
    DeviceBuffer<float> d_val, val2, val2_sorted;
    DeviceBuffer<unsigned long long> key, key_sorted;
    DeviceBuffer<unsigned> key2, key2_sorted;
    DeviceBuffer<unsigned char> tmp;
    size_t n_slots = 0;
};
constexpr int W_BUILD_LAUNCHES = 7;     // selection, keys, sort, column starts, keep, sort, CSR

// The first half of mi355rec_slim_get_W_csr, queued on the handle's stream and not waited for: also what
// mi355rec_spscorer_update_from_slim hands to the sparse scorer.
template <class T>
void build_w_on_device(mi355rec_slim *h, int topK, WBuild &w) {
    MI_REQUIRE(h->n_items <= 65535, "n_items = %d: the device-side column selection packs items into 16 bits", h->n_items);
    hipStream_t s = h->stream;
    DeviceBuffer<int> &d_idx = w.d_idx, &slot = w.slot, &slot_sorted = w.slot_sorted, &col_start = w.col_start, &d_indptr = w.d_indptr,
                      &d_indices = w.d_indices;
    DeviceBuffer<float> &d_val = w.d_val, &val2 = w.val2, &val2_sorted = w.val2_sorted;
    DeviceBuffer<unsigned long long> &key = w.key, &key_sorted = w.key_sorted;
    DeviceBuffer<unsigned> &key2 = w.key2, &key2_sorted = w.key2_sorted;
    DeviceBuffer<unsigned char> &tmp = w.tmp;
    topk_slabs_on_device<T>(h, topK, d_idx, d_val);
    const size_t n_slots = (size_t)h->n_items * topK;
    MI_REQUIRE(n_slots < (size_t)INT32_MAX, "too many slab entries");
    key.alloc(n_slots); key_sorted.alloc(n_slots); slot.alloc(n_slots); slot_sorted.alloc(n_slots);
    const unsigned grid = (unsigned)((n_slots + 255) / 256);
    hipLaunchKernelGGL(slim_w_rank_keys_kernel, dim3(grid), dim3(256), 0, s, d_idx.ptr, d_val.ptr, n_slots, topK, key.ptr, slot.ptr);
    run_with_scratch(tmp, Grow::Exact, s, n_slots, n_slots, [&](void *scratch, size_t &bytes, size_t count) {
        return rocprim::radix_sort_pairs(scratch, bytes, key.ptr, key_sorted.ptr, slot.ptr, slot_sorted.ptr, count, 0, 64, s);
    });
    col_start.alloc((size_t)h->n_items + 1);
    hipLaunchKernelGGL(slim_w_col_start_kernel, dim3((unsigned)((h->n_items + 256) / 256)), dim3(256), 0, s, key_sorted.ptr, n_slots, h->n_items, col_start.ptr);
    key2.alloc(n_slots); key2_sorted.alloc(n_slots); val2.alloc(n_slots); val2_sorted.alloc(n_slots);
    hipLaunchKernelGGL(slim_w_keep_kernel, dim3(grid), dim3(256), 0, s, key_sorted.ptr, slot_sorted.ptr, col_start.ptr, d_val.ptr, n_slots, topK, topK,
                       key2.ptr, val2.ptr);
    run_with_scratch(tmp, Grow::Exact, s, n_slots, n_slots, [&](void *scratch, size_t &bytes, size_t count) {
        return rocprim::radix_sort_pairs(scratch, bytes, key2.ptr, key2_sorted.ptr, val2.ptr, val2_sorted.ptr, count, 0, 32, s);
    });
    d_indptr.alloc((size_t)h->n_items + 1); d_indices.alloc(n_slots);
    hipLaunchKernelGGL(slim_w_csr_kernel, dim3(std::max(grid, (unsigned)((h->n_items + 256) / 256))), dim3(256), 0, s, key2_sorted.ptr, n_slots, h->n_items,
                       d_indptr.ptr, d_indices.ptr);
    MI_HIP(hipGetLastError());
    w.n_slots = n_slots;
}

// ... and the second half: the download
template <class T>
void get_w_csr_typed(mi355rec_slim *h, int topK, int *nbr_idx, float *nbr_val, int *indptr, int *indices, float *data, long long *nnz) {
    hipStream_t s = h->stream;
    WBuild w;
    build_w_on_device<T>(h, topK, w);
    w.d_indptr.download(indptr, (size_t)h->n_items + 1, s);
    MI_HIP(hipStreamSynchronize(s));
    const size_t n_kept = (size_t)indptr[h->n_items];
    *nnz = (long long)n_kept;
    if (n_kept) {
        w.d_indices.download(indices, n_kept, s);
        w.val2_sorted.download(data, n_kept, s);
    }
    if (nbr_idx) w.d_idx.download(nbr_idx, w.n_slots, s);
    if (nbr_val) w.d_val.download(nbr_val, w.n_slots, s);
    MI_HIP(hipStreamSynchronize(s));
}

// mi355rec_spscorer_update_from_slim: the first half again, with the sparse scorer's spare buffers in the place of the host
template <class T>
void spscorer_update_typed(mi355rec_slim *h, mi355rec_spscorer *sc, int topK) {
    hipStream_t s = h->stream;
    spscorer_adopt_begin(sc, s);
    WBuild w;
    build_w_on_device<T>(h, topK, w);
    const double store_bytes = h->cfg.symmetric ? (double)(h->G.count * sizeof(Granule)) : (double)h->S.count;
    spscorer_adopt(sc, s, w.d_indptr.ptr, w.d_indices.ptr, w.val2_sorted.ptr, w.n_slots, store_bytes, W_BUILD_LAUNCHES);
}

template <class T>
void topk_slabs_on_device(mi355rec_slim *h, int topK, DeviceBuffer<int> &d_idx, DeviceBuffer<float> &d_val) {
    const int n_pad = (h->n_items + 3) & ~3;
    const size_t lds = (size_t)n_pad * 4 + (size_t)AUX_WORDS * 4;
    if (lds + 2048 > 160 * 1024)
        fail(MI355REC_E_UNSUPPORTED, "n_items = %d: a row of S does not fit the 160 KiB LDS for the top-K selection", h->n_items);
    const size_t n_out = (size_t)h->n_items * topK;
    d_idx.alloc(n_out);
    d_val.alloc(n_out);
    SlimParams<T> p{};
    fill_params(h, h->set[h->cur], p);
    auto k = slim_topk_kernel<T, 1024>;
    MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int per_cu = std::max(1, std::min(2, (int)((160 * 1024) / (lds + 2048))));
    hipLaunchKernelGGL(k, dim3(std::min(h->n_items, multiprocessor_count() * per_cu)), dim3(1024), lds, h->stream, p, topK,
                       n_pad, d_idx.ptr, d_val.ptr);
    MI_HIP(hipGetLastError());
}

template <class T>
void get_topk_typed(mi355rec_slim *h, int topK, int *nbr_idx, float *nbr_val) {
    DeviceBuffer<int> d_idx;
    DeviceBuffer<float> d_val;
    topk_slabs_on_device<T>(h, topK, d_idx, d_val);
    const size_t n_out = (size_t)h->n_items * topK;
    d_idx.download(nbr_idx, n_out, h->stream);
    d_val.download(nbr_val, n_out, h->stream);
    MI_HIP(hipStreamSynchronize(h->stream));
}

template <class T>
void get_dense_typed(mi355rec_slim *h, float *S) {
    const size_t n2 = (size_t)h->n_items * h->n_items;
    DeviceBuffer<float> out;
    out.alloc(n2);
    SlimParams<T> p{};
    fill_params(h, h->set[h->cur], p);
    hipLaunchKernelGGL(slim_dense_kernel<T>, dim3((unsigned)std::min<size_t>((n2 + 255) / 256, 8192)), dim3(256), 0, h->stream, p, out.ptr);
    MI_HIP(hipGetLastError());
    out.download(S, n2, h->stream);
    MI_HIP(hipStreamSynchronize(h->stream));
}

}  // namespace

extern "C" int mi355rec_slim_create(mi355rec_slim_t *out, const mi355rec_slim_config *cfg, int32_t n_users, int32_t n_items,
                                    const int32_t *indptr, const int32_t *indices) {
    return guarded([&] {
        MI_REQUIRE(out && cfg && indptr && indices, "NULL argument");
        MI_REQUIRE(n_users > 0 && n_items > 0, "empty URM");
        MI_REQUIRE(cfg->sgd_mode >= MI355REC_SGD && cfg->sgd_mode <= MI355REC_ADAM, "Value for 'sgd_mode' not recognized (%d)",
                   cfg->sgd_mode);
        MI_REQUIRE(cfg->precision == MI355REC_F32 || cfg->precision == MI355REC_F64, "precision must be MI355REC_F32 or MI355REC_F64");
        ensure_device();
        std::unique_ptr<mi355rec_slim> h(new mi355rec_slim());
        h->cfg = *cfg;
        if (cfg->train_with_sparse_weights) {
            MI_REQUIRE(cfg->precision == MI355REC_F64, "train_with_sparse_weights needs precision MI355REC_F64 (the selections compare values)");
            MI_REQUIRE(cfg->topK >= 0, "topK must be >= 0 (0 = False)");
            h->cfg.symmetric = 0;                                // .pyx:112-113
        }
        h->n_users = n_users;
        h->n_items = n_items;
        // the symmetric store keeps float32 values inside 8-byte granules and computes in float64 whatever `precision` says
        h->f64 = cfg->precision == MI355REC_F64 || h->cfg.symmetric;
        h->nnz = (size_t)indptr[n_users];
        MI_REQUIRE(h->nnz > 0, "URM has no interactions");
        h->open(1);
        h->open_side();
        h->dispatch_timers.reserve(64);
        hipStream_t s = h->stream;
        const size_t ts = h->f64 ? sizeof(double) : sizeof(float);
        h->indptr.upload(indptr, (size_t)n_users + 1, s);
        h->indices.upload(indices, h->nnz, s);
        if (h->cfg.symmetric) {
            // Triangular_Matrix :1237-1254 the packed lower triangle
            h->G.alloc_zero((size_t)n_items * ((size_t)n_items + 1) / 2, s);
            h->oc.alloc_zero(4 * (size_t)n_items, s);
        } else {
            h->S.alloc_zero((size_t)n_items * n_items * ts, s);     // .pyx:129 dense n x n
            if (h->cfg.train_with_sparse_weights)                        // .pyx:124: an empty tree per row
                hipLaunchKernelGGL(slim_no_nodes_kernel, dim3(multiprocessor_count() * 8), dim3(256), 0, s,
                                   reinterpret_cast<unsigned long long *>(h->S.ptr), (size_t)n_items * n_items);
            h->c1.alloc_zero((size_t)n_items * ts, s);
            h->c2.alloc_zero((size_t)n_items * ts, s);
            h->ticket.alloc_zero((size_t)n_items, s);
            h->hot_rank.alloc((size_t)n_items);
            h->hot_tables.alloc_zero(3 * MAX_OWNERS, s);
            h->counters.alloc_zero(2, s);
            h->cnt_sorted.alloc((size_t)n_items);
            h->item_by_cnt.alloc((size_t)n_items);
            std::vector<int> iota((size_t)n_items);
            for (int i = 0; i < n_items; ++i) iota[(size_t)i] = i;
            h->iota.upload(iota.data(), iota.size(), s);
            MI_HIP(hipStreamSynchronize(s));                         // (iota is read from host memory)
        }
        h->queue.alloc_zero(4, s);
        h->loss_slots.alloc_zero(LOSS_SLOTS, s);
        MI_HIP(hipStreamSynchronize(s));
        *out = h.release();
    });
}

extern "C" int mi355rec_slim_run_epochs(mi355rec_slim_t h, int32_t n_epochs) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL handle");
        MI_REQUIRE(n_epochs >= 0, "n_epochs must be >= 0");
        enter_call(h);
        ReleaseScope scope(h->stream, h->side);
        if (h->f64) run_epochs_typed<double>(h, n_epochs); else run_epochs_typed<float>(h, n_epochs);
    });
}

extern "C" int mi355rec_slim_run_samples(mi355rec_slim_t h, const int32_t *u, const int32_t *i, const int32_t *j, int64_t n) {
    return guarded([&] {
        MI_REQUIRE(h && u && i && j, "NULL argument");
        MI_REQUIRE(n >= 0 && n < (1ll << 30), "n out of range");
        enter_call(h);
        if (n == 0) return;
        ReleaseScope scope(h->stream, h->side);
        StreamSet &st = h->set[h->cur ^ 1];                  // (a stream scheduled ahead for the next native epoch, if any, is given up)
        ensure_set_capacity(h, st, (size_t)n);
        st.epoch = -1;
        hipStream_t s = h->stream;
        for (int64_t t = 0; t < n; ++t)
            MI_REQUIRE(u[t] >= 0 && u[t] < h->n_users && i[t] >= 0 && i[t] < h->n_items && j[t] >= 0 && j[t] < h->n_items && i[t] != j[t],
                       "sample %lld out of range (or its positive item is its negative item)", (long long)t);
        MI_HIP(hipMemcpyAsync(st.su.ptr, u, sizeof(int) * n, hipMemcpyHostToDevice, s));
        MI_HIP(hipMemcpyAsync(st.si.ptr, i, sizeof(int) * n, hipMemcpyHostToDevice, s));
        MI_HIP(hipMemcpyAsync(st.sj.ptr, j, sizeof(int) * n, hipMemcpyHostToDevice, s));
        begin_call(h);
        double sum_profile = 0;
        // (the n samples are ONE epoch of n steps: that is what the sparse store's rebalance rule counts against)
        if (h->f64) run_epoch_stream<double>(h, st, (int)n, sum_profile); else run_epoch_stream<float>(h, st, (int)n, sum_profile);
        h->cur ^= 1;
        h->last_native = false;
        end_call(h, n, sum_profile);
    });
}

extern "C" int mi355rec_slim_get_last_samples(mi355rec_slim_t h, int32_t *u, int32_t *i, int32_t *j, int64_t cap, int64_t *n) {
    return guarded([&] {
        MI_REQUIRE(h && n, "NULL argument");
        ensure_device();
        const int64_t have = h->epochs_done > 0 && h->last_native ? h->n_users + 1 : 0;
        *n = have;
        const size_t m = (size_t)std::min<int64_t>(cap, have);
        const StreamSet &st = h->set[h->cur];
        if (u && m) st.su.download(u, m, h->stream);
        if (i && m) st.si.download(i, m, h->stream);
        if (j && m) st.sj.download(j, m, h->stream);
        MI_HIP(hipStreamSynchronize(h->stream));
    });
}

extern "C" int mi355rec_slim_get_S_topk(mi355rec_slim_t h, int32_t topK, int32_t *nbr_idx, float *nbr_val) {
    return guarded([&] {
        MI_REQUIRE(h && nbr_idx && nbr_val, "NULL argument");
        require_consistent(h);
        MI_REQUIRE(topK >= 1, "topK must be >= 1 (use mi355rec_slim_get_S_dense for the full matrix)");
        enter_call(h);
        topK = std::min(topK, h->n_items);
        if (topK > MAX_TOPK) fail(MI355REC_E_UNSUPPORTED, "topK = %d exceeds the in-LDS selection limit of %d", topK, MAX_TOPK);
        if (h->f64) get_topk_typed<double>(h, topK, nbr_idx, nbr_val); else get_topk_typed<float>(h, topK, nbr_idx, nbr_val);
    });
}

extern "C" int mi355rec_slim_get_W_csr(mi355rec_slim_t h, int32_t topK, int32_t *nbr_idx, float *nbr_val, int32_t *indptr, int32_t *indices,
                                       float *data, int64_t *nnz) {
    return guarded([&] {
        MI_REQUIRE(h && indptr && indices && data && nnz, "NULL argument");
        require_consistent(h);
        MI_REQUIRE(topK >= 1, "topK must be >= 1");
        enter_call(h);
        ReleaseScope scope(h->stream, h->side);
        topK = std::min(topK, h->n_items);
        if (topK > MAX_TOPK) fail(MI355REC_E_UNSUPPORTED, "topK = %d exceeds the in-LDS selection limit of %d", topK, MAX_TOPK);
        long long n = 0;
        if (h->f64) get_w_csr_typed<double>(h, topK, nbr_idx, nbr_val, indptr, indices, data, &n);
        else get_w_csr_typed<float>(h, topK, nbr_idx, nbr_val, indptr, indices, data, &n);
        *nnz = (int64_t)n;
    });
}

// Lives here, as mi355rec_scorer_update_from_mf lives in mf.hip: it launches this file's own read-out.  The refusals come before the
// device is touched; the scorer's stream is drained, the build and the copy are queued on this handle's stream behind its own work,
// and that stream is waited for (spscorer_adopt_begin / spscorer_adopt, handoff.hip).
extern "C" int mi355rec_spscorer_update_from_slim(mi355rec_spscorer_t scorer, mi355rec_slim_t h, int32_t topK) {
    return guarded([&] {
        MI_REQUIRE(scorer && h, "NULL handle");
        MI_REQUIRE(h->n_items == scorer->n_mid && h->n_items == scorer->n_items,
                   "the SLIM handle has %d items, the scorer's B is %d x %d (an item-based scorer over the same items is needed)", h->n_items,
                   scorer->n_mid, scorer->n_items);
        MI_REQUIRE(topK >= 1, "topK must be >= 1");
        if (h->cfg.train_with_sparse_weights)
            fail(MI355REC_E_UNSUPPORTED, "a SLIM handle created with train_with_sparse_weights cannot be handed to a scorer: reading its model "
                                         "prunes it");
        if (h->n_items > 65535)
            fail(MI355REC_E_UNSUPPORTED, "n_items = %d: the device-side column selection packs items into 16 bits", h->n_items);
        require_consistent(h);
        enter_call(h);
        ReleaseScope scope(h->stream, h->side, scorer->stream);
        topK = std::min(topK, h->n_items);
        if (topK > MAX_TOPK) fail(MI355REC_E_UNSUPPORTED, "topK = %d exceeds the in-LDS selection limit of %d", topK, MAX_TOPK);
        if (h->f64) spscorer_update_typed<double>(h, scorer, topK); else spscorer_update_typed<float>(h, scorer, topK);
    });
}

extern "C" int mi355rec_slim_get_S_sparse(mi355rec_slim_t h, int32_t *nbr_idx, float *nbr_val) {
    return guarded([&] {
        MI_REQUIRE(h && nbr_idx && nbr_val, "NULL argument");
        require_consistent(h);
        MI_REQUIRE(h->cfg.train_with_sparse_weights && h->cfg.topK >= 1, "handle was not created with train_with_sparse_weights and topK >= 1");
        ensure_device();
        const int width = h->cfg.topK;
        const size_t n_out = (size_t)h->n_items * width;
        DeviceBuffer<int> d_idx;
        DeviceBuffer<float> d_val;
        d_idx.alloc(n_out);
        d_val.alloc(n_out);
        h->dispatch_timers.reset();
        prune_rows(h, 1);
        hipLaunchKernelGGL(slim_list_kernel, dim3(std::min(h->n_items, multiprocessor_count() * 8)), dim3(PRUNE_THREADS), 0, h->stream,
                           reinterpret_cast<const unsigned long long *>(h->S.ptr), h->n_items, width, d_idx.ptr, d_val.ptr);
        MI_HIP(hipGetLastError());
        d_idx.download(nbr_idx, n_out, h->stream);
        d_val.download(nbr_val, n_out, h->stream);
        MI_HIP(hipStreamSynchronize(h->stream));
    });
}

extern "C" int mi355rec_slim_get_S_dense(mi355rec_slim_t h, float *S) {
    return guarded([&] {
        MI_REQUIRE(h && S, "NULL argument");
        require_consistent(h);
        enter_call(h);
        if (h->f64) get_dense_typed<double>(h, S); else get_dense_typed<float>(h, S);
    });
}

extern "C" int mi355rec_slim_get_stats(mi355rec_slim_t h, mi355rec_stats *stats) { return handle_get_stats(h, stats); }

extern "C" int mi355rec_slim_schedule_info(mi355rec_slim_t h, int32_t *n_owned_rows, int32_t *n_cold_steps) {
    return guarded([&] {
        MI_REQUIRE(h && n_owned_rows && n_cold_steps, "NULL argument");
        *n_owned_rows = h->last_owners;
        *n_cold_steps = h->last_cold;
    });
}

extern "C" void mi355rec_slim_destroy(mi355rec_slim_t h) { handle_destroy(h); }
