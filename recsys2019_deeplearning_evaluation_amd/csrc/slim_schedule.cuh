// slim_schedule.cuh -- what is known about a sample stream before its first step runs: the sampler, DepParams and the kernels that
// turn the stream into tickets, owners, step descriptors and last writers, and ShortProfile, the predicate that splits the two queues.
#pragma once

#include "slim_flow.cuh"

namespace mi355rec {
namespace {

template <class T>
__global__ __launch_bounds__(256) void slim_sample_kernel(SlimParams<T> p, int *su, int *si, int *sj) {
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t >= p.n_steps) return;
    int u, i, j;
    sample_bpr(p.seed, (unsigned long long)(p.epoch * (long long)p.n_steps + t), p.n_users, p.n_items, p.indptr, p.indices, u, i, j);
    su[t] = u;
    si[t] = i;
    sj[t] = j;
}

// ---- dependencies of the stream ---------------------------------------------------------------------------------------
struct DepParams {
    int n_steps, n_items;
    const int *indptr, *indices, *su, *si, *sj;
    unsigned long long *keys;       // item pass: item << 32 | step;  cell pass: cell << 32 | step
    int *vals;                      // item pass: 2 step + role;      cell pass: cell slot
    const unsigned long long *keys_sorted;
    const int *vals_sorted;
    int *seq, *iprev;
    int *len2;                      // 2 L_u per step
    const long long *cellptr;
    int *pred;
    long long n_cells;
    int step_bits;                  // cell pass: key = cell << step_bits | step (the radix sort walks as few bits as the stream needs)
    int *bad_step;                  // symmetric store: first step whose negative item is in its user's profile (INT_MAX: none)
    unsigned no_cell;               // the diagonal's stand-in: all ones in the cell field (it is read but never written: it orders nothing)
    // owned rows of the dense store
    int *run_start;                 // [n_items] first position of the item's run in the sorted pairs
    unsigned *item_cnt;             // [n_items] steps of the stream on the item (0: memset)
    const unsigned *cnt_sorted;     // item_cnt in descending order ...
    const int *item_by_cnt;         // ... and whose count it is
    int *hot_rank, *hot_item, *lst_begin, *lst_len, *n_hot;
    int max_owners, min_steps;
    unsigned char *cold_flag;       // [n_steps] 1: neither row of the step is owned
    StepDesc *desc, *own_desc;
};

__global__ __launch_bounds__(256) void slim_item_keys_kernel(const DepParams d) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= d.n_steps) return;
    d.keys[2 * t] = ((unsigned long long)d.si[t] << 32) | (unsigned)t;
    d.vals[2 * t] = 2 * t;
    d.keys[2 * t + 1] = ((unsigned long long)d.sj[t] << 32) | (unsigned)t;
    d.vals[2 * t + 1] = 2 * t + 1;
    d.len2[t] = 2 * (d.indptr[d.su[t] + 1] - d.indptr[d.su[t]]);
}

// ticket number = how many earlier steps of the stream touch the same item = position inside the item's run; the step before it
// on the item; per item the run's start and length
__global__ __launch_bounds__(256) void slim_seq_kernel(const DepParams d) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int n2 = 2 * d.n_steps;
    if (q >= n2) return;
    const unsigned long long key = d.keys_sorted[q];
    const unsigned long long first_key = key & 0xFFFFFFFF00000000ull;
    int lo = 0, hi = q;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (d.keys_sorted[mid] < first_key) lo = mid + 1; else hi = mid;
    }
    const int slot = d.vals_sorted[q];
    d.seq[slot] = q - lo;
    d.iprev[slot] = q > lo ? d.vals_sorted[q - 1] >> 1 : -1;
    const int item = (int)(key >> 32);
    if (q == lo) d.run_start[item] = q;
    if (q + 1 == n2 || (int)(d.keys_sorted[q + 1] >> 32) != item) d.item_cnt[item] = (unsigned)(q - lo + 1);
}

// The busiest rows get owners: the first max_owners items of the descending count order that have at least min_steps steps.
__global__ __launch_bounds__(256) void slim_owners_kernel(const DepParams d) {
    const int h = threadIdx.x;
    __shared__ int s_n;
    if (h == 0) s_n = 0;
    __syncthreads();
    if (h < d.max_owners && h < d.n_items && (int)d.cnt_sorted[h] >= d.min_steps) {
        const int item = d.item_by_cnt[h];
        d.hot_rank[item] = h;
        d.hot_item[h] = item;
        d.lst_begin[h] = d.run_start[item];
        d.lst_len[h] = (int)d.cnt_sorted[h];
        atomicAdd(&s_n, 1);            // (the qualifying owners are a prefix of the order)
    }
    __syncthreads();
    if (h == 0) *d.n_hot = s_n;
}

// per step, stream order (dense store: after the owners are known)
__global__ __launch_bounds__(256) void slim_desc_kernel(const DepParams d, const int symmetric) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= d.n_steps) return;
    const int u = d.su[t], i = d.si[t], j = d.sj[t];
    const int rs = d.indptr[u], L = d.indptr[u + 1] - rs;
    StepDesc e;
    e.rs = rs; e.L = L; e.i = i; e.j = j;
    if (symmetric) {
        const long long cp = d.cellptr[t];
        e.a = d.iprev[2 * t]; e.b = d.iprev[2 * t + 1]; e.t = (int)(unsigned)cp; e.c = (int)(cp >> 32);
    } else {
        e.a = d.seq[2 * t]; e.b = d.seq[2 * t + 1]; e.t = t; e.c = 0;
        d.cold_flag[t] = d.hot_rank[i] < 0 && d.hot_rank[j] < 0;
    }
    d.desc[t] = e;
}
// per (item, step) pair in sorted order: the entries of the owned rows' lists
__global__ __launch_bounds__(256) void slim_owner_desc_kernel(const DepParams d) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= 2 * d.n_steps) return;
    if (d.hot_rank[(int)(d.keys_sorted[q] >> 32)] < 0) return;
    const int slot = d.vals_sorted[q], t = slot >> 1, role = slot & 1;
    const int u = d.su[t], other = role ? d.si[t] : d.sj[t];
    StepDesc e;
    e.rs = d.indptr[u]; e.L = d.indptr[u + 1] - e.rs; e.i = other; e.j = role;
    e.a = d.seq[2 * t + (1 - role)]; e.b = d.hot_rank[other] >= 0; e.t = t; e.c = 0;
    d.own_desc[q] = e;
}

// symmetric store: one wavefront per step lists the canonical cells of its two rows
__global__ __launch_bounds__(256) void slim_cell_keys_kernel(const DepParams d) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= d.n_steps) return;
    const int u = d.su[t], i = d.si[t], j = d.sj[t];
    const int rs = d.indptr[u], L = d.indptr[u + 1] - rs;
    const long long cp = d.cellptr[t];
    for (int idx = lane; idx < L; idx += 64) {
        const int s = d.indices[rs + idx];
        // (packed lower triangle, as packed_cell: fits 32 bits up to 92 681 items)
        const unsigned ci = s == i ? d.no_cell : (unsigned)packed_cell(i, s);
        const unsigned cj = s == j ? d.no_cell : (unsigned)packed_cell(j, s);
        // A negative item that the user has seen (the reference's sampler never draws one, .pyx:224-232; a replayed stream might):
        // cell (i, j) IS cell (j, i) in this store, the step would touch it twice and wait for its own tag.  Reported, not run.
        if (s == j) atomicMin(d.bad_step, t);
        d.keys[cp + 2 * idx] = ((unsigned long long)ci << d.step_bits) | (unsigned)t;
        d.vals[cp + 2 * idx] = (int)(cp + 2 * idx);
        d.keys[cp + 2 * idx + 1] = ((unsigned long long)cj << d.step_bits) | (unsigned)t;
        d.vals[cp + 2 * idx + 1] = (int)(cp + 2 * idx + 1);
    }
}

__global__ __launch_bounds__(256) void slim_pred_kernel(const DepParams d) {
    const long long q = blockIdx.x * 256ll + threadIdx.x;
    if (q >= d.n_cells) return;
    const unsigned long long key = d.keys_sorted[q];
    const unsigned cell = (unsigned)(key >> d.step_bits);
    int pred = -1;
    if (q > 0 && cell != d.no_cell) {
        const unsigned long long before = d.keys_sorted[q - 1];
        if ((unsigned)(before >> d.step_bits) == cell) pred = (int)(before & ((1ull << d.step_bits) - 1ull));
    }
    d.pred[d.vals_sorted[q]] = pred;
}

}  // namespace
}  // namespace mi355rec

namespace {      // (not mi355rec's: the name of the rocprim::partition instantiation it is an argument of stays what it was)
using mi355rec::FLOW_BLOCK;

struct ShortProfile {
    const int *len2;
    __device__ bool operator()(const int t) const { return len2[t] <= 2 * FLOW_BLOCK; }
};

}  // namespace
