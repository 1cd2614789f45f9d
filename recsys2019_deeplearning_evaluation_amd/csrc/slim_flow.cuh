// slim_flow.cuh -- what the SLIM-BPR kernels share (SlimParams, Granule, StepDesc, the cell update, the claim / wait helpers) and the
// dense store's dataflow kernel: cold_step, owned_row, slim_dense_flow_kernel.  Included by slim.hip after common.h, sampling.cuh and
// wave.cuh; the constants the host's launch plan shares with the kernels are in slim_plan.h.
#pragma once

#include "slim_plan.h"

namespace mi355rec {
namespace {

constexpr long long SPIN_LIMIT_TICKS = 500000000ll;   // 5 s of the 100 MHz wall clock: a stuck hand-off aborts instead of hanging
constexpr unsigned long long MAIL_EMPTY = ~0ull;

struct alignas(8) Granule { float v; unsigned tag; };

// Everything a step needs before its first gather, in ONE 32-byte load (instead of stream position -> sample -> CSR bounds -> ticket
// numbers: four dependent round trips).  Three uses:
//   dense store, steps in stream order / compacted into the cold queue:  a, b = ticket numbers of items i and j
//   dense store, the list of an owned row (sorted order):  i = the OTHER item, j = role of the owned row (0 positive, 1 negative),
//                                                       a = the other item's ticket number, b = 1 if that row is owned, too
//   symmetric store, stream order:  a, b = the step before this one on item i / j (-1: none), (t, c) = first cell slot (low, high)
struct alignas(32) StepDesc { int rs, L, i, j, a, b, t, c; };

// Steps are handed to single wavefronts: one of them fetches LQ_CHUNK consecutive steps from the global in-order queue (one device
// atomic per chunk: 88 per microsecond is all one word sustains) and the wavefronts of the workgroup pop them one by one from LDS.
struct LocalQueue { int next, ready; int base[LQ_RING]; };
constexpr int NO_STEP = 0x7fffffff;

template <class T>
struct SlimParams {
    int n_users, n_items, symmetric, sgd_mode;
    T lr, li_reg, lj_reg, gamma, beta_1, beta_2, one_m_gamma, one_m_beta_1, one_m_beta_2;
    double beta_1_d, beta_2_d;
    unsigned long long seed;
    const int *indptr, *indices;
    T *S;                           // dense store: n_items x n_items
    Granule *G;                     // symmetric store: packed lower triangle of {value, tag of the step that wrote it}
    T *c1, *c2;                     // dense store: per-ITEM optimiser scalars (.pyx:177-181): cache / first moment, second moment
    Granule *oc;                    // symmetric store: the same as [n_items][4] granules (c1 high, c1 low, c2 high, c2 low)
    const int *su, *si, *sj;        // sample stream of the call
    const int *seq;                 // dense: [2 n_steps] ticket numbers of step t on item i_t (2t) and item j_t (2t + 1)
    const int *iprev;               // symmetric: [2 n_steps] the step before t on item i_t / j_t in this call (-1: none)
    const long long *cellptr;       // symmetric: first cell slot of every step (2 per profile entry: row i, row j)
    const int *pred;                // symmetric: per cell slot, the step that touched the cell last (-1: nobody in this call)
    int *ticket;                    // dense: [n_items] steps of this call completed on the item
    int *queue;                     // [0] next step (of the cold list / the short profiles), [1] abort flag, [2] next long profile
    double *loss_slots;             // [LOSS_SLOTS]
    long long epoch;                // RNG counter base
    long long steps_before;         // steps executed before this call (Adam's beta^t, .pyx:313-317)
    int n_steps;
    unsigned tag_base;              // symmetric: step t of this call writes tag tag_base + t + 1
    // dense store, owned rows
    const int *hot_rank;            // [n_items] owner of the item's row, -1: nobody (the row stays in HBM)
    const int *hot_item, *lst_begin, *lst_len;   // [MAX_OWNERS] item, first position and length of its run in the sorted pairs
    const int *n_hot;               // owners in use (decided on the device)
    const StepDesc *desc;           // symmetric store: per step, in stream order
    const int *order;               // symmetric store: the steps with short profiles in stream order, then the others backwards
    int n_short;
    int nap;                        // how much longer a wavefront sleeps between polls once it has polled 24 times in vain
    const StepDesc *cold_desc;      // dense store: the steps with no owned row, in stream order
    const StepDesc *own_desc;       // dense store: per (item, step) pair in sorted order (only the owned items' runs are filled in)
    const int *n_cold;
    unsigned long long *prof;       // optional phase clocks (MI355REC_SLIM_PROF=1), NULL otherwise
    unsigned long long *mail_x, *mail_g;   // [n_steps] steps on TWO owned rows: sum over the negative item's row, sigmoid
};

template <class T> __device__ __forceinline__ T aload(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T> __device__ __forceinline__ void astore(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ Granule gload(const Granule *p) {
    return __builtin_bit_cast(Granule, aload(reinterpret_cast<const unsigned long long *>(p)));
}
__device__ __forceinline__ void gstore(Granule *p, float v, unsigned tag) {
    astore(reinterpret_cast<unsigned long long *>(p), __builtin_bit_cast(unsigned long long, Granule{v, tag}));
}

// Triangular_Matrix.get_value/add_value (.pyx:1290-1330): in symmetric mode (r, c) with c > r lives at (c, r)
// and the store is the packed lower triangle, row r starting at r (r + 1) / 2 (:1237-1254): n (n + 1) / 2 cells
__host__ __device__ __forceinline__ size_t packed_cell(int r, int c) {
    if (c > r) { const int t = r; r = c; c = t; }
    return ((size_t)r * ((size_t)r + 1) >> 1) + (size_t)c;
}
template <class P> __device__ __forceinline__ float stored_value(const P &p, int r, int c) {      // for get_S
    return p.symmetric ? p.G[packed_cell(r, c)].v : (float)p.S[(size_t)r * p.n_items + c];
}

// The cell update v +- lr * (g - reg * v) (.pyx:283-309) with every operation rounded on its own, as the reference's scalar x86 code
// does.  A fused multiply-add is a hair more accurate -- and that hair matters to the sparse store: cells that TIE in the reference
// (a value far below the last bit of the increment it is added to: 1e-18 + 0.05) come out one unit in the last place apart with a
// fused add, and the per-row top-K selection then keeps different nodes (found with profiles of 1 850 items at 3 000 items).
template <class T>
__device__ __forceinline__ T cell_plus(T v, T lr, T g, T reg) {
#pragma clang fp contract(off)
    const T a = reg * v;
    const T b = g - a;
    const T c = lr * b;
    return v + c;
}
template <class T>
__device__ __forceinline__ T cell_minus(T v, T lr, T g, T reg) {
#pragma clang fp contract(off)
    const T a = reg * v;
    const T b = g - a;
    const T c = lr * b;
    return v - c;
}

__device__ __forceinline__ float root(float x) { return sqrtf(x); }
__device__ __forceinline__ double root(double x) { return sqrt(x); }
__device__ __forceinline__ float sigmoid_of_minus(float x) { return 1.f / (1.f + __expf(x)); }
__device__ __forceinline__ double sigmoid_of_minus(double x) { return 1.0 / (1.0 + exp(x)); }

// per-ITEM adaptive step (.pyx:398-436) on cells passed by reference; pw1 / pw2 = 1 - beta^t of this step
template <class T, class P>
__device__ __forceinline__ T slim_adapt_cells(const P &p, T g, T pw1, T pw2, T &c1, T &c2) {
    switch (p.sgd_mode) {
        case MI355REC_ADAGRAD:
            c1 = c1 + g * g;
            return g / (root(c1) + (T)1e-8);
        case MI355REC_RMSPROP:
            c1 = c1 * (T)p.gamma + (T)p.one_m_gamma * (g * g);
            return g / (root(c1) + (T)1e-8);
        case MI355REC_ADAM: {
            c1 = c1 * (T)p.beta_1 + (T)p.one_m_beta_1 * g;
            c2 = c2 * (T)p.beta_2 + (T)p.one_m_beta_2 * (g * g);
            return (c1 / pw1) / (root(c2 / pw2) + (T)1e-8);
        }
        default:
            return g;
    }
}
template <class T, class P>
__device__ __forceinline__ void adam_powers(const P &p, int t, T &pw1, T &pw2) {
    pw1 = (T)1;
    pw2 = (T)1;
    if (p.sgd_mode == MI355REC_ADAM) {
        const double tt = (double)(p.steps_before + t + 1);
        pw1 = (T)(1.0 - pow(p.beta_1_d, tt));
        pw2 = (T)(1.0 - pow(p.beta_2_d, tt));
    }
}

// ---- the stream ---------------------------------------------------------------------------------------------------------
// Every wait is a relaxed poll with a budget: a hand-off that does not arrive within SPIN_LIMIT_TICKS raises the abort flag
// (everybody stops waiting, the call fails) instead of hanging the device.
struct SpinGuard {
    unsigned polls = 0;
    long long t0 = 0;
};
template <class T>
__device__ __forceinline__ bool give_up(const SlimParams<T> &p, SpinGuard &g) {      // wave-uniform answer
    // a waiter that has polled for a while polls less often (p.nap; 0: always every 64 cycles)
    if (p.nap == 0 || g.polls < 24u) __builtin_amdgcn_s_sleep(1);
    else if (p.nap == 1) __builtin_amdgcn_s_sleep(4);
    else if (p.nap == 2) __builtin_amdgcn_s_sleep(12);
    else __builtin_amdgcn_s_sleep(32);
    if ((++g.polls & 127u) != 0) return false;
    int stop = aload(&p.queue[1]);
    const long long now = wall_clock64();
    if (g.t0 == 0) g.t0 = now;
    else if (now - g.t0 > SPIN_LIMIT_TICKS) { astore(&p.queue[1], 1); stop = 1; }
    return __builtin_amdgcn_readfirstlane(stop) != 0;
}

// A ticket says how many steps are still ahead of the waiter on that row, and no step takes less than a microsecond: a waiter
// `ahead` steps away sleeps a quarter of a microsecond per step ahead (at most 8 us) before it looks again.  (Polls are memory-side
// transactions: PMC round 4 counted 5 GB of them per epoch against 0.4 GB of algorithmic bytes.)
__device__ __forceinline__ void nap_by_distance(int ahead) {      // wave-uniform
    ahead = min(ahead - 1, 32);
    for (int n = 0; n < ahead; ++n) __builtin_amdgcn_s_sleep(8);
}

// One lane polls a word for the whole wavefront.
template <class T>
__device__ __forceinline__ bool wave_wait_word(const SlimParams<T> &p, const int *word, int want, int lane) {
    SpinGuard sg;
    for (;;) {
        int v = want;
        if (lane == 0) v = aload(word);
        v = __builtin_amdgcn_readfirstlane(v);
        if (v == want) return true;
        if (p.nap) nap_by_distance(want - v);
        if (give_up(p, sg)) return false;
    }
}
template <class T>
__device__ __forceinline__ bool wave_wait_mail(const SlimParams<T> &p, unsigned long long *word, int lane, double &out) {
    SpinGuard sg;
    for (;;) {
        unsigned long long v = 0;
        if (lane == 0) v = aload(word);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
        v = ((unsigned long long)hi << 32) | lo;
        if (v != MAIL_EMPTY) { out = __longlong_as_double((long long)v); return true; }
        if (give_up(p, sg)) return false;
    }
}

// A `volatile T *` into LDS that has lost its address space on the way (a function argument, the address of a __shared__ member) is
// read and written with flat_load / flat_store ... sc0 sc1, each behind an s_waitcnt vmcnt(0): the access goes down the vector-memory
// path, waits for every outstanding global load of the wavefront, and takes several hundred cycles -- found in round 6 on the turn word
// and the optimiser cells of an owned row, i.e. four such round trips inside every turn of the busiest row's chain.  The low 32 bits of
// a generic address inside the shared aperture are the LDS offset: through this cast the same accesses are ds_read / ds_write.
template <class T>
__device__ __forceinline__ __attribute__((address_space(3))) volatile T *as_lds(volatile T *q) {
    return (__attribute__((address_space(3))) volatile T *)(uintptr_t)(unsigned)(unsigned long long)q;
}

__device__ __forceinline__ unsigned long long shader_clock() {   // not reordered against memory operations
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}

// Next step of the in-order queue for this wavefront (NO_STEP: the queue is empty or the launch is being abandoned).  The chunks are
// fetched in the order of their generations, so what a workgroup holds is always a prefix of what it will hold: a step it has not
// handed out yet can only be waited for by steps it has not handed out either.
template <class T, class ReadyPtr, class BasesPtr>
__device__ __forceinline__ int claim_step_on(const SlimParams<T> &p, const int lane, const int k, ReadyPtr ready, BasesPtr bases) {
    const int gen = k / LQ_CHUNK, off = k % LQ_CHUNK;
    SpinGuard sg;
    unsigned spins = 0;
    if (off == 0) {
        while (__builtin_amdgcn_readfirstlane(*ready) != gen)
            if ((++spins & 1023u) == 0 && give_up(p, sg)) return NO_STEP;
        int base = 0;
        if (lane == 0) base = aload(&p.queue[1]) ? NO_STEP : atomicAdd(&p.queue[0], LQ_CHUNK);
        base = __builtin_amdgcn_readfirstlane(base);
        if (lane == 0) bases[gen % LQ_RING] = base;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) *ready = gen + 1;
        return base;
    }
    while (__builtin_amdgcn_readfirstlane(*ready) <= gen)
        if ((++spins & 1023u) == 0 && give_up(p, sg)) return NO_STEP;
    asm volatile("" ::: "memory");
    const int base = __builtin_amdgcn_readfirstlane(bases[gen % LQ_RING]);
    if (__builtin_amdgcn_readfirstlane(*ready) > gen + LQ_RING) {       // (the ring slot may have been reused: never seen, checked anyway)
        if (lane == 0) astore(&p.queue[1], 1);
        return NO_STEP;
    }
    return base >= NO_STEP - LQ_CHUNK ? NO_STEP : base + off;
}
// LDS_POLLS: the queue's two LDS words read and written as ds_read / ds_write (as_lds) instead of through the generic volatile pointers'
// flat_load ... sc0 sc1.  The dense store's cold steps want it (a poll comes back four times as fast, a claimed step starts sooner:
// epoch 1.77 -> 1.58-1.63 ms); the symmetric store's wavefronts, which ALL pass through here and are bound by the chain behind it,
// do not (10.4 -> 11.1 ms: the faster polls take issue slots from the wavefronts that work) -- both measured in round 6.
template <bool LDS_POLLS, class T>
__device__ __forceinline__ int claim_step(const SlimParams<T> &p, LocalQueue *lq, const int lane) {
    int k = 0;
    if (lane == 0) k = atomicAdd(&lq->next, 1);
    k = __builtin_amdgcn_readfirstlane(k);
    if constexpr (LDS_POLLS) return claim_step_on(p, lane, k, as_lds((volatile int *)&lq->ready), as_lds((volatile int *)lq->base));
    else return claim_step_on(p, lane, k, (volatile int *)&lq->ready, (volatile int *)lq->base);
}

// The sigmoid and the optimiser step of an OWNED row's step sit on the critical path of the whole epoch (the turn of the busiest
// row), so their instruction count matters: the argument is reduced in float64 (x log2(e) = n + f, |f| <= 1/2, exact), 2^f comes
// from v_exp_f32 and the reciprocals from v_rcp_f32 (1 ulp each): relative error of the step ~2e-7, against 1e-5 asked of the
// cells it moves.  Moments stay in float64.
__device__ __forceinline__ double fast_sigmoid_of_minus(double x) {
    const double y = fmin(fmax(x * 1.4426950408889634, -120.0), 120.0);
    const double n = rint(y);
    const float e = ldexpf(__builtin_amdgcn_exp2f((float)(y - n)), (int)n);
    return (double)__builtin_amdgcn_rcpf(1.f + e);
}
template <class P>
__device__ __forceinline__ double hot_adapt(const P &p, double g, double pw1, double pw2, double &c1, double &c2) {
    switch (p.sgd_mode) {
        case MI355REC_ADAGRAD:
            c1 = c1 + g * g;
            return (double)((float)g * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf((float)c1) + 1e-8f));
        case MI355REC_RMSPROP:
            c1 = c1 * (double)p.gamma + (double)p.one_m_gamma * (g * g);
            return (double)((float)g * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf((float)c1) + 1e-8f));
        case MI355REC_ADAM:
            c1 = c1 * (double)p.beta_1 + (double)p.one_m_beta_1 * g;
            c2 = c2 * (double)p.beta_2 + (double)p.one_m_beta_2 * (g * g);
            return (double)((float)(c1 / pw1) * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf((float)(c2 / pw2)) + 1e-8f));
        default:
            return g;
    }
}

// ---- dense store ----------------------------------------------------------------------------------------------------------
// One step on two rows in HBM, run by ONE wavefront: tickets of the two items (lanes 0 and 1 poll), gathers, reduction, the two
// per-item optimiser steps, write-through scatters, drain, tickets passed on.
template <class T>
__device__ __forceinline__ void cold_step(const SlimParams<T> &p, const StepDesc e, const int lane) {
    const int t = e.t, i = e.i, j = e.j, rs = e.rs, L = e.L;
    const size_t n = (size_t)p.n_items;
    const unsigned long long k0 = p.prof ? shader_clock() : 0ull;
    int sv[FLOW_REGS];
#pragma unroll
    for (int r = 0; r < FLOW_REGS; ++r) sv[r] = p.indices[rs + min(lane + 64 * r, L - 1)];      // L >= 1: users without interactions are never drawn
    const int want = lane == 0 ? e.a : (lane == 1 ? e.b : 0);
    {
        const int *word = &p.ticket[lane == 1 ? j : i];
        SpinGuard sg;
        for (;;) {
            const int v = lane < 2 ? aload(word) : 0;
            if (__all(v == want)) break;
            if (p.nap) nap_by_distance(max(__builtin_amdgcn_readlane(want - v, 0), __builtin_amdgcn_readlane(want - v, 1)));
            if (give_up(p, sg)) return;
        }
    }
    const unsigned long long k1 = p.prof ? shader_clock() : 0ull;
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    // the items' optimiser cells belong to whoever holds the items' tickets: lane 0 looks after item i, lane 1 after item j
    T oc1 = (T)0, oc2 = (T)0;
    if (lane < 2 && p.sgd_mode != MI355REC_SGD) {
        oc1 = aload(&p.c1[lane ? j : i]);
        if (p.sgd_mode == MI355REC_ADAM) oc2 = aload(&p.c2[lane ? j : i]);
    }
    T *Si = p.S + (size_t)i * n, *Sj = p.S + (size_t)j * n;
    T va[FLOW_REGS], vb[FLOW_REGS];
    T x = (T)0;
#pragma unroll
    for (int r = 0; r < FLOW_REGS; ++r) {       // loads from clamped, always valid addresses, masked afterwards: one wait for all of them
        va[r] = aload(Si + sv[r]);
        vb[r] = aload(Sj + sv[r]);
    }
#pragma unroll
    for (int r = 0; r < FLOW_REGS; ++r) {
        const bool live = lane + 64 * r < L;
        va[r] = live ? va[r] : (T)0;
        vb[r] = live ? vb[r] : (T)0;
        x += va[r] - vb[r];                                           // x_uij over the profile (.pyx:243-260)
    }
    for (int b0 = FLOW_BLOCK; b0 < L; b0 += FLOW_BLOCK) {             // profiles longer than 256
        int s[FLOW_REGS];
        T a[FLOW_REGS], b[FLOW_REGS];
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r) s[r] = p.indices[rs + min(b0 + lane + 64 * r, L - 1)];
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r) {
            a[r] = aload(Si + s[r]);
            b[r] = aload(Sj + s[r]);
        }
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r)
            if (b0 + lane + 64 * r < L) x += a[r] - b[r];
    }
    x = wave_sum(x);
    const T g = sigmoid_of_minus(x);                                  // .pyx:263
    T pw1, pw2;
    adam_powers(p, t, pw1, pw2);
    const T step = slim_adapt_cells(p, g, pw1, pw2, oc1, oc2);        // item i on lane 0, item j on lane 1 (.pyx:267-268)
    if (lane < 2 && p.sgd_mode != MI355REC_SGD) {
        astore(&p.c1[lane ? j : i], oc1);
        if (p.sgd_mode == MI355REC_ADAM) astore(&p.c2[lane ? j : i], oc2);
    }
    const T gi = __shfl(step, 0), gj = __shfl(step, 1);
    if (lane == 0) atomicAdd(&p.loss_slots[t & (LOSS_SLOTS - 1)], (double)x * (double)x);
    // the two rows move (.pyx:271-309); write-through stores
#pragma unroll
    for (int r = 0; r < FLOW_REGS; ++r) {
        if (lane + 64 * r < L) {
            const int s = sv[r];
            if (s != i) astore(Si + s, cell_plus(va[r], p.lr, gi, p.li_reg));
            if (s != j) astore(Sj + s, cell_minus(vb[r], p.lr, gj, p.lj_reg));
        }
    }
    for (int b0 = FLOW_BLOCK; b0 < L; b0 += FLOW_BLOCK) {
        int s[FLOW_REGS];
        T a[FLOW_REGS], b[FLOW_REGS];
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r) s[r] = p.indices[rs + min(b0 + lane + 64 * r, L - 1)];
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r) {
            a[r] = aload(Si + s[r]);
            b[r] = aload(Sj + s[r]);
        }
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r) {
            if (b0 + lane + 64 * r < L) {
                if (s[r] != i) astore(Si + s[r], cell_plus(a[r], p.lr, gi, p.li_reg));
                if (s[r] != j) astore(Sj + s[r], cell_minus(b[r], p.lr, gj, p.lj_reg));
            }
        }
    }
    // publish: drain the write-through stores, then pass the tickets on
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane < 2) astore(&p.ticket[lane ? j : i], want + 1);
    if (p.prof && lane == 0) {
        unsigned long long *o = p.prof + 8 * MAX_OWNERS;
        atomicAdd(&o[0], 1ull);
        atomicAdd(&o[1], k1 - k0);                   // profile ids + ticket wait
        atomicAdd(&o[2], shader_clock() - k1);       // gathers ... tickets passed on
    }
}

// The steps of one OWNED row, in stream order, by the 16 wavefronts of the owning workgroup in turn.  `row` is the item's row of S
// in LDS (float32), `oc` its two optimiser cells (float64).  Entry k of the row's list is step t with the row in role 0 (the
// positive item) or 1 (the negative item); the OTHER row of the step is
//   in HBM    -> this wavefront does that row's half of the step as well: waits for its ticket, gathers its cells and sums them
//                BEFORE its turn, writes them back and passes the ticket on AFTER its turn;
//   owned too -> the two owners exchange two scalars through the step's mailbox (the negative item's owner sends its sum, the
//                positive item's owner answers with the sigmoid), both inside their turns.
// A turn: LDS gather, wavefront reduction, sigmoid, the item's optimiser step, LDS scatter, turn counter + 1 -- and nothing that
// leaves the compute unit: the profile's ids (up to OWN_IDS x 64 of them, two 16-bit ids per register: a row that fits the LDS has
// fewer than 65 536 columns) are in registers before the turn starts.
constexpr int OWN_IDS = 16;

template <class T>
__device__ __forceinline__ void owned_row(const SlimParams<T> &p, const int h, float *row, volatile int *turn_generic, volatile double *oc_generic,
                                          const int lane, const int wave) {
    auto turn = as_lds(turn_generic);
    auto oc = as_lds(oc_generic);
    const int item = p.hot_item[h], first = p.lst_begin[h], len = p.lst_len[h];
    const size_t n = (size_t)p.n_items;
    const float lr = (float)p.lr, li_reg = (float)p.li_reg, lj_reg = (float)p.lj_reg;
    unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = wave; k < len; k += FLOW_WAVES) {
        const unsigned long long k0 = p.prof ? shader_clock() : 0ull;
        const StepDesc e = p.own_desc[first + k];
        const int t = e.t, role = e.j, other = e.i, rs = e.rs, L = e.L;
        unsigned ids[OWN_IDS / 2];
#pragma unroll
        for (int r = 0; r < OWN_IDS; r += 2) {
            ids[r / 2] = 0;
            if (64 * r < L) {         // (wave-uniform: chunks the profile does not reach are not fetched)
                const unsigned lo = (unsigned)p.indices[rs + min(lane + 64 * r, L - 1)];
                const unsigned hi = (unsigned)p.indices[rs + min(lane + 64 * (r + 1), L - 1)];
                ids[r / 2] = lo | (hi << 16);
            }
        }
        auto id_of = [&](int r) -> int { return (int)((ids[r / 2] >> (16 * (r & 1))) & 0xffffu); };
        const bool mail = e.b != 0;
        // ---- before the turn: the other row's half ------------------------------------------------------------------------
        T *So = p.S + (size_t)other * n;
        T vo[FLOW_REGS];
        T oc1 = (T)0, oc2 = (T)0;
        double xo = 0.0;
        int want = 0;
        unsigned long long k1 = k0;
        if (!mail) {
            want = e.a;
            if (!wave_wait_word(p, &p.ticket[other], want, lane)) return;
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            if (p.prof) k1 = shader_clock();
            if (lane == 0 && p.sgd_mode != MI355REC_SGD) {
                oc1 = aload(&p.c1[other]);
                if (p.sgd_mode == MI355REC_ADAM) oc2 = aload(&p.c2[other]);
            }
#pragma unroll
            for (int r = 0; r < FLOW_REGS; ++r) vo[r] = aload(So + id_of(r));
#pragma unroll
            for (int r = 0; r < FLOW_REGS; ++r) {
                vo[r] = lane + 64 * r < L ? vo[r] : (T)0;
                xo += (double)vo[r];
            }
#pragma unroll
            for (int blk = 1; blk < OWN_IDS / FLOW_REGS; ++blk) {         // entries 256 .. 1023: ids in registers
                if (blk * FLOW_BLOCK < L) {
                    T a[FLOW_REGS];
#pragma unroll
                    for (int r = 0; r < FLOW_REGS; ++r) a[r] = aload(So + id_of(blk * FLOW_REGS + r));
#pragma unroll
                    for (int r = 0; r < FLOW_REGS; ++r)
                        if (blk * FLOW_BLOCK + lane + 64 * r < L) xo += (double)a[r];
                }
            }
            for (int b0 = 64 * OWN_IDS; b0 < L; b0 += FLOW_BLOCK) {
                T a[FLOW_REGS];
#pragma unroll
                for (int r = 0; r < FLOW_REGS; ++r) a[r] = aload(So + p.indices[rs + min(b0 + lane + 64 * r, L - 1)]);
#pragma unroll
                for (int r = 0; r < FLOW_REGS; ++r)
                    if (b0 + lane + 64 * r < L) xo += (double)a[r];
            }
            xo = wave_sum(xo);
        }
        double pw1, pw2;
        adam_powers(p, t, pw1, pw2);
        const unsigned long long k2 = p.prof ? shader_clock() : 0ull;
        // ---- the turn -------------------------------------------------------------------------------------------------------
        {
            SpinGuard sg;
            unsigned spins = 0;
            while (__builtin_amdgcn_readfirstlane(*turn) != k)
                if ((++spins & 1023u) == 0 && give_up(p, sg)) return;
        }
        __builtin_amdgcn_s_setprio(3);
        asm volatile("" ::: "memory");
        const unsigned long long k3 = p.prof ? shader_clock() : 0ull;
        double xr = 0.0;
        float vr[FLOW_REGS];            // the cells of the first 256 entries stay in registers between the sum and the update
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r) vr[r] = lane + 64 * r < L ? row[id_of(r)] : 0.f;
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r) xr += (double)vr[r];
        if (L > FLOW_BLOCK) {           // (14 % of the ML-20M users)
#pragma unroll
            for (int r = FLOW_REGS; r < OWN_IDS; ++r)
                if (64 * r < L) xr += lane + 64 * r < L ? (double)row[id_of(r)] : 0.0;
            for (int idx = lane + 64 * OWN_IDS; idx < L; idx += 64) xr += (double)row[p.indices[rs + idx]];      // (0.7 %)
        }
        xr = wave_sum(xr);
        const unsigned long long k3a = p.prof ? shader_clock() : 0ull;
        double g, x = 0.0;
        if (!mail) {
            x = role ? xo - xr : xr - xo;                             // x_uij = sum over S[i, .] - sum over S[j, .]
            g = fast_sigmoid_of_minus(x);
        } else if (role) {      // this row is the step's negative item: send the sum, wait for the sigmoid
            if (lane == 0) astore(&p.mail_x[t], (unsigned long long)__double_as_longlong(xr));
            if (!wave_wait_mail(p, &p.mail_g[t], lane, g)) { __builtin_amdgcn_s_setprio(0); return; }
        } else {
            if (!wave_wait_mail(p, &p.mail_x[t], lane, xo)) { __builtin_amdgcn_s_setprio(0); return; }
            x = xr - xo;
            g = fast_sigmoid_of_minus(x);
            if (lane == 0) astore(&p.mail_g[t], (unsigned long long)__double_as_longlong(g));
        }
        double c1 = oc[0], c2 = oc[1];
        const double gr = hot_adapt(p, g, pw1, pw2, c1, c2);
        if (lane == 0) { oc[0] = c1; oc[1] = c2; }
        const unsigned long long k3b = p.prof ? shader_clock() : 0ull;
        // (the row's cells are float32: their update in float32 arithmetic adds ~1e-7 of the INCREMENT to the rounding of the sum)
        const float reg = role ? lj_reg : li_reg, grf = (float)gr;
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r) {
            const int s = id_of(r);
            if (lane + 64 * r < L && s != item) row[s] = role ? cell_minus(vr[r], lr, grf, reg) : cell_plus(vr[r], lr, grf, reg);
        }
        if (L > FLOW_BLOCK) {
#pragma unroll
            for (int r = FLOW_REGS; r < OWN_IDS; ++r) {
                if (64 * r < L) {
                    const int s = id_of(r);
                    if (lane + 64 * r < L && s != item) row[s] = role ? cell_minus(row[s], lr, grf, reg) : cell_plus(row[s], lr, grf, reg);
                }
            }
            for (int idx = lane + 64 * OWN_IDS; idx < L; idx += 64) {
                const int s = p.indices[rs + idx];
                if (s != item) row[s] = role ? cell_minus(row[s], lr, grf, reg) : cell_plus(row[s], lr, grf, reg);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           // the row's new cells are in LDS before the next wavefront is let in
        if (lane == 0) *turn = k + 1;
        __builtin_amdgcn_s_setprio(0);
        const unsigned long long k4 = p.prof ? shader_clock() : 0ull;
        // ---- after the turn: the other row moves, its ticket is passed on -------------------------------------------------------
        if (!mail) {
            T po1, po2;
            adam_powers(p, t, po1, po2);
            const T go = slim_adapt_cells(p, (T)g, po1, po2, oc1, oc2);
            if (lane == 0 && p.sgd_mode != MI355REC_SGD) {
                astore(&p.c1[other], oc1);
                if (p.sgd_mode == MI355REC_ADAM) astore(&p.c2[other], oc2);
            }
            const T go_all = __shfl(go, 0);                            // (lane 0 holds the item's optimiser cells)
            // (the other row is the negative item when this one is the positive: .pyx:296-309)
#pragma unroll
            for (int r = 0; r < FLOW_REGS; ++r) {
                const int s = id_of(r);
                if (lane + 64 * r < L && s != other)
                    astore(So + s, role ? cell_plus(vo[r], p.lr, go_all, p.li_reg) : cell_minus(vo[r], p.lr, go_all, p.lj_reg));
            }
#pragma unroll
            for (int blk = 1; blk < OWN_IDS / FLOW_REGS; ++blk) {
                if (blk * FLOW_BLOCK < L) {
                    T a[FLOW_REGS];
#pragma unroll
                    for (int r = 0; r < FLOW_REGS; ++r) a[r] = aload(So + id_of(blk * FLOW_REGS + r));
#pragma unroll
                    for (int r = 0; r < FLOW_REGS; ++r) {
                        const int s = id_of(blk * FLOW_REGS + r);
                        if (blk * FLOW_BLOCK + lane + 64 * r < L && s != other)
                            astore(So + s, role ? cell_plus(a[r], p.lr, go_all, p.li_reg) : cell_minus(a[r], p.lr, go_all, p.lj_reg));
                    }
                }
            }
            for (int b0 = 64 * OWN_IDS; b0 < L; b0 += FLOW_BLOCK) {
                int s[FLOW_REGS];
                T a[FLOW_REGS];
#pragma unroll
                for (int r = 0; r < FLOW_REGS; ++r) {
                    s[r] = p.indices[rs + min(b0 + lane + 64 * r, L - 1)];
                    a[r] = aload(So + s[r]);
                }
#pragma unroll
                for (int r = 0; r < FLOW_REGS; ++r)
                    if (b0 + lane + 64 * r < L && s[r] != other)
                        astore(So + s[r], role ? cell_plus(a[r], p.lr, go_all, p.li_reg) : cell_minus(a[r], p.lr, go_all, p.lj_reg));
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0) astore(&p.ticket[other], want + 1);
        }
        if (lane == 0 && !(mail && role)) atomicAdd(&p.loss_slots[t & (LOSS_SLOTS - 1)], x * x);
        if (p.prof) {
            acc[0] += 1; acc[1] += k1 - k0; acc[2] += k2 - k1; acc[3] += k3 - k2; acc[4] += k4 - k3; acc[5] += shader_clock() - k4;
            acc[6] += k3a - k3; acc[7] += k3b - k3a;
        }
    }
    if (p.prof && lane == 0) {       // entries | descriptor + ticket wait | gather + sum | wait for the turn | the turn | other row's write-back
        unsigned long long *o = p.prof + 8 * h;
        for (int c = 0; c < 8; ++c) atomicAdd(&o[c], acc[c]);
    }
}

// Workgroups 0 .. n_hot - 1 own a row each; the others (and an owner once its list is done) run the cold list.
template <class T>
__global__ __launch_bounds__(FLOW_THREADS) void slim_dense_flow_kernel(const SlimParams<T> p, const int owners) {
    extern __shared__ __attribute__((aligned(16))) float flow_lds[];
    __shared__ int s_turn;
    __shared__ LocalQueue s_queue;
    __shared__ double s_oc[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { s_queue.next = 0; s_queue.ready = 0; }
    const int n_hot = owners ? *p.n_hot : 0;
    if ((int)blockIdx.x < n_hot) {
        const int h = blockIdx.x, item = p.hot_item[h];
        T *Sr = p.S + (size_t)item * p.n_items;
        for (int c = tid; c < p.n_items; c += FLOW_THREADS) flow_lds[c] = (float)Sr[c];
        if (tid == 0) {
            s_turn = 0;
            s_oc[0] = p.sgd_mode != MI355REC_SGD ? (double)p.c1[item] : 0.0;
            s_oc[1] = p.sgd_mode == MI355REC_ADAM ? (double)p.c2[item] : 0.0;
        }
        __syncthreads();
        owned_row(p, h, flow_lds, &s_turn, s_oc, lane, wave);
        __syncthreads();
        for (int c = tid; c < p.n_items; c += FLOW_THREADS) Sr[c] = (T)flow_lds[c];
        if (tid == 0) {
            if (p.sgd_mode != MI355REC_SGD) p.c1[item] = (T)s_oc[0];
            if (p.sgd_mode == MI355REC_ADAM) p.c2[item] = (T)s_oc[1];
        }
    }
    __syncthreads();
    const int n_cold = *p.n_cold;
    for (;;) {          // in-order queue: everything a step can wait for is already running
        const int q = claim_step<true>(p, &s_queue, lane);
        if (q >= n_cold) break;
        cold_step(p, p.cold_desc[q], lane);
    }
}

}  // namespace
}  // namespace mi355rec
