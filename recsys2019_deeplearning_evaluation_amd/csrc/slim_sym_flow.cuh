// slim_sym_flow.cuh -- the symmetric store's dataflow kernel (tagged granules: sym_fetch, sym_step, sym_step_wide,
// slim_sym_flow_kernel) and slim_ordered_kernel, the one-workgroup fallback for catalogues its cell ids do not fit.
#pragma once

#include "slim_flow.cuh"

namespace mi355rec {
namespace {

// ---- symmetric store ------------------------------------------------------------------------------------------------------
// One step by ONE wavefront.  Every cell is a granule {value, tag of the step that wrote it}; the step knows which step wrote each
// of its cells last (`pred`), so it loads all its granules at once and re-loads only those whose tag is not there yet.  Its own
// stores carry its tag: nothing is drained, no flag is raised.  The optimiser cells of the two items travel as granules, too
// (lane 0: item i, lane 1: item j; float64 as two float32 halves, each with its own tag).  Between the arrival of a step's last
// tag and its stores sits the chain of the whole epoch (3 839 links at the ML-20M shape): sigmoid and optimiser step use the
// short forms of the owned rows' turns.
__device__ __forceinline__ bool tag_ok(int pred, unsigned tag, unsigned tag_base) { return pred < 0 || tag == tag_base + (unsigned)pred + 1u; }

// one block of FLOW_BLOCK profile entries: ids, last writers, granules of both rows -- fetched, then polled until every tag is there
struct SymBlock {
    int s[FLOW_REGS], pa[FLOW_REGS], pb[FLOW_REGS];
    Granule ga[FLOW_REGS], gb[FLOW_REGS];
};
__device__ __forceinline__ bool sym_fetch(const SlimParams<double> &p, const StepDesc &e, const long long cp, const int b0, const int lane,
                                          const bool poll, SymBlock &k, unsigned &repolls) {
    const int i = e.i, j = e.j, rs = e.rs, L = e.L;
#pragma unroll
    for (int r = 0; r < FLOW_REGS; ++r) {
        const int at = min(b0 + lane + 64 * r, L - 1);
        k.s[r] = p.indices[rs + at];
        if (poll) {
            const int2 pp = *reinterpret_cast<const int2 *>(p.pred + cp + 2 * at);
            k.pa[r] = pp.x;
            k.pb[r] = pp.y;
        }
    }
#pragma unroll
    for (int r = 0; r < FLOW_REGS; ++r) {
        const bool live = b0 + lane + 64 * r < L;
        k.pa[r] = live && poll ? k.pa[r] : -1;
        k.pb[r] = live && poll ? k.pb[r] : -1;
        k.ga[r] = gload(p.G + packed_cell(i, k.s[r]));
        k.gb[r] = gload(p.G + packed_cell(j, k.s[r]));
    }
    if (!poll) return true;
    SpinGuard sg;
    for (;;) {
        bool pending = false;
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r) {
            if (!tag_ok(k.pa[r], k.ga[r].tag, p.tag_base)) { pending = true; k.ga[r] = gload(p.G + packed_cell(i, k.s[r])); }
            if (!tag_ok(k.pb[r], k.gb[r].tag, p.tag_base)) { pending = true; k.gb[r] = gload(p.G + packed_cell(j, k.s[r])); }
        }
        if (!__any(pending)) return true;
        ++repolls;
        if (give_up(p, sg)) return false;
    }
}

__device__ __forceinline__ void sym_step(const SlimParams<double> &p, const int t, const int lane) {
    const StepDesc e = p.desc[t];
    const int i = e.i, j = e.j, L = e.L;
    const long long cp = (long long)(((unsigned long long)(unsigned)e.c << 32) | (unsigned)e.t);
    const unsigned long long k0 = p.prof ? shader_clock() : 0ull;
    unsigned repolls = 0;
    const unsigned my_tag = p.tag_base + (unsigned)t + 1u;
    const bool adaptive = p.sgd_mode != MI355REC_SGD, adam = p.sgd_mode == MI355REC_ADAM;
    // optimiser granules of the lane's item (requested first: they are polled last)
    Granule *oc = p.oc + 4 * (size_t)(lane == 1 ? j : i);
    const int ip = lane < 2 && adaptive ? (lane ? e.b : e.a) : -1;
    Granule o[4] = {{0.f, 0u}, {0.f, 0u}, {0.f, 0u}, {0.f, 0u}};
    if (lane < 2 && adaptive) {
        o[0] = gload(oc);
        o[1] = gload(oc + 1);
        if (adam) {
            o[2] = gload(oc + 2);
            o[3] = gload(oc + 3);
        }
    }
    SymBlock k;                                                       // the first block stays in registers for the second pass
    if (!sym_fetch(p, e, cp, 0, lane, true, k, repolls)) return;
    double x = 0.0;
#pragma unroll
    for (int r = 0; r < FLOW_REGS; ++r)
        if (lane + 64 * r < L) x += (double)k.ga[r].v - (double)k.gb[r].v;                // x_uij over the profile (.pyx:243-260)
    for (int b0 = FLOW_BLOCK; b0 < L; b0 += FLOW_BLOCK) {                                 // profiles longer than 256
        SymBlock m;
        if (!sym_fetch(p, e, cp, b0, lane, true, m, repolls)) return;
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r)
            if (b0 + lane + 64 * r < L) x += (double)m.ga[r].v - (double)m.gb[r].v;
    }
    {
        SpinGuard sg;
        for (;;) {
            bool pending = false;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if ((c < 2 || adam) && !tag_ok(ip, o[c].tag, p.tag_base)) { pending = true; o[c] = gload(oc + c); }
            if (!__any(pending)) break;
            ++repolls;
            if (give_up(p, sg)) return;
        }
    }
    const unsigned long long k1 = p.prof ? shader_clock() : 0ull;
    x = wave_sum(x);
    const double g = fast_sigmoid_of_minus(x);                                            // .pyx:263
    double pw1, pw2;
    adam_powers(p, t, pw1, pw2);
    double c1 = (double)o[0].v + (double)o[1].v, c2 = (double)o[2].v + (double)o[3].v;
    const double step = hot_adapt(p, g, pw1, pw2, c1, c2);                                // item i on lane 0, item j on lane 1 (.pyx:267-268)
    const double gi = __shfl(step, 0), gj = __shfl(step, 1);
    // the two rows move (.pyx:271-309): one write-through store per cell, value and tag together
#pragma unroll
    for (int r = 0; r < FLOW_REGS; ++r) {
        if (lane + 64 * r < L) {
            if (k.s[r] != i) gstore(p.G + packed_cell(i, k.s[r]), (float)cell_plus((double)k.ga[r].v, p.lr, gi, p.li_reg), my_tag);
            if (k.s[r] != j) gstore(p.G + packed_cell(j, k.s[r]), (float)cell_minus((double)k.gb[r].v, p.lr, gj, p.lj_reg), my_tag);
        }
    }
    if (lane < 2 && adaptive) {
        const float h1 = (float)c1;
        gstore(oc, h1, my_tag);
        gstore(oc + 1, (float)(c1 - (double)h1), my_tag);
        if (adam) {
            const float h2 = (float)c2;
            gstore(oc + 2, h2, my_tag);
            gstore(oc + 3, (float)(c2 - (double)h2), my_tag);
        }
    }
    for (int b0 = FLOW_BLOCK; b0 < L; b0 += FLOW_BLOCK) {
        // (nobody can have written these cells since they were read above: a later step waits for THIS step's tag on them)
        SymBlock m;
        sym_fetch(p, e, cp, b0, lane, false, m, repolls);
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r) {
            if (b0 + lane + 64 * r < L) {
                if (m.s[r] != i) gstore(p.G + packed_cell(i, m.s[r]), (float)cell_plus((double)m.ga[r].v, p.lr, gi, p.li_reg), my_tag);
                if (m.s[r] != j) gstore(p.G + packed_cell(j, m.s[r]), (float)cell_minus((double)m.gb[r].v, p.lr, gj, p.lj_reg), my_tag);
            }
        }
    }
    if (lane == 0) atomicAdd(&p.loss_slots[t & (LOSS_SLOTS - 1)], x * x);
    if (p.prof && lane == 0) {       // steps | descriptor .. all tags there | the rest | polling rounds that found a tag missing
        atomicAdd(&p.prof[0], 1ull);
        atomicAdd(&p.prof[1], k1 - k0);
        atomicAdd(&p.prof[2], shader_clock() - k1);
        atomicAdd(&p.prof[3], (unsigned long long)repolls);
    }
}

// A step with a LONG profile (more than FLOW_BLOCK entries) by a whole workgroup: every wavefront takes a block, so the granules
// of up to 4 096 entries are in flight together and stay in registers for the stores.  One wavefront would fetch them block after
// block, twice -- and steps with long profiles touch the most cells, so they sit on the chain of the epoch more often than
// their 14 % share of the steps: with them at one round trip per block the chain of the ML-20M shape weighs 13.5 ms, without 7.8 ms
// (scratch: chain2.c on a stream of the bench's epoch).  Every wavefront adds the sixteen partial sums in the same order and does
// the (cheap) scalar part itself: one barrier per step.
__device__ __forceinline__ bool sym_step_wide(const SlimParams<double> &p, const int t, const int lane, const int wave, double *s_x, int *s_bad) {
    const StepDesc e = p.desc[t];
    const int i = e.i, j = e.j, L = e.L;
    const long long cp = (long long)(((unsigned long long)(unsigned)e.c << 32) | (unsigned)e.t);
    const unsigned long long k0 = p.prof ? shader_clock() : 0ull;
    unsigned repolls = 0;
    const unsigned my_tag = p.tag_base + (unsigned)t + 1u;
    const bool adaptive = p.sgd_mode != MI355REC_SGD, adam = p.sgd_mode == MI355REC_ADAM;
    Granule *oc = p.oc + 4 * (size_t)(lane == 1 ? j : i);
    const int ip = lane < 2 && adaptive ? (lane ? e.b : e.a) : -1;
    Granule o[4] = {{0.f, 0u}, {0.f, 0u}, {0.f, 0u}, {0.f, 0u}};
    if (lane < 2 && adaptive) {
        o[0] = gload(oc);
        o[1] = gload(oc + 1);
        if (adam) {
            o[2] = gload(oc + 2);
            o[3] = gload(oc + 3);
        }
    }
    constexpr int ROUND = FLOW_WAVES * FLOW_BLOCK;
    const int first = wave * FLOW_BLOCK;
    bool ok = true;
    SymBlock k;
    double x = 0.0;
    if (first < L) {
        ok = sym_fetch(p, e, cp, first, lane, true, k, repolls);
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r)
            if (first + lane + 64 * r < L) x += (double)k.ga[r].v - (double)k.gb[r].v;
    }
    for (int b0 = first + ROUND; ok && b0 < L; b0 += ROUND) {                             // profiles longer than 4 096
        SymBlock m;
        ok = sym_fetch(p, e, cp, b0, lane, true, m, repolls);
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r)
            if (b0 + lane + 64 * r < L) x += (double)m.ga[r].v - (double)m.gb[r].v;
    }
    if (ok) {
        SpinGuard sg;
        for (;;) {
            bool pending = false;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if ((c < 2 || adam) && !tag_ok(ip, o[c].tag, p.tag_base)) { pending = true; o[c] = gload(oc + c); }
            if (!__any(pending)) break;
            ++repolls;
            if (give_up(p, sg)) { ok = false; break; }
        }
    }
    x = wave_sum(x);
    if (lane == 0) {
        s_x[wave] = x;
        if (!ok) *s_bad = 1;
    }
    __syncthreads();
    if (*s_bad) return false;                                                             // (the same answer in every wavefront)
    const unsigned long long k1 = p.prof ? shader_clock() : 0ull;
    x = 0.0;
#pragma unroll
    for (int w = 0; w < FLOW_WAVES; ++w) x += s_x[w];
    const double g = fast_sigmoid_of_minus(x);
    double pw1, pw2;
    adam_powers(p, t, pw1, pw2);
    double c1 = (double)o[0].v + (double)o[1].v, c2 = (double)o[2].v + (double)o[3].v;
    const double step = hot_adapt(p, g, pw1, pw2, c1, c2);
    const double gi = __shfl(step, 0), gj = __shfl(step, 1);
    if (first < L) {
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r) {
            if (first + lane + 64 * r < L) {
                if (k.s[r] != i) gstore(p.G + packed_cell(i, k.s[r]), (float)cell_plus((double)k.ga[r].v, p.lr, gi, p.li_reg), my_tag);
                if (k.s[r] != j) gstore(p.G + packed_cell(j, k.s[r]), (float)cell_minus((double)k.gb[r].v, p.lr, gj, p.lj_reg), my_tag);
            }
        }
    }
    if (wave == 0 && lane < 2 && adaptive) {
        const float h1 = (float)c1;
        gstore(oc, h1, my_tag);
        gstore(oc + 1, (float)(c1 - (double)h1), my_tag);
        if (adam) {
            const float h2 = (float)c2;
            gstore(oc + 2, h2, my_tag);
            gstore(oc + 3, (float)(c2 - (double)h2), my_tag);
        }
    }
    for (int b0 = first + ROUND; b0 < L; b0 += ROUND) {
        SymBlock m;
        sym_fetch(p, e, cp, b0, lane, false, m, repolls);
#pragma unroll
        for (int r = 0; r < FLOW_REGS; ++r) {
            if (b0 + lane + 64 * r < L) {
                if (m.s[r] != i) gstore(p.G + packed_cell(i, m.s[r]), (float)cell_plus((double)m.ga[r].v, p.lr, gi, p.li_reg), my_tag);
                if (m.s[r] != j) gstore(p.G + packed_cell(j, m.s[r]), (float)cell_minus((double)m.gb[r].v, p.lr, gj, p.lj_reg), my_tag);
            }
        }
    }
    if (wave == 0 && lane == 0) {
        atomicAdd(&p.loss_slots[t & (LOSS_SLOTS - 1)], x * x);
        if (p.prof) {                // long profiles | claim .. barrier passed | the rest | polling rounds of wavefront 0
            atomicAdd(&p.prof[4], 1ull);
            atomicAdd(&p.prof[5], k1 - k0);
            atomicAdd(&p.prof[6], shader_clock() - k1);
            atomicAdd(&p.prof[7], (unsigned long long)repolls);
        }
    }
    return true;
}

// Workgroups 0 .. long_wgs - 1 take the steps with long profiles, one step per workgroup, the others (and those once that queue is
// empty) the steps with short profiles, one per wavefront.  Both queues hand out steps in stream order and every workgroup of
// the grid is resident: the oldest step that has not run is either running or the next one of its queue, and the consumers of
// that queue that are busy are busy with older steps.
__global__ __launch_bounds__(FLOW_THREADS) void slim_sym_flow_kernel(const SlimParams<double> p, const int long_wgs) {
    __shared__ LocalQueue s_queue;
    __shared__ double s_x[FLOW_WAVES];
    __shared__ int s_next, s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { s_queue.next = 0; s_queue.ready = 0; s_bad = 0; }
    __syncthreads();
    if ((int)blockIdx.x < long_wgs) {
        const int n_long = p.n_steps - p.n_short;
        for (;;) {
            if (tid == 0) s_next = aload(&p.queue[1]) ? NO_STEP : atomicAdd(&p.queue[2], 1);
            __syncthreads();
            const int q = s_next;
            __syncthreads();
            if (q >= n_long) break;
            if (!sym_step_wide(p, p.order[p.n_steps - 1 - q], lane, wave, s_x, &s_bad)) break;
        }
    }
    for (;;) {          // in-order queue: everything a step can wait for is already running
        const int q = claim_step<false>(p, &s_queue, lane);
        if (q >= p.n_short) break;
        sym_step(p, p.order[q], lane);
    }
}

// Fallback (symmetric store with more than 92 681 items: packed cell ids no longer fit the 32-bit sort key): one workgroup runs
// the steps one after the other (plain accesses: one compute unit, one L1).
__global__ __launch_bounds__(1024) void slim_ordered_kernel(const SlimParams<double> p) {
    __shared__ double s_part[16];
    __shared__ double s_g[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = 0; t < p.n_steps; ++t) {
        const int u = p.su[t], i = p.si[t], j = p.sj[t];
        const int rs = p.indptr[u], re = p.indptr[u + 1];
        double x = 0.0;
        for (int q = rs + tid; q < re; q += 1024) {
            const int s = p.indices[q];
            x += (double)p.G[packed_cell(i, s)].v - (double)p.G[packed_cell(j, s)].v;
        }
        x = wave_sum(x);
        if (lane == 0) s_part[wave] = x;
        __syncthreads();
        if (tid == 0) {
            double tot = 0.0;
            for (int w = 0; w < 16; ++w) tot += s_part[w];
            const double g = sigmoid_of_minus(tot);
            double pw1, pw2;
            adam_powers(p, t, pw1, pw2);
            for (int e = 0; e < 2; ++e) {                                 // item i first, then j (.pyx:267-268)
                Granule *oc = p.oc + 4 * (size_t)(e ? j : i);
                double c1 = (double)oc[0].v + (double)oc[1].v, c2 = (double)oc[2].v + (double)oc[3].v;
                s_g[e] = slim_adapt_cells(p, g, pw1, pw2, c1, c2);
                const float h1 = (float)c1, h2 = (float)c2;
                oc[0].v = h1; oc[1].v = (float)(c1 - (double)h1);
                oc[2].v = h2; oc[3].v = (float)(c2 - (double)h2);
            }
            p.loss_slots[t & (LOSS_SLOTS - 1)] += tot * tot;
        }
        __syncthreads();
        const double gi = s_g[0], gj = s_g[1];
        for (int q = rs + tid; q < re; q += 1024) {
            const int s = p.indices[q];
            if (s != i) {
                Granule *c = &p.G[packed_cell(i, s)];
                c->v = (float)cell_plus((double)c->v, p.lr, gi, p.li_reg);
            }
            if (s != j) {
                Granule *c = &p.G[packed_cell(j, s)];
                c->v = (float)cell_minus((double)c->v, p.lr, gj, p.lj_reg);
            }
        }
        __threadfence_block();       // the next step of this workgroup must read what this one wrote
        __syncthreads();
    }
}

}  // namespace
}  // namespace mi355rec
