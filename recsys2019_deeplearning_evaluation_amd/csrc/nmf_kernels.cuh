// nmf_kernels.cuh -- the kernels of the NMF handle, kernels only; launched by nmf.hip  [DESIGN.md section 12].
//
//   nmf_cd_sweep_kernel  one half-sweep of coordinate descent: a row of the block per group of 16 / 32 / 64 lanes, the row in LDS (a
//                        lane owns the columns lp apart and no other lane reads them), every workgroup walking the permutation in
//                        lock-step.  Per component t: grad = W[i] . HHt[t] - XHt[i,t] as a FRESH dot product (lane-private FMAs, a
//                        butterfly over the group: every lane ends with the same bits), the projected gradient into a float64
//                        violation sum, W[i,t] = max(W[i,t] - grad / HHt[t,t], 0).  Workgroup sums are written in a fixed order and
//                        added by nmf_sum_kernel: no atomics, a sweep is bitwise repeatable.
//   nmf_sddmm_kernel     per cell of a layout, in its own cell order: wh = max(W[i] . Ht[c], eps32); <false>: q = x / wh, the value
//                        stream of the product that follows; <true>: x log(x / wh) into float64 workgroup sums (the divergence).
//                        A piece of a row per group of lanes as in the product, the row's own factors in registers, four cells at a
//                        time so that four gathered rows are in flight and the four sums share their cross-lane exchanges.
//   nmf_scale_kernel     block *= numerator / denominator (a matrix or one value per column), zero denominators replaced, the
//                        Kullback-Leibler floor on Ht.
//   nmf_colsum_*, nmf_dot_kernel, nmf_sum_kernel   float64 reductions in a fixed order.
// The constants the host shares with them (NT, EPS32, RED_BLOCKS, CS_SLABS) and every grid are in blocks_plan.h.
#pragma once

#include <hip/hip_runtime.h>

#include "blocks_plan.h"

namespace {

using namespace mi355rec::blocks;

constexpr int SD_CPL = 4;                  // columns of its own row an SDDMM lane keeps in registers
constexpr int SD_CELLS = 4;                // cells an SDDMM group works on together
constexpr double EPS64 = 2.220446049250313e-16;

// the fixed-order sum of one double per thread: thread 0 adds them by thread index
__device__ __forceinline__ void block_sum_to(double v, double *red, double *out) {
    red[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < NT; ++i) s += red[i];
        *out = s;
    }
}

__device__ __forceinline__ float group_sum(float v, int lp) {
    for (int m = lp >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(NT) void nmf_cd_sweep_kernel(float *__restrict__ W, int n, int k, int lp_shift,
                                                           const float *__restrict__ HHt, const float *__restrict__ XHt,
                                                           const int *__restrict__ perm, double *__restrict__ part) {
    extern __shared__ float w_lds[];                   // [q][thread]: column sub + q * lp of the thread's row; thread-private
    __shared__ double red[NT];
    const int lp = 1 << lp_shift, tid = threadIdx.x, sub = tid & (lp - 1);
    const int row = blockIdx.x * (NT >> lp_shift) + (tid >> lp_shift);
    const bool live = row < n;
    const size_t base = (size_t)(live ? row : n - 1) * k;              // rows past the end compute on zeros and write nothing
    const int nq = (k + lp - 1) >> lp_shift;
    for (int q = 0; q < nq; ++q) {
        const int c = sub + (q << lp_shift);
        w_lds[q * NT + tid] = (live && c < k) ? W[base + c] : 0.f;
    }
    const int group_lane0 = (tid & 63) & ~(lp - 1);
    double viol = 0.0;
    for (int s = 0; s < k; ++s) {
        const int t = perm[s];
        const float *hrow = HHt + (size_t)t * k;
        float acc = 0.f;
#pragma unroll 4
        for (int q = 0; q < nq; ++q) {
            const int c = sub + (q << lp_shift);
            if (c < k) acc = fmaf(hrow[c], w_lds[q * NT + tid], acc);
        }
        acc = group_sum(acc, lp);
        const int owner = t & (lp - 1), slot = (t >> lp_shift) * NT + tid;
        const float wt = __shfl(w_lds[slot], group_lane0 | owner);
        const float grad = acc - XHt[base + t], hess = hrow[t];
        const float pg = wt == 0.f ? fminf(0.f, grad) : grad;
        if (live && sub == 0) viol += fabs((double)pg);
        if (hess != 0.f && sub == owner) w_lds[slot] = fmaxf(wt - grad / hess, 0.f);
    }
    if (live)
        for (int q = 0; q < nq; ++q) {
            const int c = sub + (q << lp_shift);
            if (c < k) W[base + c] = w_lds[q * NT + tid];
        }
    block_sum_to(viol, red, part + blockIdx.x);
}

// one piece (at most 512 cells of one row) per group of lp lanes; A: the rows of the layout, B: the gathered side
template <bool LOG>
__global__ __launch_bounds__(NT) void nmf_sddmm_kernel(const int *__restrict__ p_row, const int *__restrict__ p_begin,
                                                        const int *__restrict__ p_end, int n_pieces, const int *__restrict__ idx,
                                                        const float *__restrict__ val, const float *__restrict__ A,
                                                        const float *__restrict__ B, int k, int lp_shift, float *__restrict__ q_out,
                                                        double *__restrict__ part) {
    __shared__ double red[NT];
    const int lp = 1 << lp_shift, tid = threadIdx.x, sub = tid & (lp - 1);
    const int piece = (blockIdx.x * NT + tid) >> lp_shift;
    const bool live = piece < n_pieces;
    const int b = live ? p_begin[piece] : 0, e = live ? p_end[piece] : 0;
    const float *arow = A + (size_t)(live ? p_row[piece] : 0) * k;
    float a[SD_CPL];
#pragma unroll
    for (int q = 0; q < SD_CPL; ++q) a[q] = (sub + q * lp < k) ? arow[sub + q * lp] : 0.f;
    double sum = 0.0;
    // the groups of a wavefront hold pieces of different lengths: every lane walks the longest one, so that the exchanges below
    // are never executed by part of a wavefront
    int len = e - b;
    for (int m = lp; m < 64; m <<= 1) len = max(len, __shfl_xor(len, m));
    const int half = lp >> 1, quarter = lp >> 2;
    const bool hi = (sub & half) != 0, hq = (sub & quarter) != 0;
    const int mine = (hi ? 2 : 0) + (hq ? 1 : 0);      // the cell of the four whose sum ends in this lane's quarter of the group
    for (int o = 0; o < len; o += SD_CELLS) {
        // four cells at a time: their gathered rows are in flight together, and the four sums over the group cost 3 + log2(lp / 4)
        // exchanges instead of 4 log2(lp)
        float acc[SD_CELLS];
        const float *brow[SD_CELLS];
#pragma unroll
        for (int u = 0; u < SD_CELLS; ++u) {
            const int j = b + o + u;
            brow[u] = j < e ? B + (size_t)idx[j] * k : nullptr;
            acc[u] = 0.f;
        }
#pragma unroll
        for (int q = 0; q < SD_CPL; ++q)
#pragma unroll
            for (int u = 0; u < SD_CELLS; ++u)
                if (brow[u] && sub + q * lp < k) acc[u] = fmaf(a[q], brow[u][sub + q * lp], acc[u]);
        for (int c = sub + SD_CPL * lp; c < k; c += lp) {
            const float ac = arow[c];
#pragma unroll
            for (int u = 0; u < SD_CELLS; ++u)
                if (brow[u]) acc[u] = fmaf(ac, brow[u][c], acc[u]);
        }
        // the upper half of the group takes over cells 2 and 3, the lower half cells 0 and 1; then the quarters split the pair
        float k0 = (hi ? acc[2] : acc[0]) + __shfl_xor(hi ? acc[0] : acc[2], half);
        float k1 = (hi ? acc[3] : acc[1]) + __shfl_xor(hi ? acc[1] : acc[3], half);
        float total = (hq ? k1 : k0) + __shfl_xor(hq ? k0 : k1, quarter);
        for (int m = quarter >> 1; m > 0; m >>= 1) total += __shfl_xor(total, m);
        const int j = b + o + mine;
        if (j < e && (sub & (quarter - 1)) == 0) {
            const float x = val ? val[j] : 1.f, wh = fmaxf(total, EPS32);
            if (LOG) {
                if (x > EPS32) sum += (double)x * log((double)x / (double)wh);
            } else {
                q_out[j] = x / wh;
            }
        }
    }
    if (LOG) block_sum_to(sum, red, part + blockIdx.x);
}

// X[i][c] *= num[i][c] / den, den = den_m[i][c] or den_v[c]; a zero den is replaced by zero_to; floor: results below eps64 become 0
__global__ __launch_bounds__(NT) void nmf_scale_kernel(float *__restrict__ X, const float *__restrict__ num, const float *__restrict__ den_m,
                                                        const float *__restrict__ den_v, size_t cells, int k, float zero_to, int floor) {
    const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e >= cells) return;
    float d = den_m ? den_m[e] : den_v[e % k];
    if (d == 0.f) d = zero_to;
    float x = X[e] * (num[e] / d);
    if (floor && (double)x < EPS64) x = 0.f;
    X[e] = x;
}

__global__ __launch_bounds__(NT) void nmf_fill_kernel(float *__restrict__ X, size_t cells, float value) {
    const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e < cells) X[e] = value;
}

// part[slab][c] = sum of X[row][c] over the slab's rows, in row order
__global__ __launch_bounds__(NT) void nmf_colsum_kernel(const float *__restrict__ X, int n, int k, int rows_per_slab, double *__restrict__ part) {
    const int c = blockIdx.y * NT + threadIdx.x, slab = blockIdx.x;
    if (c >= k) return;
    const int r0 = slab * rows_per_slab, r1 = min(n, r0 + rows_per_slab);
    double s = 0.0;
    for (int row = r0; row < r1; ++row) s += (double)X[(size_t)row * k + c];
    part[(size_t)slab * k + c] = s;
}

__global__ __launch_bounds__(NT) void nmf_colsum_reduce_kernel(const double *__restrict__ part, int n_slabs, int k, double *__restrict__ out,
                                                                float *__restrict__ out_f) {
    const int c = blockIdx.x * NT + threadIdx.x;
    if (c >= k) return;
    double s = 0.0;
    for (int slab = 0; slab < n_slabs; ++slab) s += part[(size_t)slab * k + c];
    out[c] = s;
    if (out_f) out_f[c] = (float)s;
}

__global__ __launch_bounds__(NT) void nmf_to_float_kernel(const double *__restrict__ in, float *__restrict__ out, size_t cells) {
    const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e < cells) out[e] = (float)in[e];
}

// part[block] = sum of a[i] * b[i] over the block's contiguous share of [0, len), every thread a contiguous run of it
template <class T>
__global__ __launch_bounds__(NT) void nmf_dot_kernel(const T *__restrict__ a, const T *__restrict__ b, size_t len, double *__restrict__ part) {
    __shared__ double red[NT];
    const size_t per_block = (len + gridDim.x - 1) / gridDim.x, per_thread = (per_block + NT - 1) / NT;
    const size_t b0 = (size_t)blockIdx.x * per_block, b1 = min(len, b0 + per_block);
    const size_t t0 = min(b1, b0 + (size_t)threadIdx.x * per_thread), t1 = min(b1, t0 + per_thread);
    double s = 0.0;
    for (size_t i = t0; i < t1; ++i) s += (double)a[i] * (double)b[i];
    block_sum_to(s, red, part + blockIdx.x);
}

// out[0] (+)= part[0] + part[1] + ...: one workgroup, every thread a contiguous run, the runs added by thread index
__global__ __launch_bounds__(NT) void nmf_sum_kernel(const double *__restrict__ part, int n, double *__restrict__ out, int accumulate) {
    __shared__ double red[NT];
    __shared__ double total;
    const int per_thread = (n + NT - 1) / NT;
    const int t0 = min(n, (int)threadIdx.x * per_thread), t1 = min(n, t0 + per_thread);
    double s = 0.0;
    for (int i = t0; i < t1; ++i) s += part[i];
    block_sum_to(s, red, &total);
    if (threadIdx.x == 0) out[0] = accumulate ? out[0] + total : total;
}

// the float64 scalars of a handle: the violation total of the sweeps, two sums of a divergence, the divergence
enum Scalar { SC_VIOLATION = 0, SC_A, SC_B, SC_OUT, N_SCALARS };

// scal[SC_OUT] of the two divergences from the sums the kernels above left in scal[SC_A] and scal[SC_B]
__global__ void nmf_divergence_kernel(double *scal, int loss, double norm_x, double sum_x) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    // frobenius: (|X|^2 + tr((W^T W)(H H^T)) - 2 sum (X H^T) o W) / 2;  Kullback-Leibler: sum x log(x / wh) + (sum W)(sum H) - sum x
    scal[SC_OUT] = loss == 0 ? (norm_x + scal[SC_A] - 2.0 * scal[SC_B]) / 2.0 : scal[SC_A] + scal[SC_B] - sum_x;
}

}  // namespace
