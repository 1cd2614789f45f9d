// eval_diversity.cuh -- DIVERSITY_SIMILARITY (Base/Evaluation/metrics.py:641-694 Diversity_similarity.add_recommendations, called per
// user and cutoff from Evaluator.py:353-354) over ranked lists in HBM, against a dense n_items x n_items matrix that stays in HBM.
//
//   eval_diversity_kernel        one workgroup per user (one wavefront for lists of at most 64 entries, four above).  The list's ids go to
//                                LDS once; every address D + items[i] * n_items + items[j] follows from them, so no load depends on
//                                another.  The cells of ALL cutoffs are read in one pass: cell (i, j) belongs to shell max(i + 1, j)
//                                (eval_plan.h), a shell is two runs, a run is walked by ONE thread in ascending order with eight gathers
//                                in flight, and its float64 sum goes to LDS.  A cutoff's numerator is the running sum of the shells
//                                below its length, ascending.  No atomics on values: a user's value depends on its list and the matrix
//                                only, not on the block, the path, the other cutoffs or the width of the workgroup.  A list of fewer
//                                than two items gives NaN (the reference divides by zero there).
//   eval_diversity_range_kernel  counts the cells outside [0, 1], NaN included (the assertion of metrics.py:655-656).
// Included by eval.hip, inside its `#pragma clang fp contract(off)`.
#pragma once

#include "eval_plan.h"

namespace mi355rec {
namespace {

struct DivParams {
    int n_items, width, n_cut, first;
    const int *cut;                 // [n_cut] cutoffs as given
    const int *ranked;              // [n][width], -1 padded at the end
    const void *matrix;             // [n_items][n_items] float32 or float64, row-major
    double *vals;                   // [n_eval][n_cut]
};

template <class T, int NT, int WIDTH>
__global__ __launch_bounds__(NT) void eval_diversity_kernel(const DivParams p) {
    using namespace evalplan;
    __shared__ int s_items[WIDTH];
    __shared__ double s_run[2 * WIDTH];             // run w of the list: shell w / 2 + 1, column run first
    __shared__ int s_len;
    const int t = threadIdx.x, b = blockIdx.x;
    const int *row = p.ranked + (size_t)b * p.width;
    const T *__restrict__ D = static_cast<const T *>(p.matrix);
    if (t == 0) s_len = p.width;
    __syncthreads();
    for (int j = t; j < p.width; j += NT) {
        const int item = row[j];
        s_items[j] = item;
        if (item < 0 || item >= p.n_items) atomicMin(&s_len, j);       // the list ends at the first entry that is no item
    }
    __syncthreads();
    const int len = s_len, n_runs = div_run_count(len);
    for (int w = t; w < n_runs; w += NT) {
        const DivRun r = div_run(w);
        double s = 0.0;
        int q = 0;
        for (; q + 8 <= r.count; q += 8) {
            T v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = D[div_run_cell(r, s_items, q + e, p.n_items)];
#pragma unroll
            for (int e = 0; e < 8; ++e) s += (double)v[e];
        }
        for (; q < r.count; ++q) s += (double)D[div_run_cell(r, s_items, q, p.n_items)];
        s_run[w] = s;
    }
    __syncthreads();
    for (int c = t; c < p.n_cut; c += NT) {
        const int shells = div_cutoff_shells(p.cut[c], len);
        double value = __builtin_nan("");
        if (shells > 0) {
            double numerator = 0.0;
            for (int k = 1; k <= shells; ++k) numerator += s_run[2 * (k - 1)] + s_run[2 * (k - 1) + 1];
            value = numerator / div_denominator(p.cut[c], len);
        }
        p.vals[((size_t)p.first + b) * p.n_cut + c] = value;
    }
}

template <class T>
__global__ __launch_bounds__(256) void eval_diversity_range_kernel(const T *__restrict__ D, unsigned long long cells, unsigned long long *bad) {
    __shared__ unsigned part[256];
    const int t = threadIdx.x;
    unsigned n = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + t; i < cells; i += (unsigned long long)gridDim.x * 256) {
        const T v = D[i];
        n += !(v >= (T)0 && v <= (T)1);
    }
    part[t] = n;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) part[t] += part[t + w];
        __syncthreads();
    }
    if (t == 0 && part[0]) atomicAdd(bad, (unsigned long long)part[0]);
}

template <class T>
void launch_diversity_typed(const DivParams &p, int n, hipStream_t s) {
    if (evalplan::div_threads(p.width) == 64) hipLaunchKernelGGL((eval_diversity_kernel<T, 64, evalplan::DIV_SMALL_WIDTH>), dim3(n), dim3(64), 0, s, p);
    else hipLaunchKernelGGL((eval_diversity_kernel<T, 256, evalplan::DIV_MAX_WIDTH>), dim3(n), dim3(256), 0, s, p);
}

}  // namespace
}  // namespace mi355rec
